"""Per-kernel instruction statistics of a gfx950 ISA dump (hipcc --cuda-device-only -S).

usage: python tools/isa_stats.py <file.s> [name filter]
       python tools/isa_stats.py --loads <file.s> [name filter]

The first form prints one line per kernel symbol: instruction counts, and the VGPRs, scratch and static LDS of the
code-object metadata.  --loads lists, per kernel symbol and in program order, each group of global loads (the loads
issued with no vmcnt wait between them) and the vmcnt wait that follows it: one line per dependent round trip of the
straight-line code.
"""
import re
import sys

args = sys.argv[1:]
loads_mode = bool(args) and args[0] == "--loads"
if loads_mode:
    args = args[1:]
s = open(args[0]).read()
filt = args[1] if len(args) > 1 else ""

# code-object metadata (amdhsa.kernels): per kernel name
meta = {}
for block in re.split(r"^\s*- \.agpr_count:", s[s.find("amdhsa.kernels"):], flags=re.M)[1:]:
    name = re.search(r"\.name:\s+(\S+)", block)
    if name:
        val = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        meta[name.group(1)] = (val("vgpr_count"), val("private_segment_fixed_size"), val("group_segment_fixed_size"))


def instructions(body):
    return [l.strip() for l in body.splitlines()
            if l.startswith("\t") and not l.startswith("\t.") and l.strip() and not l.strip().startswith(";")]


def load_groups(ins):
    """[(loads of the group, the wait's text or None, instructions between the last load and the wait)]"""
    groups, cur, last = [], [], 0
    for k, line in enumerate(ins):
        op = line.split()[0]
        if op.startswith("global_load"):
            cur.append(op[len("global_load_"):])
            last = k
        elif op == "s_waitcnt" and "vmcnt" in line and cur:
            groups.append((cur, re.search(r"vmcnt\(\d+\)", line).group(0), k - last - 1))
            cur = []
    if cur:
        groups.append((cur, None, 0))
    return groups


starts = [m for m in re.finditer(r"^(_Z\w+):", s, re.M)]
for i, m in enumerate(starts):
    name = m.group(1)
    if filt not in name:
        continue
    end = starts[i + 1].start() if i + 1 < len(starts) else len(s)
    body = s[m.start():end].split(".Lfunc_end")[0]
    lines = instructions(body)
    if loads_mode:
        groups = load_groups(lines)
        print(f"{name}: {len(groups)} load groups, {sum(len(g[0]) for g in groups)} global loads")
        for loads, wait, gap in groups:
            kinds = ", ".join(f"{loads.count(k)} x {k}" for k in dict.fromkeys(loads))
            print(f"    {kinds:48s} -> {wait or 'no wait'} after {gap} instructions")
        continue
    ins = [l.split()[0] for l in lines]
    cnt = lambda p: sum(1 for x in ins if x.startswith(p))
    vgpr, scratch, lds = meta.get(name, (-1, -1, -1))
    print(f"{name[:64]:64s} insts {len(ins):5d} valu {cnt('v_'):5d} salu {cnt('s_'):5d} "
          f"div_scale {cnt('v_div_scale'):3d} rcp {cnt('v_rcp_f32'):3d} sqrt {cnt('v_sqrt_f32'):3d} "
          f"cvt_f16 {cnt('v_cvt_f16') + cnt('v_cvt_pk'):3d} global_ld {cnt('global_load'):3d} ds {cnt('ds_'):3d} "
          f"vgpr {vgpr:3d} scratch {scratch} lds {lds}")
