"""Textured scenes on the ladder's room (tests/scene_ladder.py, rung emitters_3: floor, wall, two boxes, three emissive
slabs), shared by tests/test_texture_cases.py (CPU: the oracle alone proves that every case sits where its name says)
and tests/test_gpu_textures.py (GPU parity on every case).  Each case is a (scene, camera, lights) triple; `swap` and
`gains_texture` are sequences over one.

  wrap_all           mesh uvs remapped to [-2.5, 3.5]; 18 textures of odd, non-square sizes, the nine address pairs x
                     both filters, over all four material slots (sRGB base colour / emissive, unorm metallic /
                     occlusion), so texel offsets are multiples of nothing
  one_texel          1x1, 1xN and Nx1 images, each under all 18 samplers (54 textures; seven extra materials on chips)
  huge_uv            box 0's uvs scaled until u*W passes +-1e6, box 1's until it passes +-2^31 (the saturated convert)
  emitters_textured  an sRGB emissive image per slab: half black, all black, alpha below 255
  ids                texture ids U32_MAX, n_textures and n_textures + 7, one texture in all four slots, a normal map
  alpha              base-colour images with alpha below 255
  swap               uploads A (18 textures), B (5 textures of other sizes), none, A under one scene whose ids reach 17
  gains_texture      a material replacement that gives one instance a texture and takes another's away

Every texture id a case uses is either below the uploaded count or refused by has_texture (id != U32_MAX and
id < n_textures): no case can make a kernel read past the texture arrays.
"""
from __future__ import annotations

import numpy as np

import scene_ladder as sl

SEED = 0x54455843  # "TEXC"
RUNG = "emitters_3"
SIZE = sl.SIZE  # 64 x 48
FRAMES = 6
SLOTS = ("base_color_texture", "emissive_texture", "metallic_roughness_texture", "occlusion_texture")
SRGB_SLOT = {"base_color_texture": True, "emissive_texture": True, "metallic_roughness_texture": False,
             "occlusion_texture": False}
# materials of the rung, in order: floor, wall, box 0, box 1, slab 0, slab 1, slab 2
FLOOR, WALL, BOX0, BOX1, SLAB0, SLAB1, SLAB2 = range(7)
SAMPLERS = [(au, av, fl) for au in range(3) for av in range(3) for fl in range(2)]  # 18
ODD_SIZES = [(3, 5), (5, 3), (7, 2), (2, 7), (9, 4), (4, 9), (5, 7), (7, 5), (11, 3)]  # (W, H)
ONE_TEXEL_SIZES = [(1, 1), (1, 6), (5, 1)]
# 18 (material, slot) places: the four slots of floor, wall and both boxes, the emissive slot of two slabs
PLACES = [(m, s) for m in (FLOOR, WALL, BOX0, BOX1) for s in SLOTS] + [(SLAB0, "emissive_texture"),
                                                                       (SLAB2, "emissive_texture")]


def _texels(rng, w, h, lo=0, alpha=255):
    t = rng.integers(lo, 256, (h, w, 4), dtype=np.uint8)
    t[..., 3] = alpha
    return t


def _remap_uvs(scene, scale=6.0, offset=-2.5):
    for m in scene.meshes:
        m.uvs = (np.asarray(m.uvs, np.float32) * np.float32(scale) + np.float32(offset)).astype(np.float32)


def _place_samplers(scene, places, samplers, rng):
    """One texture per (material, slot) of `places`, with the k-th ((address_u, address_v, filter), (W, H)) of
    `samplers`."""
    from hikari_amd import Texture
    assert len(places) >= len(samplers)
    for (mat, slot), ((au, av, fl), (w, h)) in zip(places, samplers):
        # emissive images stay bright enough that the slabs still light the room
        tex = Texture(_texels(rng, w, h, lo=96 if slot == "emissive_texture" else 0), srgb=SRGB_SLOT[slot],
                      address_u=au, address_v=av, filter=fl)
        setattr(scene.materials[mat], slot, scene.add_texture(tex))


def wrap_all(textured=True, remap=True):
    scene, cam, lights = sl.build(RUNG)
    if remap:
        _remap_uvs(scene)
    if textured:
        _place_samplers(scene, PLACES, [(smp, ODD_SIZES[k % len(ODD_SIZES)]) for k, smp in enumerate(SAMPLERS)],
                        np.random.default_rng([SEED, 0]))
    return scene, cam, lights


ONE_TEXEL_CHIPS = 7  # extra instances of box 0 in a row before the camera, each with a material of its own


def one_texel():
    """All 54 (sampler, shape): every address pair and filter on a 1x1, a 1x6 and a 5x1 image.  Seven chips (small
    copies of box 0 with their own materials) bring the room to 14 materials, 56 slots."""
    from hikari_amd import StandardMaterial, Transform
    scene, cam, lights = sl.build(RUNG)
    _remap_uvs(scene)
    mesh = next(me for me, ma, _ in scene.instances if ma == BOX0)
    chips = []
    for k in range(ONE_TEXEL_CHIPS):
        chips.append(scene.add_material(StandardMaterial(base_color=(0.9 - 0.1 * k, 0.4 + 0.07 * k, 0.5, 1.0),
                                                         perceptual_roughness=0.5 + 0.05 * k, metallic=0.3)))
        t = Transform(np.array([-1.2 + 0.4 * k, 0.0, 1.1]), scale=np.full(3, 0.5))
        scene.add_instance(mesh, chips[-1], t.matrix())
    places = [(m, s) for m in [FLOOR, WALL, BOX0, BOX1] + chips + [SLAB0, SLAB1, SLAB2] for s in SLOTS]
    _place_samplers(scene, places, [(smp, size) for size in ONE_TEXEL_SIZES for smp in SAMPLERS],
                    np.random.default_rng([SEED, 1]))
    return scene, cam, lights


HUGE_SCALE = {BOX0: 4.0e6, BOX1: 6.0e9}  # |u| reaches half of it: u*W >= 1e6 resp. 2^31 for every W >= 1


def huge_uv(scaled=True):
    from hikari_amd import Texture
    scene, cam, lights = sl.build(RUNG)
    rng = np.random.default_rng([SEED, 2])
    k = 0
    for mat in (BOX0, BOX1):
        for slot in SLOTS:
            au, av, fl = SAMPLERS[(5 * k + 1) % 18]
            w, h = ODD_SIZES[k % len(ODD_SIZES)]
            setattr(scene.materials[mat], slot, scene.add_texture(
                Texture(_texels(rng, w, h), srgb=SRGB_SLOT[slot], address_u=au, address_v=av, filter=fl)))
            k += 1
        if scaled:
            mesh = next(me for me, ma, _ in scene.instances if ma == mat)
            uv = np.asarray(scene.meshes[mesh].uvs, np.float32)
            scene.meshes[mesh].uvs = ((uv - np.float32(0.5)) * np.float32(HUGE_SCALE[mat])).astype(np.float32)
    return scene, cam, lights


def emitters_textured(black_by_constant=False):
    """black_by_constant: slab 1 made dark by its emissive constant instead (then it is no emitter at all: the
    control that shows the textured black slab is still in the light BVH)."""
    from hikari_amd import Texture
    scene, cam, lights = sl.build(RUNG)
    rng = np.random.default_rng([SEED, 3])
    half = _texels(rng, 6, 4, lo=128)
    half[:, :3, :3] = 0
    black = np.zeros((3, 5, 4), np.uint8)
    black[..., 3] = 255
    veiled = _texels(rng, 5, 3, lo=128)
    veiled[..., 3] = rng.integers(40, 255, (3, 5), dtype=np.uint8)
    for mat, t, fl in ((SLAB0, half, 0), (SLAB1, black, 1), (SLAB2, veiled, 1)):
        scene.materials[mat].emissive_texture = scene.add_texture(Texture(t, srgb=True, address_u=0, address_v=0, filter=fl))
    if black_by_constant:
        scene.materials[SLAB1].emissive = (0.0, 0.0, 0.0, 1.0)
    return scene, cam, lights


def ids(past_the_end=True, normal_map=True):
    """Two uploaded textures.  floor: texture 0 in all four slots; wall: base colour id n_textures; box 0: base colour
    n_textures + 7 and emissive n_textures; box 1: a normal map (a valid id: light.wgsl never samples it); slab 2:
    emissive id n_textures + 7.  past_the_end=False leaves those ids at U32_MAX, normal_map=False leaves it unset."""
    from hikari_amd import Texture
    scene, cam, lights = sl.build(RUNG)
    rng = np.random.default_rng([SEED, 4])
    t0 = scene.add_texture(Texture(_texels(rng, 5, 3, lo=64), srgb=True))
    t1 = scene.add_texture(Texture(_texels(rng, 3, 7), srgb=False, filter=0))
    n = len(scene.textures)
    for slot in SLOTS:
        setattr(scene.materials[FLOOR], slot, t0)
    if past_the_end:
        scene.materials[WALL].base_color_texture = n
        scene.materials[BOX0].base_color_texture = n + 7
        scene.materials[BOX0].emissive_texture = n
        scene.materials[SLAB2].emissive_texture = n + 7
    if normal_map:
        scene.materials[BOX1].normal_map_texture = t1
    return scene, cam, lights


def alpha(opaque=False):
    """sRGB base-colour images on the floor, the wall and box 0 whose alpha varies in [20, 254] (opaque=True: the same
    rgb with alpha 255)."""
    from hikari_amd import Texture
    scene, cam, lights = sl.build(RUNG)
    rng = np.random.default_rng([SEED, 5])
    for k, mat in enumerate((FLOOR, WALL, BOX0)):
        t = _texels(rng, 5 + k, 3 + 2 * k, lo=64)
        veil = rng.integers(20, 255, t.shape[:2], dtype=np.uint8)  # drawn either way: the rgb of both variants is the same
        if not opaque:
            t[..., 3] = veil
        scene.materials[mat].base_color_texture = scene.add_texture(Texture(t, srgb=True, filter=k % 2))
    return scene, cam, lights


CASES = {"wrap_all": wrap_all, "one_texel": one_texel, "huge_uv": huge_uv, "emitters_textured": emitters_textured,
         "ids": ids, "alpha": alpha}
# the nearest neighbour each case's frames must differ from
NEIGHBOURS = {"wrap_all": lambda: wrap_all(textured=False), "one_texel": wrap_all, "huge_uv": lambda: huge_uv(False),
              "emitters_textured": lambda: sl.build(RUNG), "ids": lambda: sl.build(RUNG),
              "alpha": lambda: sl.build(RUNG)}


# ------------------------------------------------------------------ sequences
def swap_uploads():
    """(triple, [(textures, frames)]): wrap_all's scene, and the texture sets uploaded before each run of frames: A
    (its own 18), B (5 textures of other sizes and samplers: ids 5..17 turn untextured), none (the NO_TEXTURE
    pipeline), A again.  Eight frames in all; the reservoir history is carried throughout."""
    from hikari_amd import Texture
    triple = wrap_all()
    a = list(triple[0].textures)
    rng = np.random.default_rng([SEED, 6])
    b = [Texture(_texels(rng, w, h), srgb=k % 2 == 0, address_u=k % 3, address_v=(k + 1) % 3, filter=(k + 1) % 2)
         for k, (w, h) in enumerate([(4, 4), (1, 3), (13, 2), (6, 5), (2, 2)])]
    return triple, [(a, 3), (b, 2), ([], 1), (a, 2)]


def gains_texture():
    """An instance_set_cases.Case of two steps over the rung's instances: step 1 replaces the materials so that box 0
    gains a base-colour and an occlusion texture, the floor loses its base-colour texture, and slab 0 gains an emissive
    texture.  The textures (three of wrap_all's) are uploaded once."""
    import copy

    import instance_set_cases as ic
    scene, cam, lights = wrap_all(textured=False)
    full = wrap_all()[0]
    textures = full.textures[:3]
    before = copy.deepcopy(scene.materials)
    after = copy.deepcopy(scene.materials)
    before[FLOOR].base_color_texture = 0
    after[BOX0].base_color_texture = 1
    after[BOX0].occlusion_texture = 2
    after[SLAB0].emissive_texture = 1
    ents = [ic.Entity(k, mesh, mat, m) for k, (mesh, mat, m) in enumerate(scene.instances)]
    case = ic._steps(scene.meshes, [ents, ents], per_step_materials=[before, after], textures=textures)
    case.scenes[0].build()
    return case, cam, lights


# ------------------------------------------------------------------ shared by the tests
def settings(bounces=2):
    return sl.ladder_settings(bounces)


def gbuffer(triple, size=SIZE, frame=0):
    """(material index per pixel or -1, uv per pixel) of the oracle's G-buffer."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    scene, cam, lights = triple
    w, h = size
    o = Oracle(scene.desc if scene.desc is not None else scene.build(), load_noise(), w, h, 1.0, textures=scene.textures)
    o.render_gbuffer(frame_inputs(frame, cam, lights, w, h))
    depth = o.output(11).view(np.float32).reshape(h, w, 4)[..., 3]
    im = o.output(14).view(np.float32).reshape(h, w, 2)  # (instance + 0.5, material + 0.5)
    uv = o.output(15).view(np.float32).reshape(h, w, 4)[..., 2:4]
    o.close()
    return np.where(depth > 0, np.floor(im[..., 1]).astype(np.int64), -1), uv


def frames(triple, n=2, size=(32, 24), bounces=2, uploads=None):
    """Canonical frames (parity.canon_frame) of the oracle over frames 0..n-1."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    from parity import canon_frame, passes
    scene, cam, lights = triple
    w, h = size
    o = Oracle(scene.desc if scene.desc is not None else scene.build(), load_noise(), w, h, 1.0, textures=scene.textures)
    s = settings(bounces).to_c()
    out = []
    for f in range(n):
        passes(o, s, frame_inputs(f, cam, lights, w, h))
        out.append(canon_frame(o))
    o.close()
    return out


def oracle_decode_table(desc):
    """The oracle's (2, 256) texel decode table [sRGB, unorm], read through a 256x1 nearest ramp."""
    import texture_numpy as tn
    from hikari_amd import Texture, load_noise
    from oracle import Oracle
    t, uv = tn.ramp()
    o = Oracle(desc, load_noise(), 8, 8, 1.0, textures=[Texture(t, srgb=True, filter=0), Texture(t, srgb=False, filter=0)])
    lut = np.stack([o.sample_texture(0, uv)[:, 0], o.sample_texture(1, uv)[:, 0]])
    o.close()
    return lut


def python_scene(scene, lib):
    """direct_python.Scene of a built scene with its textures bound."""
    import direct_python as dp
    sc = dp.Scene(scene.arrays(), lib)
    if scene.textures:
        sc.set_textures(scene.textures, oracle_decode_table(scene.desc))
    return sc


def same_frames(a, b):
    return all(np.array_equal(x, y) for fa, fb in zip(a, b) for pa, pb in zip(fa, fb) for x, y in zip(pa, pb))
