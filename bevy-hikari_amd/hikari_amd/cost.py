"""Tree costs: the quality query behind a refit-or-rebuild decision, and a small caller-side policy.

TreeCost mirrors include/hikari_amd.h hk_tree_cost; tree_cost(nodes) is hks_tree_cost, on the host;
HikariRenderer.tree_costs asks the device for the resident trees (hk_tree_costs).  The rule is include/hk_cost.h's: each
entry node weighted by its box's half area over the root's.  Only ratios between two trees over the same shapes mean
anything."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _abi


@dataclass(frozen=True)
class TreeCost:
    """One flattened tree's cost: `inner` and `leaf` are 32.32 fixed-point sums (the expected further box tests and the
    expected shape tests of a ray that meets the root box, x 2^32), `entries` the entry nodes they were summed over,
    `root_half_area` the divisor.  A tree of one shape, or no tree, is all zeros."""
    inner: int = 0
    leaf: int = 0
    root_half_area: float = 0.0
    entries: int = 0

    def total(self, c_box: float = 1.0, c_shape: float = 1.0) -> float:
        """(c_box x inner + c_shape x leaf) / 2^32 with the caller's SAH constants."""
        return (c_box * self.inner + c_shape * self.leaf) / 4294967296.0

    @classmethod
    def from_c(cls, c: "_abi.hk_tree_cost") -> "TreeCost":
        return cls(int(c.inner), int(c.leaf), float(c.root_half_area), int(c.entries))


def tree_cost(nodes) -> TreeCost:
    """The cost of a flattened tree on the host (hks_tree_cost): `nodes` are 32-byte hk_node records, a bvh-0.7.1
    flatten of 3k - 2 nodes (a mesh's slice of the asset nodes, the instance nodes, the emissive nodes); none at all
    gives zeros.  Raises HikariError when they are not such a flatten."""
    n = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    if len(n) % 32:
        raise ValueError("nodes are 32 bytes each")
    out = _abi.hk_tree_cost()
    rc = _abi.lib().hks_tree_cost(n.ctypes.data if len(n) else None, len(n) // 32, out)
    if rc != 0:
        raise _abi.HikariError(f"hks_tree_cost refused the tree ({rc}): not a flatten of 3k - 2 nodes over k shapes")
    return TreeCost.from_c(out)


class RefitPolicy:
    """Refit until a kept tree costs more than `ratio` times what it cost at its last build, then rebuild.

    The policy is the caller's, not the library's: it remembers each tree's total() at its last build (`at_build`, by
    name: "tlas", "lights"), and after a refit `stale(now)` names the trees whose cost now exceeds ratio x that.  The
    decision itself is the pure function decide(now, at_build).  update_instances(renderer, models, local_aabbs) is the
    loop around it: refit (hk_refit_instances), query (hk_tree_costs), and where a tree is stale rebuild
    (hk_update_instances) and take the rebuilt trees' costs as the new baseline.

    `ratio` has no default: what a cost ratio is worth in frame time depends on the scene and the view (DESIGN row f14
    prints the two side by side for one scene), and the rebuild it buys has its own price.

    Known weakness: the baseline is the cost at the last BUILD, not the cost a build would have NOW.  When the shapes
    themselves became worse to partition (instances that drew together, say: tests/instance_refit_cases.py `coincident`
    costs 165.7 freshly built against 11.8 before the move), the refit tree is stale by this measure although a
    rebuild cannot do better: the policy rebuilds once for nothing, re-baselines on the result and is quiet again."""

    def __init__(self, ratio: float, c_box: float = 1.0, c_shape: float = 1.0):
        if not ratio > 0.0:
            raise ValueError("ratio must be positive")
        self.ratio = float(ratio)
        self.c_box, self.c_shape = float(c_box), float(c_shape)
        self.at_build: dict | None = None

    def totals(self, costs: dict) -> dict:
        """{name: total()} of the trees of a tree_costs() result (its "meshes" list is not the instance trees')."""
        return {k: v.total(self.c_box, self.c_shape) for k, v in costs.items() if isinstance(v, TreeCost)}

    def decide(self, now: dict, at_build: dict) -> list:
        """The names, sorted, of the trees whose total in `now` exceeds ratio x their total in `at_build` (both {name:
        total}; a name without a baseline is not stale).  Depends on nothing but its arguments and the ratio."""
        return sorted(k for k, v in now.items() if k in at_build and v > self.ratio * at_build[k])

    def stale(self, now: dict) -> list:
        return [] if self.at_build is None else self.decide(now, self.at_build)

    def rebaseline(self, renderer, stream=None) -> None:
        """Take the resident trees as built: their costs are the baseline from now on."""
        self.at_build = self.totals(renderer.tree_costs(stream=stream))

    def update_instances(self, renderer, models, local_aabbs, stream=None) -> list:
        """Move the instances with a refit; rebuild when the policy says so.  Returns the stale trees' names (empty:
        the refit stands).  The first call takes the trees it finds as built."""
        if self.at_build is None:
            self.rebaseline(renderer, stream)
        renderer.update_instances(models, local_aabbs, stream, refit=True)
        stale = self.stale(self.totals(renderer.tree_costs(stream=stream)))
        if stale:
            renderer.update_instances(models, local_aabbs, stream, refit=False)
            self.rebaseline(renderer, stream)
        return stale
