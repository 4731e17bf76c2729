/*
 * hk_cost.h — the tree cost rule, written once for both sides: the host function (csrc/hk_scene.cpp hks_tree_cost, gcc)
 * and the gfx950 kernel (csrc/hk_dynamic.hip k_tree_cost behind hk_tree_costs, hipcc) compile these bodies, like
 * hk_refit.h.
 *
 * What it restates: nothing.  The reference has no refit and so no need to ask how good a kept tree still is; the rule
 * is this project's own design and the contract of hks_tree_cost / hk_tree_costs, unpinned against any reference
 * (DESIGN §3).  It is the surface-area heuristic's expectation with the constants left out: a ray that meets the root
 * box meets a convex box inside it with probability (its half area) / (the root's half area).
 *
 * A tree is the bvh-0.7.1 flatten hk_refit.h describes: 3k - 2 hk_nodes over k shapes in pre-order, entry node i carrying
 * the box of the subtree stored in (i, exit_index); the root has no node of its own.
 *
 *   half area   e[c] = max[c] - min[c];  H(box) = (e.x * e.y + e.y * e.z) + e.z * e.x, every operation one f32 operation,
 *               left to right, never contracted into a fused multiply-add (both sides are built with -ffp-contract=off).
 *   root        k >= 2: the box that starts empty (+inf / -inf, hk_refit_empty) and is joined (hk_refit_join) with the box
 *               of node 0 and then with the box of node nodes[0].exit_index: the two top entries.  R = H(root).
 *               k == 1: there is no entry node and every field of the result is 0.
 *   weight      of entry node i: r = H(node i) / R, correctly rounded f32;
 *               q = r >= 1 ? 2^32 : r > 0 ? (uint64_t)(r * 4294967296.0f) : 0.
 *               The cast truncates; the scale by 2^32 is exact.  A NaN fails both comparisons and gives 0, and so does
 *               0 / 0 on a point-sized root.  On a well-formed tree H(node) <= R: the join and the rounding are monotone.
 *   sums        leaf    = the sum of q over the entry nodes with exit_index - i == 2: one leaf lies below each, so this
 *                         is the expected number of shape tests of a ray that meets the root box, scaled by 2^32;
 *               inner   = the sum of q over the other entry nodes: the expected number of further box tests;
 *               entries = the number of entry nodes;  root_half_area = R.
 * The sums are integers, so they have no order: the host adds down the array, the device adds partial sums as they
 * arrive, and both store the same words.  A leaf contributes nothing and its box is not read (on the host it is the
 * empty one, on the device the shape's).
 *
 * The library fixes no SAH constants: a caller forms (c_box * inner + c_shape * leaf) / 2^32 with its own.  ONLY RATIOS
 * between two trees over the same shapes mean anything: a refit tree and a rebuilt one over the same boxes share R, so
 * the ratio of their totals is the ratio of the expected work of a ray through the root box.  It says nothing about
 * rays that miss the root, about two scenes, or about frame time in absolute terms.
 */
#ifndef HK_COST_H
#define HK_COST_H

#include "hk_refit.h"

/* H of a box: min xyz, max xyz */
HK_HD float hk_cost_half_area(const float* box)
{
    const float ex = box[3] - box[0], ey = box[4] - box[1], ez = box[5] - box[2];
    return (ex * ey + ey * ez) + ez * ex;
}

/* the root box from the two top entries' boxes (min xyz, max xyz each); b NULL: node 0's box alone */
HK_HD void hk_cost_root(const float* a, const float* b, float* box)
{
    hk_refit_empty(box);
    hk_refit_join(box, a, a + 3);
    if (b) hk_refit_join(box, b, b + 3);
}

/* q of an entry node of half area h under a root of half area R */
HK_HD uint64_t hk_cost_weight(float h, float R)
{
    const float r = h / R;
    return r >= 1.0f ? (uint64_t)1 << 32 : r > 0.0f ? (uint64_t)(r * 4294967296.0f) : (uint64_t)0;
}

/* entry node i whose range ends at `exit`: one leaf below it (its q goes to `leaf`) or more (`inner`) */
HK_HD int hk_cost_over_leaf(uint32_t i, uint32_t exit) { return exit - i == 2u; }

#endif /* HK_COST_H */
