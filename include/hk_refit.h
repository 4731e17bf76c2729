/*
 * hk_refit.h — the refit rule, written once for both sides: the host functions (csrc/hk_scene.cpp hks_refit_nodes and
 * hks_refit_boxes, gcc) and the gfx950 kernels (csrc/hk_dynamic.hip k_refit_small / k_refit_large for BLAS slices,
 * k_refit_trees_small / k_refit_trees_large for the TLAS and the light BVH, hipcc) compile these bodies, like hk_skin.h.
 *
 * What it restates: nothing.  The reference rebuilds every changed mesh's BLAS (mesh.rs:77-166), and so do
 * hk_update_meshes and hk_skin_meshes.  A refit keeps a slice's topology and recomputes its boxes; the rule below is
 * this project's own design and the contract of hks_refit_nodes / hk_refit_meshes / hk_skin_meshes_refit, unpinned
 * against any reference.
 *
 * A mesh's node slice is the bvh-0.7.1 flatten of hk_scene.cpp BvhBuilder::flatten: 3k - 2 hk_nodes over k primitives,
 * node indices relative to the slice, in pre-order.  Node i is
 *   a leaf        entry_index >= HK_BVH_LEAF_FLAG, payload = the mesh-local primitive, exit_index = i + 1;
 *   an entry node entry_index = i + 1, exit_index = e: it carries the box of the subtree stored in (i, e).
 *
 * Refit of one slice, given the mesh's primitives after the deformation:
 *   shape box     S[t] of primitive t exactly as the build folds it (Aabb::grow): from empty (+inf / -inf), corners 0,
 *                 1, 2 in order, with std::fmin / std::fmax as gcc evaluates them (hk_refit_fmin / hk_refit_fmax: of two
 *                 equal operands the second, a NaN operand loses).
 *   leaves        every byte stays (on the host the box of a leaf is the empty one).
 *   entry nodes   entry_index and exit_index stay.  min[c] = the fold of S[t].min[c] over every leaf t stored in (i, e)
 *                 with hk_minf, max[c] likewise with hk_maxf.
 * hk_minf / hk_maxf (hk_math.h) take a NaN as missing data and order -0 < +0; they are commutative and associative over
 * all 2^32 patterns, so the fold has no order: the host walks the slice backwards joining child boxes, the device scans
 * each subtree's range in parallel, and both store the same words.  A component whose corners are all NaN stays
 * +inf / -inf.  Unchanged vertices give the built tree's boxes as floats (==); only the sign of a zero bound can differ,
 * which the build's fold takes by position.
 *
 * Refit over given shape boxes (hks_refit_boxes): the same rule with S[t] handed in instead of folded
 * from a primitive.  The leaf with payload t contributes S[t]; an entry node keeps entry_index and exit_index, and its
 * box becomes the hk_refit_join fold of S[t] over the leaves stored in (i, exit); leaves keep every byte.  The TLAS and
 * the light BVH are the same flatten over the instances and the emitters (the reference rebuilds both,
 * instance.rs:284-437, and so do hk_update_instances and every call that ends in it), and their shape boxes are
 *   TLAS        S[t] = instance t's world box: min / max of its hk_instance record (hk_refit_instance_box), which is
 *               what the build consumed;
 *   light BVH   S[e] = emitter e's sphere box: position[k] - radius and position[k] + radius of its hk_emissive record,
 *               each component one f32 operation (hk_refit_emitter_box), as the build derives it.
 * An instance's or an emitter's node_index names its leaf, and the leaves stay where they are: every node_index stays.
 * Unchanged models give the built trees' boxes as floats (==); a zero bound may differ in sign, as above: the build's
 * joins take std::fmin / std::fmax by position (of +0 and -0 the second operand), the refit's fold orders -0 < +0.
 */
#ifndef HK_REFIT_H
#define HK_REFIT_H

#include "hk_math.h"
#include "hk_types.h"

/* std::fmin / std::fmax as the host builder's Aabb::grow evaluates them */
HK_HD float hk_refit_fmin(float a, float b) { return (a < b || b != b) ? a : b; }
HK_HD float hk_refit_fmax(float a, float b) { return (a > b || b != b) ? a : b; }

HK_HD int hk_refit_is_leaf(uint32_t entry_index) { return entry_index >= HK_BVH_LEAF_FLAG; }
HK_HD uint32_t hk_refit_leaf_primitive(uint32_t entry_index) { return entry_index & ~HK_BVH_LEAF_FLAG; }

/* box: min xyz, max xyz */
HK_HD void hk_refit_empty(float* box)
{
    const float inf = hk_u2f(0x7F800000u);
    for (int k = 0; k < 3; ++k) {
        box[k] = inf;
        box[3 + k] = -inf;
    }
}

/* S[t]: the shape box of a primitive from its three corner positions, in corner order */
HK_HD void hk_refit_shape(const hk_primitive* p, float* box)
{
    hk_refit_empty(box);
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) {
            box[k] = hk_refit_fmin(box[k], p->vertices[c].position[k]);
            box[3 + k] = hk_refit_fmax(box[3 + k], p->vertices[c].position[k]);
        }
}

/* S[t] of the TLAS and S[e] of the light BVH, from the records */
HK_HD void hk_refit_instance_box(const hk_instance* in, float* box)
{
    for (int k = 0; k < 3; ++k) {
        box[k] = in->min[k];
        box[3 + k] = in->max[k];
    }
}
HK_HD void hk_refit_emitter_box(const hk_emissive* em, float* box)
{
    for (int k = 0; k < 3; ++k) {
        box[k] = em->position[k] - em->radius;
        box[3 + k] = em->position[k] + em->radius;
    }
}

/* one step of an entry node's fold: box joined with a shape box or with the box of a node of its subtree */
HK_HD void hk_refit_join(float* box, const float* mn, const float* mx)
{
    for (int k = 0; k < 3; ++k) {
        box[k] = hk_minf(box[k], mn[k]);
        box[3 + k] = hk_maxf(box[3 + k], mx[k]);
    }
}

#endif /* HK_REFIT_H */
