/*
 * hk_morph.h — morph targets (blend shapes) of a mesh's vertices, written once for both sides: the host builder
 * (csrc/hk_scene.cpp hks_morph_vertices, gcc) and the gfx950 kernel (csrc/hk_dynamic.hip k_morph_vertices, hipcc)
 * compile these bodies, like hk_skin.h.
 *
 * What it restates: glTF 2.0's morph-target sum (a primitive's `targets`, each a displacement per vertex, weighted by
 * the mesh's or the node's `weights`: p = base + sum_t w[t] * d[t]) and Bevy 0.11's bevy_pbr morph.wgsl (morph_vertex:
 * a loop over the targets that skips a weight of 0.0 and adds weight * morph(vertex, offset, t) to the position and
 * the normal).  Bevy 0.9 has no morph targets.  Both are RECALLED: neither is part of the reference checkout, so parity
 * with them is unpinned and the rule below is the contract.  The reference itself does not morph.
 *
 * Neither source fixes an evaluation order; this is the project's: f32 throughout, never contracted
 * (-ffp-contract=off on both compile lines).
 *   fold          per component of a vertex: acc = base, then acc = acc + w[t] * d[t] for t in ASCENDING target order:
 *                 one f32 multiply rounded, then one f32 add rounded, per target that takes part.  The deltas are
 *                 target-major: d[t] of vertex v, component a is deltas[(t * vertex_count + v) * 3 + a].
 *   taking part   only the targets with w[t] != 0: a zero of either sign is SKIPPED, as in Bevy's loop.  Observable:
 *                 a base of -0.0 stays -0.0 (-0.0 + 0 * d would be +0.0), and a zero weight on an infinite or NaN
 *                 delta is not NaN.  A NaN weight is not zero, so it takes part (and gives NaN).
 *   normal        the same fold over the normal deltas with the same weights; NOT normalised, as in hk_skin.h (hit_info
 *                 normalises).  A mesh without normal deltas keeps its base normals word for word.
 *   under a skin  the morphed position and normal are the inputs of hk_skin_position and hk_skin_normal with the
 *                 vertex's skin matrix (hk_skin.h): glTF's order, morph then skin.
 *   bounds        hk_skin.h's bounds rule over the final positions.
 */
#ifndef HK_MORPH_H
#define HK_MORPH_H

#include "hk_math.h"

#ifndef HK_MORPH_MAX_TARGETS
#define HK_MORPH_MAX_TARGETS 256u /* targets per mesh at the most */
#endif

/* does target weight w take part in the fold? */
HK_HD int hk_morph_active(float w) { return w != 0.0f; }

/* one step of the fold for one vertex: acc[a] = acc[a] + w * d[a], a = x, y, z */
HK_HD void hk_morph_add(float* acc, float w, const float* d)
{
    for (int a = 0; a < 3; ++a) acc[a] = acc[a] + w * d[a];
}

#endif /* HK_MORPH_H */
