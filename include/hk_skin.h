/*
 * hk_skin.h — linear blend skinning of a mesh's vertices, written once for both sides: the host builder
 * (csrc/hk_scene.cpp hks_skin_vertices, gcc) and the gfx950 kernels (csrc/hk_dynamic.hip k_skin_vertices and
 * k_skin_bounds, hipcc) compile these bodies, like hk_fsr.h and hk_overlay.h.
 *
 * What it restates: Bevy 0.9's bevy_pbr skinning.wgsl (skin_model: the weighted sum of four joint matrices;
 * skin_normals: inverse_transpose_3x3 of its upper-left 3 x 3 times the normal), which the mesh vertex shader applies
 * to a mesh with a SkinnedMesh component.  That file is RECALLED: Bevy is not part of the reference checkout, so
 * parity with it is unpinned and the rule below is the contract.  The reference itself does not skin
 * (README.old.md leaves "Skinned animation" unticked).
 *
 * WGSL leaves the evaluation order open; this is the project's: f32 throughout, left to right as written, never
 * contracted (-ffp-contract=off on both compile lines), `/` correctly rounded.
 *   skin matrix   M = ((w.x * J[i.x] + w.y * J[i.y]) + w.z * J[i.z]) + w.w * J[i.w], element by element; J[k] the
 *                 caller's column-major 4 x 4 (joint global transform x inverse bind pose, what SkinnedMeshUniform
 *                 holds).  The weights are used as given: no renormalisation.  Only rows 0-2 reach a stored value, so
 *                 row 3 is not formed.
 *   position      p' = ((M.c0 * p.x + M.c1 * p.y) + M.c2 * p.z) + M.c3, xyz.
 *   normal        with c0, c1, c2 the columns of mat3(M): X = cross(c1, c2), Y = cross(c2, c0), Z = cross(c0, c1),
 *                 det = dot(c2, Z); cross(a, b).x = a.y * b.z - a.z * b.y (and so on), dot = (xx' + yy') + zz'; the
 *                 columns of the inverse transpose are X / det, Y / det, Z / det, and
 *                 n' = (X' * n.x + Y' * n.y) + Z' * n.z.  NOT normalised: Bevy does not normalise there, and hit_info
 *                 normalises through instance_normal_local_to_world (light.wgsl:324-331, 513-514).  A singular
 *                 mat3(M) stores what IEEE gives (infinities and NaNs).
 *   bounds        the posed mesh's Bevy `Aabb` as hks_add_mesh derives it from vertices: std::fmin / std::fmax folded
 *                 from empty in vertex order (hk_skin_fmin / hk_skin_fmax are those two as gcc evaluates them: of two
 *                 equal operands, which zeros of either sign are, the second; a NaN operand loses), then
 *                 centre = (min + max) * 0.5f, half extents = (max - min) * 0.5f.  Independently of the order: a bound's
 *                 value is the fminf / fmaxf value, and a bound equal to zero carries the sign of the LAST vertex in
 *                 vertex order whose component is a zero (what the device's parallel reduction implements).
 */
#ifndef HK_SKIN_H
#define HK_SKIN_H

#include "hk_math.h"

/* M: 4 columns of 3 rows (M[3 * c + r]) from the four joint matrices (16 floats each, column-major) and weights */
HK_HD void hk_skin_matrix(const float* j0, const float* j1, const float* j2, const float* j3, const float* w, float* M)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) {
            const int e = 4 * c + r;
            M[3 * c + r] = ((w[0] * j0[e] + w[1] * j1[e]) + w[2] * j2[e]) + w[3] * j3[e];
        }
}

HK_HD void hk_skin_position(const float* M, const float* p, float* out)
{
    for (int r = 0; r < 3; ++r) out[r] = ((M[r] * p[0] + M[3 + r] * p[1]) + M[6 + r] * p[2]) + M[9 + r];
}

HK_HD void hk_skin_cross(const float* a, const float* b, float* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

HK_HD void hk_skin_normal(const float* M, const float* n, float* out)
{
    const float *c0 = M, *c1 = M + 3, *c2 = M + 6;
    float X[3], Y[3], Z[3];
    hk_skin_cross(c1, c2, X);
    hk_skin_cross(c2, c0, Y);
    hk_skin_cross(c0, c1, Z);
    const float det = (c2[0] * Z[0] + c2[1] * Z[1]) + c2[2] * Z[2];
    for (int r = 0; r < 3; ++r) out[r] = ((X[r] / det) * n[0] + (Y[r] / det) * n[1]) + (Z[r] / det) * n[2];
}

/* std::fmin / std::fmax as the host builder's Aabb::grow evaluates them */
HK_HD float hk_skin_fmin(float a, float b) { return (a < b || b != b) ? a : b; }
HK_HD float hk_skin_fmax(float a, float b) { return (a > b || b != b) ? a : b; }

/* Bevy `Aabb` (centre xyz, half extents xyz) of a box */
HK_HD void hk_skin_aabb(const float* mn, const float* mx, float* out)
{
    for (int k = 0; k < 3; ++k) {
        out[k] = (mn[k] + mx[k]) * 0.5f;
        out[3 + k] = (mx[k] - mn[k]) * 0.5f;
    }
}

#endif /* HK_SKIN_H */
