/*
 * hikari_scene.h — C ABI of the host-side scene builder (part of libhikari_amd.so).
 *
 * Restates bevy-hikari's `mesh_material` upload path, which the north star keeps on the
 * host: Mesh -> GpuMesh conversion with one BLAS per mesh (mod.rs:379-467), concatenation
 * into the universal vertex/primitive/node buffers (mesh.rs:106-166), material table
 * (material.rs:139-203), and `prepare_instances` (instance.rs:245-444): world AABBs, TLAS,
 * per-emitter alias tables, emissive list and light BVH.  The result is an hk_scene_desc
 * ready for hk_scene_upload.
 *
 * The BVH builder restates the third-party crate `bvh = "=0.7.1"` (Cargo.toml:21), which
 * is not in the reference checkout: SAH over 6 centroid buckets on the largest centroid
 * axis, one shape per leaf, `flatten_custom` DFS order with entry/exit skip pointers
 * (3n-2 nodes for n shapes).  Structural parity with that crate is unpinned.
 */
#ifndef HIKARI_SCENE_H
#define HIKARI_SCENE_H

#include <stdint.h>
#include "hikari_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hks_scene hks_scene;

enum { HKS_TRIANGLE_LIST = 0, HKS_TRIANGLE_STRIP = 1 };

hks_scene* hks_create(void);
void hks_destroy(hks_scene* scene);
const char* hks_last_error(const hks_scene* scene);

/* Mesh asset (Bevy `Mesh`): positions/normals xyz, uvs (u, v); indices may be NULL (=> 0..n-1).
 * Returns the mesh id (>= 0) or a negative error like `PrepareMeshError` (mod.rs:302-309). */
int hks_add_mesh(hks_scene* scene, const float* positions, const float* normals, const float* uvs,
                 uint32_t vertex_count, const uint32_t* indices, uint32_t index_count, int topology);
/* StandardMaterial as the GpuStandardMaterial record (material.rs:162-199). Returns id. */
int hks_add_material(hks_scene* scene, const hk_material* material);
/* Visible entity with (mesh, material) and its GlobalTransform (column-major 4x4). Returns id. */
int hks_add_instance(hks_scene* scene, uint32_t mesh, uint32_t material, const float* model);

/* Build BLAS/TLAS/light BVH and the flat buffers; `buckets` = SAH buckets (6 = bvh 0.7.1). */
int hks_build(hks_scene* scene, int buckets);
/* Pointers stay valid until the next hks_build / hks_destroy. */
int hks_get_desc(const hks_scene* scene, hk_scene_desc* out);

/* 1 when n >= 1 and the n column-major 4x4 matrices (n blocks of 64 bytes) are bitwise equal, 0 otherwise: the
 * property behind hk_scene_shared_transform, for callers that want it without a device. */
int hks_shared_transform(const float* matrices, uint32_t n);

/* The world box (min xyz, max xyz) of n instances from their column-major models and local boxes (6 floats each: centre
 * xyz, half extents xyz), every corner transformed in double and the box grown outward by a relative 1e-5.  Returns 1,
 * or 0 without a box (n == 0, a null pointer, a non-finite corner). */
int hks_instance_bounds(const float* models, const float* local_aabbs, uint32_t n, double aabb[6]);
/* A conservative pixel rectangle [rect[0], rect[2]) x [rect[1], rect[3]) of a width x height frame outside which no
 * primary ray of `view` (hk_render_gbuffer, any prepass jitter) can meet the box: the pixel box of its 8 projected
 * corners, grown by `guard` pixels and clipped to the frame; all zeros when the box is off screen.  Returns 1, or 0 when
 * there is no such rectangle: a corner at or behind the near plane (the eye inside or next to the box), a perspective
 * view whose world_position is not its centre of projection, non-finite input.  This is the bound behind option
 * bg_tile_skip. */
int hks_screen_bounds(const double aabb[6], const hk_view* view, uint32_t width, uint32_t height, uint32_t guard,
                      int32_t rect[4]);
/* The tone pass over a kept rectangle (hk_tone_sum, hk_tone_skip_info).  keep: a pixel rectangle [x0, y0, x1, y1) in frame
 * coordinates; window: the launch's window [col0, row0, col1, row1) in the coordinates of a plane whose row 0 is frame
 * row `row0` and whose columns are the frame's; run: the pixels of a row one thread takes (the window's column edges
 * must be multiples of it).  launch: keep within the window, in plane coordinates, its columns rounded outward to whole
 * runs.  Returns 1, or 0 with launch all zeros when nothing is to be launched (an empty keep or intersection) or an
 * argument is unusable (a null pointer, run == 0, an empty or unaligned window). */
int hks_tone_rect(const int32_t keep[4], const int32_t window[4], int32_t row0, uint32_t run, int32_t launch[4]);
/* The tiles of a launch's own grid that meet a kept rectangle (the background tile skip, hk_tile_skip_info).  keep and
 * window as for hks_tone_rect; the grid's tile (0, 0) starts at the window's first column and row and the grid has
 * ceil(columns / tile) x ceil(rows / tile) tiles of tile x tile pixels.  tiles: [tx0, ty0, tx1, ty1), the tiles holding a
 * pixel of keep (the runtime's TileKeep: a workgroup outside them returns at once; a launch over them alone would have
 * (tx1 - tx0) x (ty1 - ty0) workgroups at tile offset (tx0, ty0)).  Returns 1, or 0 with tiles all zeros when no tile is kept or an argument is unusable (a null
 * pointer, tile == 0, an empty window). */
int hks_keep_tiles(const int32_t keep[4], const int32_t window[4], int32_t row0, uint32_t tile, uint32_t tiles[4]);

/* Linear blend skinning of a mesh's vertices on the host, by the rule of include/hk_skin.h (Bevy 0.9's skinning.wgsl
 * as recalled, its evaluation order pinned there): the host side of hk_skin_meshes' contract, and what a caller without
 * a device uses.  positions / normals: the bind pose, vertex_count x 3; joint_indices: vertex_count x 4 (Uint16x4,
 * Bevy's ATTRIBUTE_JOINT_INDEX); joint_weights: vertex_count x 4, used as given; joints: joint_count column-major 4 x 4
 * matrices (joint global transform x inverse bind pose).  out_positions / out_normals: vertex_count x 3, the normals not
 * normalised; normals and out_normals may both be NULL.  out_aabb (may be NULL): the posed mesh's Bevy `Aabb`, centre
 * xyz then half extents xyz, exactly as hks_add_mesh derives a mesh's from its vertices.  Returns 0, or HK_ERR_INVALID
 * with nothing written for a null required pointer (positions, joint_indices, joint_weights, joints, out_positions;
 * normals without out_normals or the reverse), joint_count == 0 or an index >= joint_count. */
int hks_skin_vertices(const float* positions, const float* normals, const uint16_t* joint_indices,
                      const float* joint_weights, uint32_t vertex_count, const float* joints, uint32_t joint_count,
                      float* out_positions, float* out_normals, float out_aabb[6]);

/* Morph targets (blend shapes) of a mesh's vertices on the host, by the rule of include/hk_morph.h (glTF 2.0's
 * morph-target sum and Bevy 0.11's morph.wgsl as recalled, the evaluation order pinned there): the host side of
 * hk_morph_meshes' contract, and what a caller without a device uses.  positions / normals: the base, vertex_count x 3;
 * position_deltas / normal_deltas: TARGET-MAJOR, target_count x vertex_count x 3; weights: target_count.  Per component,
 * f32, never contracted: acc = base, then acc = acc + w[t] * d[t] for t ascending over the targets with w[t] != 0 (a
 * zero weight of either sign is skipped, so a base of -0.0 stays -0.0 and a zero weight on an infinite delta is not
 * NaN; a NaN weight takes part).  The normals take the same fold over normal_deltas and are NOT normalised;
 * normal_deltas == NULL copies the base normals word for word.  normals and out_normals are both NULL or both set.
 * out_aabb (may be NULL): the morphed mesh's Bevy `Aabb` as hks_skin_vertices derives a posed mesh's.  Under a skin the
 * outputs are hks_skin_vertices' positions and normals (glTF's order: morph, then skin).  Returns 0, or HK_ERR_INVALID
 * with nothing written for a null required pointer (positions, position_deltas, weights, out_positions), normals
 * without out_normals or the reverse, normal_deltas without normals, or target_count outside
 * 1 .. HK_MORPH_MAX_TARGETS.  Needs no device. */
#ifndef HK_MORPH_MAX_TARGETS
#define HK_MORPH_MAX_TARGETS 256u
#endif
int hks_morph_vertices(const float* positions, const float* normals, const float* position_deltas,
                       const float* normal_deltas, uint32_t vertex_count, const float* weights, uint32_t target_count,
                       float* out_positions, float* out_normals, float out_aabb[6]);

/* A BLAS refit on the host, by the rule of include/hk_refit.h: the host side of hk_refit_meshes' and
 * hk_skin_meshes_refit's contract, and what a caller without a device uses.  nodes: one mesh's slice of the asset nodes,
 * a bvh-0.7.1 flatten of node_count = 3 x primitive_count - 2 nodes with slice-relative indices; primitives: the mesh's
 * primitive_count primitives after the deformation.  Every entry node's box becomes the hk_minf / hk_maxf fold of the
 * shape boxes of the leaves in its range; entry_index, exit_index and every byte of a leaf stay.  One O(n) pass.
 * Returns 0, or HK_ERR_INVALID with `nodes` untouched for a null pointer, node_count != 3 x primitive_count - 2, or a
 * slice that is not a well-formed flatten: a leaf whose exit is not i + 1 or whose payload is not below primitive_count,
 * a primitive in two leaves or in none, an entry node whose entry is not i + 1 or whose exit is not in (i + 1,
 * node_count], or whose range (i, exit) is not tiled exactly by one leaf or by two entry nodes' ranges. */
int hks_refit_nodes(const hk_primitive* primitives, uint32_t primitive_count, hk_node* nodes, uint32_t node_count);

/* The same refit over GIVEN shape boxes (include/hk_refit.h): the host side of hk_refit_instances'
 * contract.  boxes: count x 6 floats, min xyz then max xyz; the leaf with payload t contributes boxes[t].  For the TLAS
 * boxes[t] is instance t's world box (the min / max of its record), for the light BVH emitter e's sphere box (position -
 * radius, position + radius, one f32 operation per component).  nodes: a bvh-0.7.1 flatten of node_count = 3 x count - 2
 * nodes.  What is stored, what stays, the refusals and the well-formedness checks are hks_refit_nodes' with count for
 * primitive_count; `nodes` is untouched on refusal.  One O(n) backwards pass, no device. */
int hks_refit_boxes(const float* boxes, uint32_t count, hk_node* nodes, uint32_t node_count);

/* The cost of a flattened tree on the host, by the rule of include/hk_cost.h: the host side of hk_tree_costs' contract,
 * and what a caller without a device uses.  nodes: `count` nodes, a bvh-0.7.1 flatten of count = 3k - 2 nodes over k
 * shapes (a mesh's slice of the asset nodes, the instance nodes, the emissive nodes).  out: every field as hikari_amd.h
 * hk_tree_cost describes; count == 0 (no tree: a scene without emitters) and count == 1 (a lone leaf) give zeros.  Leaf
 * boxes are not read.  One O(n) pass, no device.  Returns 0, or HK_ERR_INVALID with `out` untouched for a null pointer
 * (out; nodes with count != 0), a count that is not 3k - 2, or a slice that is not a well-formed flatten, by
 * hks_refit_boxes' checks. */
int hks_tree_cost(const hk_node* nodes, uint32_t count, hk_tree_cost* out);

#ifdef __cplusplus
}
#endif

#endif /* HIKARI_SCENE_H */
