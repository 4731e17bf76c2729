// hk_launch.h — kernel argument blocks and launchers shared by hk_kernels.hip and the
// host runtime (hk_runtime.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hk_device.h"
#include "../../include/hk_post.h"
#include "../../include/hk_fsr.h"
#include "../../include/hk_overlay.h"

namespace hk {

// Kernel-variant choices of the launchers (host only; hk_set_option keys in parentheses).  They pick
// among bit-identical kernels, so they change speed, never results.
struct LaunchOpts {
    int lds_scene = 1;               // ("lds_scene") 0: no LDS scene staging, 1: where it measured faster, 2: every traversal kernel
    int gbuffer_stack_full = 0;      // ("gbuffer_stack_full") shallow G-buffer walk with all GB_STACK_LDS levels
    int gbuffer_deep = 0;            // ("gbuffer_deep") the deep-scene G-buffer variant on any scene
    double gbuffer_lds_max_px = 6e5; // ("gbuffer_lds_max_px") G-buffer with the scene and its stack in LDS up to this many pixels
    double direct_w4_min_px = 4e5;   // ("direct_w4_min_px") k_direct_lit_w4 from this many pixels up
    int fused_w4 = 1;                // ("fused_w4") the 4-wave fused direct/emissive variants
    int persistent_indirect = 0;     // ("persistent_indirect") k_indirect_persist (opt-in, measured slower)
    int compact_emitter = 0;         // ("compact_emitter") the fused launch's emitter walks compacted per workgroup
    int compact_shadow = 0;          // ("compact_shadow") shadow walks compacted per workgroup (fused launch, indirect)
};

struct FrameArgs {
    Scene sc;
    Frame F;
    GBuffer G;
    const uchar4* noise;  // 16 x 64 x 64 RGBA8
    Counters cnt;
    LaunchOpts opt;       // host-side launcher choices (not read by the kernels)
};
// (host) the columns / rows a launch covers: its window (Frame::win_cols / win_rows) if set, else the plane extent given
inline uint32_t launch_cols(const Frame& F, uint32_t width) { return F.win_cols > 0 ? (uint32_t)F.win_cols : width; }
inline int32_t launch_rows(const Frame& F, int32_t rows) { return F.win_rows > 0 ? F.win_rows : rows; }

// Background tile skip (option bg_tile_skip): the tiles of a launch's own grid, [x0, x1) x [y0, y1), that can hold a
// covered pixel or a background pixel whose constants are still due.  A workgroup outside them would store nothing
// (every pixel background, every target already holding its constants: the runtime's tile_keep derives that from the
// scene's screen bound and the elision masks' history) and returns at its first instruction.  TILE_KEEP_ALL: no skip.
// (The grid stays whole: a grid of the kept tiles alone measured 8.6 % slower per frame)
struct TileKeep {
    uint32_t x0, y0, x1, y1;
};
constexpr TileKeep TILE_KEEP_ALL{0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu};

// One channel's bindings: group 5 (variance/render) + group 6 (reservoir pair) of light.rs:455-555.
struct ChannelArgs {
    ResBuf prev;          // previous_reservoir_buffer  (read)
    ResBuf cur;           // reservoir_buffer            (write)
    ResBuf prev_spatial;  // previous_spatial_reservoir_buffer
    ResBuf spatial;       // spatial_reservoir_buffer
    float* variance;
    uint2* render;
    // Background store elision (k_direct_fused / k_indirect only; nullptr elsewhere): one byte per
    // pixel recording which of the pass's physical targets already hold a background pixel's
    // constant zero words (bit r = reservoir parity r's temporal buffers, bit 2 + s = render /
    // variance slot s, bit 4 = both buffers of the spatial pair).  bg_need = the bits this frame's
    // stores target; when all are set the stores are skipped (same bits in every buffer).
    uint8_t* bg;
    uint32_t bg_need;
    // Spatial view planes (indirect channel; nullptr elsewhere): 3 planes of view_n 16-byte chunks holding
    // what spatial reuse reads from a NEIGHBOUR's temporal record, derived from the packed words this
    // frame's temporal pass stores into `cur` (store_res_view, hk_device.h).  Written by the indirect
    // temporal pass when non-null, read by k_spatial<false, ·, true>.
    uint4* view;
    uint32_t view_n;
};

// Wavefront indirect pass (config 5: material-sorted shading), see hk_kernels.hip k_wf_*.
// The live-pixel queue is split into WF_SEGS segments (tile t -> segment t % WF_SEGS, each with room
// for all its tiles' pixels) so that appends and the material histogram spread their atomics over
// WF_SEGS addresses.  ctl words: [s] live pixels of segment s, [WF_SEGS] all live pixels,
// [WF_CTL_HIST + s * bins + b] segment s's pixels in material bin b, then the same layout of bin
// write cursors.
constexpr uint32_t WF_SEGS = 64;
constexpr uint32_t WF_CTL_HIST = WF_SEGS + 16;
constexpr uint32_t WF_MAX_BINS = 4096;  // materials + 1 (misses); larger scenes use the megakernel
struct WfArgs {
    uint32_t* queue1;  // live pixels (x | local row << 16): segment s at [s * seg_cap, s * seg_cap + count)
    uint32_t* keys;    // material bin per queue1 slot
    uint32_t* queue2;  // all live pixels, grouped by material bin
    uint4* hit;        // per pixel (s plane): instance, primitive, u bits, v bits of the bounce hit
    float* hit_t;      // per pixel: its distance
    uint32_t* ctl;
    uint32_t bins;     // n_materials + 1
    uint32_t seg_cap;  // queue1 slots per segment: 256 x ceil(tiles / WF_SEGS)
};
constexpr uint32_t wf_ctl_words(uint32_t bins) { return WF_CTL_HIST + 2u * WF_SEGS * bins; }

struct ViewArgs {
    float world_position[3];
    float view_proj[16];
    float inverse_view_proj[16];
    // prepass.wgsl:30-54: the primary ray of pixel (x, y) goes through (x + 0.5 - jitter[0], y + 0.5 - jitter[1])
    float jitter[2];
    // motion vectors (prepass.wgsl:96): 0 = camera and every instance static this frame, so the
    // velocity is exactly zero and is not computed
    int motion;
    float previous_view_proj[16];
    const float* previous_models;  // 16 floats per instance: model at the previous k_gbuffer
    // background store elision (as ChannelArgs::bg): bit s = G-buffer slot s holds a miss pixel's
    // zero texels in every plane (position, normal, gradient, ids, velocity/uv, albedo); nullptr = off
    uint8_t* bg;
    uint32_t bg_need;
    // background tile skip: the tiles to run, and the primary rays of the skipped tiles' counted pixels, which the
    // workgroup of tile (0, 0) adds to the counter once
    TileKeep keep;
    uint32_t skipped_primary;
};

// All channels of one frame (post_process.rs:1199-1223 runs them one after another).
struct DenoiseArgs {
    int channels;            // 3, or 2 when indirect_bounces == 0 (post_process.rs:949-954)
    const uint2* albedo;     // S
    const uint2* render[3];  // s
    const float* variance[3];
    // a level's input (the reference's internal textures of the 3 channels, hk_kernels.hip store_level): RGB f16
    // halves packed r0 g0 | b0 r1 | g1 b1 | r2 g2, and b2 | instance bits
    uint4* rgb[4];
    uint2* bi[4];
    float* internal_variance[3];
    uint2* output[3];
    float4* nd;              // per pixel: (normalised normal, depth)
    float4* center;          // per pixel: (depth gradient x, y, luminance denominator of channels 0, 1)
    float* den2;             // per pixel: luminance denominator of channel 2
};

struct ToneArgs {
    const uint2* direct;
    const uint2* emissive;
    const uint2* indirect;  // may be null (indirect_bounces == 0)
    uint2* output;
};

// Dynamic instance update (hk_dynamic.hip): device buffers + scratch, sized by the runtime.
struct DynamicArgs {
    hk_instance* instances;
    uint32_t n_instances;
    const float* models;       // n x 16, column-major
    const float* local_aabbs;  // n x 6: local AABB center xyz, half extents xyz (Bevy Aabb)
    hk_node* tlas;             // 3n - 2 nodes
    hk_emissive* emissives;
    uint32_t n_emissives;
    const hk_material* materials;
    const hk_primitive* primitives;
    hk_alias_entry* alias;
    uint32_t n_alias;
    hk_node* lbvh;             // 3m - 2 nodes
    int buckets;
    // scratch
    float* areas;              // alias entries
    void* alias_work;          // 2 x alias entries x 8 B
    void* boxes;               // max(n, m) x 24 B
    uint32_t* idx;             // 2 x max(n, m)
    void* segments;            // 2 x max(n, m) x 12 B (a refit builds nothing: its list of large nodes lies here)
    uint32_t* flags;           // [0] singular transform, [1] TLAS split levels (G-buffer stack bound),
                               // [2] emitters, [3] alias entries of a new instance set (launch_set_instances);
                               // [2] of a refit: the listed large nodes (DYN_REFIT_SMALL counts them)
};
void launch_dynamic_update(const DynamicArgs& D, hipStream_t st);
// launch_dynamic_update one launch at a time, for a caller that times each: RECORDS, TLAS_BUILD, EMISSIVE_AREAS,
// EMISSIVES, LBVH_BUILD, BACKFILL in this order are launch_dynamic_update.  The instance refit (hk_refit_instances;
// DESIGN §0 f13) is RECORDS, EMISSIVE_AREAS, EMISSIVES, REFIT_SMALL, REFIT_LARGE: both trees keep their topology and
// get the boxes of include/hk_refit.h's rule from the records before them, no build and no backfill.  A step with
// nothing to do (no emitters; no tree that can hold a large node) launches nothing.
enum DynamicStep {
    DYN_RECORDS, DYN_TLAS_BUILD, DYN_EMISSIVE_AREAS, DYN_EMISSIVES, DYN_LBVH_BUILD, DYN_BACKFILL, DYN_REFIT_SMALL,
    DYN_REFIT_LARGE
};
void launch_dynamic_step(const DynamicArgs& D, DynamicStep step, hipStream_t st);
// One tree of the instance refit: a bvh-0.7.1 flatten of 3 x shapes - 2 nodes over the records its leaves name
// (emitters 0: hk_instance, 1: hk_emissive).  RefitTrees: the kernels' table, by value; n_nodes over all trees.
struct RefitTree {
    hk_node* nodes;
    const void* records;
    uint32_t shapes, emitters;
};
struct RefitTrees {
    RefitTree tree[2];
    uint32_t n_trees, n_nodes;
};

// Tree costs (hk_tree_costs; include/hk_cost.h): one launch over the nodes of every listed tree laid end
// to end, as RefitTrees lays two.  CostSlice: one tree, a flatten of `count` >= 1 nodes that starts at node `first` of
// the launch (the running sum of the counts before it) and whose cost goes to out[slot]; every slice has a slot of its
// own.  out: zeroed on the stream before the launch; the kernel adds into it and stores each slot's root_half_area.
struct CostSlice {
    const hk_node* nodes;
    uint32_t count, first, slot, pad;
};
void launch_tree_cost(const CostSlice* table, uint32_t n_slices, uint32_t n_nodes, hk_tree_cost* out, hipStream_t st);

// A new instance set (hk_dynamic.hip): one record per instance, the layout of hk_instance_desc.
struct InstanceDesc {
    hk_mesh_index mesh;
    uint32_t material;
    uint32_t previous;  // index in the set before, or INSTANCE_NEW
};
constexpr uint32_t INSTANCE_NEW = 0xFFFFFFFFu;
struct SetArgs {
    const InstanceDesc* set;    // D.n_instances records
    const float* prev_models;   // the previous models of the set before: n_prev x 16
    uint32_t n_prev;
    // scratch
    float* new_prev;            // n x 16: the gathered previous models of the new set
    uint2* emitter;             // n x (1 if the instance's material emits, its mesh's primitives)
};
// The instance records written whole from D.models / D.local_aabbs and S.set, the emissive records compacted in
// instance order with their alias ranges (D.n_emissives and D.n_alias: the host's totals, the room in D.emissives and
// D.alias; the device's own go to D.flags[2], [3]), then everything launch_dynamic_update rebuilds after its records.
void launch_set_instances(const DynamicArgs& D, const SetArgs& S, hipStream_t st);

// Deforming meshes (hk_dynamic.hip): one record per listed mesh, in a device table.
struct MeshUpdate {
    uint32_t vertex, vertex_count;  // the mesh's slice of the vertex array
    uint32_t primitive, shapes;     // its slice of the primitive array (shapes = triangles)
    uint32_t node0;                 // its first asset node (3 x shapes - 2 of them)
    uint32_t vertex0;               // its first vertex in the uploaded positions / normals (list order)
    uint32_t shape0;                // its first shape box in the scratch; indices and segments at 2 x shape0
    uint32_t slot;                  // its place in the list: levels[slot]
    uint32_t has_normals;           // 0: the vertices keep their normals
};
struct MeshUpdateArgs {
    const MeshUpdate* table;          // n_meshes records in list order (vertex0 and shape0 ascend)
    const MeshUpdate* table_by_size;  // the same records, the n_lds of at most mesh_lds_shapes() triangles first
    uint32_t n_meshes, n_lds;
    uint32_t n_vertices, n_shapes;    // sums over the list
    const float* positions;           // n_vertices x 3
    const float* normals;             // n_vertices x 3 (read where has_normals)
    hk_vertex* vertices;
    hk_primitive* primitives;
    hk_node* blas;
    int buckets;
    // scratch
    void* shapes;                     // n_shapes x 24 B
    uint32_t* idx;                    // 2 x n_shapes
    void* segments;                   // 2 x n_shapes x 12 B
    uint32_t* levels;                 // n_meshes: split levels of each rebuilt BLAS (G-buffer stack bound)
    // scratch of a refit, which builds nothing: it lies where idx and levels do
    uint32_t* large;                  // 2 x n_shapes: the listed slices' large entry nodes (k_refit_small lists them)
    uint32_t* n_large;                // their number
    uint32_t large_bound;             // the sum of mesh_refit_large_bound over the list; 0: no slice can hold one
};
// vertex and primitive rewrite with the shape boxes (one launch), then the BLAS builds: one workgroup per mesh, one
// launch per instantiation of the build (LDS-staged / global)
void launch_mesh_update(const MeshUpdateArgs& M, hipStream_t st);
uint32_t mesh_lds_shapes();
// A refit (hk_refit_meshes / hk_skin_meshes_refit) in place of the builds, as three launches: the rewrite
// alone; one thread per node of the listed slices (the small entry nodes refit, the large ones listed); one workgroup
// per listed large node (nothing when large_bound is 0).  Only the min / max words of entry nodes are written.
void launch_mesh_geometry(const MeshUpdateArgs& M, hipStream_t st);
void launch_refit_small(const MeshUpdateArgs& M, hipStream_t st);
void launch_refit_large(const MeshUpdateArgs& M, hipStream_t st);
// how many large entry nodes a slice over `shapes` primitives can hold at the most
uint32_t mesh_refit_large_bound(uint32_t shapes);

// Skinned meshes (hk_skin_meshes, hk_dynamic.hip): beside each posed mesh's MeshUpdate record (vertex0:
// its place in the staged position / normal streams, which k_skin_vertices writes and launch_mesh_update then reads),
// where its bind pose lies in the context's resident skin streams and its palette in the uploaded ones.
struct SkinSource {
    uint32_t skin0;      // its first vertex in the resident streams
    uint32_t joint0;     // its first matrix in the uploaded palettes
    hk_mesh_index mesh;  // its slice, as its instances' records carry it (k_skin_bounds)
};
struct SkinArgs {
    const MeshUpdate* table;        // n_meshes records in list order
    const SkinSource* sources;      // beside them
    uint32_t n_meshes, n_vertices;  // n_vertices: the sum over the list
    const float* bind_positions;    // resident: x 3
    const float* bind_normals;      // resident: x 3 (read where MeshUpdate::has_normals)
    const uint2* joint_indices;     // resident: four u16 per vertex, one 8-byte load
    const float4* joint_weights;    // resident: one 16-byte load per vertex
    const float4* palettes;         // the uploaded joint matrices, four float4 columns each
    float* positions;               // the staged streams, n_vertices x 3
    float* normals;
};
// one thread per vertex of the posed meshes: the posed position and normal into the staged streams (one launch)
void launch_skin_vertices(const SkinArgs& K, hipStream_t st);
// The posed meshes' slices as k_skin_bounds reads them: the hk_mesh_index of mesh k lies `stride` bytes after that of
// mesh k - 1 (the `mesh` member of a table of SkinSource or of MorphSource records).
struct PosedSlices {
    const void* first;
    uint32_t stride;
};
// one workgroup per posed mesh: its Bevy Aabb from the staged positions (include/hk_skin.h's bounds rule), written over
// the rows of local_aabbs (n_instances x 6) whose instance record carries the mesh's slice (one launch)
void launch_posed_bounds(const MeshUpdate* table, PosedSlices slices, uint32_t n_meshes, const float* positions,
                         const hk_instance* instances, uint32_t n_instances, float* local_aabbs, hipStream_t st);
inline void launch_skin_bounds(const SkinArgs& K, const hk_instance* instances, uint32_t n_instances, float* local_aabbs,
                               hipStream_t st)
{
    launch_posed_bounds(K.table, PosedSlices{&K.sources->mesh, (uint32_t)sizeof(SkinSource)}, K.n_meshes, K.positions,
                        instances, n_instances, local_aabbs, st);
}

// Morph targets (hk_morph_meshes, hk_dynamic.hip): beside each posed mesh's MeshUpdate record, where its
// base and its deltas lie in the context's resident morph block, its range of the uploaded active list (the targets
// whose weight is not zero, ascending), and its skin and palette when the pose gives joints.
constexpr uint32_t MORPH_NONE = 0xFFFFFFFFu;
// The targets whose delta loads k_morph_vertices issues before the first add of a batch (the adds stay in list order).
// Tried on the device: see DESIGN §0 f15.
constexpr int MORPH_BATCH = 4;
struct MorphActive {
    uint32_t target;
    float weight;
};
struct MorphSource {
    uint32_t base0;         // its first vertex in the resident base streams
    uint32_t delta0;        // its first record in the resident position deltas: target t, vertex v at delta0 + t x V + v
    uint32_t normal_delta0; // the same in the normal deltas; MORPH_NONE: the base normals as they are
    uint32_t active0, active_count;  // its range of the active list
    uint32_t skin0;         // its first vertex in the resident skin streams; MORPH_NONE: morph only
    uint32_t joint0;        // its first matrix in the uploaded palettes
    hk_mesh_index mesh;     // its slice, as its instances' records carry it (k_skin_bounds)
};
struct MorphArgs {
    const MeshUpdate* table;        // n_meshes records in list order
    const MorphSource* sources;     // beside them
    const MorphActive* active;      // the uploaded active list
    uint32_t n_meshes, n_vertices;  // n_vertices: the sum over the list
    const float* base_positions;    // resident: x 3
    const float* base_normals;      // resident: x 3 (read where MeshUpdate::has_normals)
    const float* position_deltas;   // resident: x 3 per record
    const float* normal_deltas;
    const uint2* joint_indices;     // the resident skin streams (read where a source names a skin)
    const float4* joint_weights;
    const float4* palettes;
    float* positions;               // the staged streams, n_vertices x 3
    float* normals;
};
// one thread per vertex of the posed meshes: the morphed (and skinned) position and normal into the staged streams
void launch_morph_vertices(const MorphArgs& K, hipStream_t st);

// Appended meshes (hk_add_meshes, hk_dynamic.hip): beside each mesh's MeshUpdate record (its destination slices past
// the arrays' ends, vertex0 / shape0 its place in the staged streams; has_normals is not read), where its indices lie
// and how its triangles read them.
constexpr uint32_t MESH_NO_INDICES = 0xFFFFFFFFu;
struct MeshSource {
    uint32_t index0;  // its first index in the staged index stream; MESH_NO_INDICES: 0 .. vertex_count - 1
    uint32_t strip;   // 1: a TriangleStrip (triangle t: t, t + 1, t + 2, the first two swapped for odd t), 0: a list
};
struct MeshAddArgs {
    MeshUpdateArgs M;            // M.positions / M.normals: the staged streams, vertex_count x 3 per mesh
    const MeshSource* sources;   // M.n_meshes records in list order
    const float* uvs;            // n_vertices x 2
    const uint32_t* indices;     // the indexed meshes' indices, one after another
};
// vertex and primitive records written whole with the shape boxes (one launch), then launch_mesh_update's builds
void launch_mesh_add(const MeshAddArgs& A, hipStream_t st);

// A new mesh asset list (hk_set_meshes, hk_dynamic.hip k_move_mesh_slices): one record per list entry in list order,
// so every dst ascends and the entries tile the new arrays.  All in elements, not 16-byte chunks: 3 x 2^30 primitive
// chunks pass 32 bits, the kernel multiplies in 64.
constexpr uint32_t MESH_MOVE_NEW = 0xFFFFFFFFu;
struct MeshMove {
    uint32_t dst[3];    // its first vertex, primitive and node in the new arrays
    uint32_t src[3];    // a kept entry: the same in the current arrays; src[0] == MESH_MOVE_NEW: built by this call
    uint32_t count[3];  // its vertices, primitives and nodes
};
struct MeshMoveArgs {
    const MeshMove* table;
    uint32_t n_meshes;
    uint32_t n_vertices, n_prims, n_nodes;  // the new counts of arrays 0-2
    const void* src[3];                     // the current arrays 0-2
    void* dst[3];                           // the new ones: other buffers
    uint32_t* aux;                          // the per-node mesh tables, three rows of `stride` words
    size_t stride;
};
// the kept entries' bytes gathered into the new arrays and every entry's rows of the per-node mesh tables (one launch)
void launch_mesh_move(const MeshMoveArgs& V, hipStream_t st);

// Post-process (hk_post.hip over include/hk_post.h)
struct PostArgs {
    hk_pp_frame frame;
    hk_pp_inputs in;
};
void launch_smaa(const PostArgs& P, hipStream_t st);
void launch_smaa_extrapolate(const PostArgs& P, hipStream_t st);
void launch_taa(const PostArgs& P, hipStream_t st);

// FSR1 (hk_fsr.hip over include/hk_fsr.h): EASU reads `in` (RGBA16F at s) with `easu`, RCAS reads `in` (RGBA16F at S,
// EASU's output) with `rcas`; both write `out` at S
struct FsrArgs {
    hk_pp_tex in;
    hk_pp_out out;
    hk_fsr_easu_con easu;
    float rcas;
};
void launch_fsr_easu(const FsrArgs& A, bool tiled, hipStream_t st);
void launch_fsr_rcas(const FsrArgs& A, hipStream_t st);

// Present (hk_overlay.hip over include/hk_overlay.h): `in` and `albedo` (RGBA16F planes) drawn into the viewport of the
// target at `data` (row pitch in bytes).  run: the 16-byte row-run kernel where the viewport's runs are aligned, with
// the per-pixel kernel on each row's tail; otherwise the per-pixel kernel throughout.  col0 / cols: the launcher's.
struct OverlayArgs {
    hk_pp_tex in, albedo;
    uint8_t* data;
    uint32_t pitch;
    hk_overlay_view view;
    uint32_t col0, cols;  // the viewport columns one launch covers
};
void launch_overlay(const OverlayArgs& A, bool run, hipStream_t st);

bool lane_stats_take(unsigned long long out[2 * LANE_SLOTS], hipStream_t st);
void launch_gbuffer(const FrameArgs& A, const ViewArgs& V, uint2* albedo, uint32_t stack_need, hipStream_t st);
// keep (the light launches): the background tile skip's tiles, TILE_KEEP_ALL for none
void launch_direct_fused(const FrameArgs& A, const ChannelArgs& C0, const ChannelArgs& C1, hipStream_t st,
                         const TileKeep& keep = TILE_KEEP_ALL);
void launch_albedo(const FrameArgs& A, uint2* albedo, hipStream_t st);
void launch_direct(const FrameArgs& A, const ChannelArgs& C, bool emissive_lit, hipStream_t st,
                   const TileKeep& keep = TILE_KEEP_ALL);
void launch_indirect(const FrameArgs& A, const ChannelArgs& C, bool multi, hipStream_t st, const TileKeep& keep = TILE_KEEP_ALL);
// the indirect pass's pixel stash per workgroup (IndStash: static in k_indirect, behind the scene in k_light_merged)
uint32_t indirect_stash_bytes();
// the wavefront indirect pass (one bounce): gen + compaction, bounce trace, bin scan, scatter by
// material, material-sorted shade; W.ctl must be zeroed on `st` before
void launch_indirect_wavefront(const FrameArgs& A, const ChannelArgs& C, const WfArgs& W, hipStream_t st);
void launch_spatial(const FrameArgs& A, const ChannelArgs& C, bool emissive_lit, hipStream_t st);
// the direct-light passes stage the scene in LDS (option lds_scene = 2 with a small enough scene)
bool light_lds_direct(const FrameArgs& A);
// direct_lit + emissive (fused per pixel) and the one-bounce indirect pass in one launch (k_light_merged)
// (keep_direct / keep_indirect: per role)
void launch_light_merged(const FrameArgs& A, const ChannelArgs& C0, const ChannelArgs& C1, const ChannelArgs& C2,
                         hipStream_t st, const TileKeep& keep_direct = TILE_KEEP_ALL,
                         const TileKeep& keep_indirect = TILE_KEEP_ALL);
void launch_demod(const FrameArgs& A, const DenoiseArgs& D, hipStream_t st);
void launch_denoise(const FrameArgs& A, const DenoiseArgs& D, int level, hipStream_t st);
// rect: the launch restricted to plane columns [rect[0], rect[2]) and local rows [rect[1], rect[3]) of its window
// (hks_tone_rect; only where tone_run_px(A) != 0: the run kernel takes any aligned rectangle), nullptr: the window
void launch_tone(const FrameArgs& A, const ToneArgs& T, hipStream_t st, const int32_t* rect = nullptr);
// the pixels of a row one thread of launch_tone's kernel over A takes (TONE_RUN), 0 where the per-texel kernel runs
uint32_t tone_run_px(const FrameArgs& A);
void launch_collapse_leaves(hk_node* nodes, uint32_t n, const uint32_t* node_base, const uint32_t* node_count,
                            uint32_t* scratch, hipStream_t st);
void launch_fill_leaves(hk_node* blas, uint32_t n_blas, const uint32_t* prim_offset, const hk_primitive* prims,
                        hk_node* tlas, uint32_t n_tlas, const hk_instance* inst, uint32_t n_inst, hipStream_t st);
void launch_build_wide(const hk_node* flat, uint32_t n, const uint32_t* node_base, const uint32_t* node_count,
                       float4* wide, hipStream_t st);
void launch_accumulate(const uint2* tone, float4* acc, uint32_t n, int reset, hipStream_t st);
void launch_resolve(const float4* acc, uint32_t n, float count, uint2* out, hipStream_t st);
void launch_div_check(float d, float r, uint32_t lo, uint32_t hi, unsigned long long* bad, hipStream_t st);
void launch_rcp_check(uint32_t lo, uint32_t hi, unsigned long long* bad, hipStream_t st);
void launch_count_check(const uint32_t* values, uint32_t n, unsigned long long* sum, hipStream_t st);
void launch_f16(const float* in, uint32_t n, uint16_t* out, hipStream_t st);
// false: fn is no hk_math_fn (nothing launched)
bool launch_math(int fn, const uint32_t* a, const uint32_t* b, const float* rb, uint32_t n, uint32_t* out0,
                 uint32_t* out1, hipStream_t st);
void launch_texture_check(const Scene& sc, uint32_t id, const float* uv, uint32_t n, float* out, hipStream_t st);
void launch_trace(const Scene& sc, const float* rays, const float* max_d, const float* early_d, const uint32_t* excl,
                  uint32_t n, uint32_t* hits, unsigned long long* top, hipStream_t st);

}  // namespace hk
