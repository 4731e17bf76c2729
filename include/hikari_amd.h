/*
 * hikari_amd.h — C ABI of the MI355X-native bevy-hikari integrator (libhikari_amd.so).
 *
 * A Rust shim behind bevy-hikari's unchanged `HikariPlugin` / `HikariSettings` API binds
 * these symbols.  Each entry point replaces one piece of the
 * reference's render-world code:
 *
 *   hk_create / hk_destroy      one context per camera entity: owns what `ReservoirCache`
 *                               (light.rs:342-363), `LightTextures` (light.rs:297-383) and the
 *                               denoise part of `PostProcessTextures` (post_process.rs:622-747) own
 *   hk_scene_upload             the group-2 storage buffers written by
 *                               `MeshRenderAssets::set` (mesh.rs:43-58), `InstanceRenderAssets::set`
 *                               (instance.rs:82-99) and `MaterialRenderAssets` (material.rs:196-202)
 *   hk_texture_upload           the material textures of `MaterialTextures` (material.rs:54-127), bound
 *                               as group 3 `textures` / `samplers` (light.wgsl:15-19) when the
 *                               scene has textures (the reference's non-NO_TEXTURE pipeline)
 *   hk_set_noise                the 16 blue-noise textures of `NoiseTextures` (lib.rs:189-219)
 *   hk_resize                   `prepare_light_textures` reallocation (light.rs:307-383), which
 *                               zero-fills the 10 reservoir buffers (light.rs:353-360)
 *   hk_set_gbuffer              group-1 deferred textures produced by `PrepassNode` (prepass.rs:769-851)
 *   hk_render_gbuffer           primary-ray substitute for the raster prepass (prepass.wgsl:84-100)
 *   hk_render_frame             `LightNode::run` (light.rs:590-702): albedo, then per channel the
 *                               temporal pass and (if enabled) the spatial pass
 *   hk_denoise                  the denoise block of `PostProcessNode::run` (post_process.rs:1190-1224)
 *   hk_tone_sum                 the `tone_mapping` dispatch (post_process.rs:1226-1234)
 *   hk_present                  the `Overlay` phase item's draw into the view target (overlay.rs:290-395, overlay.wgsl)
 *   hk_get_output               reading `LightTextures` / `denoise_render` / tone-mapping output
 *   hk_trace                    stand-alone ray query over the TLAS/BLAS (light.wgsl:442-486)
 *
 * Conventions: every function returns 0 on success and a negative HK_ERR_* code on
 * failure; `hk_last_error` returns the message.  No exceptions cross the ABI.  A context
 * is externally synchronized (single-threaded, like one render-graph node).  `stream` is
 * a hipStream_t (NULL = the context's own stream); all GPU work is ordered on it and
 * the functions return without waiting, except hk_get_output(..., to_host=1) and
 * hk_read_counters.  Internally a frame's G-buffer and its tail (denoise, tone-sum) may run
 * on the context's own streams, overlapping the neighbouring frames' light passes; every
 * call that reads or changes their results first waits for them on `stream`
 * (hipStreamWaitEvent), so the observable order is the stream order.  A host-side
 * hipStreamSynchronize(stream) therefore does not cover them: use a readback call, or
 * hipDeviceSynchronize.
 */
#ifndef HIKARI_AMD_H
#define HIKARI_AMD_H

#include <stddef.h>
#include <stdint.h>
#include "hk_types.h"
#include "hk_texture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HK_ABI_VERSION 3

enum {
    HK_OK = 0,
    HK_ERR_INVALID = -1,   /* bad argument / shape */
    HK_ERR_HIP = -2,       /* HIP runtime failure */
    HK_ERR_STATE = -3,     /* called in the wrong order (e.g. render before upload) */
    HK_ERR_NO_DEVICE = -4, /* no gfx950 device */
};

typedef struct hk_ctx hk_ctx;

/* A {pointer, element count} array in a scene upload. */
typedef struct hk_array {
    const void* data;
    uint32_t count;
} hk_array;

/*
 * Scene buffers in group-2 binding order (mesh_material_bindings.wgsl:5-22).  The node
 * arrays carry their element count here (the WGSL `Nodes.count` header word).  The data is
 * COPIED: the caller keeps ownership.  A new upload replaces the whole scene.
 */
typedef struct hk_scene_desc {
    hk_array vertices;       /* hk_vertex,      binding 0 */
    hk_array primitives;     /* hk_primitive,   binding 1 */
    hk_array asset_nodes;    /* hk_node,        binding 2 */
    hk_array alias_table;    /* hk_alias_entry, binding 3 */
    hk_array instances;      /* hk_instance,    binding 4 */
    hk_array instance_nodes; /* hk_node,        binding 5 */
    hk_array materials;      /* hk_material,    binding 6 */
    hk_array emissive_nodes; /* hk_node,        binding 7 */
    hk_array emissives;      /* hk_emissive,    binding 8 */
} hk_scene_desc;

/*
 * Field-for-field mirror of `HikariSettings` (lib.rs:400-433); defaults in
 * hk_settings_default() follow lib.rs:435-455.
 */
typedef struct hk_settings {
    uint32_t direct_validate_interval;
    uint32_t emissive_validate_interval;
    uint32_t max_temporal_reuse_count;
    uint32_t max_spatial_reuse_count;
    float max_reservoir_lifetime;
    float solar_angle;
    uint32_t indirect_bounces;
    float max_indirect_luminance;
    float clear_color[4]; /* linear RGBA */
    uint32_t temporal_reuse;
    uint32_t emissive_spatial_reuse;
    uint32_t indirect_spatial_reuse;
    uint32_t denoise;
    uint32_t taa;           /* 0 = Jasmine, 1 = None (hk_post_process) */
    float upscale_ratio;    /* Upscale::ratio(), clamped to [1, 2] (lib.rs:501-505) */
    uint32_t upscale;       /* 0 = SmaaTu4x (default), 1 = Fsr1: hk_post_process runs EASU + RCAS after the TAA, with the
                               sharpness of hk_set_fsr1_sharpness (Upscale::Fsr1::sharpness is not in this record) */
} hk_settings;

/* The parts of Bevy's `View` uniform the integrator reads (light.wgsl:714-727). */
typedef struct hk_view {
    float world_position[3];
    float _pad0;
    float view_proj[16];         /* column-major */
    float inverse_view_proj[16]; /* column-major, used by hk_render_gbuffer for ray generation */
    float projection[16];        /* column-major; projection[3].w == 1 => orthographic: the light passes take the
                                    orthographic view vector normalize(view_proj[0].z, [1].z, [2].z), and
                                    hk_render_gbuffer starts each primary ray at the unprojection of
                                    (ndc_x, ndc_y, 1), the near plane, and runs it along the negated view vector
                                    (otherwise: from world_position through that point) */
} hk_view;

/* The parts of Bevy's `Lights` uniform the integrator reads (light.wgsl:611,832,847,855). */
typedef struct hk_lights {
    float directional_color[4];     /* lights.directional_lights[0].color */
    float direction_to_light[3];    /* lights.directional_lights[0].direction_to_light */
    float _pad0;
    float ambient_color[4];         /* lights.ambient_color */
} hk_lights;

/* Prepass sub-pixel jitter (prepass.wgsl:30-38,52-54): the shader defs the prepass pipeline gets from
 * HikariSettings (prepass.rs:194-199) */
enum {
    HK_JITTER_NONE = 0, /* taa = None: no jitter */
    HK_JITTER_TAA = 1,  /* TEMPORAL_ANTI_ALIASING: halton index = frame_number & 15 */
    HK_JITTER_TAA_SMAA = 2, /* TEMPORAL_ANTI_ALIASING + SMAA_TU4X: index = (frame_number >> 1) & 15 */
};

/* Per-frame inputs: FrameUniform.number (view.rs:141-192) + view + lights, and the previous frame's
 * view (`PreviousViewUniform`, view.rs:31-73: projection * inverse(GlobalTransformQueue[1])) that the
 * prepass's motion vectors read (prepass.wgsl:96).  A zero-initialised tail (jitter 0,
 * has_previous_view 0) means no jitter and a static camera (previous view = this view). */
typedef struct hk_frame_inputs {
    uint32_t frame_number;
    uint32_t jitter;            /* HK_JITTER_*: hk_render_gbuffer's primary-ray jitter */
    uint32_t has_previous_view; /* 0: previous_view_proj is ignored and taken equal to view.view_proj */
    uint32_t _pad;
    hk_view view;
    hk_lights lights;
    float previous_view_proj[16]; /* column-major */
} hk_frame_inputs;

/* Output planes readable with hk_get_output. Sizes are per pixel of the plane's extent. */
typedef enum hk_output_id {
    HK_OUT_ALBEDO = 0,            /* RGBA16F, S (physical size)      */
    HK_OUT_VARIANCE_DIRECT = 1,   /* R32F, s                           */
    HK_OUT_VARIANCE_EMISSIVE = 2,
    HK_OUT_VARIANCE_INDIRECT = 3,
    HK_OUT_RENDER_DIRECT = 4,     /* RGBA16F, s                        */
    HK_OUT_RENDER_EMISSIVE = 5,
    HK_OUT_RENDER_INDIRECT = 6,
    HK_OUT_DENOISED_DIRECT = 7,   /* RGBA16F, s                        */
    HK_OUT_DENOISED_EMISSIVE = 8,
    HK_OUT_DENOISED_INDIRECT = 9,
    HK_OUT_TONE_MAPPED = 10,      /* RGBA16F, s                        */
    HK_OUT_GBUF_POSITION = 11,    /* float4, S */
    HK_OUT_GBUF_NORMAL = 12,      /* uint32 snorm8x4, S */
    HK_OUT_GBUF_DEPTH_GRADIENT = 13, /* float2, S */
    HK_OUT_GBUF_INSTANCE_MATERIAL = 14, /* float2, S */
    HK_OUT_GBUF_VELOCITY_UV = 15, /* float4, S */
    HK_OUT_DENOISE_INTERNAL_VARIANCE = 16, /* R32F, s (last channel denoised) */
    HK_OUT_ACCUMULATED = 17,      /* RGBA16F, s: hk_resolve_accumulation */
    HK_OUT_UPSCALED = 18,         /* RGBA16F, ceil(S * 2 / ratio): SMAA TU4x output (upscale_output[0]) */
    HK_OUT_TAA = 19,              /* RGBA16F: TAA Jasmine output of this frame (taa_output[head]) */
    HK_OUT_TONE_MAPPED_PREVIOUS = 20, /* RGBA16F, s: the previous frame's tone-mapped output (tone_mapping_output
                                       * [1 - head]), intact until this frame's successor's tone-sum */
    HK_OUT_FSR_EASU = 21,         /* RGBA16F, S: FSR1 EASU output (upscale_output[0] under Upscale::Fsr1) */
    HK_OUT_FSR_RCAS = 22,         /* RGBA16F, S: FSR1 RCAS output (upscale_output[1]): the frame the overlay presents */
    HK_OUT_COUNT = 23
} hk_output_id;

/* Reservoir buffer ids 0..9 as allocated by light.rs:350-361; the channel pairs
 * (temporal, spatial) are (0,4), (2,4), (6,8) + frame parity (light.rs:518-546). */
#define HK_RESERVOIR_BUFFERS 10

/* Per-frame device counters (ray queries issued; Mrays/s numerator). */
typedef struct hk_counters {
    uint64_t traverse_top;      /* traverse_top calls (light.wgsl:442) */
    uint64_t traverse_emitter;  /* emitter traverse_bottom calls in select_light_candidate (light.wgsl:687) */
    uint64_t primary;           /* primary rays of hk_render_gbuffer: one per pixel per frame */
    uint64_t primary_reused;    /* of those, the rays of frames whose planes were reused (option gbuffer_reuse), not traced */
} hk_counters;

/* ---- lifetime ---- */
int hk_abi_version(void);
/* Tuned configuration: the context creates its streams in a fixed order (caller
 * stream, two side streams — one carries no work, it only shifts the next ones — G-buffer stream,
 * tail stream), and HIP maps streams round-robin onto the process's hardware queues.  The defaults of
 * hk_set_option were measured with HIP's default GPU_MAX_HW_QUEUES=4; more queues let every stream
 * run concurrently and measured slower (cornell 1080p 0.58 -> 0.70 ms/frame). */
int hk_create(int device, hk_ctx** out_ctx);
void hk_destroy(hk_ctx* ctx);
const char* hk_last_error(const hk_ctx* ctx);
void hk_settings_default(hk_settings* out);

/* Runtime options of a context (no reference counterpart: the reference has one schedule).  Every
 * option chooses among schedules or kernel variants that produce the same bits, so results never
 * depend on them; the defaults are the measured-fastest configuration.  Nothing is read from the
 * environment.  Keys (default):
 *   pipeline_min_px (1.2e6)  frame pipelining from this many integrator pixels up
 *   pipeline_heavy_min_px (0)  ... and from this many up on frames with spatial reuse or the denoiser
 *   gbuffer_pipeline (1)     frame f's G-buffer on its own stream next to frame f-1's light passes
 *   tail_pipeline (1)        frame f's denoise / tone-sum / accumulation next to frame f+1's light passes
 *   channel_streams (1)      the indirect chain on a side stream next to direct -> emissive
 *   fuse (1), fuse_min_px (2^20)  direct_lit + emissive in one launch (identity reprojection only)
 *   merge (-1)               direct + indirect in one launch: -1 small unpipelined frames, 0 never, 1 always
 *   bg_elision (1)           skip background stores whose targets already hold their constant words
 *   spatial_view_planes (1)  the indirect temporal pass writes spatial reuse's neighbour view planes
 *   band_full_windows (0)    a band runs every pass on all its rows (no per-pass row windows)
 *   leaf_collapse (1)        leaf-collapsed node copies for the light walks (applied at the next upload)
 *   gbuffer_reuse (1)        skip the G-buffer trace when its slot already holds this frame's planes
 *                            (static camera, jitter and instances: the sub-frames of an accumulation)
 *   lds_scene (1)            0 no LDS scene staging, 1 where measured faster, 2 every traversal kernel
 *   gbuffer_stack_full (0), gbuffer_deep (0), gbuffer_lds_max_px (6e5: scene + stack in LDS on smaller
 *   frames), direct_w4_min_px (4e5), fused_w4 (1),
 *   persistent_indirect (0)  kernel-variant choices (tests force each variant with them)
 *   compact_emitter (0)      the fused direct/emissive launch runs a workgroup's emitter BLAS walks as one
 *                            compacted batch (long walks first) on frames without emissive validation
 *   compact_shadow (0)       shadow walks of a workgroup as one compacted batch (fused launch, indirect pass)
 *                            (both measured slower than the per-pixel walks: DESIGN §4)
 *   fsr_tiled (1)            FSR1 EASU with each workgroup's input footprint staged in LDS as f32 (0: every tap from
 *                            global memory); tests force both variants with it
 *   present_run (1)        hk_present stores 16-byte row runs (4 texels, RGBA16F 2) where the viewport's first texel
 *                            and the pitch are 16-byte aligned, each row's tail per texel (0: every texel on its own);
 *                            tests force both variants with it
 *   shared_xform (1)         in a scene whose instances all carry one bit-identical transform
 *                            (hk_scene_shared_transform) a walk computes its instance-local ray once instead of at
 *                            every instance it enters; 0: always the general walk
 *   bg_tile_skip (1)         workgroups of k_gbuffer and of the light passes whose 16x16 tile lies outside the scene's
 *                            screen bound (hikari_scene.h hks_screen_bounds, from the instances' world box), and whose
 *                            targets already hold a background pixel's constants (the bg_elision masks' history),
 *                            return at their first instruction, and hk_tone_sum runs over the pixel rectangle that
 *                            can hold anything but the clear colour; 0: every workgroup runs (hk_tile_skip_info,
 *                            hk_tone_skip_info)
 * hk_set_option returns HK_ERR_INVALID for an unknown key, a value outside the key's range, or a fractional value
 * for any key but the pixel-count thresholds (*_px). */
int hk_set_option(hk_ctx* ctx, const char* key, double value);
int hk_get_option(const hk_ctx* ctx, const char* key, double* value);
/* key of option `index` (0, 1, ...; NULL past the last one) */
const char* hk_option_name(int index);

/* ---- resources ---- */
int hk_scene_upload(hk_ctx* ctx, const hk_scene_desc* scene);
int hk_set_noise(hk_ctx* ctx, const uint8_t* rgba8, uint32_t count, uint32_t size);

/* Dynamic instances: `prepare_instances` (instance.rs:284-437) re-run ON THE GPU when
 * transforms change — instance records (world AABB from the 8 transformed corners of the local AABB,
 * inverse-transpose model), the TLAS (bvh 0.7.1 binned SAH, 6 buckets, rebuilt, not refitted),
 * emissive records with their alias tables, and the light BVH; bit-identical to a host rebuild
 * (hikari_scene.h hks_build) with the same transforms.  models: count x 16 floats
 * (GlobalTransform::compute_matrix, column-major); local_aabbs: count x 6 floats (the entity's
 * Bevy `Aabb`: center xyz, half_extents xyz).  count must equal the uploaded instance count
 * (same order, meshes and materials).  Waits for the stream once (singular-matrix check). */
int hk_update_instances(hk_ctx* ctx, const float* models, const float* local_aabbs, uint32_t count, void* stream);

/* Deforming meshes: what the reference does for `AssetEvent::Modified` (mesh.rs:77-166
 * extract_mesh_assets / prepare_mesh_assets run GpuMesh::try_from again, mod.rs:379-467: vertices, primitives and a
 * fresh bvh 0.7.1 BLAS; prepare_instances, instance.rs:284-437, then runs on the new mesh slices), ON THE GPU and in
 * place, for meshes whose topology is unchanged (another triangle or vertex count: hk_set_meshes, below, with the mesh
 * as a new entry at its position): the primitives keep their stored vertex indices and the uvs stay.
 * For each listed mesh the device rewrites hk_vertex.position and hk_vertex.normal of the slice (normals NULL: the
 * uploaded normals stay), the three positions of each hk_primitive from the new vertices, and rebuilds the mesh's
 * BLAS with the host builder's exact operations (hikari_scene.h hks_build: 6 buckets, node indices relative to the
 * mesh; a subtree of k shapes is 3k - 2 nodes, so the node slice stays).  The triangles' shape boxes are folded from
 * empty in vertex order 0, 1, 2 with the host's std::fmin / std::fmax, so a zero bound keeps the sign the host
 * leaves.  The device-only derivatives of the asset nodes (leaf boxes, the G-buffer wide layout, the light walks'
 * copy with its leaf collapse) are refreshed, and the G-buffer walk's stack bound becomes the TLAS depth plus the
 * deepest instanced BLAS as rebuilt (a mesh that got shallower lowers it).  Then hk_update_instances' rebuild runs:
 * instance records, TLAS, emissive areas, alias tables, emissive records and the light BVH; models and local_aabbs
 * cover every instance in upload order exactly as there.  The reference reads the entity's `Aabb` component
 * (instance.rs:193-206, 287-293), which Bevy 0.9 does not recompute when a mesh is modified: the caller supplies
 * it, the library does not derive it.  Motion vectors keep their rule (current geometry against the previous
 * models: prepass.wgsl has no previous-vertex input).  The result is bit-identical to hks_build + hk_scene_upload
 * of the deformed scene.
 * HK_ERR_INVALID with a message, the context unchanged and usable: a null pointer; count other than the instance
 * count; a `mesh` that is not the slice of an instanced mesh of the uploaded scene; a slice whose node count is not
 * 3k - 2 over k primitives of the scene; vertex_count not greater than every vertex index its primitives store, or
 * reaching past the vertex array or into another instanced mesh's vertices; a mesh listed twice.  HK_ERR_STATE
 * without a scene.  A singular model fails as in hk_update_instances (after the meshes were rebuilt).  Waits for the
 * stream once. */
typedef struct hk_mesh_update {
    hk_mesh_index mesh;     /* the slice as the instances of this mesh carry it (vertex, primitive, node[2]) */
    uint32_t vertex_count;
    const float* positions; /* vertex_count x 3 */
    const float* normals;   /* vertex_count x 3; NULL keeps the uploaded normals */
} hk_mesh_update;
int hk_update_meshes(hk_ctx* ctx, const hk_mesh_update* meshes, uint32_t mesh_count, const float* models,
                     const float* local_aabbs, uint32_t count, void* stream);

/* A new instance set: what the reference's prepare_instances (instance.rs:245-444) does with
 * InstanceEvent::Created / Modified / Removed (instance.rs:123-175), with the visibility filter and with changed
 * materials (material.rs AssetEvent::Modified), ON THE GPU and in place: entities spawned, despawned or hidden, an
 * instance given another material, an emissive colour going to or from zero.  After hk_set_instances the scene is what
 * hks_build + hk_scene_upload give for the same meshes and materials in the same order and THIS instance list in this
 * order (the reference's order is its BTreeMap's entity order; the caller supplies it, as at upload): the alias
 * table, the instances, the TLAS, the light BVH and the emissives (arrays 3, 4, 5, 7, 8) are bit-identical to that
 * host build, the emissive list re-derived from `intensity > 0` in instance order; arrays 0-2 are untouched; the
 * materials (array 6) are replaced only when `materials` is given: all of the uploaded material count.  models and
 * local_aabbs: `count` records as in hk_update_instances.  The G-buffer walk's stack bound becomes the rebuilt
 * TLAS's levels plus the deepest BLAS among the slices the new set instances (it can fall).  Waits for the stream
 * once.  hk_update_instances and hk_update_meshes afterwards take the current set: its count and order, and any
 * slice instanced or registered so far.
 *   previous: the motion vectors' previous model (transform.rs:8-44 GlobalTransformQueue) of instance i is the one
 * the last G-buffer saw for entity set[i].previous of the set before this call, or the instance's own current model
 * for HK_INSTANCE_NEW.
 *   mesh: a slice instanced at upload is taken as it is.  Any other slice of the uploaded vertex / primitive /
 * asset-node arrays (hks_build concatenates every added mesh, instanced or not) is registered on first use: it
 * must be node[1] == 3k - 2 nodes over k primitives inside the primitive array, its node range inside the asset
 * nodes, its stored vertex indices inside the vertex array, and identical to or disjoint from every slice known so
 * far.
 *   Capacity: the five arrays, the TLAS derivatives, the previous models and the scratch keep a capacity beside
 * their count; a call allocates only for a count above its capacity, and then max(count, 1.5 x capacity); nothing
 * shrinks before hk_scene_upload or hk_destroy.  Every allocation the call needs is made before anything changes: on
 * HK_ERR_HIP "out of device memory" the context is as it was.  A set without an emitter is legal (empty alias table,
 * light BVH and emissives).  An EMPTY set is not: hk_scene_upload refuses an empty scene too.
 *   HK_ERR_INVALID with a message, decided before any device work, the context unchanged and usable: a null set,
 * models or local_aabbs; count == 0; a material index >= the material count; a slice that fails the checks above; a
 * previous that is neither HK_INSTANCE_NEW nor below the count before, or used twice.  HK_ERR_STATE without a scene
 * or on a scene whose BVHs are not 3n - 2 flattened.  A singular model fails after the rebuild as in
 * hk_update_instances; the set is then the new one and a following valid call repairs it.  HK_ERR_HIP if the
 * device's emitter or alias totals differ from the host's (hk_instance_set_counts). */
#define HK_INSTANCE_NEW 0xFFFFFFFFu
typedef struct hk_instance_desc {
    hk_mesh_index mesh;   /* a mesh slice of the uploaded vertex / primitive / asset-node arrays */
    uint32_t material;    /* < uploaded material count */
    uint32_t previous;    /* this entity's index in the set before the call, or HK_INSTANCE_NEW */
} hk_instance_desc;
int hk_set_instances(hk_ctx* ctx, const hk_instance_desc* set, const float* models, const float* local_aabbs,
                     uint32_t count, const hk_material* materials, void* stream);
/* the current element counts of the nine scene arrays, hk_scene_desc order */
int hk_scene_counts(const hk_ctx* ctx, uint32_t counts[9]);

/* Appended meshes: what the reference does for `AssetEvent::Created` (mesh.rs:77-166
 * prepare_mesh_assets runs GpuMesh::try_from on a mesh asset that arrives after the scene was uploaded, as under
 * asynchronous glTF loading, and concatenates it behind the others, mesh.rs:140-163), ON THE GPU and in place.  After
 * hk_add_meshes the vertices, primitives and asset nodes (arrays 0, 1, 2) are what hks_build + hk_scene_upload give
 * when the same meshes are added with hks_add_mesh, in this order, after the meshes already there (the reference's
 * order is its BTreeMap's; the caller supplies it, as at upload).  Every earlier slice keeps its bytes and offsets
 * (node indices are mesh-relative); arrays 3-8, the instance set and the picture are untouched.  The device writes each
 * hk_vertex and hk_primitive whole from the attribute streams, folds the triangles' shape boxes with the host's
 * std::fmin / std::fmax and builds each BLAS with the host builder's exact operations (as hk_update_meshes).
 * slices[k]: mesh k's appended slice; a mesh of k triangles takes 3k - 2 nodes.  Each new mesh is a known slice at
 * once, carried by no instance: hk_set_instances spawns it and hk_update_meshes deforms it like any other, its leaves
 * carry their triangle boxes and it has its entries in the device-only derivatives, which are refreshed over the
 * whole array.  The G-buffer walk's stack bound does not move until an instance carries the mesh.  Waits for the
 * stream once (the BLAS depths).
 *   Capacity: arrays 0-2 and their device-only derivatives keep a capacity beside their count (hk_scene_capacity); a
 * call allocates only for a count above its capacity, and then max(count, 1.5 x capacity), the contents kept.  Nothing
 * shrinks before hk_scene_upload or hk_destroy, which reset them.  hk_add_meshes only appends: a mesh no instance carries
 * keeps its bytes until hk_set_meshes (below) leaves it out of its list, or the next hk_scene_upload.
 *   HK_ERR_INVALID with a message naming hks_add_mesh's error, decided on the host before any device work, the context
 * unchanged and usable: a null list or null `slices`; mesh_count == 0; positions / normals / uvs missing
 * (MissingAttributePosition / MissingAttributeNormal / MissingAttributeUV); an index >= vertex_count; a topology
 * that is neither, or a list whose index count is no multiple of 3 (IncompatiblePrimitiveTopology); fewer than 3
 * indices (NoPrimitive); totals past 0x40000000 vertices, primitives or nodes.  HK_ERR_STATE without a scene.
 *   HK_ERR_HIP "out of device memory": every allocation the call needs is made before anything changes, so the
 * context is as it was.  Any other HK_ERR_HIP (a copy, launch or wait that failed after that): the counts and the
 * known slices have not moved, they change together after the wait, but the arrays' contents are undefined; the
 * context is then good for hk_scene_upload and hk_destroy only. */
typedef struct hk_mesh_desc {      /* a Bevy `Mesh` as hks_add_mesh takes it */
    const float* positions;       /* vertex_count x 3 */
    const float* normals;         /* vertex_count x 3 */
    const float* uvs;             /* vertex_count x 2 */
    uint32_t vertex_count;
    const uint32_t* indices;      /* NULL: 0 .. vertex_count-1 */
    uint32_t index_count;         /* ignored when indices is NULL */
    uint32_t topology;            /* HKS_TRIANGLE_LIST (0) / HKS_TRIANGLE_STRIP (1), hikari_scene.h */
} hk_mesh_desc;
int hk_add_meshes(hk_ctx* ctx, const hk_mesh_desc* meshes, uint32_t mesh_count, hk_mesh_index* slices, void* stream);
/* The host arithmetic hk_add_meshes sizes its allocations and launches with (needs no device or context): the slices
 * of `meshes` appended to arrays of `before` elements and the nine counts after (only [0..2] change).  The same
 * refusals with the same codes as hk_add_meshes; their message is what hk_add_meshes_counts_error() returns on the
 * calling thread until its next hk_add_meshes_counts (an empty string after a success).  `after` may be NULL. */
int hk_add_meshes_counts(const uint32_t before[9], const hk_mesh_desc* meshes, uint32_t mesh_count,
                         hk_mesh_index* slices, uint32_t after[9]);
const char* hk_add_meshes_counts_error(void);

/* A new mesh asset list: what the reference does when mesh assets are removed (`AssetEvent::Removed`,
 * mesh.rs:89-92, 123-126), modified with another triangle or vertex count, or created with a handle that sorts ahead
 * of others: prepare_mesh_assets rebuilds the three buffers from its BTreeMap<Handle<Mesh>, GpuMesh> in key order
 * (mesh.rs:140-163), a new GpuMesh from GpuMesh::try_from (mod.rs:379-467).  hk_set_meshes does that ON THE GPU, and
 * the instance set with it: the counterpart of hk_set_instances for arrays 0, 1, 2.  After the call the scene is, byte
 * for byte, what hks_build + hk_scene_upload give when the meshes of `list` are added with hks_add_mesh in list order
 * (a kept entry standing for the mesh that produced its slice) and the instances of `set` in theirs: all nine arrays
 * and their counts.
 *   list[k]: source != NULL: a new mesh, assembled and its BLAS built as by hk_add_meshes.  source == NULL: the slice
 * `keep` of the current arrays is kept: its vertex_count vertices (the registry knows only the largest index its
 * primitives store; the host builder concatenates all of a mesh's vertices, unreferenced trailing ones too, so the
 * count is the caller's, as hk_mesh_update's), its primitives and its nodes move verbatim, node and vertex indices
 * being mesh-relative.  A kept slice is a known slice, or one that passes hk_set_instances' checks of a slice no
 * instance has carried and is registered by this call.  A slice that is not listed is gone.  A mesh replaced by one
 * of another topology is a new entry at the old one's position, the old slice not listed.
 *   slices[k]: entry k's slice in the new layout, by the running sums of vertices, primitives and 3k - 2 nodes.
 * set[i].mesh names a slice of the NEW layout (hk_set_meshes_counts gives them beforehand); previous, materials,
 * models and local_aabbs are hk_set_instances': an instance of a replaced mesh carries its old index as `previous`
 * and keeps its motion vectors.  After the call the known slices are exactly the list's, so every leaf of arrays 2
 * carries its triangle's box and hk_update_meshes deforms any of them.  Waits for the stream twice (the BLAS depths,
 * then hk_set_instances' wait).
 *   Capacity: counts 0-2 may fall, the capacities (hk_scene_capacity) never do before hk_scene_upload / hk_destroy.
 * The move is out of place, since a reorder lets source and destination ranges overlap in any way: the context keeps
 * one spare buffer per array 0-2, of at least the array's capacity from the first call on; a call writes the new
 * arrays into the spares, zeroes their tails behind the new counts, and swaps.  A call allocates where a count passes
 * its capacity (max(count, 1.5 x capacity)) or a spare is smaller than the capacity needed, so a steady cycle of
 * removals and additions allocates nothing from its second call on.  The device-only derivatives are rewritten whole.
 *   HK_ERR_INVALID with a message, decided on the host before any device work, the context unchanged and usable: a
 * null list, null `slices`, mesh_count == 0; for a new entry every refusal of hk_add_meshes, in its words ("mesh k:
 * MissingAttributeNormal" ...); a kept slice that fails hk_set_instances' slice checks ("kept slice refused: ...");
 * a kept vertex_count below what its primitives index, reaching past the vertex array or into another kept slice's
 * vertices; a slice kept twice; totals past 0x40000000; every refusal of hk_set_instances for the set, against the
 * new layout, and an instance whose mesh is none of slices[]: "its mesh is not in the new list".  HK_ERR_STATE
 * without a scene.  HK_ERR_HIP "out of device memory" from the allocations for arrays 0-2 and their derivatives, all
 * made first: the context is as it was (the set's own arrays grow as in hk_set_instances).  Any later HK_ERR_HIP: as
 * documented for hk_add_meshes.  A singular model fails after the rebuild, as in hk_set_instances. */
typedef struct hk_mesh_entry {
    const hk_mesh_desc* source;  /* non-NULL: a new mesh */
    hk_mesh_index keep;          /* source == NULL: a slice of the current arrays 0-2, kept */
    uint32_t vertex_count;       /* source == NULL: the kept mesh's vertex count */
} hk_mesh_entry;
int hk_set_meshes(hk_ctx* ctx, const hk_mesh_entry* list, uint32_t mesh_count, hk_mesh_index* slices,
                  const hk_instance_desc* set, const float* models, const float* local_aabbs, uint32_t count,
                  const hk_material* materials, void* stream);
/* The host arithmetic of the list (needs no device or context): entry k's slice in the new layout and the nine counts
 * after (only [0..2] change: [3..8] follow the set, hk_instance_set_counts).  With no context a kept slice is checked
 * against `before` and the other kept slices alone; the other refusals of the list are hk_set_meshes', with its codes.
 * The message is what hk_set_meshes_counts_error() returns on the calling thread until its next hk_set_meshes_counts
 * (an empty string after a success).  `after` may be NULL. */
int hk_set_meshes_counts(const uint32_t before[9], const hk_mesh_entry* list, uint32_t mesh_count,
                         hk_mesh_index* slices, uint32_t after[9]);
const char* hk_set_meshes_counts_error(void);

/* Skinned meshes.  The reference does not skin (its README leaves "Skinned animation" unticked); a
 * Bevy scene does, in the mesh vertex shader (bevy_pbr skinning.wgsl, recalled: include/hk_skin.h states the rule and
 * pins its evaluation order).  A path tracer needs the posed vertices in its vertex and primitive arrays and a BLAS
 * over them, so posing is hk_update_meshes with a device source: the bind pose and the rig are resident, a pose costs
 * the host one joint palette (64 bytes per joint) and one call.
 *
 * hk_set_mesh_skins replaces the context's WHOLE skin set (n == 0 drops it): for each listed mesh the bind pose, joint
 * indices and joint weights are copied into device memory the context owns, as separate streams (12-byte positions and
 * normals, one 8-byte load of the four indices, one 16-byte load of the weights per vertex).  The streams keep a
 * capacity beside their size: re-registering as many vertices or fewer allocates nothing.  Every check is made on the
 * host before any device work, and a refusal leaves the context, its former skin set included, as it was.  It renders
 * nothing and changes no scene array.  The set is dropped by hk_scene_upload and hk_set_meshes (slices move) and kept
 * by hk_add_meshes, hk_set_instances and the updates.  Waits for the stream once.
 * HK_ERR_INVALID with a message: a null list with n != 0, a null positions, joint_indices or joint_weights; `mesh` and
 * vertex_count failing hk_update_meshes' checks (not a known slice; a BLAS that is not 3k - 2 nodes; vertex_count not
 * covering the stored vertex indices, or reaching past the vertex slice); joint_count outside 1 .. 65536; a joint
 * index >= joint_count; a mesh listed twice.  HK_ERR_STATE without a scene. */
typedef struct hk_mesh_skin {
    hk_mesh_index mesh;            /* a known slice (instanced, registered, or appended by hk_add_meshes) */
    uint32_t vertex_count;         /* as hk_mesh_update's */
    const float* positions;        /* bind pose, vertex_count x 3 */
    const float* normals;          /* bind pose; NULL: the array's normals stay as they are */
    const uint16_t* joint_indices; /* vertex_count x 4 */
    const float* joint_weights;    /* vertex_count x 4 */
    uint32_t joint_count;          /* every index < joint_count; 1 .. 65536 */
} hk_mesh_skin;
int hk_set_mesh_skins(hk_ctx* ctx, const hk_mesh_skin* skins, uint32_t n, void* stream);

/* hk_skin_meshes poses the listed meshes ON THE GPU and rebuilds what depends on them.  joints: joint_count column-major
 * 4 x 4 matrices (joint global transform x inverse bind pose, Bevy's SkinnedMeshUniform).  One thread per vertex writes
 * the posed position and normal (hk_skin.h; the normal NOT normalised) where hk_update_meshes stages the host's, and
 * from there the call IS hk_update_meshes: vertices, primitives, the BLAS by the host builder's exact operations, the
 * device-only derivatives, the stack bound, then the instance rebuild with models and local_aabbs as in
 * hk_update_instances.  The library derives each posed mesh's Bevy `Aabb` from the posed vertices itself (as
 * hks_add_mesh folds a mesh's; hikari_scene.h hks_skin_vertices gives the same six floats) and uses it for every
 * instance of that mesh: the caller's local_aabbs rows of those instances are ignored (they must still be readable),
 * the rows of all other instances are used.  After the call all nine arrays are byte for byte what hks_build +
 * hk_scene_upload give for the scene whose posed meshes hold hks_skin_vertices' output; meshes not posed in this call
 * keep their bytes (a mesh posed earlier stays posed).  The bound behind bg_tile_skip stays unknown until the next
 * instance update or upload, as after hk_update_meshes.  Motion vectors keep their rule (current geometry against the
 * previous models; Bevy 0.9 has no previous-pose input either).  Waits for the stream once.  n == 0 is
 * hk_update_instances.
 * HK_ERR_INVALID with a message, the context unchanged and usable: a null pointer (poses with n != 0, a pose's joints,
 * models, local_aabbs); count other than the instance count; a pose for a mesh with no registered skin; joint_count
 * other than the skin's; a mesh posed twice; a mesh whose BLAS is not 3k - 2 nodes or whose slice no longer holds
 * its vertex_count (hk_update_meshes' checks, made again).  HK_ERR_STATE without a scene.  A singular model fails after
 * the rebuild, as in hk_update_instances. */
typedef struct hk_skin_pose {
    hk_mesh_index mesh;
    const float* joints;
    uint32_t joint_count;
} hk_skin_pose;
int hk_skin_meshes(hk_ctx* ctx, const hk_skin_pose* poses, uint32_t n, const float* models, const float* local_aabbs,
                   uint32_t count, void* stream);

/* BLAS refit: hk_update_meshes and hk_skin_meshes with the BLAS of each listed mesh REFIT, not rebuilt.
 * A refit keeps the tree the slice holds (every entry_index and exit_index, so the node count, the leaf order and
 * the depth) and recomputes the box of every entry node from the deformed primitives, by the rule of
 * include/hk_refit.h: the hk_minf / hk_maxf fold of the shape boxes of the leaves stored in the node's range.  The
 * reference has no such path (it rebuilds, mesh.rs:77-166); the rule is this library's own.  It costs a scan of the
 * slice spread over the whole device instead of a SAH build by one workgroup per mesh.
 * QUALITY DEGRADES WITH THE DEFORMATION: the tree was chosen for the vertices it was built over.  Boxes stay tight around
 * their leaves, but leaves that moved apart make sibling boxes overlap, and a tree refit far from the pose it was built
 * for walks more nodes per ray.  It stays correct: every ray finds the hits a rebuilt tree finds, up to the order in
 * which equal hits are met.  The caller decides when that matters and then calls hk_update_meshes / hk_skin_meshes on
 * the same mesh, which rebuild from the current vertices and give the host builder's tree again; the library has no
 * policy of its own, and hk_tree_costs (below) is the quality query to decide with.
 * Arguments, refusals, messages (with the function's own name in front) and states are those of hk_update_meshes and
 * hk_skin_meshes; a refusal leaves the context unchanged; mesh_count == 0 / n == 0 is hk_update_instances.  Afterwards
 * all nine arrays are what hks_build + hk_scene_upload give for the deformed scene, except that each listed mesh's
 * slice of the asset nodes is the slice before the call passed through hikari_scene.h hks_refit_nodes with the mesh's
 * new primitives (leaves carry their triangle's box on the device, as always).  The G-buffer stack bound does not move.
 * Waits for the stream once. */
int hk_refit_meshes(hk_ctx* ctx, const hk_mesh_update* meshes, uint32_t mesh_count, const float* models,
                    const float* local_aabbs, uint32_t count, void* stream);
int hk_skin_meshes_refit(hk_ctx* ctx, const hk_skin_pose* poses, uint32_t n, const float* models,
                         const float* local_aabbs, uint32_t count, void* stream);

/* Instance refit: hk_update_instances with the TLAS and the light BVH REFIT, not rebuilt.  Both trees
 * keep every entry_index and exit_index, so every node_index in the instance and emissive records stays too, and each
 * entry node's box becomes the fold of include/hk_refit.h's rule over the shape boxes of the leaves in its range: an
 * instance's world box for the TLAS, an emitter's sphere box (position -+ radius) for the light BVH.  The reference has
 * no such path (it rebuilds, instance.rs:284-437); the rule is this library's own.  The records, alias tables and
 * emitters are computed as by hk_update_instances; the two one-workgroup SAH builds and the node_index backfill are
 * replaced by one launch over all nodes of both trees and at most one more over their large nodes.
 * QUALITY DEGRADES WITH THE MOTION, as for a BLAS refit: boxes stay tight around their leaves, but instances that moved
 * apart make sibling boxes overlap, and a tree refit far from where it was built costs more to walk.  It stays correct.
 * The caller decides when that matters and then calls hk_update_instances (or any rebuilding call), which builds both
 * trees from the current boxes and gives the host builder's trees again; the library has no policy, and hk_tree_costs
 * (below) is the quality query to decide with.  A refit cannot follow a changed set: hk_set_instances and hk_set_meshes
 * always rebuild.
 * Arguments, refusals, messages (with the function's own name in front) and states are hk_update_instances': previous
 * models for the motion vectors, the shared-transform and scene-box state, the singular-transform refusal.  Afterwards
 * all nine arrays are what hks_build + hk_scene_upload give for the scene with the new models, except that the
 * instance nodes and the emissive nodes are those before the call passed through hikari_scene.h hks_refit_boxes with
 * the new instance and emitter boxes, and every node_index is the one before the call.  The G-buffer stack bound does
 * not move.  A steady refit allocates nothing.  Waits for the stream once.
 * hk_refit_meshes_all / hk_skin_meshes_refit_all: hk_refit_meshes / hk_skin_meshes_refit with the two instance trees
 * refit as well, so that no tree is built in the call. */
int hk_refit_instances(hk_ctx* ctx, const float* models, const float* local_aabbs, uint32_t count, void* stream);
int hk_refit_meshes_all(hk_ctx* ctx, const hk_mesh_update* meshes, uint32_t mesh_count, const float* models,
                        const float* local_aabbs, uint32_t count, void* stream);
int hk_skin_meshes_refit_all(hk_ctx* ctx, const hk_skin_pose* poses, uint32_t n, const float* models,
                             const float* local_aabbs, uint32_t count, void* stream);

/* Morph targets.  The other way glTF animates geometry: blend shapes, usually a face under a skeleton.
 * The reference does not morph and Bevy 0.9 has no morph targets; include/hk_morph.h states the rule (glTF 2.0's sum and
 * Bevy 0.11's morph.wgsl, both recalled) and pins its evaluation order: per component acc = base, then
 * acc = acc + w[t] * d[t] in f32, never contracted, for t ascending over the targets with w[t] != 0; normals by the same
 * fold, not normalised; under a skin the morphed position and normal are what hk_skin.h's matrix is applied to.  The
 * base and the deltas are resident on the device; a pose costs the host one weight vector (and a joint palette when
 * the mesh is also skinned) and one call.
 *
 * hk_set_mesh_morphs replaces the context's WHOLE morph set (n == 0 drops it): for each listed mesh the base positions,
 * base normals (NULL: the array's normals stay as they are) and the TARGET-MAJOR deltas (target_count x vertex_count x
 * 3 floats; normal_deltas NULL: a pose copies the base normals) are copied into ONE device block the context owns:
 * 12 B per vertex of base positions, 12 B of base normals, and 12 B (24 B with normal deltas) per vertex per target.
 * The block keeps a capacity beside its size: re-registering as many bytes or fewer allocates nothing; a failed
 * allocation leaves the former set in place.  Every check is made on the host before any device work, and a refusal
 * leaves the context, its former morph set included, as it was.  It renders nothing and changes no scene array.  The
 * set is independent of the skin set; it is dropped by hk_scene_upload and hk_set_meshes (slices move) and kept by
 * hk_add_meshes, hk_set_instances and the updates.  Waits for the stream once.
 * HK_ERR_INVALID with a message: a null list with n != 0; a null positions or position_deltas; normal_deltas without
 * normals; target_count outside 1 .. HK_MORPH_MAX_TARGETS; `mesh` and vertex_count failing hk_set_mesh_skins' checks
 * (not a known slice; a BLAS that is not 3k - 2 nodes; vertex_count not covering the stored vertex indices, or reaching
 * past the vertex slice); a mesh listed twice; more than 0x40000000 vertices, or target_count x vertex_count records,
 * in the set.  HK_ERR_STATE without a scene. */
#ifndef HK_MORPH_MAX_TARGETS
#define HK_MORPH_MAX_TARGETS 256u
#endif
typedef struct hk_mesh_morph {
    hk_mesh_index mesh;           /* a known slice (instanced, registered, or appended by hk_add_meshes) */
    uint32_t vertex_count;        /* as hk_mesh_update's */
    const float* positions;       /* base, vertex_count x 3 */
    const float* normals;         /* base; NULL: the array's normals stay as they are */
    uint32_t target_count;        /* 1 .. HK_MORPH_MAX_TARGETS */
    const float* position_deltas; /* target_count x vertex_count x 3, target-major */
    const float* normal_deltas;   /* the same shape; NULL: no normal deltas (needs normals otherwise) */
} hk_mesh_morph;
int hk_set_mesh_morphs(hk_ctx* ctx, const hk_mesh_morph* morphs, uint32_t n, void* stream);

/* hk_morph_meshes morphs the listed meshes ON THE GPU and rebuilds what depends on them, as hk_skin_meshes does for a
 * skin: one thread per vertex folds the deltas of the targets whose weight is not zero (the host compacts them into a
 * list, in ascending target order) over the resident base, applies the registered skin's matrix where the pose gives
 * joints (hk_set_mesh_skins' indices and weights; the base is the MORPH set's: the skin's bind positions and normals
 * are not read), and writes the position and normal where hk_update_meshes stages the host's.  From there the call IS
 * hk_update_meshes, with each posed mesh's Bevy `Aabb` derived on the device for every instance of that mesh: the
 * caller's local_aabbs rows of those instances are ignored (they must still be readable).  After the call all nine
 * arrays are byte for byte what hks_build + hk_scene_upload give for the scene whose posed meshes hold
 * hks_morph_vertices' output, passed through hks_skin_vertices with the registered skin's indices and weights where
 * joints are given; meshes not posed in this call keep their bytes.  hk_morph_meshes_refit / _refit_all: the same with
 * each posed BLAS refit (hk_refit_meshes' contract) / the TLAS and the light BVH refit as well (hk_refit_meshes_all's).
 * States, waits and the treatment of n == 0 (hk_update_instances / hk_refit_instances for _refit_all) are
 * hk_skin_meshes' and its refits'.
 * HK_ERR_INVALID with a message, the context unchanged and usable: a null pointer (poses with n != 0, a pose's weights,
 * models, local_aabbs); count other than the instance count; a pose for a mesh with no registered morph; target_count
 * other than the registered one; joints for a mesh with no registered skin; joint_count other than the skin's; a skin
 * and a morph that disagree on whether normals are rewritten (one registered with normals, the other without), or on
 * the vertex_count; a mesh posed twice; hk_update_meshes' checks, made again.  HK_ERR_STATE without a scene. */
typedef struct hk_morph_pose {
    hk_mesh_index mesh;
    const float* weights;  /* target_count floats */
    uint32_t target_count; /* the registered morph's */
    const float* joints;   /* NULL: morph only; else joint_count column-major 4 x 4 matrices, as hk_skin_pose's */
    uint32_t joint_count;  /* the registered skin's (ignored without joints) */
} hk_morph_pose;
int hk_morph_meshes(hk_ctx* ctx, const hk_morph_pose* poses, uint32_t n, const float* models, const float* local_aabbs,
                    uint32_t count, void* stream);
int hk_morph_meshes_refit(hk_ctx* ctx, const hk_morph_pose* poses, uint32_t n, const float* models,
                          const float* local_aabbs, uint32_t count, void* stream);
int hk_morph_meshes_refit_all(hk_ctx* ctx, const hk_morph_pose* poses, uint32_t n, const float* models,
                              const float* local_aabbs, uint32_t count, void* stream);

/* Tree costs: how expensive the resident trees are to walk, by the rule of include/hk_cost.h, computed ON
 * THE GPU from the nodes as they stand: what a caller that refits (hk_refit_instances, hk_refit_meshes, the _all calls)
 * decides a rebuild with.  The reference has no such query (it never refits); the rule is this library's own.
 *   hk_tree_cost: over the entry nodes of one flattened tree, each weighted by q = its box's half area over the root's,
 *   as a 32.32 fixed-point number: `leaf` sums q over the entry nodes above one leaf (the expected shape tests of a ray
 *   that meets the root box, x 2^32), `inner` over the others (the expected further box tests); `entries` counts them and
 *   root_half_area is the divisor.  A tree of one shape has no entry node: every field is 0.  The library fixes no SAH
 *   constants: (c_box x inner + c_shape x leaf) / 2^32 with the caller's.  Only the RATIO of two trees over the same
 *   shapes means anything (a refit tree against the same tree at its last build, or against a rebuilt one).
 * tlas / lights: the cost of the TLAS / the light BVH (zeros for a scene without emitters).  meshes[j]: the cost of the
 * BLAS of mesh mesh_ids[j], an index into the context's known slices in the order they became known: at hk_scene_upload
 * the distinct slices in the order in which the instances first carry them, then each slice as hk_set_instances
 * registered or hk_add_meshes appended it; after hk_set_meshes its list's order.  Ids may repeat and come in any order.
 * Any out pointer may be NULL: that tree is not computed.  One launch serves every listed tree; the sums are integer
 * adds, so every field is bit-reproducible and equals hikari_scene.h hks_tree_cost on the same nodes.
 * The call READS the scene and writes only scratch of its own: all nine arrays, the picture, the histories and the
 * G-buffer stack bound are untouched, and the frames that follow are bit-identical to frames without it.  The scratch
 * keeps a capacity beside its size: a steady query allocates nothing.  Waits for the stream once.
 * HK_ERR_INVALID with a message that names hk_tree_costs, the context unchanged: mesh_ids NULL with mesh_count != 0; an
 * id at or past the number of known slices.  HK_ERR_STATE without a scene. */
typedef struct hk_tree_cost {
    uint64_t inner;
    uint64_t leaf;
    float root_half_area;
    uint32_t entries;
} hk_tree_cost; /* 24 bytes */
int hk_tree_costs(hk_ctx* ctx, const uint32_t* mesh_ids, uint32_t mesh_count, hk_tree_cost* tlas, hk_tree_cost* lights,
                  hk_tree_cost* meshes, void* stream);

/* the element capacities beside hk_scene_counts' counts, hk_scene_desc order: what each array holds before a call
 * has to allocate (hk_set_instances: 3, 4, 5, 7, 8; hk_add_meshes: 0, 1, 2; array 6 never grows).  HK_ERR_STATE
 * without a scene. */
int hk_scene_capacity(const hk_ctx* ctx, uint32_t capacity[9]);
/* *shared = 1 when every instance of the current scene carries the same transform, bit for bit (hikari_scene.h
 * hks_shared_transform over the records' inverse_transpose_model at hk_scene_upload, over the models given to
 * hk_update_instances / hk_update_meshes / hk_set_instances after them), 0 otherwise.  It does not depend on option
 * shared_xform, which decides whether the walks use it.  HK_ERR_STATE without a scene. */
int hk_scene_shared_transform(const hk_ctx* ctx, int32_t* shared);
/* Background tile skip (option bg_tile_skip) of the last frame: skipped[0..2] = the workgroups that returned at once in
 * its hk_render_gbuffer launch, in hk_render_frame's direct / emissive launch(es) (per launch) and in its indirect
 * launch (0 where nothing was skipped: the option off, bg_elision off, no screen bound, a mask whose history does not
 * reach back far enough yet, a pass whose background pixels still store).  bound: the pixel rectangle [x0, y0, x1, y1)
 * of the current G-buffer's screen bound, *bounded = 1; the whole frame and 0 while there is none (host planes, the
 * eye inside the scene's box, after hk_update_meshes).  Any out pointer may be NULL.  HK_ERR_STATE before hk_resize. */
int hk_tile_skip_info(const hk_ctx* ctx, uint32_t skipped[3], int32_t bound[4], int32_t* bounded);
/* The last hk_tone_sum's launch under the same option: it runs over the pixel rectangle that can hold anything but the
 * clear colour's texel (the join of the rectangles outside which the frame's render planes hold a background pixel's
 * zero texels, as the light launches' elision masks say, and the one outside which the output slot already holds that
 * clear colour's texel from its own earlier launches), its columns outward to the kernel's pixel runs
 * (hikari_scene.h hks_tone_rect).  *skipped_pixels: the pixels of its window it left out; 0 where it ran over the whole
 * window (the option or bg_elision off, no screen bound, a slot or a render plane the host cannot vouch for: the first
 * launches after hk_resize*, another clear colour, another window, a ratio other than 1, host G-buffer planes; the
 * denoiser on; interleaved stripes; an odd plane width).  rect: the frame rectangle [x0, y0, x1, y1) it ran over, all
 * zeros when nothing was launched (every texel already held the clear colour).  Either out pointer may be NULL.
 * HK_ERR_STATE before hk_resize. */
int hk_tone_skip_info(const hk_ctx* ctx, uint64_t* skipped_pixels, int32_t rect[4]);
/* The host arithmetic hk_set_instances sizes its allocations and launches with (needs no device or context): the
 * nine counts after `set` replaces the instances of the host-built `uploaded` scene: the instances, 3n - 2 TLAS
 * nodes, the emitters (255 * emissive[3] * |emissive.rgb| > 0 in float, so a NaN does not emit; `materials`, if
 * given, instead of the uploaded ones), the alias entries (the emitters' primitives) and 3m - 2 light-BVH nodes.
 * `previous` is not read.  HK_ERR_INVALID: count == 0, a material index out of range, a slice that fails
 * hk_set_instances' checks. */
int hk_instance_set_counts(const hk_scene_desc* uploaded, const hk_instance_desc* set, uint32_t count,
                           const hk_material* materials, uint32_t counts[9]);
/* LDS staging of a scene, computed on the host with the launchers' own arithmetic (needs no device or context):
 * the bytes the traversal kernels of `plan` (0: the light passes' arrays, hk_scene_desc's nine; 1: the G-buffer
 * walk's vertices, primitives, instances and the two wide node layouts) copy into LDS, each array rounded up to
 * 16 bytes, and the limit up to which a scene is staged at all (option lds_scene).  bytes <= limit: staged. */
int hk_scene_stage_bytes(const hk_scene_desc* scene, int plan, uint32_t* bytes, uint32_t* limit);
/* The indirect pass's LDS per workgroup for a scene under the default staging (host arithmetic, no device): the
 * bytes of its per-pixel stash (68 per thread), stash plus staged scene (the stash alone for a scene past the
 * staging limit), and what one workgroup may allocate.  total <= limit for every scene. */
int hk_scene_indirect_lds(const hk_scene_desc* scene, uint32_t* stash, uint32_t* total, uint32_t* limit);
/* The G-buffer walk's stack bound for a scene as hk_scene_upload computes it (inner levels of the TLAS plus those
 * of the deepest instanced BLAS) and the levels the shallow walk can keep in LDS: need <= lds_levels takes the
 * shallow kernel, whose stack follows a staged scene only while bytes + need * 2048 <= limit + 16384. */
int hk_scene_gbuffer_stack(const hk_scene_desc* scene, uint32_t* need, uint32_t* lds_levels);
/* copy group-2 scene array `array` (0..8, hk_scene_desc order) back from the device (test/debug) */
int hk_read_scene_array(hk_ctx* ctx, int array, void* dst, size_t bytes);

/* Post-process after tone mapping (post_process.rs:1236-1276): SMAA TU4x temporal 2x upsampling
 * (smaa.wgsl `smaa_tu4x` + `smaa_tu4x_extrapolate`, when settings->upscale == 0) then TAA Jasmine
 * (taa.wgsl, when settings->taa == 0).  Reads the previous frame's tone-mapped output and G-buffer
 * position / velocity planes (the reference's ping-pong textures, prepass.rs:309-317, head =
 * frame_number % 2).  With settings->upscale == 1 (Upscale::Fsr1) the TAA runs at s and FSR1 follows
 * (post_process.rs:1279-1308; include/hk_fsr.h): EASU upscales the TAA output (the tone-mapped plane when the
 * TAA is off) from s to S into HK_OUT_FSR_EASU, RCAS sharpens that into HK_OUT_FSR_RCAS, the displayed frame.
 * Both planes are allocated by the first such call (until then they have no hk_output_info).  Whole-frame
 * contexts only. */
int hk_post_process(hk_ctx* ctx, const hk_settings* settings, const hk_frame_inputs* inputs, void* stream);
/* Upscale::Fsr1::sharpness of the context (lib.rs:478-513): stops of sharpness reduction, 0 (the default) = maximum
 * sharpness; RCAS scales its lobe by exp2(-sharpness).  Not clamped, as the reference does not; a non-finite value
 * returns HK_ERR_INVALID.  Takes effect at the next hk_post_process. */
int hk_set_fsr1_sharpness(hk_ctx* ctx, float sharpness);

/* Present: the reference's last stage, the `Overlay` phase item's draw (overlay.rs, overlay.wgsl; include/hk_overlay.h
 * states every step).  The displayed plane is drawn through the linear sampler into the camera's viewport of a view
 * target: Rgba8UnormSrgb / Bgra8UnormSrgb, or Rgba16Float under HDR, which also undoes tone_mapping.wgsl's Reinhard
 * curve (overlay.rs:111-116).  A texel whose sample holds a NaN takes the albedo's sample instead (HK_OUT_ALBEDO, at S).
 * Texels outside the viewport are not written.
 * input -1 chooses the plane as overlay.rs:227-231 does from `settings`: Fsr1 -> HK_OUT_FSR_RCAS, SmaaTu4x with
 * Taa::None -> HK_OUT_UPSCALED, SmaaTu4x with Jasmine -> HK_OUT_TAA; another RGBA16F HK_OUT_* id shows that plane
 * (debug views; `settings` may then be NULL).
 * Errors: HK_ERR_STATE when the input plane does not exist yet (no hk_post_process that produces it) or the context
 * is a band; HK_ERR_INVALID for an unknown format, an input that is not RGBA16F, a zero dimension, a viewport outside
 * the target, a pitch below a row or not a multiple of the texel size, `data` not aligned to the texel size, or a
 * pitch with data == NULL (the context's plane has packed rows).  A failed call launches nothing.
 * Ordering: like hk_post_process, the call runs on `stream` after the frame's G-buffer and tail (device-side waits),
 * and the following hk_render_gbuffer calls wait for it before they overwrite the albedo slot it reads; a
 * caller-owned target is the caller's to order: it is written on `stream`, in stream order. */
enum { HK_PRESENT_RGBA8_SRGB = 0, HK_PRESENT_BGRA8_SRGB = 1, HK_PRESENT_RGBA16F = 2 };
typedef struct hk_present_target {
    void*    data;            /* device memory; NULL: the context's own present plane */
    uint32_t width, height;   /* texels of the whole target */
    uint32_t pitch;           /* bytes per row; 0 = width * bytes per texel */
    uint32_t format;          /* HK_PRESENT_* */
    uint32_t vp_x, vp_y, vp_w, vp_h;  /* camera.viewport; vp_w == 0: the whole target */
    int32_t  input;           /* -1: overlay.rs:227-231's choice; else an RGBA16F HK_OUT_* id */
} hk_present_target;
int hk_present(hk_ctx* ctx, const hk_settings* settings, const hk_present_target* target, void* stream);
/* The context's own present plane (hk_present with data == NULL): allocated by the first such call, reallocated when
 * the size or the format changes, released by hk_resize; both return HK_ERR_STATE before it exists.  It is
 * deliberately not an HK_OUT_* id: its texel size and format follow the last call.  hk_get_present copies all of it
 * (bytes = width * height * bytes per texel, rows packed) on `stream`, in stream order after the hk_present that
 * wrote it; to_host != 0 waits for the copy. */
int hk_present_info(const hk_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* bytes_per_texel, uint32_t* format);
int hk_get_present(hk_ctx* ctx, void* dst, size_t bytes, int to_host, void* stream);

/* Sub-frame accumulation (N integrator sub-frames per displayed frame, each
 * exactly one reference frame): hk_accumulate adds the current tone-mapped output (HK_OUT_TONE_MAPPED)
 * to an f32 RGBA accumulator, restarting it when reset != 0; hk_resolve_accumulation writes
 * accumulator / count (RGBA16F) to HK_OUT_ACCUMULATED, the plane a displayed frame all-gathers. */
int hk_accumulate(hk_ctx* ctx, int reset, void* stream);
int hk_resolve_accumulation(hk_ctx* ctx, void* stream);

/* Material textures: hk_material.*_texture ids index this array (material.rs:78-86, U32_MAX =
 * none).  Each entry is a Bevy `GpuImage` level 0 (RGBA8, row-major, `width * height * 4`
 * bytes; base colour / emissive images are sRGB, metallic-roughness / occlusion linear) with its
 * `ImageSampler` (address mode per axis, magnification filter).  Sampling is defined in
 * include/hk_texture.h.  Copies the texels; re-upload replaces; count 0 removes all. */
typedef struct hk_texture {
    uint32_t width, height;
    uint32_t format;               /* HK_TEXTURE_RGBA8_SRGB / HK_TEXTURE_RGBA8_UNORM */
    uint32_t address_u, address_v; /* HK_ADDRESS_CLAMP_TO_EDGE / _REPEAT / _MIRROR_REPEAT */
    uint32_t filter;               /* HK_FILTER_NEAREST / HK_FILTER_LINEAR */
    const uint8_t* rgba8;
} hk_texture;
int hk_texture_upload(hk_ctx* ctx, const hk_texture* textures, uint32_t count);
/* physical size S = (width, height); integrator size s = ceil(S / ratio) (light.rs:318-319).
 * band_y0/band_rows select a horizontal band of the frame (multi-GPU); (0, height) = whole frame. */
int hk_resize(hk_ctx* ctx, uint32_t width, uint32_t height, float upscale_ratio,
              uint32_t band_y0, uint32_t band_rows);

/* Interleaved-stripe decomposition for N GPUs (no reference counterpart: the reference renders
 * on one device).  The context holds the 8-row stripes rank, rank + world, rank + 2 world, ... of a
 * width x height frame (upscale ratio 1.0), so every rank gets an equal share of every screen
 * region: balanced work where contiguous bands are not (cornell: the box fills the middle rows).
 * Only for frames without neighbour reads — spatial reuse and the denoiser return HK_ERR_STATE in
 * this mode; those use contiguous bands + halo (hk_resize with band rows).  Local row l holds
 * global row (l / 8 * world + rank) * 8 + l % 8; hk_band_info reports row0 = 0, rows = core_rows
 * = the local row count.  world == 1 is hk_resize of the whole frame. */
int hk_resize_striped(hk_ctx* ctx, uint32_t width, uint32_t height, uint32_t rank, uint32_t world);
/* rows of halo recomputed above and below a band by hk_resize (default 40, enough for spatial
 * reuse + 4 a-trous levels + the variance blur: 20 + 15 + 1); 0 is exact when spatial reuse and
 * denoise are both off.  Call before hk_resize. */
int hk_set_band_halo(hk_ctx* ctx, uint32_t rows);
/* 2-D tile decomposition for N GPUs (no reference counterpart; north_star: "frames tile-partition across the 8
 * GPUs"): the context renders the frame's columns [x0, x0 + cols) of rows [y0, y0 + rows) plus a halo of
 * hk_set_band_halo pixels on every side (upscale ratio 1.0).  The planes hold the band's rows (rows + halo) at full
 * width; every pass runs only on the columns and rows the later passes read (core +- its reach), so the core
 * rectangle is bit-identical to a whole-frame render for a static camera.  Each channel runs on its widest window
 * from the first frame, so settings changes need no refill (hk_band_window_grow lists nothing).  Ray counters count
 * the core rectangle only. */
int hk_resize_tile(hk_ctx* ctx, uint32_t width, uint32_t height, uint32_t x0, uint32_t cols, uint32_t y0,
                   uint32_t rows);
/* a tile's own columns (global); 0 and the frame width for row bands and whole frames */
int hk_tile_info(const hk_ctx* ctx, int32_t* col0, int32_t* cols);
/* band geometry after hk_resize: local rows [0, rows) hold global rows [row0, row0+rows);
 * the band's own (non-halo) rows are local [core_row0, core_row0+core_rows) */
int hk_band_info(const hk_ctx* ctx, int32_t* row0, int32_t* rows, int32_t* core_row0, int32_t* core_rows);
/* Band window refill (no reference counterpart: the reference renders one whole frame, whose temporal passes run
 * on every pixel whatever the spatial flags, light.rs:656-699).  A band runs each channel's light passes on its
 * core rows +- the margin `settings` needs (that channel's spatial range plus the denoiser's reach); a setting turned
 * on later widens the margin for good, and the rows it takes in hold records this band never computed.  Their
 * owner (the band whose core rows they are) holds them exactly.  For the next hk_render_frame with `settings`,
 * ranges[4 k + 0..3] = (frame row, rows) above the core and (frame row, rows) below it of reservoir buffer k's
 * records to take from the owners (rows 0 = none), k = 0..HK_RESERVOIR_BUFFERS-1; returns how many buffers need
 * any (< 0: error).  commit != 0 then widens the margins as hk_render_frame would, without zero-filling: call it
 * after loading the rows (hk_reservoir_rows).  Without a committed refill hk_render_frame zero-fills the new rows
 * (as hk_resize does, light.rs:355-358).  Call between frames: after the last frame's hk_render_frame (and this
 * frame's hk_render_gbuffer), on every band of the frame. */
int hk_band_window_grow(hk_ctx* ctx, const hk_settings* settings, int32_t* ranges, int commit);
/* The records of frame rows [frame_row0, frame_row0 + rows) of reservoir buffer `id`, which must lie in this
 * context's band: out of the context (store = 0) into `data`, or from `data` into it (store = 1).  `data` is host
 * memory or a device pointer of any device of the process, in the row-exchange layout: 4 x rows x width chunks of
 * 16 bytes (the context's four record chunks, each a plane of rows x width), the layout the same call of another
 * band's context reads and writes.  Ordered after the frame work queued so far; blocking. */
int hk_reservoir_rows(hk_ctx* ctx, int id, int32_t frame_row0, int32_t rows, void* data, int store, void* stream);

/* ---- per frame ---- */
/* Primary-ray G-buffer (prepass.wgsl:84-100).  Pixel (x, y) traces the ray through
 * (x + 0.5 - jx, y + 0.5 - jy), j = the frame's halton jitter in pixels (inputs->jitter), and writes
 * velocity = clip_to_uv(view_proj * model * p) - clip_to_uv(previous_view_proj * previous_model * p)
 * for the hit's object-space point p (prepass.wgsl:49-50,96).  previous_model is the instance's model
 * as of the previous hk_render_gbuffer call (GlobalTransformQueue, transform.rs:32-44; after
 * hk_scene_upload: the uploaded model), so instances moved by hk_update_instances get motion vectors
 * for one frame. */
int hk_render_gbuffer(hk_ctx* ctx, const hk_frame_inputs* inputs, void* stream);
/* plane: 0..4 = position, normal, depth_gradient, instance_material, velocity_uv
 * (full S-sized planes, or the band's rows); device_ptr != 0 => data is a device pointer */
int hk_set_gbuffer_plane(hk_ctx* ctx, int plane, const void* data, size_t bytes, int device_ptr,
                         void* stream);
int hk_render_frame(hk_ctx* ctx, const hk_settings* settings, const hk_frame_inputs* inputs,
                    void* stream);
int hk_denoise(hk_ctx* ctx, const hk_settings* settings, const hk_frame_inputs* inputs, void* stream);
int hk_tone_sum(hk_ctx* ctx, const hk_settings* settings, void* stream);

/* ---- readback / state ---- */
int hk_output_info(const hk_ctx* ctx, int output_id, uint32_t* width, uint32_t* height,
                   uint32_t* bytes_per_pixel);
/* rows [row0, row0+rows) of the plane (rows = 0 => all) */
int hk_get_output(hk_ctx* ctx, int output_id, void* dst, size_t bytes, int to_host, void* stream);
/* Device address of an output plane for zero-copy readers.  The planes of the G-buffer, render /
 * variance targets and albedo alternate between two slots from frame to frame, so the address is
 * valid for the current frame only; work on `stream` sees the plane's final contents after
 * hk_sync(ctx, stream) (the frame's G-buffer and tail may still run on the context's own streams).
 * The planes are read-only for the caller: the light passes skip background stores whose targets
 * already hold their constant words (background store elision), which a foreign write would break;
 * planes and reservoirs are written through hk_set_gbuffer_plane / hk_load_reservoirs only.
 * hk_present follows the same rule from the inside: it reads the albedo and its input plane on `stream` after the
 * context's own streams (the waits of hk_sync), and the next hk_render_gbuffer waits for it. */
const void* hk_output_device_ptr(hk_ctx* ctx, int output_id);
/* Make `stream` wait (device-side) for all work the context queued on its own streams. */
int hk_sync(hk_ctx* ctx, void* stream);
/* Integrator layout of the indirect pass (light.wgsl:1263-1498, one bounce): 0 = one thread per
 * pixel (default); 1 = wavefront with material-sorted shading (BASELINE configs[4]): live pixels
 * compacted into a queue, the bounce walk writes SoA hit records, the queue is grouped by the hit's
 * material and the shading / NEE / shadow / temporal tail runs in that order.  Same results. */
int hk_set_wavefront(hk_ctx* ctx, int enable);
/* copy band-local rows [row0, row0+rows) of an output plane (e.g. the band's core rows for the
 * multi-GPU all-gather); dst is host (to_host=1) or device memory.  On a stream other than the one
 * the frame sequence runs on (e.g. a communication stream), the copy waits only for the work that
 * produced the plane, device-side, and the context's next write of that plane waits for the copy: the
 * frame stream itself never waits for the copy or for what follows it on `stream`. */
int hk_copy_output_rows(hk_ctx* ctx, int output_id, uint32_t row0, uint32_t rows, void* dst, int to_host,
                        void* stream);
/* the same for the rectangle of band-local rows [row0, row0+rows) x columns [col0, col0+cols) (a tile's core rows and
 * columns), written with row pitch dst_pitch bytes (0: cols x bytes per pixel, packed) */
int hk_copy_output_rect(hk_ctx* ctx, int output_id, uint32_t row0, uint32_t rows, uint32_t col0, uint32_t cols,
                        void* dst, size_t dst_pitch, int to_host, void* stream);
/* copy reservoir buffer `id` (0..9) in the reference's AoS PackedReservoir layout */
int hk_dump_reservoirs(hk_ctx* ctx, int id, hk_packed_reservoir* dst, size_t count, void* stream);
int hk_load_reservoirs(hk_ctx* ctx, int id, const hk_packed_reservoir* src, size_t count, void* stream);
int hk_reset_counters(hk_ctx* ctx, void* stream);
int hk_read_counters(hk_ctx* ctx, hk_counters* out, void* stream);
/* mean duration (ms) of each kernel of the last hk_render_frame/hk_denoise call, if timing is enabled */
int hk_enable_kernel_timing(hk_ctx* ctx, int enable);
int hk_kernel_timing(hk_ctx* ctx, const char** names, float* ms, int capacity);
/* traverse_top lane statistics per kernel name since hk_create, in builds compiled with
 * -DHK_LANE_STATS (experiments; the product build returns 0 entries): per walk iteration the wave's
 * active lanes, so active / (64 x iterations) is the walk's SIMD lane efficiency */
int hk_lane_stats(hk_ctx* ctx, const char** names, unsigned long long* active, unsigned long long* iterations,
                  int capacity);
/* time only frames whose frame_number % every == 0 (default 1: every frame), so the timing
 * events of a long measured run do not perturb most of its frames */
int hk_set_kernel_timing_interval(hk_ctx* ctx, uint32_t every);

/* ---- stand-alone ray query (minimum slice: light.wgsl:442-486) ----
 * rays: n records of {origin xyz, direction xyz} (6 floats, host or device memory)
 * per ray: max_distance, early_distance, exclude_instance (arrays of n, may be NULL =>
 * closest-hit defaults F32_MAX, 0, 0xFFFFFFFF).
 * hits: n records of {u, v, distance (f32), instance_index, primitive_index (u32)}. */
int hk_trace(hk_ctx* ctx, const float* rays, const float* max_distance, const float* early_distance,
             const uint32_t* exclude_instance, uint32_t n, void* hits, int device_ptrs, void* stream);

/* ---- self-test of the device f16 conversion (pack2x16float, light.wgsl:173-216 pack_reservoir)
 * converts n host floats with the kernels' own conversion; out: n f16 bit patterns (host) */
int hk_selftest_f16(hk_ctx* ctx, const float* in, uint32_t n, uint16_t* out);
/* ---- self-test of the kernels' division by a frame dimension (div_by, hk_device.h): counts the
 * f32 bit patterns x in [lo, hi) (both signs) where div_by(x, divisor) != x / divisor */
int hk_selftest_div(hk_ctx* ctx, float divisor, uint32_t lo, uint32_t hi, uint64_t* mismatches);
/* ---- self-test of the kernels' reciprocal (rcp_exact, hk_device.h): counts the f32 bit patterns
 * x in [lo, hi) (both signs) where rcp_exact(x) != 1 / x (IEEE) */
int hk_selftest_rcp(hk_ctx* ctx, uint32_t lo, uint32_t hi, uint64_t* mismatches);
/* ---- self-test of the kernels' ray-counter reduction (wave_count, hk_device.h): thread i of 256-thread workgroups
 * counts values[i] (n host words; the last workgroup's other threads count nothing); sum: the sharded counter's total */
int hk_selftest_count(hk_ctx* ctx, const uint32_t* values, uint32_t n, uint64_t* sum);
/* ---- self-test of the kernels' texture sampler (sample_material_texture, hk_device.h; include/hk_texture.h):
 * samples uploaded texture `texture` at n host uv pairs (2 floats each); out: n x 4 host floats.
 * HK_ERR_INVALID, before any launch: texture >= the uploaded count (none uploaded included), or uv / out NULL with
 * n > 0.  n == 0 does nothing. */
int hk_selftest_texture(hk_ctx* ctx, uint32_t texture, const float* uv, uint32_t n, float* out);
/* ---- self-test of the kernels' scalar functions (include/hk_math.h as hipcc compiles it for the device, and the
 * arithmetic helpers of hk_device.h), so that the device's bits can be compared with the host's on given inputs
 * (oracle hko_math_array, tests/test_gpu_math.py).  One function id per call; element i is computed by thread i of
 * 256-thread workgroups, each id calling its function as the frame kernels do.  Operands and results are 32-bit
 * words: f32 bit patterns, or u32 codes where the function takes or returns one. */
enum hk_math_fn {
    /* hk_math.h transcendentals */
    HK_MATH_EXP2 = 0,            /* hk_exp2(a) */
    HK_MATH_EXP,                 /* hk_exp(a) */
    HK_MATH_EXP_WEIGHT,          /* hk_exp_weight(a) */
    HK_MATH_LOG2,                /* hk_log2(a) */
    HK_MATH_POW,                 /* hk_pow(a, b) */
    HK_MATH_POW2,                /* hk_pow2(a) */
    HK_MATH_POW5,                /* hk_pow5(a) */
    HK_MATH_POW16,               /* hk_pow16(a) */
    HK_MATH_SINCOS,              /* hk_sincos(a): out0 = sin, out1 = cos */
    /* hk_math.h packing */
    HK_MATH_UNORM16,             /* hk_unorm16(a): f32 -> code */
    HK_MATH_SNORM8,              /* hk_snorm8(a): f32 -> code */
    HK_MATH_UNPACK_UNORM16_FAST, /* hk_unpack_unorm16_fast(a): code -> f32 */
    HK_MATH_UNPACK_SNORM8_FAST,  /* hk_unpack_snorm8_fast(a, b & 3): byte lane b of word a -> f32 */
    HK_MATH_UNORM8_FAST,         /* hk_unorm8_fast(a): code -> f32 */
    HK_MATH_RANDOM_FLOAT,        /* hk_random_float(a): u32 -> f32 */
    /* hk_math.h small operations */
    HK_MATH_FRACT,               /* hk_fract(a) */
    HK_MATH_MINF,                /* hk_minf(a, b) */
    HK_MATH_MAXF,                /* hk_maxf(a, b) */
    HK_MATH_SATURATE,            /* hk_saturate(a) */
    HK_MATH_SIGNF,               /* hk_signf(a) */
    /* hk_device.h arithmetic (host reference: the IEEE operation) */
    HK_MATH_DIV,                 /* a / b, the divide behind operator/ */
    HK_MATH_SQRT,                /* sqrtf(a), the one in length() */
    HK_MATH_RCP_EXACT,           /* rcp_exact(a); reference 1 / a */
    HK_MATH_RCP_FAST,            /* one component of inv(): rcp_fast(a) where rcp_fast_ok(a), else 1.0f / a */
    HK_MATH_DIV_BY,              /* div_by(a, b, RN(1 / b)), the reciprocal evaluated on the host; reference a / b */
    HK_MATH_F2U32,               /* f2u32(a): saturating f32 -> u32 */
    HK_MATH_F2I32,               /* f2i32(a): saturating f32 -> i32 */
    /* hk_device.h f16 decode */
    HK_MATH_UNPACK_F16,          /* out0 = unpack_lo16float(a), out1 = unpack_hi16float(a) (out1 may be NULL) */
    HK_MATH_COUNT
};
/* a, b: n host words each (b may be NULL for the one-operand ids); out0, out1: n host words each (out1 may be NULL
 * except for HK_MATH_SINCOS).  HK_ERR_INVALID, before any launch: an unknown fn, a required pointer NULL with n > 0,
 * out1 NULL for HK_MATH_SINCOS.  n == 0 does nothing. */
int hk_selftest_math(hk_ctx* ctx, int fn, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out0,
                     uint32_t* out1);

#ifdef __cplusplus
}
#endif

#endif /* HIKARI_AMD_H */
