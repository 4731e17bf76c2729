// hk_runtime.hip — host runtime behind the C ABI (include/hikari_amd.h).
//
// One hk_ctx per camera entity owns everything the reference keeps per view:
//   ReservoirCache (light.rs:342-363)        -> 10 SoA reservoir buffers in HBM
//   LightTextures (light.rs:297-383)          -> albedo (S), variance[3], render[3] (s)
//   PostProcessTextures denoise part (post_process.rs:710-714) -> internal[4] (packed: dn_rgb / dn_bi), internal variance,
//                                               denoised[3], tone-mapped output
//   group-2 scene buffers (mesh_material/mod.rs:488-598) -> device copies of the std430 arrays
// hk_render_frame issues the kernels in LightNode::run order (light.rs:646-699) and
// hk_denoise in PostProcessNode::run order (post_process.rs:1190-1224).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/hikari_amd.h"
#include "../../include/hikari_scene.h"
#include "hk_launch.h"

using namespace hk;

namespace {
constexpr int32_t BAND_HALO = 40;  // >= 36 rows: 20 (spatial reuse) + 15 (a-trous) + 1 (variance blur)
// 3 counters (top, emitter, primary) x COUNTER_SHARDS lines of 64 B
constexpr size_t COUNTER_SPAN = (size_t)COUNTER_SHARDS * COUNTER_STRIDE;  // u64 per counter
constexpr size_t COUNTER_BYTES = 3 * COUNTER_SPAN * sizeof(unsigned long long);
constexpr size_t PERSIST_BYTES = (size_t)PERSIST_KINDS * PERSIST_LINES * PERSIST_LINE * sizeof(unsigned long long);

struct TimedLaunch {
    const char* name;
    hipEvent_t start, stop;
};

// Runtime options (hk_set_option / hk_get_option): each picks among schedules or kernel variants that
// produce the same bits, so they change speed only.  Read once per call from the context (no environment
// variables on the frame path); the defaults are the measured-fastest configuration.
enum Opt {
    OPT_PIPELINE_MIN_PX,     // frame pipelining (G-buffer / tail streams) from this many integrator pixels up
    OPT_PIPELINE_HEAVY_MIN_PX,  // ... and from this many up on frames with spatial reuse or the denoiser
    OPT_GBUFFER_PIPELINE,    // k_gbuffer of frame f on its own stream next to frame f-1's light passes
    OPT_TAIL_PIPELINE,       // denoise + tone-sum of frame f on their own stream next to frame f+1
    OPT_CHANNEL_STREAMS,     // the indirect chain on a side stream next to direct -> emissive
    OPT_FUSE,                // k_direct_fused when every reprojection is the identity
    OPT_FUSE_MIN_PX,         // ... from this many pixels up
    OPT_MERGE,               // k_light_merged: -1 auto (small unpipelined frames), 0 never, 1 whenever possible
    OPT_BG_ELISION,          // background store elision (bg_elide)
    OPT_SPATIAL_VIEW,        // spatial view planes written by the indirect temporal pass
    OPT_BAND_FULL_WINDOWS,   // every pass of a band on all its rows (no per-pass row windows)
    OPT_LEAF_COLLAPSE,       // leaf-collapsed node copies for the light walks (at scene upload / update)
    OPT_GBUFFER_REUSE,       // skip k_gbuffer when its slot already holds this frame's planes (static sub-frames)
    OPT_LDS_SCENE,           // LaunchOpts
    OPT_GBUFFER_STACK_FULL,
    OPT_GBUFFER_DEEP,
    OPT_GBUFFER_LDS_MAX_PX,
    OPT_DIRECT_W4_MIN_PX,
    OPT_FUSED_W4,
    OPT_PERSISTENT_INDIRECT,
    OPT_COMPACT_EMITTER,
    OPT_COMPACT_SHADOW,
    OPT_FSR_TILED,           // EASU with its input footprint staged in LDS (hk_fsr.hip)
    OPT_PRESENT_RUN,         // hk_present stores 16-byte row runs where the viewport's runs are aligned (hk_overlay.hip)
    OPT_SHARED_XFORM,        // one local ray per walk where every instance carries the same transform (Scene::shared_xform)
    OPT_BG_TILE_SKIP,        // workgroups outside the scene's screen bound return at once (TileKeep)
    OPT_COUNT
};
struct OptDef {
    const char* key;
    double def, lo, hi;
};
constexpr OptDef OPTS[OPT_COUNT] = {
    {"pipeline_min_px", 1.2e6, 0.0, 1e12}, {"pipeline_heavy_min_px", 0.0, 0.0, 1e12},
    {"gbuffer_pipeline", 1, 0, 1},         {"tail_pipeline", 1, 0, 1},
    {"channel_streams", 1, 0, 1},          {"fuse", 1, 0, 1},              {"fuse_min_px", 1048576.0, 0.0, 1e12},
    {"merge", -1, -1, 1},                  {"bg_elision", 1, 0, 1},        {"spatial_view_planes", 1, 0, 1},
    {"band_full_windows", 0, 0, 1},        {"leaf_collapse", 1, 0, 1},     {"gbuffer_reuse", 1, 0, 1},
    {"lds_scene", 1, 0, 2},                {"gbuffer_stack_full", 0, 0, 1}, {"gbuffer_deep", 0, 0, 1},
    {"gbuffer_lds_max_px", 6e5, 0.0, 1e12},
    {"direct_w4_min_px", 4e5, 0.0, 1e12},  {"fused_w4", 1, 0, 1},          {"persistent_indirect", 0, 0, 1},
    {"compact_emitter", 0, 0, 1},          {"compact_shadow", 0, 0, 1},    {"fsr_tiled", 1, 0, 1},
    {"present_run", 1, 0, 1},              {"shared_xform", 1, 0, 1},      {"bg_tile_skip", 1, 0, 1},
};

// One slot of the planes k_gbuffer double-buffers (hk_ctx::g / g_prev: swapped on each hk_render_gbuffer) so a
// frame's G-buffer can be traced ahead.  A host upload (hk_set_gbuffer_plane) swaps the position or the velocity
// plane alone, so the members of one slot need not come from the same allocation round.
struct GSlot {
    float4* position = nullptr;
    uint32_t* normal = nullptr;
    float2* depth_gradient = nullptr;
    float2* instance_material = nullptr;
    float4* velocity_uv = nullptr;
    uint2* albedo = nullptr;  // the light targets' albedo plane (k_gbuffer writes it with the others)
};

// The flags and counters of FrameSchedule: what its reset() returns to the values below.
struct ScheduleState {
    // G-buffer pipelining: k_gbuffer of frame f runs on gb_stream, next to frame f-1's light passes
    bool gb_pending = false;   // a k_gbuffer launch was made on gb_stream
    bool gb_serial = true;     // the next k_gbuffer runs in caller-stream order
    bool post_pending = false;
    bool gb_call_rec = false;  // the last call recorded ev_gb_call (it was pipelined)
    uint32_t gb_calls = 0;
    // fork shortcut bookkeeping (hk_render_frame): at each hk_render_gbuffer entry (by call parity) the counts
    // of FrameSchedule::other_picks / frame_st_epoch; the latest k_gbuffer ran on gb_stream (gb_on_gs) after the
    // caller stream at the previous call's entry (gb_wait_*: the counts there) and after frame tail gb_tail_seq;
    // the previous hk_render_frame ran its indirect chain on the side stream only (rf_side_only)
    uint64_t entry_other[2] = {0, 0}, entry_epoch[2] = {0, 0};
    bool gb_on_gs = false, gb_wait_valid = false, rf_side_only = false;
    uint64_t gb_wait_other = 0, gb_wait_epoch = 0, gb_tail_seq = 0;
    // hk_render_frame calls (rf_seq) and the latest one that recorded ev_rf (rf_rec_seq, with the counts
    // there); the ev_rf the open tail waited for (tail_rf), per G-buffer slot the one its last tail
    // waited for; per call parity, at hk_render_gbuffer's entry: the latest hk_render_frame and whether
    // only the frame sequence ran since it recorded ev_rf (entry_clean)
    uint64_t rf_seq = 0, rf_rec_seq = 0, rf_other = 0, rf_epoch = 0, tail_rf = 0;
    uint64_t gslot_rf[2] = {0, 0}, entry_rf[2] = {0, 0};
    bool entry_clean[2] = {false, false};
    // Frame-tail pipelining: the demodulation, a-trous levels and tone-sum of frame f run on dn_stream next to
    // frame f+1's light passes.  Slot events: the latest tail work that read render slot r / G-buffer slot g.
    bool rslot_rec[2] = {false, false}, gslot_rec[2] = {false, false};
    // tail_end calls so far, and the one that last recorded each slot event (0: none)
    uint64_t tail_seq = 0, rslot_seq[2] = {0, 0}, gslot_seq[2] = {0, 0};
    uint32_t rslot = 0, gslot = 0;  // current render / G-buffer slot
    bool dn_pending = false;        // work was queued on dn_stream
    bool rf_swapped = false;        // the latest hk_render_frame wrote the other render slot
    bool tail_open = false;         // dn_stream already waits for that frame (ev_rf)
};

// Everything that orders a context's work across streams: the streams and events, and which waits are due.
// A new stream dependency is added here (and nowhere else in hk_ctx).
struct FrameSchedule : ScheduleState {
    std::string* error = nullptr;  // hk_ctx::error
    // channel fork-join: the indirect chain on side[1] next to direct_lit -> emissive (side[0]: see create)
    hipStream_t side[2] = {nullptr, nullptr};
    hipStream_t gb_stream = nullptr, dn_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    hipEvent_t ev_gb_done = nullptr;                // after the latest k_gbuffer launch on gb_stream
    hipEvent_t ev_gb_call[2] = {nullptr, nullptr};  // caller stream at the entry of the last two pipelined calls
    hipEvent_t ev_post = nullptr;                   // after a post-process read of the previous slot
    hipEvent_t ev_rf = nullptr;                     // caller stream, end of the latest hk_render_frame
    hipEvent_t ev_rslot[2] = {nullptr, nullptr}, ev_gslot[2] = {nullptr, nullptr};
    hipEvent_t ev_dn_last = nullptr;                // dn_stream, after its latest work
    hipEvent_t ev_frame_mark = nullptr;  // the frame stream's position, waited for by a foreign-stream copy
    // reads of output planes on streams other than the frame sequence's (hk_copy_output_rows): the plane
    // and an event after the copy; the next write of that plane waits for it (ext_wait)
    std::vector<std::pair<const void*, hipEvent_t>> ext_reads;
    std::vector<hipEvent_t> ext_pool;
    // API calls outside the frame sequence, the frame sequence's stream and its changes (pick / pick_frame)
    uint64_t other_picks = 0, frame_st_epoch = 0;
    hipStream_t frame_st = nullptr;

    std::array<hipEvent_t*, 14> events()
    {
        return {&ev_fork,     &ev_join[0],  &ev_join[1],  &ev_gb_done,  &ev_gb_call[0], &ev_gb_call[1], &ev_post,
                &ev_rf,       &ev_rslot[0], &ev_rslot[1], &ev_gslot[0], &ev_gslot[1],   &ev_dn_last,    &ev_frame_mark};
    }
    int fail(const char* msg) const
    {
        *error = msg;
        return HK_ERR_HIP;
    }
    int create(std::string* err)
    {
        error = err;
        // side[1] runs the indirect chain.  side[0] carries no work but is kept: streams are mapped
        // round-robin onto the process's hardware queues (GPU_MAX_HW_QUEUES = 4), and without it the
        // G-buffer / tail streams land on queues that serialise them behind the light passes
        // (cornell 1080p 0.601 -> 0.674 ms/frame measured without it).  Keep this creation order.
        for (hipStream_t* s : {&side[0], &side[1], &gb_stream, &dn_stream})
            if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) return HK_ERR_HIP;
        for (hipEvent_t* e : events())
            if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return HK_ERR_HIP;
        return HK_OK;
    }
    void destroy()
    {
        for (auto& r : ext_reads) ext_pool.push_back(r.second);
        for (hipEvent_t e : ext_pool) (void)hipEventDestroy(e);
        for (hipStream_t s : side)
            if (s) (void)hipStreamSynchronize(s);
        for (hipEvent_t* e : events())
            if (*e) (void)hipEventDestroy(*e);
        for (hipStream_t s : {side[0], side[1], gb_stream, dn_stream})
            if (s) (void)hipStreamDestroy(s);
    }
    // A resize: resize_impl has synchronised the context's streams and freed every plane, and synchronises the
    // device before it returns, so every event recorded so far has completed by the next API call and a cleared
    // flag only skips a wait on a completed event.  Every flag and counter returns to a new context's value.
    // What persists: the streams and events themselves, ext_reads / ext_pool (they own events; a stale entry costs
    // one wait on a completed event), and other_picks / frame_st / frame_st_epoch (they describe the caller's
    // streams, not the targets: a foreign-stream copy after a resize still has to know the frame stream).
    void reset() { static_cast<ScheduleState&>(*this) = ScheduleState{}; }

    // Work that reads G-buffer planes, counters or targets, or that changes the scene, first waits
    // for any k_gbuffer launched ahead on gb_stream and any denoise / tone-sum queued on dn_stream
    // (hipStreamWaitEvent: device-side, no host wait).
    int gb_join(hipStream_t st, bool with_denoise = true) const
    {
        if (gb_pending && hipStreamWaitEvent(st, ev_gb_done, 0) != hipSuccess)
            return fail("hipStreamWaitEvent(G-buffer) failed");
        if (with_denoise && dn_pending && hipStreamWaitEvent(st, ev_dn_last, 0) != hipSuccess)
            return fail("hipStreamWaitEvent(denoise) failed");
        return HK_OK;
    }
    // The next write of `plane` (nullptr: of any plane) waits on `st` for the foreign-stream copies that read it.
    int ext_wait(hipStream_t st, const void* plane)
    {
        for (size_t k = 0; k < ext_reads.size();) {
            if (plane && ext_reads[k].first != plane) {
                ++k;
                continue;
            }
            if (hipStreamWaitEvent(st, ext_reads[k].second, 0) != hipSuccess)
                return fail("hipStreamWaitEvent(output read) failed");
            ext_pool.push_back(ext_reads[k].second);
            ext_reads[k] = ext_reads.back();
            ext_reads.pop_back();
        }
        return HK_OK;
    }
    // frame-tail work on dn_stream: it starts after the frame's hk_render_frame (ev_rf) and marks
    // the render / G-buffer slots it read
    int tail_begin()
    {
        if (!tail_open) {
            if (hipStreamWaitEvent(dn_stream, ev_rf, 0) != hipSuccess) return fail("hipStreamWaitEvent(frame) failed");
            tail_rf = rf_rec_seq;
        }
        tail_open = true;
        return HK_OK;
    }
    int tail_end()
    {
        if (hipEventRecord(ev_rslot[rslot], dn_stream) != hipSuccess ||
            hipEventRecord(ev_gslot[gslot], dn_stream) != hipSuccess ||
            hipEventRecord(ev_dn_last, dn_stream) != hipSuccess)
            return fail("hipEventRecord(frame tail) failed");
        rslot_rec[rslot] = gslot_rec[gslot] = true;
        tail_seq++;
        rslot_seq[rslot] = gslot_seq[gslot] = tail_seq;
        gslot_rf[gslot] = tail_rf;
        dn_pending = true;
        return HK_OK;
    }
    // the scene, sizes or G-buffer planes change on the caller's stream: the next k_gbuffer must run
    // in caller-stream order (and a synchronous change waits for the one in flight)
    int gb_serialize(bool host_sync)
    {
        gb_serial = true;
        if (host_sync && gb_stream && hipStreamSynchronize(gb_stream) != hipSuccess)
            return fail("hipStreamSynchronize(G-buffer stream) failed");
        if (host_sync && dn_stream && hipStreamSynchronize(dn_stream) != hipSuccess)
            return fail("hipStreamSynchronize(denoise stream) failed");
        return HK_OK;
    }

    // The three conditions under which a wait packet is dropped (each one ahead of a kernel delays it).
    // hk_render_gbuffer, pipelined, slot g = gslot ^ 1, w = the call parity whose entry marker it would wait for:
    // frame f-2's tail (dn_stream) read this slot; it waited for ev_rf of a hk_render_frame (gslot_rf).
    // When that is the one whose ev_rf marked the caller stream where the previous call's entry
    // marker stands (nothing but the frame sequence ran in between: entry_clean) or a later one, the
    // tail's event implies the entry marker, and k_gbuffer waits for the tail alone: one packet fewer
    // ahead of it in the queue it shares with the indirect chain.
    bool tail_covers(uint32_t w, uint32_t g) const
    {
        return gb_call_rec && gslot_rec[g] && entry_clean[w] && entry_rf[w] > 0 && gslot_rf[g] >= entry_rf[w];
    }
    // hk_render_frame: this frame's G-buffer ran pipelined on gb_stream after the caller stream at the previous
    // hk_render_gbuffer's entry (W), and since W only the frame sequence ran, on this stream (no other
    // API call, no stream change): frame f-1's hk_render_frame, denoise, tone-sum and this frame's
    // hk_render_gbuffer.  See the fork there.
    bool gb_fresh() const
    {
        return gb_on_gs && gb_wait_valid && other_picks == gb_wait_other && frame_st_epoch == gb_wait_epoch && gb_pending;
    }
    // hk_render_frame: the render slot's last reader (frame f-2's tail) is also covered by ev_gb_done when
    // k_gbuffer waited for that tail or a later one (dn_stream is in order)
    bool slot_covered() const { return gb_fresh() && rslot_seq[rslot] <= gb_tail_seq; }
};

// Background tile skip (option bg_tile_skip).
// The guard band of the scene's screen bound (hks_screen_bounds), in pixels: the bound is exact in double and already
// holds the prepass jitter (< 1 px); what is left is the f32 rounding of a primary ray's direction and of the walk's
// box tests, some 1e-6 of the frame's width, so 4 px is three orders of magnitude above it.
constexpr uint32_t TILE_SKIP_GUARD = 4;
// A pixel rectangle [x0, x1) x [y0, y1) in frame coordinates.
struct PxRect {
    int32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    bool empty() const { return x1 <= x0 || y1 <= y0; }
    static PxRect all() { return PxRect{0, 0, INT32_MAX, INT32_MAX}; }
    PxRect join(const PxRect& o) const
    {
        if (empty()) return o;
        if (o.empty()) return *this;
        return PxRect{std::min(x0, o.x0), std::min(y0, o.y0), std::max(x1, o.x1), std::max(y1, o.y1)};
    }
};
// What the host knows of an elision mask's bytes (gbmask, bgmask[k]) without reading them.  The kernels' rule
// (k_gbuffer, bg_elide): a covered pixel zeroes its byte; a background pixel sets the bits its launch asks for and
// keeps the others, but for the pair bit (4), which a launch that does not ask for it clears.  So bit b is set in
// every byte outside cover[b], the bounding rectangle of the screen bounds of every masked launch since (and
// including) the last one that asked for b: that launch set it there, or skipped a tile because it was set already,
// and every pixel there has been background since.  known[b] is false until such a launch ran on the mask as it is
// (reset: the mask was zero-filled or dropped).
struct MaskHistory {
    static constexpr int BITS = 5;
    PxRect cover[BITS];
    bool known[BITS] = {};
    void reset()
    {
        for (bool& k : known) k = false;
    }
    // A masked launch asking for the bits `need`, all of whose pixels outside `now` are background.  true: outside
    // `keep` every byte already has all of `need`, so a workgroup there stores nothing and writes no byte.
    bool launch(uint32_t need, const PxRect& now, PxRect& keep)
    {
        bool ok = true;
        keep = now;
        for (int b = 0; b < BITS; ++b) {
            if (!(need >> b & 1u)) continue;
            if (!known[b]) ok = false;
            else keep = keep.join(cover[b]);
        }
        for (int b = 0; b < BITS; ++b) {
            if (need >> b & 1u) {
                cover[b] = now;
                known[b] = true;
            } else if (b == 4) {
                known[b] = false;
            } else if (known[b]) {
                cover[b] = cover[b].join(now);
            }
        }
        return ok;
    }
};
// What the host knows of a tone slot's texels (tone_buf[k]) without reading them.  k_tone_run's rule (tone_texel): a
// pixel whose render texels are the zero texels (a background pixel's, bg_elide) gets the clear colour's texel, whatever
// else the frame holds.  So after a launch with clear colour `clear` over window `key`, whose input planes held the
// zero texel at every pixel outside `cover`, every texel of the window outside `cover` is that clear-colour texel: the
// launch stored it there, or left those pixels out because the record before it already said so (hk_tone_sum).
// known is false until such a launch ran on the slot as it is (reset: the slot was reallocated, or a launch stored texels
// the host cannot name).
struct ToneHistory {
    bool known = false;
    PxRect cover;
    float clear[4] = {};   // compared bit for bit
    int32_t key[4] = {};   // the launch window: local row 0, rows, column 0, columns
    void reset() { known = false; }
    bool holds(const float* clear_color, const int32_t* window) const
    {
        return known && std::memcmp(clear, clear_color, sizeof(clear)) == 0 && std::memcmp(key, window, sizeof(key)) == 0;
    }
};
}  // namespace

struct hk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
    double opt[OPT_COUNT];  // hk_set_option
    bool on(Opt o) const { return opt[o] != 0.0; }

    // scene
    void* buf[9] = {};
    uint32_t count[9] = {};
    hk_node* walk_nodes[2] = {nullptr, nullptr};  // BLAS / TLAS copies of the light walks (leaf-collapsed)
    uint32_t* collapse_scratch = nullptr;
    float4* blas_wide = nullptr;  // G-buffer traversal layout (k_build_wide)
    float4* tlas_wide = nullptr;
    uint32_t gb_stack_need = 0;   // TLAS + BLAS subtree depth bound of closest_hit_ordered
    bool heavy = false;           // the last hk_render_frame had spatial reuse or followed a denoised frame (pipeline_size)
    int dn_calls = 0;             // hk_denoise calls since the last hk_render_frame
    uint32_t gb_blas_depth = 0;   // BLAS part of it (the TLAS part changes with hk_update_instances)
    uint32_t gb_tlas_depth = 0;   // TLAS part of it: set at upload and by every TLAS build; a refit keeps the tree
    void* dyn_scratch = nullptr;  // hk_update_instances scratch (sized at upload)
    size_t dyn_bytes = 0;
    // hk_tree_costs: the device block (slice table, accumulators), its bytes, and the host sides of both, which keep
    // their capacity from call to call
    void* cost_scratch = nullptr;
    size_t cost_bytes = 0;
    std::vector<CostSlice> cost_table;
    std::vector<hk_tree_cost> cost_host;
    // hk_update_meshes: the instanced meshes as upload recorded them (slice, vertices their primitives index, BLAS
    // depth), the per-node mesh tables of the BLAS derivatives (primitive offset, node base, node count) and scratch
    struct MeshSlice {
        hk_mesh_index index;
        uint32_t vertex_need;  // largest stored vertex index + 1; U32_MAX: the slices do not fit the arrays
        uint32_t depth;        // inner levels of its BLAS
        uint32_t used = 0;     // instances of the current set that carry it (hk_set_instances can leave it none)
    };
    std::vector<MeshSlice> meshes;
    // element capacities of the scene arrays (reserve_scene grows them, and with them the buffers FOLLOWERS names:
    // tlas_wide and walk_nodes[1] follow cap[5], prev_models follows cap[4]) and of collapse_scratch, and the
    // materials' emissive as uploaded or last replaced (4 floats each: the host's emitter count)
    size_t cap[9] = {};
    size_t collapse_cap = 0;
    std::vector<float> emissive;
    uint32_t* blas_aux = nullptr;  // three rows (primitive offset, node base, node count) of aux_stride words each
    size_t aux_stride = 0;         // = cap[2]: hk_add_meshes grows the rows with the asset nodes
    void* mesh_scratch = nullptr;
    size_t mesh_bytes = 0;
    // hk_set_meshes: one spare buffer per array 0-2 (null before the first call), which a call fills and swaps with
    // buf[i]; spare_cap: its elements
    void* spare[3] = {};
    size_t spare_cap[3] = {};
    // hk_set_mesh_skins: the registered skins (slice, vertices, joints, where its vertices lie in the streams) and one
    // device block carved into the four resident streams at skin_cap vertices each (bind positions x 12, bind normals
    // x 12, joint indices x 8, joint weights x 16); skin_cap stays where a smaller set follows a larger one
    struct Skin {
        hk_mesh_index index;
        uint32_t vertex_count, joint_count, vertex0;
        bool has_normals;
    };
    std::vector<Skin> skins;
    void* skin_block = nullptr;
    size_t skin_cap = 0;
    // hk_set_mesh_morphs: the registered morphs (slice, vertices, targets, where its base and its delta records lie)
    // and one device block carved into the four resident streams at the set's own totals (base positions and base
    // normals x 12 per vertex, position deltas and normal deltas x 12 per record); morph_cap: the block's bytes, which
    // stay where a smaller set follows a larger one
    struct Morph {
        hk_mesh_index index;
        uint32_t vertex_count, target_count, vertex0, delta0, normal_delta0;  // normal_delta0 MORPH_NONE: none
        bool has_normals;
    };
    std::vector<Morph> morphs;
    void* morph_block = nullptr;
    size_t morph_cap = 0;
    uint64_t morph_total[3] = {};  // the set's vertices, position delta records, normal delta records
    // GlobalTransformQueue[1] of every instance (transform.rs:32-44): the models as of the previous
    // k_gbuffer, read by its motion vectors; refreshed after a k_gbuffer that followed an update
    float* prev_models = nullptr;
    bool models_dirty = false;   // hk_update_instances ran since the last k_gbuffer
    bool velocity_zero = true;   // the current G-buffer's velocity plane is all zero (k_gbuffer, no motion)
    bool has_scene = false;
    // every instance record holds the same inverse_transpose_model bits (hks_shared_transform): set where the
    // records change, at hk_scene_upload from the records and in rebuild_instances from the models they derive from
    bool shared_transform = false;
    uchar4* noise = nullptr;
    bool has_noise = false;
    // material textures (hk_texture_upload)
    hk_texture_desc* tex_desc = nullptr;
    uint32_t* texels = nullptr;
    float* tex_lut = nullptr;
    uint32_t n_textures = 0;

    // sizes
    uint32_t S[2] = {0, 0}, s[2] = {0, 0};
    float ratio = 1.0f;
    int32_t S_row0 = 0, S_rows = 0, s_row0 = 0, s_rows = 0;
    int32_t core_row0 = 0, core_rows = 0;
    int32_t halo = BAND_HALO;
    int32_t stripe_n = 0, stripe_k = 0;  // interleaved stripes (hk_resize_striped), stripe_n >= 2
    bool albedo_fresh = false;  // the albedo target matches the G-buffer (k_gbuffer wrote both)
    bool sized = false;

    // G-buffer (band-local, S-wide): this frame's planes and the previous frame's (prepass.rs:309-317 swap)
    GSlot g, g_prev;
    FrameSchedule sch;  // everything that orders work across streams
    uint32_t head = 0;  // frame_number % 2 (PostProcessTextures.head)
    // light targets (albedo: GSlot); render / variance are double-buffered for frame-tail pipelining (sch.rslot)
    float* variance[3] = {}, *variance_alt[3] = {};
    uint2* render[3] = {}, *render_alt[3] = {};
    uint4* reservoirs[HK_RESERVOIR_BUFFERS] = {};
    uint32_t res_n = 0;
    // background store elision masks (ChannelArgs::bg): [0] the fused direct/emissive pair, [1] the
    // indirect channel; valid = the mask describes the buffers' contents for pass window key
    uint8_t* bgmask[2] = {};
    bool bg_valid[2] = {false, false};
    // a band's per-channel row-window margins, sticky maxima since hk_resize (band_windows): -1 = none yet
    int32_t win_out = -1, win_emi = -1, win_ind = -1;
    // a 2-D tile's own columns (hk_resize_tile): global [core_col0, core_col0 + core_cols); 0 / S.x otherwise
    int32_t core_col0 = 0, core_cols = 0;
    int32_t bg_key[2][2] = {};
    uint8_t* gbmask = nullptr;  // the G-buffer's (ViewArgs::bg), per S pixel
    uint4* sp_view = nullptr;   // spatial view planes of the indirect channel (ChannelArgs::view), 3 x res_n
    bool gb_valid = false;
    int32_t gb_key[2] = {};
    // Background tile skip: the world box of every instance while the host knows it (hk_scene_upload from the
    // records, the instance updates from their models and local boxes; not after hk_update_meshes), the screen
    // bound of the k_gbuffer that wrote each G-buffer slot (the whole plane: none), the masks' histories (gbmask,
    // bgmask[0..1]) and the workgroups the last frame's launches skipped (k_gbuffer, direct / emissive, indirect)
    double scene_box[6] = {};
    bool scene_box_valid = false;
    PxRect grect[2] = {PxRect::all(), PxRect::all()};
    MaskHistory gb_hist, bg_hist[2];
    uint32_t tiles_skipped[3] = {};
    // Tone pass over the kept rectangle: each tone slot's history, and the last hk_tone_sum's launch (the pixels of its
    // window it left out, the frame rectangle it ran over; hk_tone_skip_info)
    ToneHistory tone_hist[2];
    uint64_t tone_skipped = 0;
    int32_t tone_rect[4] = {};
    // denoise
    uint4* dn_rgb[4] = {};        // a-trous level inputs, the 3 channels packed (DenoiseArgs::rgb / bi)
    uint2* dn_bi[4] = {};
    float* internal_variance[3] = {};
    float4* dn_nd = nullptr;      // (normal, depth) per pixel (k_demod3)
    float4* dn_center = nullptr;  // (depth gradient, luminance denominators of channels 0, 1) per pixel
    float* dn_den2 = nullptr;     // luminance denominator of channel 2 per pixel
    int last_denoised_channels = 3;
    uint2* denoised[3] = {};
    uint2* tone_buf[2] = {};      // tone_mapping_output[2], written at [head]
    uint2* upscale = nullptr;     // upscale_output[0] (SMAA TU4x), U = ceil(S * 2 / ratio)
    uint2* taa_buf[2] = {};       // taa_output[2]
    uint32_t upscale_wh[2] = {0, 0}, taa_wh[2] = {0, 0};
    uint2* fsr_buf[2] = {};       // upscale_output[0..1] under FSR1 (EASU, RCAS), S
    float fsr_sharpness = 0.0f;   // Upscale::Fsr1::sharpness (hk_set_fsr1_sharpness)
    uint8_t* present_buf = nullptr;  // the context's own present plane (hk_present with data == NULL), packed rows
    uint32_t present_wh[2] = {0, 0}, present_format = 0;
    float4* accum = nullptr;     // sub-frame accumulator (hk_accumulate), allocated on first use
    uint2* accum_out = nullptr;
    uint32_t accum_n = 0;
    // counters (top, emitter, primary)
    unsigned long long* counters = nullptr;
    unsigned long long* persist = nullptr;  // persistent-wave tile claim counters (Counters::persist)
    // wavefront indirect pass (hk_set_wavefront): queues, SoA hit records, control words
    bool wavefront = false;
    uint32_t* wf_queue1 = nullptr;
    uint32_t* wf_keys = nullptr;
    uint32_t* wf_queue2 = nullptr;
    uint4* wf_hit = nullptr;
    float* wf_hit_t = nullptr;
    uint32_t* wf_ctl = nullptr;
    uint32_t wf_seg_cap = 0;

    // G-buffer reuse (option gbuffer_reuse): what produced the planes now in each G-buffer slot — the
    // view, jitter and band window of the k_gbuffer that wrote them and the input generation at that
    // time (bumped by every scene / texture / instance / size / host-plane / option change)
    struct GbSig {
        float view[3 + 16 + 16 + 16 + 2];
        int32_t win[2];
        uint64_t gen;
        bool valid;
    } gsig[2] = {};
    uint64_t gen = 1;
    uint64_t primary_reused = 0;  // primary rays of the skipped launches (since hk_reset_counters)

    // timing
    bool timing = false;
    uint32_t timing_every = 1;   // time frames with frame_number % timing_every == 0
    bool timing_frame = true;    // the current frame is one of them
    std::vector<TimedLaunch> pending;
    std::vector<hipEvent_t> event_pool;
    std::vector<std::string> timing_names;
    std::vector<double> timing_ms;
    std::vector<uint64_t> timing_n;
    // traverse_top lane statistics per timed launch name (instrumented builds, hk_lane_stats)
    std::vector<std::string> lane_names;
    std::vector<unsigned long long> lane_act, lane_its;
};

namespace {

int fail(hk_ctx* c, int code, const std::string& msg)
{
    if (c) c->error = msg;
    return code;
}

#define HK_HIP(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail((c), HK_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
    } while (0)

// Every API call that enqueues work resolves its stream here.  The frame sequence (hk_render_gbuffer,
// hk_render_frame, hk_denoise, hk_tone_sum) uses pick_frame; the count of the other calls and a change
// of the frame sequence's stream tell hk_render_frame what ran since k_gbuffer's wait point (the fork
// shortcut there).
hipStream_t pick(hk_ctx* c, void* stream)
{
    c->sch.other_picks++;
    return stream ? (hipStream_t)stream : c->stream;
}
hipStream_t pick_frame(hk_ctx* c, void* stream)
{
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (s != c->sch.frame_st) {
        c->sch.frame_st = s;
        c->sch.frame_st_epoch++;
    }
    return s;
}

#define HK_TRY(expr)            \
    do {                        \
        int _r = (expr);        \
        if (_r != HK_OK) return _r; \
    } while (0)

// a 2-D tile (hk_resize_tile): the context owns some of the columns only
bool tile_columns(const hk_ctx* c) { return c->core_cols > 0 && c->core_cols < (int32_t)c->S[0]; }
// Frame pipelining pays on large frames: on a small stripe of traversal + NEE alone (a 2- to 8-way split
// of 1080p: <= 1 Mpx, 0.1-0.25 ms frames) the cross-stream waits cost more than the overlap hides
// (cornell 8-way stripe 0.145 -> 0.172 ms), on a 1080p frame or a 4K band it gains.  A frame with spatial
// reuse or the denoiser (`heavy`: this frame's spatial settings, or hk_denoise in the previous frame) has a
// long G-buffer and tail to hide, and pipelines at every size: scene 1080p 2-way band 1.12 -> 0.92 ms,
// 8-way 0.50 -> 0.45, city 4K 8-way 0.90 -> 0.86 (profiles/r05/c21).  Only the schedule changes, never
// the results.
// (the pixels of the band's rows, at a 2-D tile's columns + halo: the work its launches cover)
double ctx_px(const hk_ctx* c)
{
    double cols = (double)c->s[0];
    if (tile_columns(c))
        cols = (double)(std::min((int32_t)c->s[0], c->core_col0 + c->core_cols + c->halo) - std::max(0, c->core_col0 - c->halo));
    return cols * (double)c->s_rows;
}
bool pipeline_size(const hk_ctx* c)
{
    const double px = ctx_px(c);
    return px >= c->opt[OPT_PIPELINE_MIN_PX] || (c->heavy && px >= c->opt[OPT_PIPELINE_HEAVY_MIN_PX]);
}
bool dn_pipeline_enabled(const hk_ctx* c) { return c->on(OPT_TAIL_PIPELINE) && pipeline_size(c); }

template <typename T>
void release(T*& p)
{
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

// Every device target whose size follows hk_resize, named once: resize_impl allocates from this table and
// free_targets releases from it, so a new plane is its typed member in hk_ctx plus one line here.  Only those two
// walk the table; the frame path reads the typed members.
struct Target {
    void** ptr;
    size_t bpp;     // bytes per pixel
    char plane;     // sized by 'S': S[0] x S_rows pixels, 's': s[0] x s_rows; 0: allocated on first use where it
                    // is needed (hk_post_process, hk_accumulate, ensure_wavefront) and only released from here
    uint32_t mult;  // planes per buffer
    bool zero;      // zero-filled by hk_resize
};
std::vector<Target> targets(hk_ctx* c)
{
    std::vector<Target> t;
    auto add = [&t](auto*& p, char plane, uint32_t mult = 1, bool zero = true) {
        t.push_back(Target{(void**)&p, sizeof(*p), plane, mult, zero});
    };
    for (GSlot* g : {&c->g, &c->g_prev}) {
        add(g->position, 'S');
        add(g->normal, 'S');
        add(g->depth_gradient, 'S');
        add(g->instance_material, 'S');
        add(g->velocity_uv, 'S');
        add(g->albedo, 'S');
    }
    for (int i = 0; i < 3; ++i) {
        add(c->variance[i], 's');
        add(c->render[i], 's');
        add(c->variance_alt[i], 's');
        add(c->render_alt[i], 's');
        add(c->denoised[i], 's');
        add(c->internal_variance[i], 's');
    }
    for (auto& r : c->reservoirs) add(r, 's', 4);  // light.rs:355-358 zero-fill
    // (the elision masks are not zero-filled: their valid flags are cleared instead)
    for (auto& m : c->bgmask) add(m, 's', 1, false);
    add(c->gbmask, 'S', 1, false);
    add(c->sp_view, 's', VIEW_PLANES);
    for (int i = 0; i < 4; ++i) {
        add(c->dn_rgb[i], 's');
        add(c->dn_bi[i], 's');
    }
    add(c->dn_nd, 's');
    add(c->dn_center, 's');
    add(c->dn_den2, 's');
    for (auto& b : c->tone_buf) add(b, 's');
    add(c->upscale, 0);
    for (auto& b : c->taa_buf) add(b, 0);
    for (auto& b : c->fsr_buf) add(b, 0);
    add(c->present_buf, 0);
    add(c->accum, 0);
    add(c->accum_out, 0);
    add(c->wf_queue1, 0);
    add(c->wf_keys, 0);
    add(c->wf_queue2, 0);
    add(c->wf_hit, 0);
    add(c->wf_hit_t, 0);
    add(c->wf_ctl, 0);
    return t;
}

void free_targets(hk_ctx* c)
{
    for (const Target& t : targets(c)) release(*t.ptr);
    c->bg_valid[0] = c->bg_valid[1] = c->gb_valid = false;
    c->grect[0] = c->grect[1] = PxRect::all();
    c->tiles_skipped[0] = c->tiles_skipped[1] = c->tiles_skipped[2] = 0;
    c->tone_hist[0].reset();
    c->tone_hist[1].reset();
    c->tone_skipped = 0;
    c->tone_rect[0] = c->tone_rect[1] = c->tone_rect[2] = c->tone_rect[3] = 0;
    c->upscale_wh[0] = c->upscale_wh[1] = c->taa_wh[0] = c->taa_wh[1] = 0;
    c->present_wh[0] = c->present_wh[1] = 0;
    c->accum_n = 0;
    c->sch.reset();
    c->sized = false;
}

// the wavefront pass's buffers, allocated on first use after a resize (s-plane sized)
int ensure_wavefront(hk_ctx* c)
{
    if (c->wf_ctl) return HK_OK;
    const size_t n = (size_t)c->s[0] * (size_t)c->s_rows;
    const size_t tiles = (size_t)((c->s[0] + 15u) / 16u) * (size_t)(((uint32_t)c->s_rows + 15u) / 16u);
    c->wf_seg_cap = (uint32_t)(256u * ((tiles + WF_SEGS - 1u) / WF_SEGS));
    HK_HIP(c, hipMalloc(&c->wf_queue1, (size_t)WF_SEGS * c->wf_seg_cap * 4));
    HK_HIP(c, hipMalloc(&c->wf_keys, (size_t)WF_SEGS * c->wf_seg_cap * 4));
    HK_HIP(c, hipMalloc(&c->wf_queue2, n * 4));
    HK_HIP(c, hipMalloc(&c->wf_hit, n * sizeof(uint4)));
    HK_HIP(c, hipMalloc(&c->wf_hit_t, n * 4));
    HK_HIP(c, hipMalloc(&c->wf_ctl, (size_t)wf_ctl_words(WF_MAX_BINS) * 4));
    return HK_OK;
}

hipEvent_t take_event(hk_ctx* c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// Launch wrapper: records HIP events around the kernel on its own stream when timing is on.
void lane_stats_account(hk_ctx* c, const char* name, hipStream_t st)
{
    unsigned long long v[2 * LANE_SLOTS];
    if (!lane_stats_take(v, st)) return;
    static const char* const stage[LANE_SLOTS] = {"", "/neighbour", "/march_tap", "/record_tests", "/merge",
                                                    "/instance_entry"};
    for (int slot = 0; slot < LANE_SLOTS; ++slot) {
        if (!v[2 * slot + 1]) continue;
        const std::string key = std::string(name) + stage[slot];
        size_t k = 0;
        for (; k < c->lane_names.size(); ++k)
            if (c->lane_names[k] == key) break;
        if (k == c->lane_names.size()) {
            c->lane_names.push_back(key);
            c->lane_act.push_back(0);
            c->lane_its.push_back(0);
        }
        c->lane_act[k] += v[2 * slot];
        c->lane_its[k] += v[2 * slot + 1];
    }
}

template <typename F>
void timed(hk_ctx* c, const char* name, hipStream_t st, F&& launch)
{
#ifdef HK_LANE_STATS
    // instrumented build: attribute the walk statistics to this launch (serialises the streams)
    (void)hipDeviceSynchronize();
    unsigned long long drop[2 * LANE_SLOTS];
    (void)lane_stats_take(drop, st);
    launch();
    lane_stats_account(c, name, st);
    return;
#endif
    if (!c->timing || !c->timing_frame) {
        launch();
        return;
    }
    TimedLaunch t{name, take_event(c), take_event(c)};
    (void)hipEventRecord(t.start, st);
    launch();
    (void)hipEventRecord(t.stop, st);
    c->pending.push_back(t);
}

void flush_timing(hk_ctx* c)
{
    for (TimedLaunch& t : c->pending) {
        (void)hipEventSynchronize(t.stop);
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, t.start, t.stop);
        size_t k = 0;
        for (; k < c->timing_names.size(); ++k)
            if (c->timing_names[k] == t.name) break;
        if (k == c->timing_names.size()) {
            c->timing_names.push_back(t.name);
            c->timing_ms.push_back(0.0);
            c->timing_n.push_back(0);
        }
        c->timing_ms[k] += ms;
        c->timing_n[k] += 1;
        c->event_pool.push_back(t.start);
        c->event_pool.push_back(t.stop);
    }
    c->pending.clear();
}

// Scene::bytes of a scene with these element counts (hk_scene_desc order; arrays 9 and 10 are the wide
// layouts of the asset and instance nodes, WIDE_NODE_BYTES per node): what stage_bytes sums per plan
constexpr size_t WIDE_NODE_BYTES = 64;
constexpr size_t SCENE_ELEM[9] = {sizeof(hk_vertex), sizeof(hk_primitive), sizeof(hk_node), sizeof(hk_alias_entry),
                                  sizeof(hk_instance), sizeof(hk_node), sizeof(hk_material), sizeof(hk_node),
                                  sizeof(hk_emissive)};
static void scene_array_bytes(const uint32_t* count, uint32_t* bytes)
{
    for (int k = 0; k < 9; ++k) bytes[k] = (uint32_t)std::min<size_t>((size_t)count[k] * SCENE_ELEM[k], 0xFFFFFFF0u);
    bytes[9] = (uint32_t)std::min<size_t>((size_t)count[2] * WIDE_NODE_BYTES, 0xFFFFFFF0u);
    bytes[10] = (uint32_t)std::min<size_t>((size_t)count[5] * WIDE_NODE_BYTES, 0xFFFFFFF0u);
}

FrameArgs frame_args(hk_ctx* c, const hk_settings* st, const hk_frame_inputs* in)
{
    FrameArgs A;
    std::memset(&A, 0, sizeof(A));
    A.sc.vertices = (const hk_vertex*)c->buf[0];
    A.sc.primitives = (const hk_primitive*)c->buf[1];
    A.sc.asset_nodes = c->walk_nodes[0];  // leaf-collapsed copies (launch_collapse_leaves)
    A.sc.alias_table = (const hk_alias_entry*)c->buf[3];
    A.sc.instances = (const hk_instance*)c->buf[4];
    A.sc.instance_nodes = c->walk_nodes[1];
    A.sc.materials = (const hk_material*)c->buf[6];
    A.sc.emissive_nodes = (const hk_node*)c->buf[7];
    A.sc.emissives = (const hk_emissive*)c->buf[8];
    A.sc.n_instances = c->count[4];
    A.sc.n_instance_nodes = c->count[5];
    A.sc.n_materials = c->count[6];
    A.sc.n_emissive_nodes = c->count[7];
    A.sc.blas_wide = c->blas_wide;
    A.sc.tlas_wide = c->tlas_wide;
    A.sc.textures = c->tex_desc;
    A.sc.texels = c->texels;
    A.sc.texture_lut = c->tex_lut;
    A.sc.n_textures = c->n_textures;
    A.sc.shared_xform = c->shared_transform && c->on(OPT_SHARED_XFORM);
    scene_array_bytes(c->count, A.sc.bytes);
    Frame& F = A.F;
    hk_settings def;
    hk_settings_default(&def);
    if (!st) st = &def;
    F.number = in ? in->frame_number : 0u;
    F.direct_validate_interval = st->direct_validate_interval;
    F.emissive_validate_interval = st->emissive_validate_interval;
    F.max_temporal_reuse_count = st->max_temporal_reuse_count;
    F.max_spatial_reuse_count = st->max_spatial_reuse_count;
    F.indirect_bounces = st->indirect_bounces;
    F.temporal_reuse = st->temporal_reuse;
    F.max_reservoir_lifetime = st->max_reservoir_lifetime;
    F.max_indirect_luminance = st->max_indirect_luminance;
    F.upscale_ratio = c->ratio;
    F.cos_solar_angle = hk_cos(st->solar_angle);  // same implementation as the device side
    for (int i = 0; i < 4; ++i) F.clear_color[i] = st->clear_color[i];
    if (in) {
        for (int i = 0; i < 3; ++i) {
            F.view_world_position[i] = in->view.world_position[i];
            F.view_proj_z[i] = in->view.view_proj[4 * i + 2];
            F.directional_color[i] = in->lights.directional_color[i];
            F.direction_to_light[i] = in->lights.direction_to_light[i];
            F.ambient_color[i] = in->lights.ambient_color[i];
        }
        F.orthographic = in->view.projection[15] == 1.0f;
    }
    F.S[0] = c->S[0];
    F.S[1] = c->S[1];
    F.inv_S[0] = 1.0f / (float)c->S[0];
    F.inv_S[1] = 1.0f / (float)c->S[1];
    for (int el = 0; el < 2; ++el) {
        const uint32_t count = el ? 8u : 16u;
        const float range = el ? 10.0f : 20.0f;
        for (uint32_t i = 1u; i <= 16u; ++i) {
            float py = i <= count ? std::sqrt((float)i / (float)count) * range : 0.0f;
            float interval = std::fmax(1.0f, py / 5.0f);
            float q = py / interval;
            F.sp_py[el][i - 1] = py;
            F.sp_tap_interval[el][i - 1] = interval;
            F.sp_tap_count[el][i - 1] = q > 0.0f ? (q >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)q) : 0u;
        }
    }
    for (uint32_t tc = 0; tc < 7; ++tc)
        for (uint32_t j = 0; j < 6; ++j) F.sp_tap_t[tc][j] = (float)j / (float)(tc + 1u);
    F.inv_s[0] = 1.0f / (float)c->s[0];
    F.inv_s[1] = 1.0f / (float)c->s[1];
    F.s[0] = c->s[0];
    F.s[1] = c->s[1];
    F.S_row0 = c->S_row0;
    F.S_rows = c->S_rows;
    F.s_row0 = c->s_row0;
    F.s_rows = c->s_rows;
    F.count_y0 = c->s_row0 + c->core_row0;
    F.count_y1 = F.count_y0 + c->core_rows;
    // G-buffer rows: whole frame, or (ratio 1 bands) the same rows as the integrator
    F.count_Sy0 = c->S_row0 + c->core_row0;
    F.count_Sy1 = c->S_rows == (int32_t)c->S[1] && c->core_rows == (int32_t)c->s[1] ? (int32_t)c->S[1]
                                                                                      : F.count_Sy0 + c->core_rows;
    // columns: a tile's own (ratio 1, so the same for the G-buffer), every column otherwise
    const bool tile = tile_columns(c);
    F.count_x0 = tile ? c->core_col0 : 0;
    F.count_x1 = tile ? c->core_col0 + c->core_cols : INT32_MAX;
    F.win_col0 = F.win_cols = 0;
    F.stripe_n = c->stripe_n;
    F.stripe_k = c->stripe_k;
    if (c->stripe_n >= 2) {  // every local row is one of this context's own rows
        F.count_y0 = F.count_Sy0 = 0;
        F.count_y1 = (int32_t)c->s[1];
        F.count_Sy1 = (int32_t)c->S[1];
    }
    A.G.position = c->g.position;
    A.G.normal = c->g.normal;
    A.G.depth_gradient = c->g.depth_gradient;
    A.G.instance_material = c->g.instance_material;
    A.G.velocity_uv = c->g.velocity_uv;
    A.noise = c->noise;
    A.cnt.top = c->counters;
    A.cnt.emitter = c->counters + COUNTER_SPAN;
    A.cnt.primary = c->counters + 2 * COUNTER_SPAN;
    A.cnt.persist = c->persist;
    A.opt.lds_scene = (int)c->opt[OPT_LDS_SCENE];
    A.opt.gbuffer_stack_full = c->on(OPT_GBUFFER_STACK_FULL);
    A.opt.gbuffer_deep = c->on(OPT_GBUFFER_DEEP);
    A.opt.gbuffer_lds_max_px = c->opt[OPT_GBUFFER_LDS_MAX_PX];
    A.opt.direct_w4_min_px = c->opt[OPT_DIRECT_W4_MIN_PX];
    A.opt.fused_w4 = c->on(OPT_FUSED_W4);
    A.opt.persistent_indirect = c->on(OPT_PERSISTENT_INDIRECT);
    A.opt.compact_emitter = c->on(OPT_COMPACT_EMITTER);
    A.opt.compact_shadow = c->on(OPT_COMPACT_SHADOW);
    return A;
}

// Per-pass launch windows of a row band (hk_resize with a halo).  A band recomputes halo rows so
// that its own ("core") rows see exactly the inputs of a whole-frame render; each pass needs
// fewer of them than the one before it, counted back from the tone-sum (core rows only):
//   the a-trous levels L3..L0 read their input at +-1, 2, 4, 8 px (denoise.wgsl:101-114), so
//   L3, L2, L1, L0 run on core +-0, 1, 3, 7 rows and demodulation on +-15; its 3x3 variance blur
//   (denoise.wgsl:151-159) reads the light passes' render / variance at +-16 (OUT);
//   spatial reuse runs on core +-OUT and reads the temporal reservoirs and the G-buffer depth
//   within its RANGE (20 px indirect, 10 emissive: light.wgsl:1568-1600), so each channel's temporal
//   pass runs on core +-(OUT + its RANGE) — direct_lit has no spatial pass (light.rs:656-676), so the
//   direct / emissive launch needs only +-OUT when emissive spatial reuse is off — and the G-buffer on
//   core +-(OUT + 20).
// For a static camera every other read is the pixel's own (temporal reprojection is the
// identity), so the core rows stay bit-identical to the whole frame (test_gpu_row_bands_*),
// with 1.15x instead of 1.30x the work of an 8-way city 4K band.  Rows outside a pass's window
// keep stale values that no windowed pass reads; a settings change that widens a window (band_windows) takes the
// history of the rows it brings in from their owner bands (or zero-fills them) and keeps the window wide from
// then on.  Option band_full_windows: every pass on all rows.
constexpr int32_t DENOISE_OUT_REACH = 16, SPATIAL_RANGE = 20, EMISSIVE_SPATIAL_RANGE = 10;
constexpr int32_t GBUFFER_REACH = DENOISE_OUT_REACH + SPATIAL_RANGE;
// Only for a static frame: under camera or instance motion temporal reprojection reads the previous
// frame's reservoirs at other rows, so every pass runs on the whole band (velocity_zero is set by
// hk_render_gbuffer before its own window is taken, and cleared by a host G-buffer plane upload).
bool band_windowed(const hk_ctx* c)
{
    return !(c->stripe_n >= 2 || (c->core_rows >= c->s_rows && !tile_columns(c)) || c->S_rows != c->s_rows ||
             !c->velocity_zero || c->on(OPT_BAND_FULL_WINDOWS));
}
// (a 2-D tile: the columns core +- margin as well; its planes are full width, so only the launches shrink)
FrameArgs pass_window(const hk_ctx* c, FrameArgs A, int32_t margin)
{
    if (!band_windowed(c)) return A;
    const int32_t lo = std::max(0, c->core_row0 - margin);
    const int32_t hi = std::min(c->s_rows, c->core_row0 + c->core_rows + margin);
    A.F.win_row0 = lo;
    A.F.win_rows = hi - lo;
    if (tile_columns(c)) {
        const int32_t c0 = std::max(0, c->core_col0 - margin);
        const int32_t c1 = std::min((int32_t)c->s[0], c->core_col0 + c->core_cols + margin);
        A.F.win_col0 = c0;
        A.F.win_cols = c1 - c0;
    }
    return A;
}
// option bg_elision = 0 switches background store elision off (the G-buffer's and the light passes'
// masks are both dropped while it is off)
bool bg_elision_off(const hk_ctx* c) { return !c->on(OPT_BG_ELISION); }
int32_t light_out_reach(const hk_settings* st) { return st->denoise ? DENOISE_OUT_REACH : 0; }
// The settings-dependent margins of a band's light-pass windows (pass_window) as sticky maxima: a
// setting turned on later (denoise, emissive or indirect spatial reuse) widens its channel's window, and the rows
// it brings in hold records no pass of this band has updated since it was sized (or since a motion frame ran
// every pass on the whole band).  A whole-frame render holds those rows' history — its temporal passes run on every
// pixel whatever the spatial flags (light.rs:656-699) — and so does the band whose core the rows belong to (its
// core rows equal the whole frame's).  window_growth lists the rows per reservoir buffer; the host copies them
// from their owners between frames (hk_band_window_grow, hk_reservoir_rows: bands.refill_windows), and the frame
// after that is bit-identical to a whole-frame render (test_gpu_row_bands_settings_toggle).  A window that grows
// without the refill (hk_render_frame first) has its new rows zero-filled instead, as hk_resize zero-fills the
// buffers (light.rs:355-358): exact again once the history has refilled.  The window never narrows.
struct WindowGrowth {
    int32_t want[3];                // the margins `st` needs: spatial pass (out), direct + emissive, indirect
    int32_t rows[HK_RESERVOIR_BUFFERS][2][2];  // per buffer, above / below the core: local rows [r0, r1) to fill
    bool grows, fill;               // some margin widens; its new rows need history (a windowed frame, not the first)
};
WindowGrowth window_growth(const hk_ctx* c, const hk_settings* st)
{
    WindowGrowth G{};
    const int32_t out = light_out_reach(st);
    G.want[0] = out;
    G.want[1] = out + (st->emissive_spatial_reuse ? EMISSIVE_SPATIAL_RANGE : 0);
    G.want[2] = out + (st->indirect_spatial_reuse ? SPATIAL_RANGE : 0);
    if (tile_columns(c)) {
        // a 2-D tile runs every channel on its widest window from the first frame (every setting on): its window
        // never grows, so a settings change needs no refill (the row bands' refill moves rows, not rectangles)
        G.want[0] = DENOISE_OUT_REACH;
        G.want[1] = DENOISE_OUT_REACH + EMISSIVE_SPATIAL_RANGE;
        G.want[2] = DENOISE_OUT_REACH + SPATIAL_RANGE;
    }
    const int32_t have[3] = {c->win_out, c->win_emi, c->win_ind};
    // the buffers whose records the group's window holds: spatial pairs 4/5, 8/9; direct + emissive 0-5; indirect 6-9
    static const uint32_t members[3] = {0x330u, 0x03Fu, 0x3C0u};
    const bool windowed = band_windowed(c);
    const int32_t core0 = c->core_row0, core1 = c->core_row0 + c->core_rows;
    for (int b = 0; b < HK_RESERVOIR_BUFFERS; ++b) {
        G.rows[b][0][0] = G.rows[b][1][0] = INT32_MAX;
        G.rows[b][0][1] = G.rows[b][1][1] = INT32_MIN;
    }
    for (int g = 0; g < 3; ++g) {
        const int32_t old = have[g], m = std::max(old, G.want[g]);
        if (m == old) continue;
        G.grows = true;
        if (old < 0 || !windowed) continue;  // zero-filled since hk_resize, or every row computed this frame
        G.fill = true;
        const int32_t span[2][2] = {{std::max(0, core0 - m), std::max(0, core0 - old)},
                                    {std::min(c->s_rows, core1 + old), std::min(c->s_rows, core1 + m)}};
        for (int b = 0; b < HK_RESERVOIR_BUFFERS; ++b) {
            if (!(members[g] >> b & 1u)) continue;
            // union over the groups: the rows between two groups' spans lie in the narrower group's old window,
            // which this band computed exactly, so they equal the owner's records as well
            for (int side = 0; side < 2; ++side) {
                if (span[side][1] <= span[side][0]) continue;
                G.rows[b][side][0] = std::min(G.rows[b][side][0], span[side][0]);
                G.rows[b][side][1] = std::max(G.rows[b][side][1], span[side][1]);
            }
        }
    }
    for (int b = 0; b < HK_RESERVOIR_BUFFERS; ++b)
        for (int side = 0; side < 2; ++side)
            if (G.rows[b][side][1] <= G.rows[b][side][0]) G.rows[b][side][0] = G.rows[b][side][1] = 0;
    return G;
}
void commit_growth(hk_ctx* c, const WindowGrowth& G)
{
    int32_t* have[3] = {&c->win_out, &c->win_emi, &c->win_ind};
    for (int g = 0; g < 3; ++g) *have[g] = std::max(*have[g], G.want[g]);
}
int band_windows(hk_ctx* c, const hk_settings* st, hipStream_t s)
{
    const WindowGrowth G = window_growth(c, st);
    if (!G.grows) return HK_OK;
    commit_growth(c, G);
    if (!G.fill) return HK_OK;
    const size_t w = c->s[0];
    for (int b = 0; b < HK_RESERVOIR_BUFFERS; ++b)
        for (int side = 0; side < 2; ++side) {
            const int32_t r0 = G.rows[b][side][0], r1 = G.rows[b][side][1];
            if (r1 <= r0) continue;
            for (uint32_t plane = 0; plane < 4; ++plane)
                HK_HIP(c, hipMemsetAsync(c->reservoirs[b] + (size_t)plane * c->res_n + (size_t)r0 * w, 0,
                                         (size_t)(r1 - r0) * w * sizeof(uint4), s));
        }
    c->bg_valid[0] = c->bg_valid[1] = false;  // the elision masks no longer describe the buffers
    return HK_OK;
}


// The primary rays a k_gbuffer launch over A counts (its active pixels on the rows it counts: k_gbuffer's
// n_primary), for the launches G-buffer reuse skips.
uint64_t gbuffer_primary_rays(const FrameArgs& A)
{
    const Frame& F = A.F;
    const int32_t w0 = F.win_rows > 0 ? F.win_row0 : 0, w1 = w0 + launch_rows(F, F.S_rows);
    if (F.stripe_n >= 2) return (uint64_t)F.S[0] * (uint64_t)(w1 - w0);
    const int32_t lo = std::max(F.S_row0 + w0, F.count_Sy0), hi = std::min(F.S_row0 + w1, F.count_Sy1);
    const int32_t c0 = F.win_cols > 0 ? F.win_col0 : 0, c1 = c0 + (int32_t)launch_cols(F, F.S[0]);
    const int32_t x0 = std::max(c0, F.count_x0), x1 = std::min(c1, F.count_x1);
    return hi > lo && x1 > x0 ? (uint64_t)(x1 - x0) * (uint64_t)(hi - lo) : 0u;
}

// Background tile skip: the tiles of launch A's grid (over a plane `width` wide whose local row 0 is frame row
// `row0`) that meet the pixel rectangle `keep`, grown outward to the grid's own 16x16 tiles; *skipped: the
// workgroups outside them.  TILE_KEEP_ALL when none is.  Interleaved stripes keep every tile (their rows are not
// contiguous in the frame).
TileKeep tile_keep(const FrameArgs& A, uint32_t width, int32_t row0, int32_t rows, const PxRect& keep, uint32_t* skipped)
{
    const Frame& F = A.F;
    *skipped = 0;
    if (F.stripe_n >= 2) return TILE_KEEP_ALL;
    const int32_t ox = F.win_cols > 0 ? F.win_col0 : 0, oy = F.win_rows > 0 ? F.win_row0 : 0;
    const int32_t window[4] = {ox, oy, ox + (int32_t)launch_cols(F, width), oy + launch_rows(F, rows)};
    const int64_t gx = (launch_cols(F, width) + 15u) / 16u, gy = ((uint32_t)launch_rows(F, rows) + 15u) / 16u;
    const int32_t kr[4] = {keep.x0, keep.y0, keep.x1, keep.y1};
    uint32_t t[4];
    (void)hks_keep_tiles(kr, window, row0, 16u, t);  // (all zeros when no tile is kept)
    const TileKeep K{t[0], t[1], t[2], t[3]};
    *skipped = (uint32_t)(gx * gy) - (K.x1 - K.x0) * (K.y1 - K.y0);
    return *skipped ? K : TILE_KEEP_ALL;
}
// the primary rays k_gbuffer would count on the tiles outside K (gbuffer_primary_rays less the kept tiles' share)
uint64_t gbuffer_skipped_rays(const FrameArgs& A, const TileKeep& K)
{
    const Frame& F = A.F;
    const uint64_t all = gbuffer_primary_rays(A);
    if (K.x1 <= K.x0 || K.y1 <= K.y0) return all;
    const int32_t w0 = F.win_rows > 0 ? F.win_row0 : 0, w1 = w0 + launch_rows(F, F.S_rows);
    const int32_t c0 = F.win_cols > 0 ? F.win_col0 : 0, c1 = c0 + (int32_t)launch_cols(F, F.S[0]);
    // the kept tiles' active pixels, in frame coordinates, within the counted region
    const int32_t ky0 = std::min<int64_t>(w0 + 16 * (int64_t)K.y0, w1), ky1 = std::min<int64_t>(w0 + 16 * (int64_t)K.y1, w1);
    const int32_t kx0 = std::min<int64_t>(c0 + 16 * (int64_t)K.x0, c1), kx1 = std::min<int64_t>(c0 + 16 * (int64_t)K.x1, c1);
    const int32_t lo = std::max(F.S_row0 + ky0, F.count_Sy0), hi = std::min(F.S_row0 + ky1, F.count_Sy1);
    const int32_t x0 = std::max(kx0, F.count_x0), x1 = std::min(kx1, F.count_x1);
    const uint64_t kept = hi > lo && x1 > x0 ? (uint64_t)(x1 - x0) * (uint64_t)(hi - lo) : 0u;
    return all - kept;
}

int check_ready(hk_ctx* c, bool need_scene)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    if (need_scene && !c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (need_scene && !c->has_noise) return fail(c, HK_ERR_STATE, "no blue noise uploaded (hk_set_noise)");
    return HK_OK;
}

}  // namespace

extern "C" {

int hk_abi_version(void) { return HK_ABI_VERSION; }

void hk_settings_default(hk_settings* o)
{
    // HikariSettings::default() (lib.rs:435-455); upscale ratio defaults to SMAA_TU_2_0
    o->direct_validate_interval = 3;
    o->emissive_validate_interval = 5;
    o->max_temporal_reuse_count = 50;
    o->max_spatial_reuse_count = 800;
    o->max_reservoir_lifetime = 100.0f;
    o->solar_angle = 0.046f;
    o->indirect_bounces = 1;
    o->max_indirect_luminance = 10.0f;
    // Color::rgb(0.4, 0.4, 0.4) is sRGB; as linear RGBA
    float l = std::pow((0.4f + 0.055f) / 1.055f, 2.4f);
    o->clear_color[0] = o->clear_color[1] = o->clear_color[2] = l;
    o->clear_color[3] = 1.0f;
    o->temporal_reuse = 1;
    o->emissive_spatial_reuse = 0;
    o->indirect_spatial_reuse = 1;
    o->denoise = 1;
    o->taa = 0;
    o->upscale_ratio = 2.0f;
    o->upscale = 0;
}

int hk_create(int device, hk_ctx** out)
{
    if (!out) return HK_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return HK_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return HK_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HK_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HK_ERR_NO_DEVICE;
    hk_ctx* c = new hk_ctx();
    c->device = device;
    for (int k = 0; k < OPT_COUNT; ++k) c->opt[k] = OPTS[k].def;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->counters, COUNTER_BYTES) != hipSuccess || hipMemset(c->counters, 0, COUNTER_BYTES) != hipSuccess ||
        hipMalloc(&c->persist, PERSIST_BYTES) != hipSuccess || hipMemset(c->persist, 0, PERSIST_BYTES) != hipSuccess) {
        delete c;
        return HK_ERR_HIP;
    }
    if (c->sch.create(&c->error) != HK_OK) {
        hk_destroy(c);
        return HK_ERR_HIP;
    }
    *out = c;
    return HK_OK;
}

void hk_destroy(hk_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->sch.gb_stream) (void)hipStreamSynchronize(c->sch.gb_stream);
    if (c->sch.dn_stream) (void)hipStreamSynchronize(c->sch.dn_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_targets(c);
    for (int i = 0; i < 9; ++i) release(c->buf[i]);
    for (int i = 0; i < 3; ++i) release(c->spare[i]);
    release(c->blas_wide);
    release(c->tlas_wide);
    release(c->walk_nodes[0]);
    release(c->walk_nodes[1]);
    release(c->collapse_scratch);
    release(c->dyn_scratch);
    release(c->cost_scratch);
    release(c->blas_aux);
    release(c->mesh_scratch);
    release(c->skin_block);
    release(c->morph_block);
    release(c->prev_models);
    release(c->tex_desc);
    release(c->texels);
    release(c->tex_lut);
    release(c->noise);
    release(c->counters);
    release(c->persist);
    for (auto& t : c->pending) {
        c->event_pool.push_back(t.start);
        c->event_pool.push_back(t.stop);
    }
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    c->sch.destroy();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* hk_last_error(const hk_ctx* c) { return c ? c->error.c_str() : "null context"; }

int hk_set_option(hk_ctx* c, const char* key, double value)
{
    if (!c || !key) return HK_ERR_INVALID;
    for (int k = 0; k < OPT_COUNT; ++k) {
        if (std::strcmp(OPTS[k].key, key) != 0) continue;
        if (!(value >= OPTS[k].lo && value <= OPTS[k].hi))
            return fail(c, HK_ERR_INVALID, std::string("option ") + key + " out of range");
        // every key but the pixel-count thresholds is an on/off switch or a mode: integers only
        if (!std::strstr(key, "_px") && value != std::floor(value))
            return fail(c, HK_ERR_INVALID, std::string("option ") + key + " takes an integer value");
        c->opt[k] = value;
        c->gen++;  // (G-buffer reuse: planes written under other options are not reused)
        if (k == OPT_BAND_FULL_WINDOWS) c->bg_valid[0] = c->bg_valid[1] = c->gb_valid = false;  // new windows
        return HK_OK;
    }
    return fail(c, HK_ERR_INVALID, std::string("unknown option ") + key);
}

int hk_get_option(const hk_ctx* c, const char* key, double* value)
{
    if (!c || !key || !value) return HK_ERR_INVALID;
    for (int k = 0; k < OPT_COUNT; ++k)
        if (std::strcmp(OPTS[k].key, key) == 0) {
            *value = c->opt[k];
            return HK_OK;
        }
    return HK_ERR_INVALID;
}

const char* hk_option_name(int index) { return index >= 0 && index < OPT_COUNT ? OPTS[index].key : nullptr; }

// Allocation size of a scene array that stage_scene may copy: its last 16-byte chunk is read whole, so the
// size is rounded up to 16 (hk_alias_entry is 8 bytes; an empty array keeps one zeroed element)
static size_t staged_alloc_bytes(size_t count, size_t elem) { return ((count ? count : 1) * elem + 15) & ~(size_t)15; }

// Stack bound of closest_hit_ordered for a scene (pushes along a path <= inner subtree starts on it): the inner
// levels of the TLAS plus those of the deepest instanced BLAS.  false: an instance's node range is outside the
// asset nodes.
static uint32_t flat_depth(const hk_node* f, uint32_t count)
{
    std::vector<uint32_t> dep(count + 1, 0);
    uint32_t best = 0;
    for (uint32_t p = count; p-- > 0;) {
        if (f[p].entry_index >= HK_BVH_LEAF_FLAG) continue;
        uint32_t q = f[p].exit_index;
        uint32_t dl = p + 1 < count ? dep[p + 1] : 0, dr = q < count && q + 1 < count ? dep[q + 1] : 0;
        dep[p] = 1 + (dl > dr ? dl : dr);
    }
    for (uint32_t p = 0; p < count; ++p) best = dep[p] > best ? dep[p] : best;
    return best;
}
static bool scene_stack_need(const hk_scene_desc* d, uint32_t* need, uint32_t* blas_depth_out)
{
    const uint32_t n_blas = d->asset_nodes.count, n_tlas = d->instance_nodes.count;
    const hk_instance* inst = (const hk_instance*)d->instances.data;
    const hk_node* blas = (const hk_node*)d->asset_nodes.data;
    const hk_node* tlas = (const hk_node*)d->instance_nodes.data;
    uint32_t blas_depth = 0;
    for (uint32_t k = 0; k < d->instances.count; ++k) {
        const hk_mesh_index& m = inst[k].mesh;
        if ((size_t)m.node[0] + m.node[1] > n_blas) return false;
        uint32_t dd = flat_depth(blas + m.node[0], m.node[1]);
        blas_depth = dd > blas_depth ? dd : blas_depth;
    }
    *need = flat_depth(tlas, n_tlas) + blas_depth;
    if (blas_depth_out) *blas_depth_out = blas_depth;
    return true;
}

// the nine arrays of a host scene and their counts, in array order
static std::array<const hk_array*, 9> desc_arrays(const hk_scene_desc* d)
{
    return {&d->vertices, &d->primitives, &d->asset_nodes, &d->alias_table, &d->instances,
            &d->instance_nodes, &d->materials, &d->emissive_nodes, &d->emissives};
}
static std::array<uint32_t, 9> desc_counts(const hk_scene_desc* d)
{
    std::array<uint32_t, 9> n;
    for (int i = 0; i < 9; ++i) n[i] = desc_arrays(d)[i]->count;
    return n;
}

static bool scene_desc_ok(const hk_scene_desc* d)
{
    for (const hk_array* a : desc_arrays(d))
        if (a->count && !a->data) return false;
    return true;
}

// the emissive of each material record, 4 floats each: what the host's emitter count reads (material_emits)
static std::vector<float> emissive_of(const hk_material* materials, uint32_t n)
{
    std::vector<float> e(4 * (size_t)n);
    for (uint32_t k = 0; k < n; ++k) std::memcpy(&e[4 * (size_t)k], materials[k].emissive, 16);
    return e;
}

// The registry of mesh slices (hk_ctx::meshes): where slice x stands in it (reg.size(): nowhere), and the deepest BLAS
// among the slices an instance carries
static size_t find_slice(const std::vector<hk_ctx::MeshSlice>& reg, const hk_mesh_index& x)
{
    size_t k = 0;
    while (k < reg.size() && std::memcmp(&reg[k].index, &x, sizeof(x)) != 0) ++k;
    return k;
}
static uint32_t used_depth(const std::vector<hk_ctx::MeshSlice>& reg)
{
    uint32_t depth = 0;
    for (const hk_ctx::MeshSlice& s : reg)
        if (s.used) depth = std::max(depth, s.depth);
    return depth;
}

// A mesh slice of a host-built scene as hk_update_meshes and hk_set_instances keep it: the vertices its primitives
// index and its BLAS depth (the node range is inside the asset nodes)
static hk_ctx::MeshSlice host_mesh_slice(const hk_scene_desc* d, const hk_mesh_index& m)
{
    hk_ctx::MeshSlice s{m, HK_U32_MAX, flat_depth((const hk_node*)d->asset_nodes.data + m.node[0], m.node[1])};
    const uint32_t tris = (m.node[1] + 2u) / 3u;
    if (m.node[1] && (m.node[1] + 2u) % 3u == 0 && (size_t)m.primitive + tris <= d->primitives.count &&
        m.vertex < d->vertices.count) {
        const hk_primitive* pr = (const hk_primitive*)d->primitives.data + m.primitive;
        uint32_t top = 0;
        for (uint32_t t = 0; t < tris; ++t)
            for (int v = 0; v < 3; ++v) top = std::max(top, pr[t].vertices[v].index);
        if (top < d->vertices.count - m.vertex) s.vertex_need = top + 1u;
    }
    return s;
}

// The registry of a host-built scene: the distinct slices its instances carry, in the order of their first use, each
// with the instances that carry it.  false: an instance's node range is outside the asset nodes.
static bool host_registry(const hk_scene_desc* d, std::vector<hk_ctx::MeshSlice>* reg)
{
    const hk_instance* inst = (const hk_instance*)d->instances.data;
    reg->clear();
    for (uint32_t k = 0; k < d->instances.count; ++k) {
        const hk_mesh_index& m = inst[k].mesh;
        if ((size_t)m.node[0] + m.node[1] > d->asset_nodes.count) return false;
        const size_t at = find_slice(*reg, m);
        if (at == reg->size()) reg->push_back(host_mesh_slice(d, m));
        (*reg)[at].used++;
    }
    return true;
}

int hk_scene_stage_bytes(const hk_scene_desc* d, int plan, uint32_t* bytes, uint32_t* limit)
{
    if (!d || (plan != PLAN_LIGHT && plan != PLAN_GBUFFER)) return HK_ERR_INVALID;
    uint32_t b[SCENE_ARRAYS];
    scene_array_bytes(desc_counts(d).data(), b);
    if (bytes) *bytes = stage_bytes(b, plan);
    if (limit) *limit = LDS_SCENE_MAX;
    return HK_OK;
}

int hk_scene_indirect_lds(const hk_scene_desc* d, uint32_t* stash, uint32_t* total, uint32_t* limit)
{
    uint32_t scene = 0;
    const int rc = hk_scene_stage_bytes(d, PLAN_LIGHT, &scene, nullptr);
    if (rc != HK_OK) return rc;
    const bool staged = scene <= LDS_SCENE_MAX;
    const uint32_t s = indirect_stash_bytes();
    if (stash) *stash = s;
    if (total) *total = (staged ? scene : 0u) + s;
    if (limit) *limit = LDS_WORKGROUP_MAX;
    return HK_OK;
}

int hk_scene_gbuffer_stack(const hk_scene_desc* d, uint32_t* need, uint32_t* lds_levels)
{
    if (!d || !scene_desc_ok(d)) return HK_ERR_INVALID;
    uint32_t n = 0;
    if (!scene_stack_need(d, &n, nullptr)) return HK_ERR_INVALID;
    if (need) *need = n;
    if (lds_levels) *lds_levels = (uint32_t)GB_STACK_LDS;
    return HK_OK;
}

// The buffers that are sized by a scene array's capacity beside the array itself: bytes per element of cap[array], and
// the byte a new one is filled with (FOLLOWER_AUX, the three rows of blas_aux at stride cap[2]: U32_MAX behind the
// registered nodes).  follower_slot: where the context keeps follower k.
struct Follower {
    int array;
    size_t bytes;
    int fill;
};
constexpr Follower FOLLOWERS[] = {{2, WIDE_NODE_BYTES, 0}, {2, sizeof(hk_node), 0}, {2, 12, 0xFF},
                                  {5, WIDE_NODE_BYTES, 0}, {5, sizeof(hk_node), 0}, {4, 64, 0}};
constexpr int N_FOLLOWERS = sizeof(FOLLOWERS) / sizeof(FOLLOWERS[0]), FOLLOWER_AUX = 2;
static void** follower_slot(hk_ctx* c, int k)
{
    void** slot[N_FOLLOWERS] = {(void**)&c->blas_wide, (void**)&c->walk_nodes[0], (void**)&c->blas_aux,
                                (void**)&c->tlas_wide, (void**)&c->walk_nodes[1], (void**)&c->prev_models};
    return slot[k];
}

// device-only derivatives of the asset nodes, over the whole array of n_blas nodes: leaf boxes, the G-buffer wide layout
// and the light walks' copy, leaf-collapsed (k_collapse_decide); the array itself stays as it is (hk_read_scene_array,
// the wide layout and the instance rebuild read it)
static void refresh_blas_derivatives(hk_ctx* c, hipStream_t st, uint32_t n_blas)
{
    launch_fill_leaves((hk_node*)c->buf[2], n_blas, c->blas_aux, (const hk_primitive*)c->buf[1], nullptr, 0, nullptr, 0,
                       st);
    launch_build_wide((const hk_node*)c->buf[2], n_blas, c->blas_aux + c->aux_stride, c->blas_aux + 2 * c->aux_stride,
                      c->blas_wide, st);
    (void)hipMemcpyAsync(c->walk_nodes[0], c->buf[2], (size_t)n_blas * sizeof(hk_node), hipMemcpyDeviceToDevice, st);
    if (c->on(OPT_LEAF_COLLAPSE))
        launch_collapse_leaves(c->walk_nodes[0], n_blas, c->blas_aux + c->aux_stride, c->blas_aux + 2 * c->aux_stride,
                               c->collapse_scratch, st);
}
// the same of the TLAS, over the current instances and instance nodes
static void refresh_tlas_derivatives(hk_ctx* c, hipStream_t st)
{
    const uint32_t n_tlas = c->count[5];
    launch_fill_leaves(nullptr, 0, nullptr, nullptr, (hk_node*)c->buf[5], n_tlas, (const hk_instance*)c->buf[4],
                       c->count[4], st);
    launch_build_wide((const hk_node*)c->buf[5], n_tlas, nullptr, nullptr, c->tlas_wide, st);
    (void)hipMemcpyAsync(c->walk_nodes[1], c->buf[5], (size_t)n_tlas * sizeof(hk_node), hipMemcpyDeviceToDevice, st);
    if (c->on(OPT_LEAF_COLLAPSE))
        launch_collapse_leaves(c->walk_nodes[1], n_tlas, nullptr, nullptr, c->collapse_scratch, st);
}

// The rows of the per-node mesh tables (blas_aux: primitive offset, node base, node count) over the node ranges of
// `list`, in list order, on `st`: one copy per row and run of slices whose node ranges follow one another.  rows: the
// host side of the copies, which the caller keeps past the call's wait.
static int write_mesh_rows(hk_ctx* c, const hk_mesh_index* list, size_t n, hipStream_t st, std::vector<uint32_t>* rows)
{
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) total += list[k].node[1];
    rows->resize(3 * total);
    for (size_t k = 0, at = 0; k < n; at += list[k++].node[1]) {
        const uint32_t value[3] = {list[k].primitive, list[k].node[0], list[k].node[1]};
        for (size_t r = 0; r < 3; ++r) std::fill_n(rows->begin() + r * total + at, list[k].node[1], value[r]);
    }
    for (size_t k = 0, at = 0; k < n;) {
        size_t end = k, len = 0;
        do len += list[end++].node[1];
        while (end < n && list[end].node[0] == list[end - 1].node[0] + list[end - 1].node[1]);
        for (size_t r = 0; r < 3 && len; ++r)
            HK_HIP(c, hipMemcpyAsync(c->blas_aux + r * c->aux_stride + list[k].node[0], rows->data() + r * total + at,
                                     len * 4, hipMemcpyHostToDevice, st));
        at += len;
        k = end;
    }
    return HK_OK;
}

int hk_scene_upload(hk_ctx* c, const hk_scene_desc* d)
{
    if (!c || !d) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    HK_TRY(c->sch.gb_serialize(true));
    const std::array<const hk_array*, 9> arr = desc_arrays(d);
    const size_t* elem = SCENE_ELEM;
    if (d->instances.count == 0 || d->materials.count == 0)
        return fail(c, HK_ERR_INVALID, "scene needs at least one instance and one material");
    c->gen++;
    c->shared_transform = false;
    c->scene_box_valid = false;
    if (!scene_desc_ok(d)) return fail(c, HK_ERR_INVALID, "scene array with count but no data");
    HK_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i) {
        release(c->spare[i]);
        c->spare_cap[i] = 0;
    }
    for (int i = 0; i < 9; ++i) {
        release(c->buf[i]);
        size_t bytes = staged_alloc_bytes(arr[i]->count, elem[i]);
        HK_HIP(c, hipMalloc(&c->buf[i], bytes));
        HK_HIP(c, hipMemset(c->buf[i], 0, bytes));
        if (arr[i]->count) HK_HIP(c, hipMemcpy(c->buf[i], arr[i]->data, arr[i]->count * elem[i], hipMemcpyHostToDevice));
        c->count[i] = arr[i]->count;
        c->cap[i] = arr[i]->count ? arr[i]->count : 1;
    }
    c->emissive = emissive_of((const hk_material*)d->materials.data, d->materials.count);
    c->skins.clear();  // (the slices are another scene's; the streams keep their capacity)
    c->morphs.clear();
    // the instanced meshes: each distinct slice once, with the vertices its primitives index and its BLAS depth
    // (gb_blas_depth is the maximum of these)
    if (!host_registry(d, &c->meshes)) return fail(c, HK_ERR_INVALID, "instance mesh node range outside asset nodes");
    // BLAS node -> primitive offset / node range of the mesh that owns it (k_fill_blas_leaves, k_build_wide), from the
    // instances' mesh indices: in instance order, so that the last instance wins where host-built slices overlap
    const uint32_t n_blas = d->asset_nodes.count, n_tlas = d->instance_nodes.count;
    std::vector<uint32_t> prim_offset(n_blas, HK_U32_MAX), node_base(n_blas, HK_U32_MAX), node_count(n_blas, 0);
    const hk_instance* inst = (const hk_instance*)d->instances.data;
    for (uint32_t k = 0; k < d->instances.count; ++k) {
        const hk_mesh_index& m = inst[k].mesh;
        for (uint32_t j = 0; j < m.node[1]; ++j) {
            prim_offset[m.node[0] + j] = m.primitive;
            node_base[m.node[0] + j] = m.node[0];
            node_count[m.node[0] + j] = m.node[1];
        }
    }
    (void)scene_stack_need(d, &c->gb_stack_need, &c->gb_blas_depth);  // (node ranges checked above)
    c->gb_tlas_depth = c->gb_stack_need - c->gb_blas_depth;
    release(c->dyn_scratch);
    c->dyn_bytes = 0;
    release(c->mesh_scratch);
    c->mesh_bytes = 0;
    // (the wide layouts and the walk-node copies are 64 and 32 bytes per node: whole 16-byte chunks for stage_scene
    // without rounding)
    for (int k = 0; k < N_FOLLOWERS; ++k) {
        release(*follower_slot(c, k));
        HK_HIP(c, hipMalloc(follower_slot(c, k), c->cap[FOLLOWERS[k].array] * FOLLOWERS[k].bytes));
    }
    release(c->collapse_scratch);
    c->collapse_cap = std::max<uint32_t>(1u, std::max(n_blas, n_tlas));
    HK_HIP(c, hipMalloc(&c->collapse_scratch, c->collapse_cap * 4));
    const size_t stride = c->aux_stride = c->cap[2];
    if (n_blas) {
        HK_HIP(c, hipMemcpy(c->blas_aux, prim_offset.data(), (size_t)n_blas * 4, hipMemcpyHostToDevice));
        HK_HIP(c, hipMemcpy(c->blas_aux + stride, node_base.data(), (size_t)n_blas * 4, hipMemcpyHostToDevice));
        HK_HIP(c, hipMemcpy(c->blas_aux + 2 * stride, node_count.data(), (size_t)n_blas * 4, hipMemcpyHostToDevice));
    }
    refresh_blas_derivatives(c, c->stream, n_blas);
    refresh_tlas_derivatives(c, c->stream);
    HK_HIP(c, hipGetLastError());
    // previous models = the uploaded ones (GlobalTransformQueue([matrix; 2]) for a new entity)
    HK_HIP(c, hipMemcpy2DAsync(c->prev_models, 64, (const char*)c->buf[4] + offsetof(hk_instance, model),
                               sizeof(hk_instance), 64, d->instances.count, hipMemcpyDeviceToDevice, c->stream));
    c->models_dirty = false;
    HK_HIP(c, hipStreamSynchronize(c->stream));
    {   // what the walks read: the records' inverse_transpose_model
        std::vector<float> itm(16 * (size_t)d->instances.count);
        for (uint32_t k = 0; k < d->instances.count; ++k) std::memcpy(&itm[16 * (size_t)k], inst[k].inverse_transpose_model, 64);
        c->shared_transform = hks_shared_transform(itm.data(), d->instances.count) != 0;
    }
    {   // the world box of the instances (background tile skip): their records' boxes, which the TLAS leaves carry
        double* b = c->scene_box;
        for (int a = 0; a < 3; ++a) {
            b[a] = INFINITY;
            b[3 + a] = -INFINITY;
        }
        c->scene_box_valid = true;
        for (uint32_t k = 0; k < d->instances.count; ++k)
            for (int a = 0; a < 3; ++a) {
                c->scene_box_valid &= std::isfinite(inst[k].min[a]) && std::isfinite(inst[k].max[a]);
                b[a] = std::fmin(b[a], (double)inst[k].min[a]);
                b[3 + a] = std::fmax(b[3 + a], (double)inst[k].max[a]);
            }
    }
    c->has_scene = true;
    return HK_OK;
}

// The BLAS levels hk_update_meshes rebuilt, read back in the instance rebuild's one wait
struct MeshLevels {
    const uint32_t* device;
    std::vector<uint32_t> slice;  // c->meshes index of each listed mesh
};

// What hk_set_instances decided on the host before the rebuild (plan_instance_set): the new set, the nine counts
// after it, and the mesh slice each instance carries
struct SetChange {
    const hk_instance_desc* set = nullptr;
    const hk_material* materials = nullptr;  // all count[6] records, or null: the materials stay
    uint32_t counts[9] = {};
    std::vector<uint32_t> slice;             // per instance: its index in the known slices followed by `fresh`
    std::vector<hk_ctx::MeshSlice> fresh;    // the slices to register, in the order of their first use
};

// Where the host arithmetic reads a slice's primitives and nodes: a host-built scene, or a context's device arrays
struct SliceReader {
    const hk_scene_desc* desc;
    const hk_ctx* ctx;
    bool read(int array, uint32_t first, uint32_t n, void* dst) const
    {
        const size_t elem = SCENE_ELEM[array], at = (size_t)first * elem, bytes = (size_t)n * elem;
        if (desc) {
            std::memcpy(dst, (const char*)(array == 1 ? desc->primitives.data : desc->asset_nodes.data) + at, bytes);
            return true;
        }
        return hipMemcpy(dst, (const char*)ctx->buf[array] + at, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
};

static bool ranges_meet(size_t a, size_t na, size_t b, size_t nb) { return a < b + nb && b < a + na; }

// A slice's shape against the array counts (check_new_slice, and hk_set_meshes for a kept slice); null: it fits
static const char* slice_shape_error(const hk_mesh_index& x, const uint32_t* count)
{
    const uint32_t nc = x.node[1], k = (nc + 2u) / 3u;
    if (nc == 0 || (nc + 2u) % 3u != 0) return "its BLAS is not 3k - 2 nodes over k primitives";
    if ((size_t)x.primitive + k > count[1]) return "its primitives reach past the primitive array";
    if ((size_t)x.node[0] + nc > count[2]) return "its nodes reach past the asset nodes";
    if (x.vertex >= count[0]) return "its vertices begin past the vertex array";
    return nullptr;
}

// A slice no instance has carried so far (hikari_amd.h hk_set_instances "mesh"): its shape against the array counts,
// against every slice known so far, and what upload records for an instanced mesh.  `why` says what failed.
static int check_new_slice(const hk_mesh_index& x, const uint32_t* count, const std::vector<hk_ctx::MeshSlice>& known,
                           const std::vector<hk_ctx::MeshSlice>& fresh, const SliceReader& rd, hk_ctx::MeshSlice* out,
                           std::string* why)
{
    const uint32_t nc = x.node[1], k = (nc + 2u) / 3u;
    auto no = [&](const char* text) {
        *why = text;
        return HK_ERR_INVALID;
    };
    if (const char* shape = slice_shape_error(x, count)) return no(shape);
    for (const std::vector<hk_ctx::MeshSlice>* list : {&known, &fresh})
        for (const hk_ctx::MeshSlice& o : *list)
            if (ranges_meet(x.primitive, k, o.index.primitive, (o.index.node[1] + 2u) / 3u) ||
                ranges_meet(x.node[0], nc, o.index.node[0], o.index.node[1]))
                return no("it partly overlaps another mesh slice");
    std::vector<hk_primitive> prims(k);
    std::vector<hk_node> nodes(nc);
    if (!rd.read(1, x.primitive, k, prims.data()) || !rd.read(2, x.node[0], nc, nodes.data())) {
        *why = "its primitives and nodes could not be read back";
        return HK_ERR_HIP;
    }
    uint32_t top = 0;
    for (const hk_primitive& p : prims)
        for (int v = 0; v < 3; ++v) top = std::max(top, p.vertices[v].index);
    if (top >= count[0] - x.vertex) return no("its vertex indices reach past the vertex array");
    for (const std::vector<hk_ctx::MeshSlice>* list : {&known, &fresh})
        for (const hk_ctx::MeshSlice& o : *list)
            if (o.vertex_need != HK_U32_MAX && ranges_meet(x.vertex, top + 1u, o.index.vertex, o.vertex_need))
                return no("its vertices overlap another mesh slice's");
    *out = hk_ctx::MeshSlice{x, top + 1u, flat_depth(nodes.data(), nc)};
    return HK_OK;
}

// hks_build's emitter test (hk_scene.cpp: 255 a |rgb| > 0 in float; false for a NaN), as k_set_instances evaluates it
static bool material_emits(const float* e)
{
    const float intensity = (255.0f * e[3]) * std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    return intensity > 0.0f;
}

// The host arithmetic of a new instance set: every refusal that needs no device, the slices to register and the nine
// counts after the set (count: the counts before; emissive: 4 floats per material).  closed: `known` is every slice
// there is (hk_set_meshes' new list), so an unknown one is refused, not registered.
static int plan_instance_set(const uint32_t* count, const std::vector<hk_ctx::MeshSlice>& known, const float* emissive,
                             const hk_instance_desc* set, uint32_t n, const SliceReader& rd, SetChange* out,
                             std::string* why, bool closed = false)
{
    if (n == 0) {
        *why = "an empty instance set (hk_scene_upload refuses an empty scene too)";
        return HK_ERR_INVALID;
    }
    if (n > 0x20000000u) {
        *why = "too many instances";
        return HK_ERR_INVALID;
    }
    out->set = set;
    out->slice.resize(n);
    out->fresh.clear();
    uint64_t n_em = 0, n_alias = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const hk_instance_desc& d = set[i];
        const std::string who = "instance " + std::to_string(i) + ": ";
        if (d.material >= count[6]) {
            *why = who + "material index out of range";
            return HK_ERR_INVALID;
        }
        size_t at = find_slice(known, d.mesh);
        if (at == known.size()) at += find_slice(out->fresh, d.mesh);
        if (at == known.size() + out->fresh.size() && closed) {
            *why = who + "its mesh is not in the new list";
            return HK_ERR_INVALID;
        }
        if (at == known.size() + out->fresh.size()) {
            hk_ctx::MeshSlice f;
            std::string text;
            const int rc = check_new_slice(d.mesh, count, known, out->fresh, rd, &f, &text);
            if (rc != HK_OK) {
                *why = who + "mesh slice refused: " + text;
                return rc;
            }
            out->fresh.push_back(f);
        }
        out->slice[i] = (uint32_t)at;
        if (material_emits(emissive + 4 * (size_t)d.material)) {
            n_em++;
            n_alias += (d.mesh.node[1] + 2u) / 3u;
        }
    }
    if (n_alias > 0x40000000u) {
        *why = "too many alias entries";
        return HK_ERR_INVALID;
    }
    std::memcpy(out->counts, count, sizeof(out->counts));
    out->counts[3] = (uint32_t)n_alias;
    out->counts[4] = n;
    out->counts[5] = 3u * n - 2u;
    out->counts[7] = n_em ? 3u * (uint32_t)n_em - 2u : 0u;
    out->counts[8] = (uint32_t)n_em;
    return HK_OK;
}

// Device buffers that are freed when the scope that holds them ends
struct Buffers {
    std::vector<void*> p;
    ~Buffers()
    {
        for (void* q : p) (void)hipFree(q);
    }
};

// Room for the counts after a call (hikari_amd.h "Capacity" of hk_set_instances, hk_add_meshes and hk_set_meshes), on
// `st` ahead of the kernels that write the arrays.  grow: the arrays (bits) that may be allocated anew, each only when
// its count passes its capacity, and then at max(count, 1.5 x capacity), with the buffers that follow it
// (FOLLOWERS); collapse_scratch by the same rule, mesh_scratch and dyn_scratch to the bytes asked for.  keep: the
// arrays (bits) whose contents move into a new buffer; of the others a new buffer is zeroed whole and one that stays
// gets staged_alloc_bytes' zeroed tail behind its new count, their records being rewritten by the caller's kernels.
// spares: arrays 0-2 are written out of place (hk_set_meshes): each gets its spare, allocated anew only where it is
// smaller than the capacity asked for, and zeroed behind the new count; the array it was becomes the spare
// (c->spare[i] afterwards: where the kernels read the old contents).
// First every allocation, with the context untouched: a failure frees them and leaves the context as it was.  Then
// the pointers, so that nothing allocated is lost on a failed enqueue, then the fills and copies.  The buffers that
// were replaced go to `old`, which the caller holds past the call's wait: work in flight, and a gather of the
// previous models as they were (prev_models), may still read them.
static int reserve_scene(hk_ctx* c, const char* who, const uint32_t* counts, uint32_t grow, uint32_t keep, bool spares,
                         size_t mesh_need, size_t dyn_need, hipStream_t st, Buffers* old)
{
    Buffers fresh;
    bool ok = true;
    auto grown = [](size_t need, size_t cap) { return std::max(need, cap + cap / 2); };
    auto alloc = [&](size_t bytes) -> void* {
        void* nb = nullptr;
        ok = ok && hipMalloc(&nb, bytes) == hipSuccess;
        if (ok) fresh.p.push_back(nb);
        return nb;
    };
    size_t cap[9];
    void *nbuf[9] = {}, *nfol[N_FOLLOWERS] = {};
    for (int i = 0; i < 9; ++i) {
        cap[i] = c->cap[i];
        if (!(grow >> i & 1u)) continue;
        if (counts[i] > cap[i]) cap[i] = grown(counts[i], cap[i]);
        const bool spare = spares && i < 3;
        if (spare && c->spare_cap[i] >= cap[i]) cap[i] = c->spare_cap[i];
        else if (spare || cap[i] != c->cap[i]) nbuf[i] = alloc(staged_alloc_bytes(cap[i], SCENE_ELEM[i]));
    }
    for (int k = 0; k < N_FOLLOWERS; ++k) {
        const Follower& f = FOLLOWERS[k];
        if (cap[f.array] != c->cap[f.array]) nfol[k] = alloc(cap[f.array] * f.bytes);
    }
    const size_t collapse_need = std::max<size_t>(1, std::max(counts[2], counts[5]));
    const size_t collapse_cap = collapse_need > c->collapse_cap ? grown(collapse_need, c->collapse_cap) : c->collapse_cap;
    void* n_collapse = collapse_cap != c->collapse_cap ? alloc(collapse_cap * 4) : nullptr;
    void* n_mesh = c->mesh_bytes < mesh_need ? alloc(mesh_need) : nullptr;
    void* n_dyn = c->dyn_bytes < dyn_need ? alloc(dyn_need) : nullptr;
    if (!ok) return fail(c, HK_ERR_HIP, std::string(who) + ": out of device memory");
    fresh.p.clear();  // (all of them go into the context below)
    auto put = [&](void** slot, void* nb) {
        if (*slot) old->p.push_back(*slot);
        *slot = nb;
    };
    const void *buf_was[9], *fol_was[N_FOLLOWERS];
    for (int i = 0; i < 9; ++i) {
        buf_was[i] = c->buf[i];
        if (spares && i < 3 && (grow >> i & 1u)) {
            if (nbuf[i]) {
                put(&c->spare[i], nbuf[i]);
                c->spare_cap[i] = cap[i];
            }
            std::swap(c->buf[i], c->spare[i]);
            std::swap(c->cap[i], c->spare_cap[i]);
        } else if (nbuf[i]) {
            put(&c->buf[i], nbuf[i]);
            c->cap[i] = cap[i];
        }
    }
    for (int k = 0; k < N_FOLLOWERS; ++k) {
        fol_was[k] = *follower_slot(c, k);
        if (nfol[k]) put(follower_slot(c, k), nfol[k]);
    }
    const size_t stride_was = c->aux_stride;
    c->aux_stride = c->cap[2];
    if (n_collapse) {
        put((void**)&c->collapse_scratch, n_collapse);
        c->collapse_cap = collapse_cap;
    }
    if (n_mesh) {
        put(&c->mesh_scratch, n_mesh);
        c->mesh_bytes = mesh_need;
    }
    if (n_dyn) {
        put(&c->dyn_scratch, n_dyn);
        c->dyn_bytes = dyn_need;
    }
    for (int i = 0; i < 9; ++i) {
        if (!(grow >> i & 1u)) continue;
        const bool kept = keep >> i & 1u;
        const size_t have = (size_t)c->count[i] * SCENE_ELEM[i];
        // staged_alloc_bytes' tail behind the new count reads zero (an empty array keeps one zeroed element): of a
        // buffer that is new to the array, all that is behind the count
        const bool swapped = nbuf[i] || (spares && i < 3);
        const size_t end = staged_alloc_bytes(swapped ? c->cap[i] : counts[i], SCENE_ELEM[i]);
        const size_t at = nbuf[i] ? 0 : kept ? end : (size_t)counts[i] * SCENE_ELEM[i];
        if (end > at) HK_HIP(c, hipMemsetAsync((char*)c->buf[i] + at, 0, end - at, st));
        if (nbuf[i] && kept && have) HK_HIP(c, hipMemcpyAsync(nbuf[i], buf_was[i], have, hipMemcpyDeviceToDevice, st));
    }
    for (int k = 0; k < N_FOLLOWERS; ++k) {
        const Follower& f = FOLLOWERS[k];
        if (!nfol[k]) continue;
        HK_HIP(c, hipMemsetAsync(nfol[k], f.fill, c->cap[f.array] * f.bytes, st));
        const size_t have = keep >> f.array & 1u ? c->count[f.array] : 0;
        if (!have) continue;
        if (k != FOLLOWER_AUX) HK_HIP(c, hipMemcpyAsync(nfol[k], fol_was[k], have * f.bytes, hipMemcpyDeviceToDevice, st));
        for (size_t r = 0; r < 3 && k == FOLLOWER_AUX; ++r)  // the per-node mesh tables, re-laid at the new stride
            HK_HIP(c, hipMemcpyAsync((uint32_t*)nfol[k] + r * c->aux_stride, (const uint32_t*)fol_was[k] + r * stride_was,
                                     have * 4, hipMemcpyDeviceToDevice, st));
    }
    return HK_OK;
}

// A scratch block carved into parts of the given bytes, each rounded up to 256: the bytes they take together, and the
// parts' pointers in *scratch, which is allocated anew (to exactly that) where it holds fewer than that
static size_t carve_bytes(const size_t* bytes, int n)
{
    size_t total = 0;
    for (int k = 0; k < n; ++k) total += (bytes[k] + 255) & ~(size_t)255;
    return total;
}
static int carve(hk_ctx* c, void** scratch, size_t* have, const size_t* bytes, int n, char** part)
{
    const size_t total = carve_bytes(bytes, n);
    if (*have < total) {
        release(*scratch);
        *have = 0;
        HK_HIP(c, hipMalloc(scratch, total));
        *have = total;
    }
    char* p = (char*)*scratch;
    for (int k = 0; k < n; ++k) {
        part[k] = p;
        p += carve_bytes(bytes + k, 1);
    }
    return HK_OK;
}

// The instance rebuild on `st` (after the mesh rebuild of hk_update_meshes, if any) and its one wait: the one body of
// hk_update_instances, hk_update_meshes and hk_set_instances.  set: the new instance set that replaces the current one
// (null: the current set with new models).  mesh_work (hk_skin_meshes): what the caller enqueues on `st` between the
// uploads and the instance kernels, given the device copy of local_aabbs, whose rows it may overwrite.  ml with no
// slices (a refit): meshes changed and no depth did.
// refit (hk_refit_instances and the _all calls; never with a set, whose topology is another): the TLAS and
// the light BVH keep their trees and get new boxes by include/hk_refit.h's rule, in place of the two builds and the
// backfill.  No TLAS is built, so nobody writes flags[1]: the TLAS depth is the context's, which a build alone moves.
// Everything else, the one wait included, is the rebuilding call's.
static int rebuild_instances(hk_ctx* c, const float* models, const float* local_aabbs, uint32_t count, hipStream_t st,
                             const MeshLevels* ml, const SetChange* set = nullptr,
                             const std::function<void(float*)>* mesh_work = nullptr, bool refit = false)
{
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.gb_serialize(false));
    const uint32_t* counts = set ? set->counts : c->count;
    const uint32_t n = count, m = counts[8], n_alias = counts[3];
    const uint32_t nm = n > m ? n : m;
    const size_t ns = set ? n : 0;  // (scratch of a set change only)
    const size_t sz[] = {(size_t)n * 64, (size_t)n * 24, (size_t)(n_alias ? n_alias : 1) * 4,
                         (size_t)(n_alias ? n_alias : 1) * 16, (size_t)nm * 24, (size_t)nm * 8, (size_t)nm * 24,
                         (size_t)3 * n * 4, 16, ns * sizeof(InstanceDesc), ns * 64, ns * 8};
    constexpr int PARTS = sizeof(sz) / sizeof(sz[0]);
    // what reserve_scene replaced, freed on every way out: the gather reads the previous models of the set before
    // where they were
    Buffers old;
    const float* prev_before = c->prev_models;
    const uint32_t n_before = c->count[4];
    std::vector<uint32_t> rows;  // (write_mesh_rows' host side, alive past the wait)
    if (set)  // (first, so that a failed allocation leaves the context as it was)
        HK_TRY(reserve_scene(c, "hk_set_instances", counts, 1u << 3 | 1u << 4 | 1u << 5 | 1u << 7 | 1u << 8, 0, false, 0,
                             carve_bytes(sz, PARTS), st, &old));
    c->gen++;
    c->shared_transform = false;  // (the general walks, should this call fail half-way)
    c->scene_box_valid = false;   // (likewise: no tile skip)
    if (set) {
        if (!set->fresh.empty()) {  // register the new slices: their rows of the per-node mesh tables, then the derivatives
            std::vector<hk_mesh_index> list;
            for (const hk_ctx::MeshSlice& f : set->fresh) {
                list.push_back(f.index);
                c->meshes.push_back(f);
            }
            HK_TRY(write_mesh_rows(c, list.data(), list.size(), st, &rows));
            refresh_blas_derivatives(c, st, c->count[2]);
        }
        for (hk_ctx::MeshSlice& s : c->meshes) s.used = 0;
        for (uint32_t k : set->slice) c->meshes[k].used++;
        c->gb_blas_depth = used_depth(c->meshes);
        for (int i : {3, 4, 5, 7, 8}) c->count[i] = counts[i];
        if (set->materials) {
            c->emissive = emissive_of(set->materials, c->count[6]);
            HK_HIP(c, hipMemcpyAsync(c->buf[6], set->materials, (size_t)c->count[6] * sizeof(hk_material),
                                     hipMemcpyHostToDevice, st));
        }
    }
    char* part[PARTS];
    HK_TRY(carve(c, &c->dyn_scratch, &c->dyn_bytes, sz, PARTS, part));
    HK_HIP(c, hipMemcpyAsync(part[0], models, (size_t)n * 64, hipMemcpyHostToDevice, st));
    HK_HIP(c, hipMemcpyAsync(part[1], local_aabbs, (size_t)n * 24, hipMemcpyHostToDevice, st));
    HK_HIP(c, hipMemsetAsync(part[8], 0, 16, st));
    if (set) HK_HIP(c, hipMemcpyAsync(part[9], set->set, (size_t)n * sizeof(InstanceDesc), hipMemcpyHostToDevice, st));
    if (mesh_work) (*mesh_work)((float*)part[1]);
    DynamicArgs D;
    D.instances = (hk_instance*)c->buf[4];
    D.n_instances = n;
    D.models = (const float*)part[0];
    D.local_aabbs = (const float*)part[1];
    D.tlas = (hk_node*)c->buf[5];
    D.emissives = (hk_emissive*)c->buf[8];
    D.n_emissives = m;
    D.materials = (const hk_material*)c->buf[6];
    D.primitives = (const hk_primitive*)c->buf[1];
    D.alias = (hk_alias_entry*)c->buf[3];
    D.n_alias = n_alias;
    D.lbvh = (hk_node*)c->buf[7];
    D.buckets = 6;  // bvh 0.7.1 NUM_BUCKETS (hks_build default)
    D.areas = (float*)part[2];
    D.alias_work = part[3];
    D.boxes = part[4];
    D.idx = (uint32_t*)part[5];
    D.segments = part[6];
    D.flags = (uint32_t*)part[8];
    SetArgs S;
    S.set = (const InstanceDesc*)part[9];
    S.prev_models = prev_before;
    S.n_prev = n_before;
    S.new_prev = (float*)part[10];
    S.emitter = (uint2*)part[11];
    // (the spans inside the call's own: one per launch, the same launches in the same order as launch_dynamic_update)
    auto step = [&](const char* name, DynamicStep s) { timed(c, name, st, [&] { launch_dynamic_step(D, s, st); }); };
    timed(c, set ? "set_instances" : refit ? "refit_instances" : "update_instances", st, [&] {
        if (set) {
            launch_set_instances(D, S, st);
            (void)hipMemcpyAsync(c->prev_models, S.new_prev, (size_t)n * 64, hipMemcpyDeviceToDevice, st);
        } else {
            step("instances.records", DYN_RECORDS);
            if (!refit) step("instances.tlas_build", DYN_TLAS_BUILD);
            step("instances.emissive_areas", DYN_EMISSIVE_AREAS);
            step("instances.emissives", DYN_EMISSIVES);
            if (refit) {
                step("instances.refit_small", DYN_REFIT_SMALL);
                step("instances.refit_large", DYN_REFIT_LARGE);
            } else {
                step("instances.lbvh_build", DYN_LBVH_BUILD);
                step("instances.backfill", DYN_BACKFILL);
            }
        }
        timed(c, "instances.derivatives", st, [&] { refresh_tlas_derivatives(c, st); });
    });
    HK_HIP(c, hipGetLastError());
    uint32_t flags[4] = {0, 0, 0, 0};
    std::vector<uint32_t> levels(ml ? ml->slice.size() : 0);
    HK_HIP(c, hipMemcpyAsync(flags, part[8], 16, hipMemcpyDeviceToHost, st));
    if (!levels.empty())
        HK_HIP(c, hipMemcpyAsync(levels.data(), ml->device, levels.size() * 4, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    if (ml) {  // the deepest instanced BLAS now: a mesh that became shallower lowers the bound
        for (size_t k = 0; k < levels.size(); ++k) c->meshes[ml->slice[k]].depth = levels[k];
        c->gb_blas_depth = used_depth(c->meshes);
    }
    if (!refit) c->gb_tlas_depth = flags[1];
    if (ml || set) c->gb_stack_need = c->gb_tlas_depth + c->gb_blas_depth;
    if (set && (flags[2] != m || flags[3] != n_alias))
        return fail(c, HK_ERR_HIP, "hk_set_instances: the device counted " + std::to_string(flags[2]) + " emitters and " +
                                       std::to_string(flags[3]) + " alias entries, the host " + std::to_string(m) +
                                       " and " + std::to_string(n_alias));
    if (flags[0]) return fail(c, HK_ERR_INVALID, "singular instance transform");
    c->gb_stack_need = c->gb_tlas_depth + c->gb_blas_depth;
    c->models_dirty = true;  // the next G-buffer reads the models before this update as the previous ones
    // one kernel derives every record's inverse_transpose_model from its model with the same code: equal model bits
    // give equal record bits
    c->shared_transform = hks_shared_transform(models, n) != 0;
    // the instances' world box from what the device derived their boxes from; after a mesh rebuild the local boxes
    // are the caller's word about vertices the host has not looked at, so the box stays unknown (no tile skip) until
    // the next instance update or upload
    c->scene_box_valid = !ml && hks_instance_bounds(models, local_aabbs, n, c->scene_box) != 0;
    return HK_OK;
}

// the TLAS and the light BVH are 3n - 2 nodes over their n leaves, as the device builds them
static int scene_rebuildable(hk_ctx* c)
{
    if (c->count[5] != 3u * c->count[4] - 2u || (c->count[8] && c->count[7] != 3u * c->count[8] - 2u))
        return fail(c, HK_ERR_STATE, "scene BVHs are not bvh-0.7.1 flattened (3n - 2 nodes); cannot rebuild");
    return HK_OK;
}

// the checks hk_update_instances and hk_update_meshes share; HK_OK: the scene can be rebuilt with `count` instances
static int update_args_ok(hk_ctx* c, uint32_t count, const char* who)
{
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (count != c->count[4]) return fail(c, HK_ERR_INVALID, std::string(who) + " needs every instance, in upload order");
    return scene_rebuildable(c);
}

int hk_update_instances(hk_ctx* c, const float* models, const float* local_aabbs, uint32_t count, void* stream)
{
    if (!c || !models || !local_aabbs) return HK_ERR_INVALID;
    HK_TRY(update_args_ok(c, count, "hk_update_instances"));
    (void)hipSetDevice(c->device);
    return rebuild_instances(c, models, local_aabbs, count, pick(c, stream), nullptr);
}
int hk_refit_instances(hk_ctx* c, const float* models, const float* local_aabbs, uint32_t count, void* stream)
{
    if (!c || !models || !local_aabbs) return HK_ERR_INVALID;
    HK_TRY(update_args_ok(c, count, "hk_refit_instances"));
    (void)hipSetDevice(c->device);
    return rebuild_instances(c, models, local_aabbs, count, pick(c, stream), nullptr, nullptr, nullptr, true);
}

// Tree costs (include/hk_cost.h).  Every check first; then the table of the trees asked for (slot 0: the
// TLAS, 1: the light BVH, 2 + j: mesh_ids[j]'s slice from the registry; a tree without nodes has no table entry and
// keeps its zeros), the zeroed accumulators, one launch and one readback on `st`, and the call's one wait.  Only the
// scratch is written: the scene arrays are read as the last edit's wait left them, so nothing is joined or serialized.
int hk_tree_costs(hk_ctx* c, const uint32_t* mesh_ids, uint32_t mesh_count, hk_tree_cost* tlas, hk_tree_cost* lights,
                  hk_tree_cost* meshes, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (mesh_count && !mesh_ids) return fail(c, HK_ERR_INVALID, "hk_tree_costs: null pointer");
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    for (uint32_t j = 0; j < mesh_count; ++j)
        if (mesh_ids[j] >= c->meshes.size())
            return fail(c, HK_ERR_INVALID, "hk_tree_costs: mesh " + std::to_string(mesh_ids[j]) + " of " +
                                               std::to_string(c->meshes.size()) + " known mesh slices");
    const uint32_t n_listed = meshes ? mesh_count : 0u;
    const size_t slots = 2u + (size_t)n_listed;
    std::vector<CostSlice>& table = c->cost_table;
    table.clear();
    uint64_t n_nodes = 0;
    auto add = [&](const void* nodes, uint32_t count, uint32_t slot) {
        if (count == 0u) return;
        table.push_back(CostSlice{(const hk_node*)nodes, count, (uint32_t)n_nodes, slot, 0u});
        n_nodes += count;
    };
    if (tlas) add(c->buf[5], c->count[5], 0u);
    if (lights) add(c->buf[7], c->count[7], 1u);
    for (uint32_t j = 0; j < n_listed && n_nodes <= 0xFFFFFFFFull; ++j) {
        const hk_mesh_index& m = c->meshes[mesh_ids[j]].index;  // (inside the asset nodes: checked where it became known)
        add((const hk_node*)c->buf[2] + m.node[0], m.node[1], 2u + j);
    }
    if (n_nodes > 0xFFFFFF00ull) return fail(c, HK_ERR_INVALID, "hk_tree_costs: more than 2^32 nodes listed");
    c->cost_host.assign(slots, hk_tree_cost{0, 0, 0.0f, 0});
    if (!table.empty()) {
        (void)hipSetDevice(c->device);
        hipStream_t st = pick(c, stream);
        const size_t sz[] = {table.size() * sizeof(CostSlice), slots * sizeof(hk_tree_cost)};
        char* part[2];
        HK_TRY(carve(c, &c->cost_scratch, &c->cost_bytes, sz, 2, part));
        HK_HIP(c, hipMemcpyAsync(part[0], table.data(), sz[0], hipMemcpyHostToDevice, st));
        HK_HIP(c, hipMemsetAsync(part[1], 0, sz[1], st));
        timed(c, "tree_costs", st, [&] {
            launch_tree_cost((const CostSlice*)part[0], (uint32_t)table.size(), (uint32_t)n_nodes, (hk_tree_cost*)part[1],
                             st);
        });
        HK_HIP(c, hipGetLastError());
        HK_HIP(c, hipMemcpyAsync(c->cost_host.data(), part[1], sz[1], hipMemcpyDeviceToHost, st));
        HK_HIP(c, hipStreamSynchronize(st));
    }
    if (tlas) *tlas = c->cost_host[0];
    if (lights) *lights = c->cost_host[1];
    for (uint32_t j = 0; j < n_listed; ++j) meshes[j] = c->cost_host[2u + j];
    return HK_OK;
}

// Meshes on their way to a build (hk_update_meshes, hk_add_meshes and the new entries of hk_set_meshes): the tables in
// list order and by size, where each mesh's indices lie, and the bytes of scratch they, the attribute and index streams
// and the builds' shape boxes, indices, segments and levels take (sz: one entry per part; the last is the caller's
// own, `extra` bytes).
struct MeshStaging {
    std::vector<MeshUpdate> tab, by_size;
    std::vector<MeshSource> sources;
    uint32_t n_lds = 0, n_vertices = 0, n_shapes = 0, n_indices = 0;
    uint32_t large_bound = 0;  // (a refit: MeshUpdateArgs::large_bound)
    static constexpr int PARTS = 12;
    size_t sz[PARTS] = {};
    size_t total = 0;
};

// meshes[k] goes to slices[k] with tris[k] triangles.  A deformed mesh (hk_update_meshes) has no uvs and no indices,
// and may have no normals: MeshUpdate::has_normals says so, and its part of the normal stream is left unwritten.  refit:
// the meshes are refit, not built, so the table by size and the segments take no room (the list of large nodes lies
// where the indices would, its counter where the levels would).
static void plan_mesh_staging(const std::vector<const hk_mesh_desc*>& meshes, const hk_mesh_index* slices,
                              const uint32_t* tris, uint64_t n_vertices, uint64_t n_shapes, uint64_t n_indices,
                              size_t extra, MeshStaging* S, bool refit = false)
{
    const uint32_t n = (uint32_t)meshes.size();
    S->tab.resize(n);
    S->sources.resize(n);
    S->n_vertices = (uint32_t)n_vertices;
    S->n_shapes = (uint32_t)n_shapes;
    S->n_indices = (uint32_t)n_indices;
    uint32_t v0 = 0, s0 = 0, i0 = 0;
    bool uvs = false;
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_index& x = slices[k];
        const hk_mesh_desc& m = *meshes[k];
        S->tab[k] = MeshUpdate{x.vertex, m.vertex_count, x.primitive, tris[k], x.node[0], v0, s0, k, m.normals ? 1u : 0u};
        S->sources[k] = MeshSource{m.indices ? i0 : MESH_NO_INDICES, m.topology == HKS_TRIANGLE_STRIP ? 1u : 0u};
        v0 += m.vertex_count;
        s0 += tris[k];
        if (m.indices) i0 += m.index_count;
        uvs = uvs || m.uvs;
        S->n_lds += tris[k] <= mesh_lds_shapes() ? 1u : 0u;
        S->large_bound += mesh_refit_large_bound(tris[k]);
    }
    for (int big = 0; big < 2; ++big)
        for (const MeshUpdate& m : S->tab)
            if ((m.shapes > mesh_lds_shapes()) == (big == 1)) S->by_size.push_back(m);
    const size_t nv = S->n_vertices, ns = S->n_shapes;
    const size_t sz[MeshStaging::PARTS] = {(size_t)n * sizeof(MeshUpdate), refit ? 0 : (size_t)n * sizeof(MeshUpdate),
                                           (size_t)n * sizeof(MeshSource), nv * 12, nv * 12, uvs ? nv * 8 : 0,
                                           (size_t)(S->n_indices ? S->n_indices : 1) * 4, ns * 24, ns * 8,
                                           refit ? 0 : ns * 24, (size_t)n * 4, extra};
    std::memcpy(S->sz, sz, sizeof(sz));
    S->total = carve_bytes(sz, MeshStaging::PARTS);
}

// The tables and streams copied into c->mesh_scratch on `st`, and the launch arguments over them, the destinations
// c->buf[0..2].  *extra: the caller's part.
static int enqueue_mesh_staging(hk_ctx* c, const std::vector<const hk_mesh_desc*>& meshes, const MeshStaging& S,
                                hipStream_t st, MeshAddArgs* A, char** extra)
{
    char* part[MeshStaging::PARTS];
    HK_TRY(carve(c, &c->mesh_scratch, &c->mesh_bytes, S.sz, MeshStaging::PARTS, part));
    const size_t n = meshes.size();
    if (n) {
        HK_HIP(c, hipMemcpyAsync(part[0], S.tab.data(), n * sizeof(MeshUpdate), hipMemcpyHostToDevice, st));
        if (S.sz[1])
            HK_HIP(c, hipMemcpyAsync(part[1], S.by_size.data(), n * sizeof(MeshUpdate), hipMemcpyHostToDevice, st));
        HK_HIP(c, hipMemcpyAsync(part[2], S.sources.data(), n * sizeof(MeshSource), hipMemcpyHostToDevice, st));
    }
    for (size_t k = 0; k < n; ++k) {
        const hk_mesh_desc& m = *meshes[k];
        const size_t v0 = S.tab[k].vertex0, nv = m.vertex_count;
        const struct {
            int part;
            const float* from;
            size_t bytes;
        } streams[] = {{3, m.positions, 12}, {4, m.normals, 12}, {5, m.uvs, 8}};
        for (const auto& a : streams)
            if (nv && a.from)
                HK_HIP(c, hipMemcpyAsync(part[a.part] + v0 * a.bytes, a.from, nv * a.bytes, hipMemcpyHostToDevice, st));
        if (m.indices)
            HK_HIP(c, hipMemcpyAsync(part[6] + (size_t)S.sources[k].index0 * 4, m.indices, (size_t)m.index_count * 4,
                                     hipMemcpyHostToDevice, st));
    }
    MeshUpdateArgs& M = A->M;
    M.table = (const MeshUpdate*)part[0];
    M.table_by_size = (const MeshUpdate*)part[1];
    M.n_meshes = (uint32_t)n;
    M.n_lds = S.n_lds;
    M.n_vertices = S.n_vertices;
    M.n_shapes = S.n_shapes;
    M.positions = (const float*)part[3];
    M.normals = (const float*)part[4];
    M.vertices = (hk_vertex*)c->buf[0];
    M.primitives = (hk_primitive*)c->buf[1];
    M.blas = (hk_node*)c->buf[2];
    M.buckets = 6;  // bvh 0.7.1 NUM_BUCKETS (hks_build default)
    M.shapes = part[7];
    M.idx = (uint32_t*)part[8];
    M.segments = part[9];
    M.levels = (uint32_t*)part[10];
    M.large = (uint32_t*)part[8];
    M.n_large = (uint32_t*)part[10];
    M.large_bound = S.large_bound;
    A->sources = (const MeshSource*)part[2];
    A->uvs = (const float*)part[5];
    A->indices = (const uint32_t*)part[6];
    if (extra) *extra = part[11];
    return HK_OK;
}

// The checks of a mesh whose vertices are rewritten in place (hk_update_meshes, hk_set_mesh_skins, hk_skin_meshes), `who`
// in front of the message, for the known slice c->meshes[at]: a BLAS the device can rebuild, and a vertex_count that
// covers the stored indices and stays inside the slice.
static int mesh_rewritable(hk_ctx* c, const std::string& who, size_t at, uint32_t vertex_count)
{
    const hk_ctx::MeshSlice& s = c->meshes[at];
    const hk_mesh_index& mesh = s.index;
    if (s.vertex_need == HK_U32_MAX)
        return fail(c, HK_ERR_INVALID, who + ": its BLAS is not 3k - 2 nodes over k primitives of the scene; cannot rebuild");
    // the vertex slice ends where the array or the next instanced mesh's vertices begin
    uint32_t room = c->count[0] - mesh.vertex;
    for (const hk_ctx::MeshSlice& o : c->meshes)
        if (o.index.vertex > mesh.vertex) room = std::min(room, o.index.vertex - mesh.vertex);
    if (vertex_count < s.vertex_need)
        return fail(c, HK_ERR_INVALID, who + ": vertex_count does not cover the vertex indices of its primitives");
    if (vertex_count > room)
        return fail(c, HK_ERR_INVALID, who + ": vertex_count reaches past its vertex slice");
    return HK_OK;
}

// The refit of the listed slices behind the rewrite, in place of launch_mesh_update's builds, each launch
// timed under its own name
static void enqueue_mesh_refit(hk_ctx* c, const MeshUpdateArgs& M, hipStream_t st)
{
    timed(c, "refit_geometry", st, [&] { launch_mesh_geometry(M, st); });
    timed(c, "refit_small", st, [&] { launch_refit_small(M, st); });
    timed(c, "refit_large", st, [&] { launch_refit_large(M, st); });
    timed(c, "refit_derivatives", st, [&] { refresh_blas_derivatives(c, st, c->count[2]); });
}

// hk_update_meshes (fn = "hk_update_meshes"), hk_refit_meshes and hk_refit_meshes_all: one body, the BLAS step apart
// (refit) and the instance trees kept or not (refit_trees)
static int update_meshes(hk_ctx* c, const std::string& fn, bool refit, bool refit_trees, const hk_mesh_update* meshes,
                         uint32_t mesh_count, const float* models, const float* local_aabbs, uint32_t count, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!meshes || !models || !local_aabbs) return fail(c, HK_ERR_INVALID, fn + ": null pointer");
    HK_TRY(update_args_ok(c, count, fn.c_str()));
    // every listed mesh against what upload recorded (no device work before the list is accepted whole): a staged mesh
    // without uvs and indices
    std::vector<hk_mesh_desc> descs(mesh_count);
    std::vector<const hk_mesh_desc*> list(mesh_count);
    std::vector<hk_mesh_index> slices(mesh_count);
    std::vector<uint32_t> tris(mesh_count);
    MeshLevels ml;
    ml.slice.resize(mesh_count);
    uint32_t n_vertices = 0, n_shapes = 0;
    for (uint32_t k = 0; k < mesh_count; ++k) {
        const hk_mesh_update& u = meshes[k];
        const std::string who = fn + ": mesh " + std::to_string(k);
        if (!u.positions) return fail(c, HK_ERR_INVALID, who + " has no positions");
        const size_t at = find_slice(c->meshes, u.mesh);
        if (at == c->meshes.size()) return fail(c, HK_ERR_INVALID, who + " is not an instanced mesh of the uploaded scene");
        for (uint32_t j = 0; j < k; ++j)
            if (ml.slice[j] == at) return fail(c, HK_ERR_INVALID, who + " is listed twice");
        HK_TRY(mesh_rewritable(c, who, at, u.vertex_count));
        tris[k] = (u.mesh.node[1] + 2u) / 3u;
        if ((size_t)n_vertices + u.vertex_count > 0x40000000u || (size_t)n_shapes + tris[k] > 0x40000000u)
            return fail(c, HK_ERR_INVALID, fn + ": too many vertices or primitives in one call");
        descs[k] = hk_mesh_desc{u.positions, u.normals, nullptr, u.vertex_count, nullptr, 0u, HKS_TRIANGLE_LIST};
        list[k] = &descs[k];
        slices[k] = u.mesh;
        ml.slice[k] = (uint32_t)at;
        n_vertices += u.vertex_count;
        n_shapes += tris[k];
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    if (mesh_count == 0)
        return rebuild_instances(c, models, local_aabbs, count, st, nullptr, nullptr, nullptr, refit_trees);
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.gb_serialize(false));
    MeshStaging stage;
    plan_mesh_staging(list, slices.data(), tris.data(), n_vertices, n_shapes, 0, 0, &stage, refit);
    MeshAddArgs A;
    HK_TRY(enqueue_mesh_staging(c, list, stage, st, &A, nullptr));
    if (refit)
        enqueue_mesh_refit(c, A.M, st);
    else
        timed(c, "update_meshes", st, [&] {
            launch_mesh_update(A.M, st);
            refresh_blas_derivatives(c, st, c->count[2]);
        });
    HK_HIP(c, hipGetLastError());
    ml.device = A.M.levels;
    if (refit) ml.slice.clear();  // the topology stays, and so does every depth: no levels to read back
    return rebuild_instances(c, models, local_aabbs, count, st, &ml, nullptr, nullptr, refit_trees);
}
int hk_update_meshes(hk_ctx* c, const hk_mesh_update* meshes, uint32_t mesh_count, const float* models,
                     const float* local_aabbs, uint32_t count, void* stream)
{
    return update_meshes(c, "hk_update_meshes", false, false, meshes, mesh_count, models, local_aabbs, count, stream);
}
int hk_refit_meshes(hk_ctx* c, const hk_mesh_update* meshes, uint32_t mesh_count, const float* models,
                    const float* local_aabbs, uint32_t count, void* stream)
{
    return update_meshes(c, "hk_refit_meshes", true, false, meshes, mesh_count, models, local_aabbs, count, stream);
}
int hk_refit_meshes_all(hk_ctx* c, const hk_mesh_update* meshes, uint32_t mesh_count, const float* models,
                        const float* local_aabbs, uint32_t count, void* stream)
{
    return update_meshes(c, "hk_refit_meshes_all", true, true, meshes, mesh_count, models, local_aabbs, count, stream);
}

// The four resident skin streams in one block at `cap` vertices each (hk_ctx::skin_block), every stream 256-aligned
struct SkinStreams {
    float* positions;
    float* normals;
    uint2* indices;
    float4* weights;
    size_t bytes;
};
static SkinStreams skin_streams(void* block, size_t cap)
{
    const size_t sz[4] = {cap * 12, cap * 12, cap * 8, cap * 16};
    char* p = (char*)block;
    SkinStreams s;
    s.positions = (float*)p;
    s.normals = (float*)(p + carve_bytes(sz, 1));
    s.indices = (uint2*)(p + carve_bytes(sz, 2));
    s.weights = (float4*)(p + carve_bytes(sz, 3));
    s.bytes = carve_bytes(sz, 4);
    return s;
}
static size_t find_skin(const std::vector<hk_ctx::Skin>& skins, const hk_mesh_index& x)
{
    size_t k = 0;
    while (k < skins.size() && std::memcmp(&skins[k].index, &x, sizeof(x)) != 0) ++k;
    return k;
}

int hk_set_mesh_skins(hk_ctx* c, const hk_mesh_skin* skins, uint32_t n, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (n && !skins) return fail(c, HK_ERR_INVALID, "hk_set_mesh_skins: null pointer");
    // the whole list on the host first: a refusal leaves the set before as it was
    std::vector<hk_ctx::Skin> set(n);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_skin& s = skins[k];
        const std::string who = "hk_set_mesh_skins: skin " + std::to_string(k);
        if (!s.positions || !s.joint_indices || !s.joint_weights)
            return fail(c, HK_ERR_INVALID, who + " has a null pointer (positions, joint_indices, joint_weights)");
        const size_t at = find_slice(c->meshes, s.mesh);
        if (at == c->meshes.size()) return fail(c, HK_ERR_INVALID, who + " is not a known mesh slice of the scene");
        for (uint32_t j = 0; j < k; ++j)
            if (std::memcmp(&set[j].index, &s.mesh, sizeof(s.mesh)) == 0)
                return fail(c, HK_ERR_INVALID, who + " is listed twice");
        HK_TRY(mesh_rewritable(c, who, at, s.vertex_count));
        if (s.joint_count == 0 || s.joint_count > 65536u)
            return fail(c, HK_ERR_INVALID, who + ": joint_count is outside 1 .. 65536");
        for (size_t i = 0; i < 4 * (size_t)s.vertex_count; ++i)
            if (s.joint_indices[i] >= s.joint_count)
                return fail(c, HK_ERR_INVALID, who + ": vertex " + std::to_string(i / 4) + " has a joint index " +
                                                   std::to_string(s.joint_indices[i]) + " >= joint_count");
        if (total + s.vertex_count > 0x40000000u) return fail(c, HK_ERR_INVALID, "hk_set_mesh_skins: too many vertices");
        set[k] = hk_ctx::Skin{s.mesh, s.vertex_count, s.joint_count, (uint32_t)total, s.normals != nullptr};
        total += s.vertex_count;
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    if (total > c->skin_cap) {  // (the new block first: out of memory leaves the set before in place)
        void* block = nullptr;
        HK_HIP(c, hipMalloc(&block, skin_streams((void*)0, (size_t)total).bytes));
        HK_HIP(c, hipStreamSynchronize(st));
        release(c->skin_block);
        c->skin_block = block;
        c->skin_cap = (size_t)total;
    }
    c->skins.clear();  // (the streams are overwritten from here on)
    const SkinStreams S = skin_streams(c->skin_block, c->skin_cap);
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_skin& s = skins[k];
        const size_t v0 = set[k].vertex0, nv = s.vertex_count;
        if (!nv) continue;
        HK_HIP(c, hipMemcpyAsync(S.positions + 3 * v0, s.positions, nv * 12, hipMemcpyHostToDevice, st));
        if (s.normals) HK_HIP(c, hipMemcpyAsync(S.normals + 3 * v0, s.normals, nv * 12, hipMemcpyHostToDevice, st));
        HK_HIP(c, hipMemcpyAsync(S.indices + v0, s.joint_indices, nv * 8, hipMemcpyHostToDevice, st));
        HK_HIP(c, hipMemcpyAsync(S.weights + v0, s.joint_weights, nv * 16, hipMemcpyHostToDevice, st));
    }
    HK_HIP(c, hipStreamSynchronize(st));
    c->skins = std::move(set);
    return HK_OK;
}

// hk_skin_meshes (fn = "hk_skin_meshes"), hk_skin_meshes_refit and hk_skin_meshes_refit_all: one body, the BLAS step
// apart (refit) and the instance trees kept or not (refit_trees)
static int skin_meshes(hk_ctx* c, const std::string& fn, bool refit, bool refit_trees, const hk_skin_pose* poses,
                       uint32_t n, const float* models, const float* local_aabbs, uint32_t count, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!models || !local_aabbs || (n && !poses)) return fail(c, HK_ERR_INVALID, fn + ": null pointer");
    HK_TRY(update_args_ok(c, count, fn.c_str()));
    // every pose against the registered skins and the registry, before any device work: each a staged mesh with no
    // host streams (k_skin_vertices fills its part of them)
    std::vector<hk_mesh_desc> descs(n);
    std::vector<const hk_mesh_desc*> list(n);
    std::vector<hk_mesh_index> slices(n);
    std::vector<uint32_t> tris(n);
    std::vector<size_t> skin_of(n);
    std::vector<SkinSource> sources(n);
    MeshLevels ml;
    ml.slice.resize(n);
    uint64_t n_vertices = 0, n_shapes = 0, n_joints = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const hk_skin_pose& p = poses[k];
        const std::string who = fn + ": pose " + std::to_string(k);
        if (!p.joints) return fail(c, HK_ERR_INVALID, who + " has a null pointer (joints)");
        const size_t sk = find_skin(c->skins, p.mesh);
        if (sk == c->skins.size())
            return fail(c, HK_ERR_INVALID, who + " names a mesh with no registered skin (hk_set_mesh_skins)");
        for (uint32_t j = 0; j < k; ++j)
            if (skin_of[j] == sk) return fail(c, HK_ERR_INVALID, who + " poses a mesh twice");
        const hk_ctx::Skin& s = c->skins[sk];
        if (p.joint_count != s.joint_count)
            return fail(c, HK_ERR_INVALID, who + ": joint_count " + std::to_string(p.joint_count) +
                                               " differs from the registered skin's " + std::to_string(s.joint_count));
        const size_t at = find_slice(c->meshes, s.index);
        if (at == c->meshes.size()) return fail(c, HK_ERR_INVALID, who + " is not a known mesh slice of the scene");
        HK_TRY(mesh_rewritable(c, who, at, s.vertex_count));
        tris[k] = (s.index.node[1] + 2u) / 3u;
        if (n_vertices + s.vertex_count > 0x40000000u || n_shapes + tris[k] > 0x40000000u)
            return fail(c, HK_ERR_INVALID, fn + ": too many vertices or primitives in one call");
        descs[k] = hk_mesh_desc{nullptr, nullptr, nullptr, s.vertex_count, nullptr, 0u, HKS_TRIANGLE_LIST};
        list[k] = &descs[k];
        slices[k] = s.index;
        skin_of[k] = sk;
        sources[k] = SkinSource{s.vertex0, (uint32_t)n_joints, s.index};
        ml.slice[k] = (uint32_t)at;
        n_vertices += s.vertex_count;
        n_shapes += tris[k];
        n_joints += s.joint_count;
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    if (n == 0) return rebuild_instances(c, models, local_aabbs, count, st, nullptr, nullptr, nullptr, refit_trees);
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.gb_serialize(false));
    // the caller's part of the staging: the palettes one after another, then the SkinSource table
    const size_t palette_bytes = ((size_t)n_joints * 64 + 255) & ~(size_t)255;
    MeshStaging stage;
    plan_mesh_staging(list, slices.data(), tris.data(), n_vertices, n_shapes, 0,
                      palette_bytes + (size_t)n * sizeof(SkinSource), &stage, refit);
    for (std::vector<MeshUpdate>* t : {&stage.tab, &stage.by_size})
        for (MeshUpdate& m : *t) m.has_normals = c->skins[skin_of[m.slot]].has_normals ? 1u : 0u;
    MeshAddArgs A;
    char* extra = nullptr;
    HK_TRY(enqueue_mesh_staging(c, list, stage, st, &A, &extra));
    for (uint32_t k = 0; k < n; ++k)
        HK_HIP(c, hipMemcpyAsync(extra + (size_t)sources[k].joint0 * 64, poses[k].joints, (size_t)poses[k].joint_count * 64,
                                 hipMemcpyHostToDevice, st));
    HK_HIP(c, hipMemcpyAsync(extra + palette_bytes, sources.data(), (size_t)n * sizeof(SkinSource), hipMemcpyHostToDevice, st));
    const SkinStreams S = skin_streams(c->skin_block, c->skin_cap);
    SkinArgs K;
    K.table = A.M.table;
    K.sources = (const SkinSource*)(extra + palette_bytes);
    K.n_meshes = n;
    K.n_vertices = (uint32_t)n_vertices;
    K.bind_positions = S.positions;
    K.bind_normals = S.normals;
    K.joint_indices = S.indices;
    K.joint_weights = S.weights;
    K.palettes = (const float4*)extra;
    K.positions = const_cast<float*>(A.M.positions);
    K.normals = const_cast<float*>(A.M.normals);
    // after rebuild_instances' uploads, so that the posed boxes land on the device copy of local_aabbs
    const std::function<void(float*)> work = [&](float* device_aabbs) {
        if (refit) {
            timed(c, "refit_skin_vertices", st, [&] { launch_skin_vertices(K, st); });
            enqueue_mesh_refit(c, A.M, st);
            timed(c, "refit_skin_bounds", st,
                  [&] { launch_skin_bounds(K, (const hk_instance*)c->buf[4], count, device_aabbs, st); });
            return;
        }
        timed(c, "skin_meshes", st, [&] {
            launch_skin_vertices(K, st);
            launch_mesh_update(A.M, st);
            refresh_blas_derivatives(c, st, c->count[2]);
            launch_skin_bounds(K, (const hk_instance*)c->buf[4], count, device_aabbs, st);
        });
    };
    ml.device = A.M.levels;
    if (refit) ml.slice.clear();  // the topology stays, and so does every depth: no levels to read back
    return rebuild_instances(c, models, local_aabbs, count, st, &ml, nullptr, &work, refit_trees);
}
int hk_skin_meshes(hk_ctx* c, const hk_skin_pose* poses, uint32_t n, const float* models, const float* local_aabbs,
                   uint32_t count, void* stream)
{
    return skin_meshes(c, "hk_skin_meshes", false, false, poses, n, models, local_aabbs, count, stream);
}
int hk_skin_meshes_refit(hk_ctx* c, const hk_skin_pose* poses, uint32_t n, const float* models, const float* local_aabbs,
                         uint32_t count, void* stream)
{
    return skin_meshes(c, "hk_skin_meshes_refit", true, false, poses, n, models, local_aabbs, count, stream);
}
int hk_skin_meshes_refit_all(hk_ctx* c, const hk_skin_pose* poses, uint32_t n, const float* models,
                             const float* local_aabbs, uint32_t count, void* stream)
{
    return skin_meshes(c, "hk_skin_meshes_refit_all", true, true, poses, n, models, local_aabbs, count, stream);
}

// The four resident morph streams in one block, carved at the set's own totals (hk_ctx::morph_total), every stream
// 256-aligned
struct MorphStreams {
    float* positions;
    float* normals;
    float* position_deltas;
    float* normal_deltas;
    size_t bytes;
};
static MorphStreams morph_streams(void* block, const uint64_t total[3])
{
    const size_t sz[4] = {(size_t)total[0] * 12, (size_t)total[0] * 12, (size_t)total[1] * 12, (size_t)total[2] * 12};
    char* p = (char*)block;
    MorphStreams s;
    s.positions = (float*)p;
    s.normals = (float*)(p + carve_bytes(sz, 1));
    s.position_deltas = (float*)(p + carve_bytes(sz, 2));
    s.normal_deltas = (float*)(p + carve_bytes(sz, 3));
    s.bytes = carve_bytes(sz, 4);
    return s;
}
static size_t find_morph(const std::vector<hk_ctx::Morph>& morphs, const hk_mesh_index& x)
{
    size_t k = 0;
    while (k < morphs.size() && std::memcmp(&morphs[k].index, &x, sizeof(x)) != 0) ++k;
    return k;
}

int hk_set_mesh_morphs(hk_ctx* c, const hk_mesh_morph* morphs, uint32_t n, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (n && !morphs) return fail(c, HK_ERR_INVALID, "hk_set_mesh_morphs: null pointer");
    // the whole list on the host first: a refusal leaves the set before as it was
    std::vector<hk_ctx::Morph> set(n);
    uint64_t total[3] = {0, 0, 0};
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_morph& s = morphs[k];
        const std::string who = "hk_set_mesh_morphs: morph " + std::to_string(k);
        if (!s.positions || !s.position_deltas)
            return fail(c, HK_ERR_INVALID, who + " has a null pointer (positions, position_deltas)");
        if (s.normal_deltas && !s.normals) return fail(c, HK_ERR_INVALID, who + " has normal_deltas without normals");
        if (s.target_count == 0 || s.target_count > HK_MORPH_MAX_TARGETS)
            return fail(c, HK_ERR_INVALID, who + ": target_count is outside 1 .. " + std::to_string(HK_MORPH_MAX_TARGETS));
        const size_t at = find_slice(c->meshes, s.mesh);
        if (at == c->meshes.size()) return fail(c, HK_ERR_INVALID, who + " is not a known mesh slice of the scene");
        for (uint32_t j = 0; j < k; ++j)
            if (std::memcmp(&set[j].index, &s.mesh, sizeof(s.mesh)) == 0)
                return fail(c, HK_ERR_INVALID, who + " is listed twice");
        HK_TRY(mesh_rewritable(c, who, at, s.vertex_count));
        const uint64_t records = (uint64_t)s.target_count * s.vertex_count;
        if (total[0] + s.vertex_count > 0x40000000u || total[1] + records > 0x40000000u)
            return fail(c, HK_ERR_INVALID, "hk_set_mesh_morphs: too many vertices or target_count x vertex_count records");
        set[k] = hk_ctx::Morph{s.mesh, s.vertex_count, s.target_count, (uint32_t)total[0], (uint32_t)total[1],
                               s.normal_deltas ? (uint32_t)total[2] : MORPH_NONE, s.normals != nullptr};
        total[0] += s.vertex_count;
        total[1] += records;
        if (s.normal_deltas) total[2] += records;
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    const size_t bytes = morph_streams((void*)0, total).bytes;
    if (bytes > c->morph_cap) {  // (the new block first: out of memory leaves the set before in place)
        void* block = nullptr;
        HK_HIP(c, hipMalloc(&block, bytes));
        HK_HIP(c, hipStreamSynchronize(st));
        release(c->morph_block);
        c->morph_block = block;
        c->morph_cap = bytes;
    }
    c->morphs.clear();  // (the streams are overwritten from here on)
    std::memcpy(c->morph_total, total, sizeof(total));
    const MorphStreams S = morph_streams(c->morph_block, total);
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_morph& s = morphs[k];
        const size_t v0 = set[k].vertex0, nv = s.vertex_count, nr = nv * s.target_count;
        if (!nv) continue;
        HK_HIP(c, hipMemcpyAsync(S.positions + 3 * v0, s.positions, nv * 12, hipMemcpyHostToDevice, st));
        if (s.normals) HK_HIP(c, hipMemcpyAsync(S.normals + 3 * v0, s.normals, nv * 12, hipMemcpyHostToDevice, st));
        HK_HIP(c, hipMemcpyAsync(S.position_deltas + 3 * (size_t)set[k].delta0, s.position_deltas, nr * 12,
                                 hipMemcpyHostToDevice, st));
        if (s.normal_deltas)
            HK_HIP(c, hipMemcpyAsync(S.normal_deltas + 3 * (size_t)set[k].normal_delta0, s.normal_deltas, nr * 12,
                                     hipMemcpyHostToDevice, st));
    }
    HK_HIP(c, hipStreamSynchronize(st));
    c->morphs = std::move(set);
    return HK_OK;
}

// hk_morph_meshes (fn = "hk_morph_meshes"), hk_morph_meshes_refit and hk_morph_meshes_refit_all: one body, the BLAS step
// apart (refit) and the instance trees kept or not (refit_trees), switched as skin_meshes switches them
static int morph_meshes(hk_ctx* c, const std::string& fn, bool refit, bool refit_trees, const hk_morph_pose* poses,
                        uint32_t n, const float* models, const float* local_aabbs, uint32_t count, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!models || !local_aabbs || (n && !poses)) return fail(c, HK_ERR_INVALID, fn + ": null pointer");
    HK_TRY(update_args_ok(c, count, fn.c_str()));
    // every pose against the registered morphs, skins and the registry, before any device work: each a staged mesh with
    // no host streams (k_morph_vertices fills its part of them); the active lists one after another
    std::vector<hk_mesh_desc> descs(n);
    std::vector<const hk_mesh_desc*> list(n);
    std::vector<hk_mesh_index> slices(n);
    std::vector<uint32_t> tris(n);
    std::vector<size_t> morph_of(n);
    std::vector<MorphSource> sources(n);
    std::vector<MorphActive> active;
    MeshLevels ml;
    ml.slice.resize(n);
    uint64_t n_vertices = 0, n_shapes = 0, n_joints = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const hk_morph_pose& p = poses[k];
        const std::string who = fn + ": pose " + std::to_string(k);
        if (!p.weights) return fail(c, HK_ERR_INVALID, who + " has a null pointer (weights)");
        const size_t mk = find_morph(c->morphs, p.mesh);
        if (mk == c->morphs.size())
            return fail(c, HK_ERR_INVALID, who + " names a mesh with no registered morph (hk_set_mesh_morphs)");
        for (uint32_t j = 0; j < k; ++j)
            if (morph_of[j] == mk) return fail(c, HK_ERR_INVALID, who + " poses a mesh twice");
        const hk_ctx::Morph& s = c->morphs[mk];
        if (p.target_count != s.target_count)
            return fail(c, HK_ERR_INVALID, who + ": target_count " + std::to_string(p.target_count) +
                                               " differs from the registered morph's " + std::to_string(s.target_count));
        uint32_t skin0 = MORPH_NONE;
        if (p.joints) {
            const size_t sk = find_skin(c->skins, p.mesh);
            if (sk == c->skins.size())
                return fail(c, HK_ERR_INVALID, who + " gives joints for a mesh with no registered skin (hk_set_mesh_skins)");
            const hk_ctx::Skin& sn = c->skins[sk];
            if (p.joint_count != sn.joint_count)
                return fail(c, HK_ERR_INVALID, who + ": joint_count " + std::to_string(p.joint_count) +
                                                   " differs from the registered skin's " + std::to_string(sn.joint_count));
            if (sn.has_normals != s.has_normals)
                return fail(c, HK_ERR_INVALID, who + ": its skin and its morph disagree on whether normals are rewritten");
            if (sn.vertex_count != s.vertex_count)
                return fail(c, HK_ERR_INVALID, who + ": its skin and its morph disagree on the vertex_count");
            skin0 = sn.vertex0;
        }
        const size_t at = find_slice(c->meshes, s.index);
        if (at == c->meshes.size()) return fail(c, HK_ERR_INVALID, who + " is not a known mesh slice of the scene");
        HK_TRY(mesh_rewritable(c, who, at, s.vertex_count));
        tris[k] = (s.index.node[1] + 2u) / 3u;
        if (n_vertices + s.vertex_count > 0x40000000u || n_shapes + tris[k] > 0x40000000u)
            return fail(c, HK_ERR_INVALID, fn + ": too many vertices or primitives in one call");
        descs[k] = hk_mesh_desc{nullptr, nullptr, nullptr, s.vertex_count, nullptr, 0u, HKS_TRIANGLE_LIST};
        list[k] = &descs[k];
        slices[k] = s.index;
        morph_of[k] = mk;
        const uint32_t active0 = (uint32_t)active.size();
        for (uint32_t t = 0; t < s.target_count; ++t)
            if (p.weights[t] != 0.0f) active.push_back(MorphActive{t, p.weights[t]});  // (hk_morph.h: hk_morph_active)
        sources[k] = MorphSource{s.vertex0, s.delta0, s.normal_delta0, active0, (uint32_t)active.size() - active0,
                                 skin0,     (uint32_t)n_joints, s.index};
        ml.slice[k] = (uint32_t)at;
        n_vertices += s.vertex_count;
        n_shapes += tris[k];
        if (p.joints) n_joints += p.joint_count;
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    if (n == 0) return rebuild_instances(c, models, local_aabbs, count, st, nullptr, nullptr, nullptr, refit_trees);
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.gb_serialize(false));
    // the caller's part of the staging: the palettes one after another, the active list, then the MorphSource table
    const size_t palette_bytes = ((size_t)n_joints * 64 + 255) & ~(size_t)255;
    const size_t active_bytes = (active.size() * sizeof(MorphActive) + 255) & ~(size_t)255;
    MeshStaging stage;
    plan_mesh_staging(list, slices.data(), tris.data(), n_vertices, n_shapes, 0,
                      palette_bytes + active_bytes + (size_t)n * sizeof(MorphSource), &stage, refit);
    for (std::vector<MeshUpdate>* t : {&stage.tab, &stage.by_size})
        for (MeshUpdate& m : *t) m.has_normals = c->morphs[morph_of[m.slot]].has_normals ? 1u : 0u;
    MeshAddArgs A;
    char* extra = nullptr;
    HK_TRY(enqueue_mesh_staging(c, list, stage, st, &A, &extra));
    for (uint32_t k = 0; k < n; ++k)
        if (poses[k].joints)
            HK_HIP(c, hipMemcpyAsync(extra + (size_t)sources[k].joint0 * 64, poses[k].joints,
                                     (size_t)poses[k].joint_count * 64, hipMemcpyHostToDevice, st));
    if (!active.empty())
        HK_HIP(c, hipMemcpyAsync(extra + palette_bytes, active.data(), active.size() * sizeof(MorphActive),
                                 hipMemcpyHostToDevice, st));
    HK_HIP(c, hipMemcpyAsync(extra + palette_bytes + active_bytes, sources.data(), (size_t)n * sizeof(MorphSource),
                             hipMemcpyHostToDevice, st));
    const MorphStreams S = morph_streams(c->morph_block, c->morph_total);
    const SkinStreams R = skin_streams(c->skin_block, c->skin_cap);
    MorphArgs K;
    K.table = A.M.table;
    K.sources = (const MorphSource*)(extra + palette_bytes + active_bytes);
    K.active = (const MorphActive*)(extra + palette_bytes);
    K.n_meshes = n;
    K.n_vertices = (uint32_t)n_vertices;
    K.base_positions = S.positions;
    K.base_normals = S.normals;
    K.position_deltas = S.position_deltas;
    K.normal_deltas = S.normal_deltas;
    K.joint_indices = R.indices;
    K.joint_weights = R.weights;
    K.palettes = (const float4*)extra;
    K.positions = const_cast<float*>(A.M.positions);
    K.normals = const_cast<float*>(A.M.normals);
    const PosedSlices posed{&K.sources->mesh, (uint32_t)sizeof(MorphSource)};
    // after rebuild_instances' uploads, so that the posed boxes land on the device copy of local_aabbs
    const std::function<void(float*)> work = [&](float* device_aabbs) {
        const auto bounds = [&] {
            launch_posed_bounds(K.table, posed, n, K.positions, (const hk_instance*)c->buf[4], count, device_aabbs, st);
        };
        if (refit) {
            timed(c, "refit_morph_vertices", st, [&] { launch_morph_vertices(K, st); });
            enqueue_mesh_refit(c, A.M, st);
            timed(c, "refit_morph_bounds", st, bounds);
            return;
        }
        timed(c, "morph_meshes", st, [&] {
            launch_morph_vertices(K, st);
            launch_mesh_update(A.M, st);
            refresh_blas_derivatives(c, st, c->count[2]);
            bounds();
        });
    };
    ml.device = A.M.levels;
    if (refit) ml.slice.clear();  // the topology stays, and so does every depth: no levels to read back
    return rebuild_instances(c, models, local_aabbs, count, st, &ml, nullptr, &work, refit_trees);
}
int hk_morph_meshes(hk_ctx* c, const hk_morph_pose* poses, uint32_t n, const float* models, const float* local_aabbs,
                    uint32_t count, void* stream)
{
    return morph_meshes(c, "hk_morph_meshes", false, false, poses, n, models, local_aabbs, count, stream);
}
int hk_morph_meshes_refit(hk_ctx* c, const hk_morph_pose* poses, uint32_t n, const float* models,
                          const float* local_aabbs, uint32_t count, void* stream)
{
    return morph_meshes(c, "hk_morph_meshes_refit", true, false, poses, n, models, local_aabbs, count, stream);
}
int hk_morph_meshes_refit_all(hk_ctx* c, const hk_morph_pose* poses, uint32_t n, const float* models,
                              const float* local_aabbs, uint32_t count, void* stream)
{
    return morph_meshes(c, "hk_morph_meshes_refit_all", true, true, poses, n, models, local_aabbs, count, stream);
}

// the checks hk_set_instances and hk_set_meshes share before the set is planned: the scene's BVHs can be rebuilt, and
// the previous indices name the set before, each once
static int set_args_ok(hk_ctx* c, const hk_instance_desc* set, uint32_t count, const char* who)
{
    HK_TRY(scene_rebuildable(c));
    std::vector<bool> taken(c->count[4], false);
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t p = set[i].previous;
        if (p == HK_INSTANCE_NEW) continue;
        const std::string at = std::string(who) + ": instance " + std::to_string(i);
        if (p >= c->count[4]) return fail(c, HK_ERR_INVALID, at + ": previous is not an index of the set before");
        if (taken[p]) return fail(c, HK_ERR_INVALID, at + ": previous is used twice");
        taken[p] = true;
    }
    return HK_OK;
}

int hk_set_instances(hk_ctx* c, const hk_instance_desc* set, const float* models, const float* local_aabbs,
                     uint32_t count, const hk_material* materials, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!set || !models || !local_aabbs) return fail(c, HK_ERR_INVALID, "hk_set_instances: null pointer");
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    HK_TRY(set_args_ok(c, set, count, "hk_set_instances"));
    (void)hipSetDevice(c->device);
    const std::vector<float> emissive = materials ? emissive_of(materials, c->count[6]) : c->emissive;
    SetChange change;
    std::string why;
    const int rc = plan_instance_set(c->count, c->meshes, emissive.data(), set, count,
                                     SliceReader{nullptr, c}, &change, &why);
    if (rc != HK_OK) return fail(c, rc, "hk_set_instances: " + why);
    change.materials = materials;
    return rebuild_instances(c, models, local_aabbs, count, pick(c, stream), nullptr, &change);
}

int hk_scene_counts(const hk_ctx* c, uint32_t counts[9])
{
    if (!c || !counts) return HK_ERR_INVALID;
    if (!c->has_scene) return HK_ERR_STATE;
    std::memcpy(counts, c->count, sizeof(c->count));
    return HK_OK;
}

// ---- hk_add_meshes
// What hk_add_meshes decides on the host before any device work: each mesh's appended slice, its triangles, the
// vertices its indices reach (MeshSlice::vertex_need, from the scan that refuses an index out of range) and the counts
// after.
struct MeshAddPlan {
    std::vector<hk_mesh_index> slices;
    std::vector<uint32_t> tris, vertex_need;
    uint32_t after[9] = {};
    uint64_t n_vertices = 0, n_shapes = 0, n_indices = 0;  // sums over the list (indices: of the indexed meshes)
};
constexpr uint64_t MESH_TOTAL_MAX = 0x40000000u;  // hk_update_meshes' bound on vertices and primitives

// hks_add_mesh's checks of one new mesh, in its order: null when it passes, with its triangles and the vertices its
// indices reach (plan_add_meshes and plan_set_meshes)
static const char* new_mesh_error(const hk_mesh_desc& m, uint32_t* tris_out, uint32_t* need_out)
{
    if (!m.positions) return "MissingAttributePosition";
    if (!m.normals) return "MissingAttributeNormal";
    if (!m.uvs) return "MissingAttributeUV";
    const uint32_t ni = m.indices ? m.index_count : m.vertex_count;
    uint32_t top = 0;
    if (m.indices) {
        for (uint32_t i = 0; i < ni; ++i) {
            if (m.indices[i] >= m.vertex_count) return "index out of range";
            top = std::max(top, m.indices[i]);
        }
    } else if (ni) {
        top = ni - 1u;
    }
    uint32_t tris = 0;
    if (m.topology == HKS_TRIANGLE_LIST) {
        if (ni % 3u != 0) return "IncompatiblePrimitiveTopology";
        tris = ni / 3u;
    } else if (m.topology == HKS_TRIANGLE_STRIP) {
        tris = ni >= 3u ? ni - 2u : 0u;
    } else {
        return "IncompatiblePrimitiveTopology";
    }
    if (tris == 0) return "NoPrimitive";
    *tris_out = tris;
    *need_out = top + 1u;
    return nullptr;
}

static int plan_add_meshes(const uint32_t* before, const hk_mesh_desc* meshes, uint32_t n, MeshAddPlan* out,
                           std::string* why)
{
    auto no = [&](const std::string& text) {
        *why = text;
        return HK_ERR_INVALID;
    };
    if (!meshes) return no("null mesh list");
    if (n == 0) return no("an empty mesh list");
    out->slices.resize(n);
    out->tris.resize(n);
    out->vertex_need.resize(n);
    uint64_t at[3] = {before[0], before[1], before[2]};
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_desc& m = meshes[k];
        const std::string who = "mesh " + std::to_string(k) + ": ";
        uint32_t tris = 0, need = 0;
        if (const char* text = new_mesh_error(m, &tris, &need)) return no(who + text);
        out->slices[k] = hk_mesh_index{(uint32_t)at[0], (uint32_t)at[1], {(uint32_t)at[2], 3u * tris - 2u}};
        out->tris[k] = tris;
        out->vertex_need[k] = need;
        at[0] += m.vertex_count;
        at[1] += tris;
        at[2] += 3u * (uint64_t)tris - 2u;
        out->n_vertices += m.vertex_count;
        out->n_shapes += tris;
        if (m.indices) out->n_indices += m.index_count;
        if (at[0] > MESH_TOTAL_MAX || at[1] > MESH_TOTAL_MAX || at[2] > MESH_TOTAL_MAX || out->n_indices > MESH_TOTAL_MAX)
            return no("too many vertices, primitives or nodes");
    }
    std::memcpy(out->after, before, sizeof(out->after));
    for (int i = 0; i < 3; ++i) out->after[i] = (uint32_t)at[i];
    return HK_OK;
}

// the message of the calling thread's last hk_add_meshes_counts / hk_set_meshes_counts, which have no context to keep
// it (empty: it succeeded), one string each; counts_refusal: a refusal of `call` kept in its string
static thread_local std::string counts_error, set_counts_error;
const char* hk_add_meshes_counts_error(void) { return counts_error.c_str(); }
const char* hk_set_meshes_counts_error(void) { return set_counts_error.c_str(); }
static int counts_refusal(std::string& kept, const char* call, const std::string& text)
{
    kept = std::string(call) + ": " + text;
    return HK_ERR_INVALID;
}

int hk_add_meshes_counts(const uint32_t before[9], const hk_mesh_desc* meshes, uint32_t mesh_count,
                         hk_mesh_index* slices, uint32_t after[9])
{
    counts_error.clear();
    if (!before) return counts_refusal(counts_error, "hk_add_meshes", "null counts");
    if (!slices) return counts_refusal(counts_error, "hk_add_meshes", "null slices");
    MeshAddPlan plan;
    std::string why;
    if (plan_add_meshes(before, meshes, mesh_count, &plan, &why) != HK_OK)
        return counts_refusal(counts_error, "hk_add_meshes", why);
    std::memcpy(slices, plan.slices.data(), plan.slices.size() * sizeof(hk_mesh_index));
    if (after) std::memcpy(after, plan.after, sizeof(plan.after));
    return HK_OK;
}

int hk_add_meshes(hk_ctx* c, const hk_mesh_desc* meshes, uint32_t mesh_count, hk_mesh_index* slices, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (!slices) return fail(c, HK_ERR_INVALID, "hk_add_meshes: null slices");
    MeshAddPlan plan;
    {
        std::string why;
        const int rc = plan_add_meshes(c->count, meshes, mesh_count, &plan, &why);
        if (rc != HK_OK) return fail(c, rc, "hk_add_meshes: " + why);
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.gb_serialize(false));
    std::vector<const hk_mesh_desc*> list(mesh_count);
    for (uint32_t k = 0; k < mesh_count; ++k) list[k] = meshes + k;
    MeshStaging stage;
    plan_mesh_staging(list, plan.slices.data(), plan.tris.data(), plan.n_vertices, plan.n_shapes, plan.n_indices, 0, &stage);
    // Room (hikari_amd.h hk_add_meshes "Capacity"): the grown arrays take their contents; the buffers they leave are
    // freed after the call's one wait, or on the way out
    Buffers old;
    HK_TRY(reserve_scene(c, "hk_add_meshes", plan.after, 7u, 7u, false, stage.total, 0, st, &old));
    MeshAddArgs A;
    HK_TRY(enqueue_mesh_staging(c, list, stage, st, &A, nullptr));
    std::vector<uint32_t> rows;  // the new meshes' rows of the per-node mesh tables
    HK_TRY(write_mesh_rows(c, plan.slices.data(), plan.slices.size(), st, &rows));
    timed(c, "add_meshes", st, [&] {
        launch_mesh_add(A, st);
        refresh_blas_derivatives(c, st, plan.after[2]);  // over the whole array, as hk_update_meshes
    });
    HK_HIP(c, hipGetLastError());
    std::vector<uint32_t> levels(mesh_count);
    HK_HIP(c, hipMemcpyAsync(levels.data(), A.M.levels, levels.size() * 4, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    // the counts, the registry and the G-buffer reuse generation move together, once the device is done
    for (int i = 0; i < 3; ++i) c->count[i] = plan.after[i];
    c->gen++;
    for (uint32_t k = 0; k < mesh_count; ++k) {
        c->meshes.push_back(hk_ctx::MeshSlice{plan.slices[k], plan.vertex_need[k], levels[k], 0u});
        slices[k] = plan.slices[k];
    }
    return HK_OK;
}

// ---- hk_set_meshes
// What hk_set_meshes decides on the host before any device work: every entry's slice in the new layout, the registry
// after the call (the list; a new entry's depth comes from its build), the new entries apart for the build, and the
// counts after.
struct MeshSetPlan {
    std::vector<hk_mesh_index> slices;
    std::vector<MeshMove> moves;               // one per entry, list order
    std::vector<hk_ctx::MeshSlice> registry;   // one per entry, list order
    std::vector<uint32_t> source_entry;        // the list index of each new entry
    std::vector<const hk_mesh_desc*> sources;  // the new entries, in list order, with their slices and triangles
    std::vector<hk_mesh_index> source_slices;
    std::vector<uint32_t> tris;
    uint32_t after[9] = {};
    uint64_t n_vertices = 0, n_shapes = 0, n_indices = 0;  // sums over the new entries
};

// known / rd: the context's registry and arrays; both null: the context-free arithmetic of hk_set_meshes_counts, which
// cannot look a kept slice up or read it back and checks it against the counts and the other kept slices alone.
static int plan_set_meshes(const uint32_t* before, const std::vector<hk_ctx::MeshSlice>* known, const SliceReader* rd,
                           const hk_mesh_entry* list, uint32_t n, MeshSetPlan* out, std::string* why)
{
    auto no = [&](const std::string& text) {
        *why = text;
        return HK_ERR_INVALID;
    };
    if (!list) return no("null mesh list");
    if (n == 0) return no("an empty mesh list");
    out->slices.resize(n);
    out->moves.resize(n);
    out->registry.resize(n);
    struct Kept {
        hk_mesh_index x;
        uint32_t vertices;
    };
    std::vector<Kept> kept;
    std::vector<hk_ctx::MeshSlice> fresh;  // the kept slices this call registers
    uint64_t at[3] = {0, 0, 0};
    for (uint32_t k = 0; k < n; ++k) {
        const hk_mesh_entry& e = list[k];
        const std::string who = "mesh " + std::to_string(k) + ": ";
        uint32_t tris = 0, need = 0, depth = 0, vertices = 0;
        MeshMove& mv = out->moves[k];
        if (e.source) {
            if (const char* text = new_mesh_error(*e.source, &tris, &need)) return no(who + text);
            vertices = e.source->vertex_count;
            mv.src[0] = mv.src[1] = mv.src[2] = MESH_MOVE_NEW;
            out->source_entry.push_back(k);
            out->sources.push_back(e.source);
            out->tris.push_back(tris);
            out->n_vertices += vertices;
            out->n_shapes += tris;
            if (e.source->indices) out->n_indices += e.source->index_count;
        } else {
            const hk_mesh_index& x = e.keep;
            vertices = e.vertex_count;
            if (const char* text = slice_shape_error(x, before)) return no(who + "kept slice refused: " + text);
            tris = (x.node[1] + 2u) / 3u;
            for (const Kept& o : kept)
                if (std::memcmp(&o.x, &x, sizeof(x)) == 0) return no(who + "the slice is kept twice");
            if (known) {
                const size_t at = find_slice(*known, x);
                const hk_ctx::MeshSlice* s = at < known->size() ? &(*known)[at] : nullptr;
                hk_ctx::MeshSlice f;
                if (!s) {
                    std::string text;
                    const int rc = check_new_slice(x, before, *known, fresh, *rd, &f, &text);
                    if (rc != HK_OK) {
                        *why = who + "kept slice refused: " + text;
                        return rc;
                    }
                    fresh.push_back(f);
                    s = &f;
                }
                if (s->vertex_need == HK_U32_MAX)
                    return no(who + "kept slice refused: its BLAS is not 3k - 2 nodes over k primitives of the scene");
                need = s->vertex_need;
                depth = s->depth;
            }
            if (vertices < std::max(need, 1u))
                return no(who + "vertex_count does not cover the vertex indices of its primitives");
            if ((uint64_t)x.vertex + vertices > before[0]) return no(who + "vertex_count reaches past the vertex array");
            for (const Kept& o : kept) {
                if (ranges_meet(x.primitive, tris, o.x.primitive, (o.x.node[1] + 2u) / 3u) ||
                    ranges_meet(x.node[0], x.node[1], o.x.node[0], o.x.node[1]))
                    return no(who + "it partly overlaps another kept slice");
                if (ranges_meet(x.vertex, vertices, o.x.vertex, o.vertices))
                    return no(who + "vertex_count reaches into another kept slice's vertices");
            }
            kept.push_back(Kept{x, vertices});
            mv.src[0] = x.vertex;
            mv.src[1] = x.primitive;
            mv.src[2] = x.node[0];
        }
        const uint32_t nodes = 3u * tris - 2u;
        const hk_mesh_index to{(uint32_t)at[0], (uint32_t)at[1], {(uint32_t)at[2], nodes}};
        out->slices[k] = to;
        if (e.source) out->source_slices.push_back(to);
        out->registry[k] = hk_ctx::MeshSlice{to, need, depth, 0u};
        mv.dst[0] = to.vertex;
        mv.dst[1] = to.primitive;
        mv.dst[2] = to.node[0];
        mv.count[0] = vertices;
        mv.count[1] = tris;
        mv.count[2] = nodes;
        at[0] += vertices;
        at[1] += tris;
        at[2] += nodes;
        if (at[0] > MESH_TOTAL_MAX || at[1] > MESH_TOTAL_MAX || at[2] > MESH_TOTAL_MAX || out->n_indices > MESH_TOTAL_MAX)
            return no("too many vertices, primitives or nodes");
    }
    std::memcpy(out->after, before, sizeof(out->after));
    for (int i = 0; i < 3; ++i) out->after[i] = (uint32_t)at[i];
    return HK_OK;
}

int hk_set_meshes_counts(const uint32_t before[9], const hk_mesh_entry* list, uint32_t mesh_count, hk_mesh_index* slices,
                         uint32_t after[9])
{
    set_counts_error.clear();
    if (!before) return counts_refusal(set_counts_error, "hk_set_meshes", "null counts");
    if (!slices) return counts_refusal(set_counts_error, "hk_set_meshes", "null slices");
    MeshSetPlan plan;
    std::string why;
    if (plan_set_meshes(before, nullptr, nullptr, list, mesh_count, &plan, &why) != HK_OK)
        return counts_refusal(set_counts_error, "hk_set_meshes", why);
    std::memcpy(slices, plan.slices.data(), plan.slices.size() * sizeof(hk_mesh_index));
    if (after) std::memcpy(after, plan.after, sizeof(plan.after));
    return HK_OK;
}

int hk_set_meshes(hk_ctx* c, const hk_mesh_entry* list, uint32_t mesh_count, hk_mesh_index* slices,
                  const hk_instance_desc* set, const float* models, const float* local_aabbs, uint32_t count,
                  const hk_material* materials, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (!slices) return fail(c, HK_ERR_INVALID, "hk_set_meshes: null slices");
    if (!set || !models || !local_aabbs) return fail(c, HK_ERR_INVALID, "hk_set_meshes: null pointer");
    (void)hipSetDevice(c->device);
    // everything the host can refuse, first: the list against the current arrays and registry, then the set against
    // the new ones
    const SliceReader rd{nullptr, c};
    MeshSetPlan plan;
    std::string why;
    int rc = plan_set_meshes(c->count, &c->meshes, &rd, list, mesh_count, &plan, &why);
    if (rc != HK_OK) return fail(c, rc, "hk_set_meshes: " + why);
    HK_TRY(set_args_ok(c, set, count, "hk_set_meshes"));
    const std::vector<float> emissive = materials ? emissive_of(materials, c->count[6]) : c->emissive;
    SetChange change;
    rc = plan_instance_set(plan.after, plan.registry, emissive.data(), set, count, rd, &change, &why, true);
    if (rc != HK_OK) return fail(c, rc, "hk_set_meshes: " + why);
    change.materials = materials;
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.gb_serialize(false));
    const uint32_t n_sources = (uint32_t)plan.sources.size();
    MeshStaging stage;
    plan_mesh_staging(plan.sources, plan.source_slices.data(), plan.tris.data(), plan.n_vertices, plan.n_shapes,
                      plan.n_indices, (size_t)mesh_count * sizeof(MeshMove), &stage);
    // Room (hikari_amd.h hk_set_meshes "Capacity").  The move is out of place: arrays 0-2 are written into their spares,
    // which are then the arrays, and the arrays the spares.  The derivatives, which are rewritten whole, are allocated
    // anew only where the node capacity grows.
    Buffers old;
    HK_TRY(reserve_scene(c, "hk_set_meshes", plan.after, 7u, 0u, true, stage.total, 0, st, &old));
    HK_HIP(c, hipMemsetAsync(c->blas_aux, 0xFF, c->aux_stride * 12, st));  // (behind the count: U32_MAX, as at upload)
    MeshAddArgs A;
    char* table = nullptr;
    HK_TRY(enqueue_mesh_staging(c, plan.sources, stage, st, &A, &table));
    HK_HIP(c, hipMemcpyAsync(table, plan.moves.data(), (size_t)mesh_count * sizeof(MeshMove), hipMemcpyHostToDevice, st));
    MeshMoveArgs V;
    V.table = (const MeshMove*)table;
    V.n_meshes = mesh_count;
    V.n_vertices = plan.after[0];
    V.n_prims = plan.after[1];
    V.n_nodes = plan.after[2];
    for (int i = 0; i < 3; ++i) {
        V.src[i] = c->spare[i];  // (the array as it was)
        V.dst[i] = c->buf[i];
    }
    V.aux = c->blas_aux;
    V.stride = c->aux_stride;
    timed(c, "move_meshes", st, [&] { launch_mesh_move(V, st); });
    timed(c, "set_meshes", st, [&] {
        if (n_sources) launch_mesh_add(A, st);
        refresh_blas_derivatives(c, st, plan.after[2]);
    });
    HK_HIP(c, hipGetLastError());
    std::vector<uint32_t> levels(n_sources);
    if (n_sources) HK_HIP(c, hipMemcpyAsync(levels.data(), A.M.levels, levels.size() * 4, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    // the counts and the registry move together, once the device is done; then the set, planned against them
    for (uint32_t k = 0; k < n_sources; ++k) plan.registry[plan.source_entry[k]].depth = levels[k];
    for (int i = 0; i < 3; ++i) c->count[i] = plan.after[i];
    c->meshes = plan.registry;
    c->skins.clear();  // (the slices moved: hk_set_mesh_skins registers the new ones)
    c->morphs.clear();  // (and hk_set_mesh_morphs)
    std::memcpy(slices, plan.slices.data(), plan.slices.size() * sizeof(hk_mesh_index));
    return rebuild_instances(c, models, local_aabbs, count, st, nullptr, &change);
}

int hk_scene_capacity(const hk_ctx* c, uint32_t capacity[9])
{
    if (!c || !capacity) return HK_ERR_INVALID;
    if (!c->has_scene) return HK_ERR_STATE;
    for (int i = 0; i < 9; ++i) capacity[i] = (uint32_t)c->cap[i];
    return HK_OK;
}

int hk_scene_shared_transform(const hk_ctx* c, int32_t* shared)
{
    if (!c || !shared) return HK_ERR_INVALID;
    if (!c->has_scene) return HK_ERR_STATE;
    *shared = c->shared_transform ? 1 : 0;
    return HK_OK;
}

int hk_tile_skip_info(const hk_ctx* c, uint32_t skipped[3], int32_t bound[4], int32_t* bounded)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->sized) return HK_ERR_STATE;
    if (skipped)
        for (int k = 0; k < 3; ++k) skipped[k] = c->tiles_skipped[k];
    const PxRect& r = c->grect[c->sch.gslot];
    const bool none = r.x1 == INT32_MAX;
    if (bound) {
        bound[0] = none ? 0 : r.x0;
        bound[1] = none ? 0 : r.y0;
        bound[2] = none ? (int32_t)c->S[0] : r.x1;
        bound[3] = none ? (int32_t)c->S[1] : r.y1;
    }
    if (bounded) *bounded = none ? 0 : 1;
    return HK_OK;
}

int hk_tone_skip_info(const hk_ctx* c, uint64_t* skipped_pixels, int32_t rect[4])
{
    if (!c) return HK_ERR_INVALID;
    if (!c->sized) return HK_ERR_STATE;
    if (skipped_pixels) *skipped_pixels = c->tone_skipped;
    if (rect)
        for (int k = 0; k < 4; ++k) rect[k] = c->tone_rect[k];
    return HK_OK;
}

int hk_instance_set_counts(const hk_scene_desc* d, const hk_instance_desc* set, uint32_t count,
                           const hk_material* materials, uint32_t counts[9])
{
    if (!d || !set || !counts || !scene_desc_ok(d)) return HK_ERR_INVALID;
    std::vector<hk_ctx::MeshSlice> known;
    if (!host_registry(d, &known)) return HK_ERR_INVALID;
    const std::vector<float> emissive =
        emissive_of(materials ? materials : (const hk_material*)d->materials.data, d->materials.count);
    SetChange change;
    std::string why;
    const int rc = plan_instance_set(desc_counts(d).data(), known, emissive.data(), set, count, SliceReader{d, nullptr},
                                     &change, &why);
    if (rc != HK_OK) return rc;
    std::memcpy(counts, change.counts, sizeof(change.counts));
    return HK_OK;
}

int hk_read_scene_array(hk_ctx* c, int array, void* dst, size_t bytes)
{
    if (!c || !dst || array < 0 || array > 8) return HK_ERR_INVALID;
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    const size_t have = (size_t)c->count[array] * SCENE_ELEM[array];
    if (bytes < have) return fail(c, HK_ERR_INVALID, "destination too small");
    (void)hipSetDevice(c->device);
    HK_HIP(c, hipStreamSynchronize(c->stream));
    if (have) HK_HIP(c, hipMemcpy(dst, c->buf[array], have, hipMemcpyDeviceToHost));
    return HK_OK;
}

int hk_texture_upload(hk_ctx* c, const hk_texture* t, uint32_t count)
{
    if (!c || (count && !t)) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    HK_TRY(c->sch.gb_serialize(true));
    std::vector<hk_texture_desc> desc(count);
    uint64_t total = 0;
    c->gen++;
    for (uint32_t i = 0; i < count; ++i) {
        if (!t[i].width || !t[i].height || !t[i].rgba8) return fail(c, HK_ERR_INVALID, "texture without texels");
        if (t[i].format > HK_TEXTURE_RGBA8_UNORM || t[i].address_u > HK_ADDRESS_MIRROR_REPEAT ||
            t[i].address_v > HK_ADDRESS_MIRROR_REPEAT || t[i].filter > HK_FILTER_LINEAR)
            return fail(c, HK_ERR_INVALID, "unknown texture format / address mode / filter");
        desc[i] = hk_texture_desc{(uint32_t)total, t[i].width, t[i].height, t[i].format, t[i].address_u,
                                  t[i].address_v, t[i].filter, 0u};
        total += (uint64_t)t[i].width * t[i].height;
        if (total > 0xFFFFFFFFull) return fail(c, HK_ERR_INVALID, "more than 2^32 texels");
    }
    HK_HIP(c, hipStreamSynchronize(c->stream));
    release(c->tex_desc);
    release(c->texels);
    c->n_textures = 0;
    if (count == 0) return HK_OK;
    if (!c->tex_lut) {
        float lut[512];
        hk_texture_build_lut(lut);
        HK_HIP(c, hipMalloc(&c->tex_lut, sizeof(lut)));
        HK_HIP(c, hipMemcpy(c->tex_lut, lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    HK_HIP(c, hipMalloc(&c->tex_desc, count * sizeof(hk_texture_desc)));
    HK_HIP(c, hipMemcpy(c->tex_desc, desc.data(), count * sizeof(hk_texture_desc), hipMemcpyHostToDevice));
    HK_HIP(c, hipMalloc(&c->texels, total * 4));
    for (uint32_t i = 0; i < count; ++i)
        HK_HIP(c, hipMemcpy(c->texels + desc[i].offset, t[i].rgba8, (size_t)t[i].width * t[i].height * 4,
                            hipMemcpyHostToDevice));
    c->n_textures = count;
    return HK_OK;
}

int hk_set_noise(hk_ctx* c, const uint8_t* rgba, uint32_t count, uint32_t size)
{
    if (!c || !rgba) return HK_ERR_INVALID;
    if (count != 16 || size != 64) return fail(c, HK_ERR_INVALID, "blue noise must be 16 textures of 64x64 RGBA8");
    (void)hipSetDevice(c->device);
    HK_TRY(c->sch.gb_serialize(true));
    if (!c->noise) HK_HIP(c, hipMalloc(&c->noise, 16 * 64 * 64 * 4));
    HK_HIP(c, hipMemcpy(c->noise, rgba, 16 * 64 * 64 * 4, hipMemcpyHostToDevice));
    c->has_noise = true;
    return HK_OK;
}

static int resize_impl(hk_ctx* c, uint32_t width, uint32_t height, float ratio, uint32_t band_y0, uint32_t band_rows,
                       uint32_t stripe_n, uint32_t stripe_k, uint32_t col0 = 0u, uint32_t cols = 0u);

int hk_resize(hk_ctx* c, uint32_t width, uint32_t height, float ratio, uint32_t band_y0, uint32_t band_rows)
{
    return resize_impl(c, width, height, ratio, band_y0, band_rows, 0u, 0u);
}

int hk_resize_tile(hk_ctx* c, uint32_t width, uint32_t height, uint32_t x0, uint32_t cols, uint32_t y0, uint32_t rows)
{
    if (!c || cols == 0 || rows == 0) return HK_ERR_INVALID;
    if (x0 + cols > width || y0 + rows > height) return fail(c, HK_ERR_INVALID, "tile outside the frame");
    return resize_impl(c, width, height, 1.0f, y0, rows, 0u, 0u, x0, cols);
}

int hk_tile_info(const hk_ctx* c, int32_t* col0, int32_t* cols)
{
    if (!c || !c->sized) return HK_ERR_STATE;
    if (col0) *col0 = c->core_col0;
    if (cols) *cols = c->core_cols;
    return HK_OK;
}

int hk_resize_striped(hk_ctx* c, uint32_t width, uint32_t height, uint32_t rank, uint32_t world)
{
    if (!c || world == 0 || rank >= world) return HK_ERR_INVALID;
    if (world == 1) return resize_impl(c, width, height, 1.0f, 0u, 0u, 0u, 0u);
    return resize_impl(c, width, height, 1.0f, 0u, 0u, world, rank);
}

static int resize_impl(hk_ctx* c, uint32_t width, uint32_t height, float ratio, uint32_t band_y0, uint32_t band_rows,
                       uint32_t stripe_n, uint32_t stripe_k, uint32_t col0, uint32_t cols)
{
    if (!c || width == 0 || height == 0) return HK_ERR_INVALID;
    if (cols == 0) {
        col0 = 0;
        cols = width;
    }
    (void)hipSetDevice(c->device);
    ratio = ratio < 1.0f ? 1.0f : (ratio > 2.0f ? 2.0f : ratio);  // Upscale::ratio (lib.rs:501-505)
    if (band_rows == 0) {
        band_y0 = 0;
        band_rows = height;
    }
    if (band_y0 + band_rows > height) return fail(c, HK_ERR_INVALID, "band outside the frame");
    bool whole = band_y0 == 0 && band_rows == height;
    if (!whole && ratio != 1.0f) return fail(c, HK_ERR_INVALID, "row bands require upscale ratio 1.0");
    const bool tile_cols = cols < width;
    if (tile_cols && (ratio != 1.0f || stripe_n >= 2)) return fail(c, HK_ERR_INVALID, "tiles require upscale ratio 1.0");
    uint32_t stripe_rows = 0;  // rows of stripes k, k + n, ... (STRIPE_H rows each, the last one may be short)
    if (stripe_n >= 2) {
        if (stripe_n > (height + STRIPE_H - 1) / STRIPE_H)
            return fail(c, HK_ERR_INVALID, "more stripe ranks than stripes in the frame");
        for (uint32_t t = stripe_k; t * STRIPE_H < height; t += stripe_n)
            stripe_rows += height - t * STRIPE_H < (uint32_t)STRIPE_H ? height - t * STRIPE_H : (uint32_t)STRIPE_H;
        whole = false;
    }
    HK_HIP(c, hipStreamSynchronize(c->stream));
    HK_HIP(c, hipStreamSynchronize(c->sch.gb_stream));
    HK_HIP(c, hipStreamSynchronize(c->sch.dn_stream));
    free_targets(c);
    c->gen++;
    c->albedo_fresh = false;
    c->S[0] = width;
    c->S[1] = height;
    c->ratio = ratio;
    float scale = 1.0f / ratio;  // light.rs:318-319: ceil(scale * size)
    c->s[0] = (uint32_t)std::ceil(scale * (float)width);
    c->s[1] = (uint32_t)std::ceil(scale * (float)height);
    c->stripe_n = (int32_t)stripe_n;
    c->stripe_k = (int32_t)stripe_k;
    c->core_col0 = (int32_t)col0;
    c->core_cols = (int32_t)cols;
    if (stripe_n >= 2) {
        c->S_row0 = c->s_row0 = 0;
        c->S_rows = c->s_rows = (int32_t)stripe_rows;
        c->core_row0 = 0;
        c->core_rows = (int32_t)stripe_rows;
    } else if (whole) {
        c->S_row0 = 0;
        c->S_rows = (int32_t)height;
        c->s_row0 = 0;
        c->s_rows = (int32_t)c->s[1];
        c->core_row0 = 0;
        c->core_rows = (int32_t)c->s[1];
    } else {
        int32_t r0 = (int32_t)band_y0 - c->halo;
        int32_t r1 = (int32_t)(band_y0 + band_rows) + c->halo;
        r0 = r0 < 0 ? 0 : r0;
        r1 = r1 > (int32_t)height ? (int32_t)height : r1;
        c->S_row0 = c->s_row0 = r0;
        c->S_rows = c->s_rows = r1 - r0;
        c->core_row0 = (int32_t)band_y0 - r0;
        c->core_rows = (int32_t)band_rows;
    }
    const size_t SP = (size_t)width * c->S_rows, sp = (size_t)c->s[0] * c->s_rows;
    c->res_n = (uint32_t)sp;
    c->win_out = c->win_emi = c->win_ind = -1;
    for (const Target& t : targets(c)) {
        if (!t.plane) continue;
        const size_t bytes = (t.plane == 'S' ? SP : sp) * t.bpp * t.mult;
        HK_HIP(c, hipMalloc(t.ptr, bytes));
        if (t.zero) HK_HIP(c, hipMemset(*t.ptr, 0, bytes));
    }
    HK_HIP(c, hipDeviceSynchronize());
    c->sized = true;
    return HK_OK;
}

int hk_set_band_halo(hk_ctx* c, uint32_t rows)
{
    if (!c || rows > 4096) return HK_ERR_INVALID;
    c->halo = (int32_t)rows;
    c->bg_valid[0] = c->bg_valid[1] = false;
    c->gen++;
    return HK_OK;
}

int hk_band_info(const hk_ctx* c, int32_t* row0, int32_t* rows, int32_t* core_row0, int32_t* core_rows)
{
    if (!c || !c->sized) return HK_ERR_STATE;
    if (row0) *row0 = c->s_row0;
    if (rows) *rows = c->s_rows;
    if (core_row0) *core_row0 = c->core_row0;
    if (core_rows) *core_rows = c->core_rows;
    return HK_OK;
}

int hk_render_gbuffer(hk_ctx* c, const hk_frame_inputs* in, void* stream)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!in) return fail(c, HK_ERR_INVALID, "null frame inputs");
    if (c->gb_stack_need > (uint32_t)GB_STACK)
        return fail(c, HK_ERR_INVALID, "scene BVH too deep for the G-buffer traversal stack (TLAS + BLAS depth > 64)");
    if (in->jitter > HK_JITTER_TAA_SMAA) return fail(c, HK_ERR_INVALID, "unknown jitter mode");
    (void)hipSetDevice(c->device);
    hipStream_t st = pick_frame(c, stream);
    // Pipelining: this frame's planes go to the slot frame f-2 used.  Its readers are the work
    // enqueued on the caller's stream before the previous hk_render_gbuffer call (frame f-2's
    // passes, denoise, tone-sum, readbacks) and a post-process of frame f-1 (it reads the previous
    // slot); k_gbuffer waits for exactly those on gb_stream and so overlaps frame f-1's light
    // passes.  A scene / size / plane change since the last call serialises it instead.
    const bool pipeline = c->on(OPT_GBUFFER_PIPELINE);
    // Event markers are recorded only on the pipelined path: each one between two kernels of a stream
    // costs it ~6 us (cornell 8-way stripe, where the serial frame is 3 kernels), and the serial path
    // has no other stream waiting on them.
    FrameSchedule& q = c->sch;
    const uint32_t e = q.gb_calls & 1u;
    hipStream_t gs = st;
    // G-buffer reuse: the slot this frame's planes go to (the other one) already holds exactly them when the
    // k_gbuffer that wrote it saw the same view, jitter and band window, nothing it reads changed since
    // (generation) and nothing moved (no motion vectors: the velocity plane is zero in both).  The planes
    // then stay as they are, bit for bit what a new trace would store (the 16
    // sub-frames of a displayed frame share camera and scene).  Only the primary-ray counter differs: it
    // counts rays traced.
    hk_ctx::GbSig sig;
    std::memset(&sig, 0, sizeof(sig));
    {
        float* v = sig.view;
        for (int i = 0; i < 3; ++i) *v++ = in->view.world_position[i];
        for (int i = 0; i < 16; ++i) *v++ = in->view.view_proj[i];
        for (int i = 0; i < 16; ++i) *v++ = in->view.inverse_view_proj[i];
        for (int i = 0; i < 16; ++i) *v++ = in->has_previous_view ? in->previous_view_proj[i] : in->view.view_proj[i];
        *v++ = in->view.projection[15];
        *v++ = (float)in->jitter;
        sig.gen = c->gen;
        sig.valid = true;
    }
    const bool jitter_static = in->jitter == HK_JITTER_NONE;
    const bool still = !c->models_dirty &&
                       std::memcmp(sig.view + 3, sig.view + 3 + 32, 16 * sizeof(float)) == 0;  // previous view = view
    const bool pipe = pipeline && pipeline_size(c) && !q.gb_serial && q.gb_calls > 0;
    q.entry_other[e] = q.other_picks;
    q.entry_epoch[e] = q.frame_st_epoch;
    q.entry_rf[e] = q.rf_seq;
    q.entry_clean[e] = q.rf_seq > 0 && q.rf_rec_seq == q.rf_seq && q.other_picks == q.rf_other && q.frame_st_epoch == q.rf_epoch;
    q.gb_tail_seq = 0;
    q.gb_wait_valid = false;
    // a new frame: this frame's planes replace the previous ones (prepass.rs:309-317); the one whole-slot swap
    auto next_slot = [&] {
        std::swap(c->g, c->g_prev);
        q.gslot ^= 1u;
        c->head = in->frame_number & 1u;
        c->timing_frame = in->frame_number % c->timing_every == 0u;
    };
    {
        const uint32_t next = q.gslot ^ 1u;  // the slot this frame's planes go to
        FrameArgs W = pass_window(c, frame_args(c, nullptr, in), GBUFFER_REACH);
        sig.win[0] = W.F.win_row0;
        sig.win[1] = W.F.win_rows;
        const hk_ctx::GbSig& have = c->gsig[next];
        if (c->on(OPT_GBUFFER_REUSE) && still && jitter_static && have.valid && c->velocity_zero &&
            c->albedo_fresh && have.gen == sig.gen && have.win[0] == sig.win[0] &&
            have.win[1] == sig.win[1] && std::memcmp(have.view, sig.view, sizeof(sig.view)) == 0 && !q.gb_serial && q.gb_calls > 0) {
            // (the previous frame's G-buffer came from k_gbuffer too — albedo_fresh, velocity_zero — so both
            // slots hold traced planes of a still camera)
            next_slot();
            // (post_pending stays: a post-process read both slots, and the next launch overwrites one)
            // no launch to reason about: the next hk_render_frame records its fork marker
            q.gb_call_rec = false;
            q.gb_on_gs = false;
            q.gb_calls++;
            c->primary_reused += gbuffer_primary_rays(W);
            c->tiles_skipped[0] = 0;  // (no launch)
            return HK_OK;
        }
    }
    if (pipe) {
        HK_HIP(c, hipEventRecord(q.ev_gb_call[e], st));
        gs = q.gb_stream;
        // the caller stream at the previous call's entry; when that call was serial (its k_gbuffer ran
        // on st, no record), the caller stream now.  The previous pipelined k_gbuffer is earlier on gs.
        const uint32_t w = q.gb_call_rec ? e ^ 1u : e;
        const uint32_t g = q.gslot ^ 1u;
        if (!q.tail_covers(w, g)) HK_HIP(c, hipStreamWaitEvent(gs, q.ev_gb_call[w], 0));
        q.gb_wait_valid = true;
        q.gb_wait_other = q.entry_other[w];
        q.gb_wait_epoch = q.entry_epoch[w];
        if (q.post_pending) HK_HIP(c, hipStreamWaitEvent(gs, q.ev_post, 0));
        if (q.gslot_rec[g]) {
            HK_HIP(c, hipStreamWaitEvent(gs, q.ev_gslot[g], 0));
            q.gb_tail_seq = q.gslot_seq[g];
        }
    } else {
        HK_TRY(q.gb_join(st));
    }
    q.post_pending = false;
    next_slot();
    FrameArgs A = frame_args(c, nullptr, in);
    ViewArgs V;
    for (int i = 0; i < 3; ++i) V.world_position[i] = in->view.world_position[i];
    std::memcpy(V.view_proj, in->view.view_proj, sizeof(V.view_proj));
    std::memcpy(V.inverse_view_proj, in->view.inverse_view_proj, sizeof(V.inverse_view_proj));
    // prepass.wgsl:30-38 frame_jitter (HALTON, view.rs:130-139), in pixels (jitter = 2 h / viewport
    // in NDC, added to clip.xy with y flipped: the surface point seen at a pixel centre c is the one
    // that projects to c - h without jitter)
    static const float HALTON[8][4] = {
        {0.000000f, 0.000000f, 0.500000f, 0.333333f}, {0.250000f, 0.666667f, 0.750000f, 0.111111f},
        {0.125000f, 0.444444f, 0.625000f, 0.777778f}, {0.375000f, 0.222222f, 0.875000f, 0.555556f},
        {0.062500f, 0.888889f, 0.562500f, 0.037037f}, {0.312500f, 0.370370f, 0.812500f, 0.703704f},
        {0.187500f, 0.148148f, 0.687500f, 0.481481f}, {0.437500f, 0.814815f, 0.937500f, 0.259259f}};
    V.jitter[0] = V.jitter[1] = 0.0f;
    if (in->jitter != HK_JITTER_NONE) {
        const uint32_t index = in->jitter == HK_JITTER_TAA_SMAA ? (in->frame_number >> 1) & 15u : in->frame_number & 15u;
        const float* h = HALTON[index >> 1];
        V.jitter[0] = (index & 1u) == 0u ? h[0] : h[2];
        V.jitter[1] = (index & 1u) == 0u ? h[1] : h[3];
    }
    // motion vectors: previous view (PreviousViewUniform) and previous models (GlobalTransformQueue)
    const float* pvp = in->has_previous_view ? in->previous_view_proj : in->view.view_proj;
    std::memcpy(V.previous_view_proj, pvp, sizeof(V.previous_view_proj));
    V.motion = (c->models_dirty || std::memcmp(pvp, in->view.view_proj, sizeof(V.previous_view_proj)) != 0) ? 1 : 0;
    V.previous_models = c->prev_models;
    c->velocity_zero = V.motion == 0;
    // full_screen_albedo is fused into the G-buffer kernel (it has every input in registers);
    // hk_render_frame runs it on its own only for host-supplied G-buffers
    A = pass_window(c, A, GBUFFER_REACH);
    V.bg = nullptr;
    V.bg_need = 0;
    // background tile skip: this frame's screen bound of the scene, kept with the slot for the light passes
    V.keep = TILE_KEEP_ALL;
    V.skipped_primary = 0;
    c->tiles_skipped[0] = 0;
    PxRect now = PxRect::all();
    int32_t bound[4];
    if (c->scene_box_valid && hks_screen_bounds(c->scene_box, &in->view, c->S[0], c->S[1], TILE_SKIP_GUARD, bound))
        now = PxRect{bound[0], bound[1], bound[2], bound[3]};
    c->grect[q.gslot] = now;
    if (bg_elision_off(c)) {
        c->gb_valid = false;  // the mask is rebuilt from zero when elision is switched back on
        c->gb_hist.reset();
    } else {
        if (!c->gb_valid || c->gb_key[0] != A.F.win_row0 || c->gb_key[1] != A.F.win_rows) {
            HK_HIP(c, hipMemsetAsync(c->gbmask, 0, (size_t)c->S[0] * c->S_rows, gs));
            c->gb_valid = true;
            c->gb_key[0] = A.F.win_row0;
            c->gb_key[1] = A.F.win_rows;
            c->gb_hist.reset();
        }
        V.bg = c->gbmask;
        V.bg_need = 1u << q.gslot;  // the planes' physical slot (swapped with gslot above)
        // a tile outside the bounds of every launch since this slot's last one holds the slot's bit in every byte
        // (MaskHistory): its workgroup would trace 256 misses and store nothing
        PxRect keep;
        if (c->gb_hist.launch(V.bg_need, now, keep) && c->on(OPT_BG_TILE_SKIP)) {
            V.keep = tile_keep(A, c->S[0], c->S_row0, c->S_rows, keep, &c->tiles_skipped[0]);
            if (c->tiles_skipped[0]) V.skipped_primary = (uint32_t)gbuffer_skipped_rays(A, V.keep);
        }
    }
    for (const void* plane : std::initializer_list<const void*>{c->g.position, c->g.velocity_uv, c->g.normal, c->g.depth_gradient,
                                                                c->g.instance_material, c->g.albedo})
        HK_TRY(q.ext_wait(gs, plane));
    timed(c, "gbuffer", gs, [&] { launch_gbuffer(A, V, c->g.albedo, c->gb_stack_need, gs); });
    sig.win[0] = A.F.win_row0;
    sig.win[1] = A.F.win_rows;
    sig.valid = V.motion == 0;
    c->gsig[q.gslot] = sig;
    if (c->models_dirty) {  // this frame's models become the next frame's previous ones
        HK_HIP(c, hipMemcpy2DAsync(c->prev_models, 64, (const char*)c->buf[4] + offsetof(hk_instance, model),
                                   sizeof(hk_instance), 64, c->count[4], hipMemcpyDeviceToDevice, gs));
        c->models_dirty = false;
    }
    if (gs != st) {
        HK_HIP(c, hipEventRecord(q.ev_gb_done, gs));
        q.gb_pending = true;
    }
    q.gb_call_rec = pipe;
    q.gb_on_gs = gs != st;
    q.gb_serial = false;
    q.gb_calls++;
    c->albedo_fresh = true;
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

int hk_set_gbuffer_plane(hk_ctx* c, int plane, const void* data, size_t bytes, int device_ptr, void* stream)
{
    if (!c || !data) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    c->albedo_fresh = false;
    size_t SP = (size_t)c->S[0] * c->S_rows;
    void* dst = nullptr;
    size_t need = 0;
    switch (plane) {
    case 0: dst = c->g.position; need = SP * 16; break;
    case 1: dst = c->g.normal; need = SP * 4; break;
    case 2: dst = c->g.depth_gradient; need = SP * 8; break;
    case 3: dst = c->g.instance_material; need = SP * 8; break;
    case 4: dst = c->g.velocity_uv; need = SP * 16; break;
    default: return fail(c, HK_ERR_INVALID, "unknown G-buffer plane");
    }
    if (bytes != need) return fail(c, HK_ERR_INVALID, "G-buffer plane size mismatch");
    c->gen++;
    c->gb_valid = false;  // host planes: the G-buffer elision mask no longer describes the slots
    c->grect[0] = c->grect[1] = PxRect::all();  // ... nor does a screen bound
    c->tiles_skipped[0] = 0;
    // host planes may carry any velocity: the identity-reprojection paths (fused launch, band row windows,
    // the direct pair's elision) stay off until the next k_gbuffer of a static frame
    c->velocity_zero = false;
    // a new frame's position / velocity plane: the current one becomes the previous (prepass.rs:309-317)
    if (plane == 0) {
        std::swap(c->g.position, c->g_prev.position);
        dst = c->g.position;
    } else if (plane == 4) {
        std::swap(c->g.velocity_uv, c->g_prev.velocity_uv);
        dst = c->g.velocity_uv;
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.ext_wait(st, dst));
    HK_TRY(c->sch.gb_serialize(false));
    HK_HIP(c, hipMemcpyAsync(dst, data, bytes, device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!device_ptr) HK_HIP(c, hipStreamSynchronize(st));
    return HK_OK;
}

static ChannelArgs channel(hk_ctx* c, uint32_t number, int ch)
{
    // LightBindGroup reservoir pairs (light.rs:518-546); head = frame % 2 (light.rs:376)
    static const int pairs[3][2] = {{0, 4}, {2, 4}, {6, 8}};
    uint32_t current = number % 2u, previous = 1u - current;
    ChannelArgs C;
    C.bg = nullptr;
    C.bg_need = 0;
    C.view = nullptr;
    C.view_n = 0;
    C.prev = ResBuf{c->reservoirs[current + pairs[ch][0]], c->res_n};
    C.cur = ResBuf{c->reservoirs[previous + pairs[ch][0]], c->res_n};
    C.prev_spatial = ResBuf{c->reservoirs[current + pairs[ch][1]], c->res_n};
    C.spatial = ResBuf{c->reservoirs[previous + pairs[ch][1]], c->res_n};
    C.variance = c->variance[ch];
    C.render = c->render[ch];
    return C;
}

// The background elision mask k (0: direct/emissive pair, 1: indirect) for a launch over window A
// of this frame, or nullptr when the launch does not use it (use = false: another kernel writes the
// channel's targets this frame, so the mask is dropped and rebuilt from zero the next time).
// K: the launch's tiles under the background tile skip.  A tile is left out when the G-buffer the pass reads (use:
// k_gbuffer's, at ratio 1; its screen bound is grect) is background on all of it and every byte there holds all of
// bg_need (MaskHistory) — with the pair among them: without it a background pixel still stores the pair (BG_SKIP_OWN:
// the direct pair under motion, a channel whose spatial reuse rewrites it).
static int bg_mask(hk_ctx* c, int k, const FrameArgs& A, bool use, bool pair, hipStream_t st, ChannelArgs& C, TileKeep& K)
{
    C.bg = nullptr;
    C.bg_need = 0;
    K = TILE_KEEP_ALL;
    c->tiles_skipped[1 + k] = 0;
    if (!use || bg_elision_off(c)) {
        c->bg_valid[k] = false;
        c->bg_hist[k].reset();
        return HK_OK;
    }
    if (!c->bg_valid[k] || c->bg_key[k][0] != A.F.win_row0 || c->bg_key[k][1] != A.F.win_rows) {
        HK_HIP(c, hipMemsetAsync(c->bgmask[k], 0, c->res_n, st));
        c->bg_valid[k] = true;
        c->bg_key[k][0] = A.F.win_row0;
        c->bg_key[k][1] = A.F.win_rows;
        c->bg_hist[k].reset();
    }
    C.bg = c->bgmask[k];
    // targets of this frame: reservoir parity (the temporal buffer), render / variance slot, and
    // (pair: no spatial reuse pass rewrites it) the spatial pair, both of whose buffers are stored
    C.bg_need = (1u << (A.F.number & 1u)) | (4u << c->sch.rslot) | (pair ? 16u : 0u);
    PxRect keep;
    if (c->bg_hist[k].launch(C.bg_need, c->grect[c->sch.gslot], keep) && pair && c->on(OPT_BG_TILE_SKIP))
        K = tile_keep(A, c->s[0], c->s_row0, c->s_rows, keep, &c->tiles_skipped[1 + k]);
    return HK_OK;
}

int hk_render_frame(hk_ctx* c, const hk_settings* settings, const hk_frame_inputs* in, void* stream)
{
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!settings || !in) return fail(c, HK_ERR_INVALID, "null settings or frame inputs");
    float want = settings->upscale_ratio < 1.0f ? 1.0f : (settings->upscale_ratio > 2.0f ? 2.0f : settings->upscale_ratio);
    if (want != c->ratio) return fail(c, HK_ERR_STATE, "settings.upscale_ratio differs from the hk_resize ratio");
    // every argument / state check before any scheduling state changes: a rejected call leaves the
    // next frame's pipelining as it was
    if (c->stripe_n >= 2 && (settings->emissive_spatial_reuse || settings->indirect_spatial_reuse))
        return fail(c, HK_ERR_STATE, "interleaved stripes (hk_resize_striped) exclude spatial reuse: it reads neighbours");
    (void)hipSetDevice(c->device);
    hipStream_t st = pick_frame(c, stream);
    c->heavy = settings->indirect_spatial_reuse || settings->emissive_spatial_reuse || c->dn_calls > 0;  // pipeline_size
    c->dn_calls = 0;
    // Frame-tail pipelining: with all three channels rendered, this frame's render / variance
    // targets are the other slot, last read by frame f-2's denoise / tone-sum, so frame f-1's tail
    // (on dn_stream) can still be running while this frame's light passes start.
    const bool swap = dn_pipeline_enabled(c) && settings->indirect_bounces >= 1u;
    FrameSchedule& q = c->sch;
    const bool gb_fresh = q.gb_fresh();  // see the fork below
    if (swap) {
        for (int ch = 0; ch < 3; ++ch) {
            std::swap(c->render[ch], c->render_alt[ch]);
            std::swap(c->variance[ch], c->variance_alt[ch]);
        }
        q.rslot ^= 1u;
    }
    // the render slot's last reader (frame f-2's tail); each wait packet costs the stream latency
    const bool slot_wait = swap && q.rslot_rec[q.rslot];
    const bool slot_covered = q.slot_covered();
    if (slot_wait && !slot_covered) HK_HIP(c, hipStreamWaitEvent(st, q.ev_rslot[q.rslot], 0));
    // (k_albedo rewrites the albedo plane a previous tail may still read: full join then)
    HK_TRY(q.gb_join(st, !swap || !c->albedo_fresh));
    // foreign-stream copies of the planes this call writes wait on st; when the indirect chain's own planes
    // are among them, its side stream must fork from st after those waits (no fork shortcut below)
    bool had_ext = false;
    for (const auto& r : q.ext_reads) had_ext |= r.first == c->render[2] || r.first == c->variance[2];
    if (!q.ext_reads.empty()) {
        HK_TRY(q.ext_wait(st, c->g.albedo));
        for (int ch = 0; ch < 3; ++ch) {
            HK_TRY(q.ext_wait(st, c->render[ch]));
            HK_TRY(q.ext_wait(st, c->variance[ch]));
        }
    }
    q.rf_swapped = swap;
    q.tail_open = false;
    c->head = in->frame_number & 1u;
    c->timing_frame = in->frame_number % c->timing_every == 0u;
    FrameArgs A = frame_args(c, settings, in);
    // The indirect channel owns reservoir buffers 6-9 (light.rs:518-546 pairs (6,8)); direct and
    // emissive share the spatial pair 4/5 and stay in reference order.  So the indirect chain can
    // run concurrently with albedo -> direct -> emissive: it goes to a side stream and joins
    // before returning.  The latency-bound traversal kernels leave issue slots and memory-level
    // parallelism idle, so the overlap pays even when one pass fills the GPU (cornell 1080p
    // 0.81 -> 0.77 ms/frame; 64x64 0.26 -> 0.18 ms).  Per-kernel event timings then include the
    // overlap.  Option channel_streams = 0 restores the serial order.
    const bool fork = c->on(OPT_CHANNEL_STREAMS);
    // fork_events: the indirect chain really runs on the side stream (not when k_light_merged takes it)
    bool fork_events = false;
    hipStream_t s1 = st, s2 = fork ? q.side[1] : st;
    const FrameArgs A_all = A;
    if (!c->albedo_fresh) {
        const FrameArgs AG = pass_window(c, A_all, GBUFFER_REACH);
        timed(c, "full_screen_albedo", st, [&] { launch_albedo(AG, c->g.albedo, st); });
    }
    // per-pass row windows of a band (pass_window): each channel's temporal pass on the rows its spatial
    // pass reads (core +-(OUT + that channel's range): direct_lit has no spatial pass, light.rs:656-676),
    // then spatial reuse.  A: the indirect channel; AE: direct + emissive.
    // (sticky margins: band_windows)
    HK_TRY(band_windows(c, settings, st));
    A = pass_window(c, A_all, c->win_ind);
    FrameArgs AE = pass_window(c, A_all, c->win_emi);
    const FrameArgs AS = pass_window(c, A_all, c->win_out);
    ChannelArgs C0 = channel(c, A.F.number, 0);
    ChannelArgs C1 = channel(c, A.F.number, 1);
    // direct_lit + emissive in one launch when every reprojection is the identity: see
    // k_direct_fused.  That needs a zero velocity plane (k_gbuffer of a frame without camera or
    // instance motion: velocity_zero; host planes may hold any velocity) at upscale ratio 1 (the
    // deferred jitter is the identity).  Only for frames of >= 1 Mpx: there it saves a launch and a
    // tail (cornell 1080p 0.652 -> 0.622 ms); on a small band (a 4- or 8-way split) the two passes
    // on their own overlap the indirect chain better (0.143 vs 0.151 ms).  Options fuse, fuse_min_px.
    const bool fuse = c->albedo_fresh && c->velocity_zero && c->ratio == 1.0f &&
                      ctx_px(c) >= c->opt[OPT_FUSE_MIN_PX] && c->on(OPT_FUSE);
    // background elision (bg_mask, hk_kernels.hip bg_elide); the separate launches share the pair's mask
    // (direct_pass).  A background pixel's own targets (temporal record, render, variance) are written by
    // that pixel alone, so they elide with or without motion.  Under motion the temporal passes also scatter
    // into the previous spatial buffer at reprojected pixels (light.wgsl:1092-1095, 1199-1202, 1453-1457),
    // and the record they scatter there is the zero reservoir (check_previous_reservoir zeroes it before the
    // store): the indirect channel's background constant, so its pair bit stays true; the direct pair's
    // background record is background_reservoir (count 1), so its pair elides only under the identity
    // reprojection — bg_elide rewrites a background byte without the pair bit whenever the frame's targets
    // do not include it, so a motion frame clears it.
    const bool identity = c->albedo_fresh && c->velocity_zero && c->ratio == 1.0f;
    const bool elide = c->albedo_fresh && c->ratio == 1.0f;
    ChannelArgs C2 = channel(c, A.F.number, 2);
    // spatial view planes (ChannelArgs::view): the indirect temporal pass writes them next to the records
    // it stores, this frame's spatial pass reads its neighbours from them.  Only when that temporal pass
    // stores its records (temporal_reuse; otherwise `cur` keeps older records the planes do not mirror).
    // Option spatial_view_planes = 0: off (the spatial pass gathers the records' own planes).
    if (settings->indirect_spatial_reuse && settings->temporal_reuse && c->on(OPT_SPATIAL_VIEW)) {
        C2.view = c->sp_view;
        C2.view_n = c->res_n;
    }
    bool multi = settings->indirect_bounces >= 2u;
    // the wavefront pipeline covers one bounce and scenes with up to WF_MAX_BINS - 1 materials
    const bool wf = c->wavefront && !multi && c->count[6] + 1u <= WF_MAX_BINS;
    // direct_lit + emissive (fused per pixel) and the one-bounce indirect pass in ONE launch
    // (k_light_merged), replacing the indirect side stream and its fork / join events.  It needs the
    // fused launch's conditions (identity reprojection) and a direct pass that does not stage the scene.
    // By default on the frames that are not pipelined (pipeline_size: < 1.2 Mpx, the 2- to 8-way
    // stripes of 1080p) and have no spatial reuse: there each kernel lasts a few wave lifetimes and
    // the fork / join events' latency is a large part of the frame (cornell stripes 2-way 0.270 ->
    // 0.263, 4-way 0.164 -> 0.160, 8-way 0.144 -> 0.112 ms/frame with the serial path's event
    // elision); on pipelined frames the streams overlap better (1080p 0.472 vs 0.486, city 4K 6.25
    // vs 7.21: spatial reuse would wait for the direct pass).  Not in the isolated-kernel measurement
    // mode (channel_streams = 0).  Option merge: 1 whenever possible, 0 never, -1 this default.
    const bool merge_possible = identity && fork && !multi && !wf && !light_lds_direct(A) && c->on(OPT_FUSE);
    const bool merge_default = !pipeline_size(c) && !settings->indirect_spatial_reuse && !settings->emissive_spatial_reuse;
    const bool merge = merge_possible && (c->opt[OPT_MERGE] < 0.0 ? merge_default : c->on(OPT_MERGE));
    // (one grid for all three channels: the wider window)
    if (merge) A = AE = pass_window(c, A_all, std::max(c->win_ind, c->win_emi));
    if (fork && !merge) {
        if (gb_fresh && q.rf_side_only && swap && c->albedo_fresh && !had_ext) {
            // The fork marker would make the side stream wait for the caller stream here.  What the
            // indirect chain reads of that stream's work: the work before W (k_gbuffer waited for it),
            // frame f-1's hk_render_frame (its indirect chain ran on the side stream itself; the rest of
            // it — k_albedo did not run, direct / emissive passes, their masks — writes buffers the chain
            // does not read), frame f-1's tail (on dn_stream; it reads the other render slot and no
            // reservoir), frame f-2's tail (the render slot this frame writes: covered when k_gbuffer
            // waited for that tail or a later one) and the G-buffer.  So the side stream waits for
            // ev_gb_done alone: every packet queued ahead of a kernel delays it, and the side stream
            // shares its hardware queue with gb_stream (cornell 1080p 0.472 -> 0.45 ms/frame).
            if (slot_wait && !slot_covered) HK_HIP(c, hipStreamWaitEvent(s2, q.ev_rslot[q.rslot], 0));
            HK_HIP(c, hipStreamWaitEvent(s2, q.ev_gb_done, 0));
        } else {
            HK_HIP(c, hipEventRecord(q.ev_fork, st));
            HK_HIP(c, hipStreamWaitEvent(s2, q.ev_fork, 0));
        }
        fork_events = true;
    }
    // background tile skip (bg_mask): the tiles each channel group runs; the opt-in variants that take no TileKeep
    // (compacted, persistent, wavefront) run every tile
    TileKeep KD, KI;
    const bool no_keep = A.opt.compact_emitter || A.opt.compact_shadow || A.opt.persistent_indirect || wf;
    auto keep_all = [&](TileKeep& K, int k) {
        if (!no_keep) return;
        K = TILE_KEEP_ALL;
        c->tiles_skipped[1 + k] = 0;
    };
    HK_TRY(bg_mask(c, 0, AE, elide, identity && !settings->emissive_spatial_reuse, st, C0, KD));
    keep_all(KD, 0);
    C1.bg = C0.bg;
    C1.bg_need = C0.bg_need;
    if (merge) {
        // (the elision mask of the indirect channel is prepared on the launch stream)
        HK_TRY(bg_mask(c, 1, A, elide, !settings->indirect_spatial_reuse, st, C2, KI));
        keep_all(KI, 1);
        timed(c, "light_merged", st, [&] { launch_light_merged(A, C0, C1, C2, st, KD, KI); });
        if (settings->emissive_spatial_reuse)
            timed(c, "emissive_spatial_reuse", st, [&] { launch_spatial(AS, C1, true, st); });
        if (settings->indirect_spatial_reuse)
            timed(c, "indirect_spatial_reuse", st, [&] { launch_spatial(AS, C2, false, st); });
    } else {
        if (fuse) {
            timed(c, "direct_lit_emissive", st, [&] { launch_direct_fused(AE, C0, C1, st, KD); });
        } else {
            timed(c, "direct_lit", st, [&] { launch_direct(AE, C0, false, st, KD); });
            timed(c, "direct_emissive", s1, [&] { launch_direct(AE, C1, true, s1, KD); });
        }
        if (settings->emissive_spatial_reuse) timed(c, "emissive_spatial_reuse", s1, [&] { launch_spatial(AS, C1, true, s1); });
        // (the wavefront pass elides in its generation stage, which classifies every pixel)
        HK_TRY(bg_mask(c, 1, A, elide, !settings->indirect_spatial_reuse, s2, C2, KI));
        keep_all(KI, 1);
        if (wf) {
            HK_TRY(ensure_wavefront(c));
            WfArgs W{c->wf_queue1, c->wf_keys, c->wf_queue2, c->wf_hit, c->wf_hit_t, c->wf_ctl, c->count[6] + 1u,
                     c->wf_seg_cap};
            HK_HIP(c, hipMemsetAsync(W.ctl, 0, (size_t)wf_ctl_words(W.bins) * 4, s2));
            timed(c, "indirect_wavefront", s2, [&] { launch_indirect_wavefront(A, C2, W, s2); });
        } else {
            timed(c, multi ? "indirect_multiple_bounces" : "indirect_lit_ambient", s2, [&] { launch_indirect(A, C2, multi, s2, KI); });
        }
        if (settings->indirect_spatial_reuse) timed(c, "indirect_spatial_reuse", s2, [&] { launch_spatial(AS, C2, false, s2); });
    }
    if (fork_events) {
        HK_HIP(c, hipEventRecord(q.ev_join[1], s2));
        HK_HIP(c, hipStreamWaitEvent(st, q.ev_join[1], 0));
    }
    q.rf_side_only = fork_events && c->albedo_fresh;  // (no k_albedo on the caller stream)
    q.rf_seq++;
    if (swap) {
        HK_HIP(c, hipEventRecord(q.ev_rf, st));
        q.rf_rec_seq = q.rf_seq;
        q.rf_other = q.other_picks;
        q.rf_epoch = q.frame_st_epoch;
    }
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

int hk_denoise(hk_ctx* c, const hk_settings* settings, const hk_frame_inputs* in, void* stream)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!settings || !in) return fail(c, HK_ERR_INVALID, "null settings or frame inputs");
    if (!settings->denoise) return HK_OK;
    if (c->stripe_n >= 2) return fail(c, HK_ERR_STATE, "interleaved stripes (hk_resize_striped) exclude the denoiser: it reads neighbours");
    c->dn_calls++;
    (void)hipSetDevice(c->device);
    hipStream_t caller = pick_frame(c, stream);
    // after a slot-swapping hk_render_frame: on dn_stream, next to the following frame's passes
    const bool async = c->sch.rf_swapped;
    hipStream_t st = async ? c->sch.dn_stream : caller;
    if (async) HK_TRY(c->sch.tail_begin());
    else HK_TRY(c->sch.gb_join(st));
    for (int ch = 0; ch < 3; ++ch) {
        HK_TRY(c->sch.ext_wait(st, c->denoised[ch]));
        HK_TRY(c->sch.ext_wait(st, c->internal_variance[ch]));  // HK_OUT_DENOISE_INTERNAL_VARIANCE copies
    }
    FrameArgs A = frame_args(c, settings, in);
    int channels = settings->indirect_bounces == 0u ? 2 : 3;  // post_process.rs:949-954
    DenoiseArgs D;
    std::memset(&D, 0, sizeof(D));
    D.channels = channels;
    D.albedo = c->g.albedo;
    for (int ch = 0; ch < 3; ++ch) {
        D.render[ch] = c->render[ch];
        D.variance[ch] = c->variance[ch];
        D.internal_variance[ch] = c->internal_variance[ch];
        D.output[ch] = c->denoised[ch];
    }
    for (int i = 0; i < 4; ++i) {
        D.rgb[i] = c->dn_rgb[i];
        D.bi[i] = c->dn_bi[i];
    }
    D.nd = c->dn_nd;
    D.center = c->dn_center;
    D.den2 = c->dn_den2;
    c->last_denoised_channels = channels;
    // band windows (pass_window): demodulation on core +-15, the levels on +-7, 3, 1, 0
    const FrameArgs AD = pass_window(c, A, DENOISE_OUT_REACH - 1);
    timed(c, "demodulation", st, [&] { launch_demod(AD, D, st); });
    static constexpr int32_t LEVEL_REACH[4] = {7, 3, 1, 0};
    for (int level = 0; level < 4; ++level) {
        const FrameArgs AL = pass_window(c, A, LEVEL_REACH[level]);
        timed(c, "denoise", st, [&] { launch_denoise(AL, D, level, st); });
    }
    if (async) HK_TRY(c->sch.tail_end());
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

int hk_tone_sum(hk_ctx* c, const hk_settings* settings, void* stream)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!settings) return fail(c, HK_ERR_INVALID, "null settings");
    (void)hipSetDevice(c->device);
    // after a slot-swapping hk_render_frame: on dn_stream (after that frame's denoise, if any)
    const bool async = c->sch.rf_swapped;
    hipStream_t st = async ? c->sch.dn_stream : pick_frame(c, stream);
    if (async) HK_TRY(c->sch.tail_begin());
    else HK_TRY(c->sch.gb_join(st));
    hk_frame_inputs dummy;
    std::memset(&dummy, 0, sizeof(dummy));
    const FrameArgs A = pass_window(c, frame_args(c, settings, &dummy), 0);
    ToneArgs T;
    T.direct = settings->denoise ? c->denoised[0] : c->render[0];
    T.emissive = settings->denoise ? c->denoised[1] : c->render[1];
    T.indirect = settings->indirect_bounces == 0u ? nullptr : (settings->denoise ? c->denoised[2] : c->render[2]);
    T.output = c->tone_buf[c->head];
    HK_TRY(c->sch.ext_wait(st, T.output));
    // Tone pass over the kept rectangle.  `in`: outside it every input plane holds the zero texel, as the light
    // launches' mask histories say of this render slot (a masked launch leaves the slot's bit in every byte outside
    // its G-buffer's screen bound, and the bit stands for a zero render texel: bg_elide; the indirect plane only where
    // the pass reads it).  Not known, and the launch whole: elision or the tile skip off, a light launch without its
    // mask (host planes, a ratio other than 1), a mask dropped since, interleaved stripes, the per-texel kernel, and
    // the denoiser's planes (a background pixel's denoised texel is not shown here to be constant).
    const int32_t ly0 = A.F.win_rows > 0 ? A.F.win_row0 : 0, x0 = A.F.win_cols > 0 ? A.F.win_col0 : 0;
    const int32_t window[4] = {x0, ly0, x0 + (int32_t)launch_cols(A.F, A.F.s[0]), ly0 + launch_rows(A.F, A.F.s_rows)};
    const int32_t key[4] = {window[1], window[3] - window[1], window[0], window[2] - window[0]};
    const uint32_t run = tone_run_px(A);
    PxRect in = PxRect::all();
    bool in_known = run != 0u && !settings->denoise && !bg_elision_off(c) && c->on(OPT_BG_TILE_SKIP) && c->stripe_n < 2;
    for (int k = 0; in_known && k < (T.indirect ? 2 : 1); ++k) {
        const int bit = 2 + (int)c->sch.rslot;
        in_known = c->bg_valid[k] && c->bg_hist[k].known[bit];
        if (in_known) in = k == 0 ? c->bg_hist[k].cover[bit] : in.join(c->bg_hist[k].cover[bit]);
    }
    // the launch: the inputs' rectangle joined with the one outside which the slot already holds this clear colour's
    // texel; the slot's record afterwards: outside `in` the launch stored that texel or found it there
    ToneHistory& H = c->tone_hist[c->head];
    const int64_t all_px = (int64_t)(window[2] - window[0]) * (int64_t)(window[3] - window[1]);
    int32_t rect[4] = {window[0], window[1], window[2], window[3]};
    bool any = true;
    if (in_known && H.holds(settings->clear_color, key)) {
        const PxRect keep = in.join(H.cover);
        const int32_t kr[4] = {keep.x0, keep.y0, keep.x1, keep.y1};
        any = hks_tone_rect(kr, window, c->s_row0, run, rect) != 0;
    }
    if (in_known) {
        H.known = true;
        H.cover = in;
        std::memcpy(H.clear, settings->clear_color, sizeof(H.clear));
        std::memcpy(H.key, key, sizeof(H.key));
    } else {
        H.reset();
    }
    c->tone_skipped = (uint64_t)(all_px - (any ? (int64_t)(rect[2] - rect[0]) * (int64_t)(rect[3] - rect[1]) : 0));
    for (int k = 0; k < 4; ++k) c->tone_rect[k] = any ? rect[k] + ((k & 1) ? c->s_row0 : 0) : 0;
    if (any) timed(c, "tone_mapping", st, [&] { launch_tone(A, T, st, c->tone_skipped ? rect : nullptr); });
    if (async) HK_TRY(c->sch.tail_end());
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

int hk_post_process(hk_ctx* c, const hk_settings* st, const hk_frame_inputs* in, void* stream)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!st || !in) return fail(c, HK_ERR_INVALID, "null settings or frame inputs");
    if (c->S_rows != (int32_t)c->S[1]) return fail(c, HK_ERR_STATE, "hk_post_process (SMAA TU4x, TAA, FSR1) needs a whole-frame context");
    (void)hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    HK_TRY(c->sch.gb_join(s));
    c->head = in->frame_number & 1u;
    const uint32_t head = c->head;
    HK_TRY(c->sch.ext_wait(s, c->upscale));
    HK_TRY(c->sch.ext_wait(s, c->taa_buf[head]));
    for (auto& b : c->fsr_buf) HK_TRY(c->sch.ext_wait(s, b));
    // post_process.rs:663-731 sizes: ceil(S * scale), scale = 1 / ratio, x 2 after SMAA TU4x
    float scale = 1.0f / c->ratio;
    const bool smaa = st->upscale == 0u, fsr = st->upscale == 1u, taa = st->taa == 0u;
    PostArgs P;
    P.frame.number = in->frame_number;
    for (int k = 0; k < 4; ++k) P.frame.clear_color[k] = st->clear_color[k];
    P.frame.upscale_ratio = c->ratio;
    auto tex = [](const void* d, uint32_t w, uint32_t h, uint32_t f16, uint32_t comps) {
        hk_pp_tex t;
        t.data = d, t.w = w, t.h = h, t.f16 = f16, t.comps = comps;
        return t;
    };
    const uint32_t S0 = c->S[0], S1 = c->S[1];
    P.in.position = tex(c->g.position, S0, S1, 0, 4);
    P.in.previous_position = tex(c->g_prev.position, S0, S1, 0, 4);
    P.in.velocity_uv = tex(c->g.velocity_uv, S0, S1, 0, 4);
    P.in.previous_velocity_uv = tex(c->g_prev.velocity_uv, S0, S1, 0, 4);
    P.in.instance_material = tex(c->g.instance_material, S0, S1, 0, 2);
    hk_pp_tex taa_input = tex(c->tone_buf[head], c->s[0], c->s[1], 1, 4);
    if (smaa) {
        scale *= 2.0f;
        const uint32_t U0 = (uint32_t)std::ceil((float)S0 * scale), U1 = (uint32_t)std::ceil((float)S1 * scale);
        if (!c->upscale || c->upscale_wh[0] != U0 || c->upscale_wh[1] != U1) {
            release(c->upscale);
            HK_HIP(c, hipMalloc(&c->upscale, (size_t)U0 * U1 * sizeof(uint2)));
            HK_HIP(c, hipMemset(c->upscale, 0, (size_t)U0 * U1 * sizeof(uint2)));
            c->upscale_wh[0] = U0, c->upscale_wh[1] = U1;
        }
        P.in.render = tex(c->tone_buf[head], c->s[0], c->s[1], 1, 4);
        P.in.previous_render = tex(c->tone_buf[1u - head], c->s[0], c->s[1], 1, 4);
        P.in.output = hk_pp_out{(uint16_t*)c->upscale, U0, U1};
        timed(c, "smaa_tu4x", s, [&] { launch_smaa(P, s); });
        timed(c, "smaa_tu4x_extrapolate", s, [&] { launch_smaa_extrapolate(P, s); });
        taa_input = tex(c->upscale, U0, U1, 1, 4);
    }
    if (taa) {
        const uint32_t T0 = (uint32_t)std::ceil((float)S0 * scale), T1 = (uint32_t)std::ceil((float)S1 * scale);
        if (!c->taa_buf[0] || c->taa_wh[0] != T0 || c->taa_wh[1] != T1) {
            for (int k = 0; k < 2; ++k) {
                release(c->taa_buf[k]);
                HK_HIP(c, hipMalloc(&c->taa_buf[k], (size_t)T0 * T1 * sizeof(uint2)));
                HK_HIP(c, hipMemset(c->taa_buf[k], 0, (size_t)T0 * T1 * sizeof(uint2)));
            }
            c->taa_wh[0] = T0, c->taa_wh[1] = T1;
        }
        P.in.render = taa_input;
        P.in.previous_render = tex(c->taa_buf[1u - head], T0, T1, 1, 4);
        P.in.output = hk_pp_out{(uint16_t*)c->taa_buf[head], T0, T1};
        timed(c, "taa_jasmine", s, [&] { launch_taa(P, s); });
        taa_input = tex(c->taa_buf[head], T0, T1, 1, 4);
    }
    if (fsr) {
        // post_process.rs:1279-1308: EASU from the TAA output (the tone-mapped plane when TAA is off) at s to
        // upscale_output[0] at S, RCAS from there to upscale_output[1]
        if ((uint64_t)S0 * S1 >= (1ull << 31)) return fail(c, HK_ERR_INVALID, "FSR1 output above 2^31 pixels");
        for (auto& b : c->fsr_buf)
            if (!b) {
                HK_HIP(c, hipMalloc(&b, (size_t)S0 * S1 * sizeof(uint2)));
                HK_HIP(c, hipMemset(b, 0, (size_t)S0 * S1 * sizeof(uint2)));
            }
        FsrArgs A;
        A.in = taa_input;
        A.out = hk_pp_out{(uint16_t*)c->fsr_buf[0], S0, S1};
        hk_fsr_easu_constants(&A.easu, (float)A.in.w, (float)A.in.h, (float)S0, (float)S1);
        A.rcas = hk_fsr_rcas_constant(c->fsr_sharpness);
        const bool tiled = c->on(OPT_FSR_TILED);
        timed(c, "fsr_easu", s, [&] { launch_fsr_easu(A, tiled, s); });
        A.in = tex(c->fsr_buf[0], S0, S1, 1, 4);
        A.out = hk_pp_out{(uint16_t*)c->fsr_buf[1], S0, S1};
        timed(c, "fsr_rcas", s, [&] { launch_fsr_rcas(A, s); });
    }
    // the next k_gbuffer overwrites the previous-frame planes read here
    HK_HIP(c, hipEventRecord(c->sch.ev_post, s));
    c->sch.post_pending = true;
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

// Sub-frame accumulation is part of the frame sequence: after a slot-swapping hk_render_frame it runs in
// the frame's tail on dn_stream (after the tone-sum it reads), next to the following sub-frame's light
// passes; otherwise on the caller's stream.  Only these two calls touch the accumulator.
int hk_accumulate(hk_ctx* c, int reset, void* stream)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    (void)hipSetDevice(c->device);
    const bool async = c->sch.rf_swapped && c->sch.tail_open;  // this frame's tone-sum ran in the tail
    hipStream_t st = async ? c->sch.dn_stream : pick_frame(c, stream);
    if (async) HK_TRY(c->sch.tail_begin());
    else HK_TRY(c->sch.gb_join(st));
    const size_t n = (size_t)c->s[0] * (size_t)c->s_rows;
    if (!c->accum) {
        HK_HIP(c, hipMalloc(&c->accum, n * sizeof(float4)));
        HK_HIP(c, hipMalloc(&c->accum_out, n * sizeof(uint2)));
        HK_HIP(c, hipMemset(c->accum_out, 0, n * sizeof(uint2)));
        reset = 1;
    }
    if (reset) c->accum_n = 0;
    timed(c, "accumulate", st, [&] { launch_accumulate(c->tone_buf[c->head], c->accum, (uint32_t)n, reset, st); });
    if (async) HK_TRY(c->sch.tail_end());
    HK_HIP(c, hipGetLastError());
    c->accum_n += 1;
    return HK_OK;
}

int hk_resolve_accumulation(hk_ctx* c, void* stream)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!c->accum || c->accum_n == 0) return fail(c, HK_ERR_STATE, "nothing accumulated (hk_accumulate)");
    (void)hipSetDevice(c->device);
    const bool async = c->sch.rf_swapped && c->sch.tail_open;
    hipStream_t st = async ? c->sch.dn_stream : pick_frame(c, stream);
    if (async) HK_TRY(c->sch.tail_begin());
    else HK_TRY(c->sch.gb_join(st));
    HK_TRY(c->sch.ext_wait(st, c->accum_out));
    const size_t n = (size_t)c->s[0] * (size_t)c->s_rows;
    timed(c, "resolve", st, [&] { launch_resolve(c->accum, (uint32_t)n, (float)c->accum_n, c->accum_out, st); });
    if (async) HK_TRY(c->sch.tail_end());
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

static void* output_ptr(hk_ctx* c, int id, uint32_t* w, uint32_t* h, uint32_t* bpp)
{
    uint32_t W = c->s[0], H = (uint32_t)c->s_rows, B = 8;
    void* p = nullptr;
    auto S_plane = [&](void* plane, uint32_t bpp) { p = plane, W = c->S[0], H = (uint32_t)c->S_rows, B = bpp; };
    switch (id) {
    case HK_OUT_ALBEDO: S_plane(c->g.albedo, 8); break;
    case HK_OUT_VARIANCE_DIRECT: case HK_OUT_VARIANCE_EMISSIVE: case HK_OUT_VARIANCE_INDIRECT:
        p = c->variance[id - HK_OUT_VARIANCE_DIRECT]; B = 4; break;
    case HK_OUT_RENDER_DIRECT: case HK_OUT_RENDER_EMISSIVE: case HK_OUT_RENDER_INDIRECT:
        p = c->render[id - HK_OUT_RENDER_DIRECT]; break;
    case HK_OUT_DENOISED_DIRECT: case HK_OUT_DENOISED_EMISSIVE: case HK_OUT_DENOISED_INDIRECT:
        p = c->denoised[id - HK_OUT_DENOISED_DIRECT]; break;
    case HK_OUT_TONE_MAPPED: p = c->tone_buf[c->head]; break;
    case HK_OUT_TONE_MAPPED_PREVIOUS: p = c->tone_buf[c->head ^ 1u]; break;
    case HK_OUT_UPSCALED: p = c->upscale; W = c->upscale_wh[0]; H = c->upscale_wh[1]; break;
    case HK_OUT_TAA: p = c->taa_buf[c->head]; W = c->taa_wh[0]; H = c->taa_wh[1]; break;
    case HK_OUT_ACCUMULATED: p = c->accum_out; break;
    case HK_OUT_FSR_EASU: S_plane(c->fsr_buf[0], 8); break;
    case HK_OUT_FSR_RCAS: S_plane(c->fsr_buf[1], 8); break;
    case HK_OUT_GBUF_POSITION: S_plane(c->g.position, 16); break;
    case HK_OUT_GBUF_NORMAL: S_plane(c->g.normal, 4); break;
    case HK_OUT_GBUF_DEPTH_GRADIENT: S_plane(c->g.depth_gradient, 8); break;
    case HK_OUT_GBUF_INSTANCE_MATERIAL: S_plane(c->g.instance_material, 8); break;
    case HK_OUT_GBUF_VELOCITY_UV: S_plane(c->g.velocity_uv, 16); break;
    case HK_OUT_DENOISE_INTERNAL_VARIANCE: p = c->internal_variance[c->last_denoised_channels - 1]; B = 4; break;
    default: return nullptr;
    }
    if (w) *w = W;
    if (h) *h = H;
    if (bpp) *bpp = B;
    return p;
}

int hk_output_info(const hk_ctx* c, int id, uint32_t* w, uint32_t* h, uint32_t* bpp)
{
    if (!c || !c->sized) return HK_ERR_STATE;
    return output_ptr(const_cast<hk_ctx*>(c), id, w, h, bpp) ? HK_OK : HK_ERR_INVALID;
}

const void* hk_output_device_ptr(hk_ctx* c, int id)
{
    if (!c || !c->sized) return nullptr;
    return output_ptr(c, id, nullptr, nullptr, nullptr);
}

int hk_lane_stats(hk_ctx* c, const char** names, unsigned long long* active, unsigned long long* iterations,
                  int capacity)
{
    if (!c) return HK_ERR_INVALID;
    const int n = (int)c->lane_names.size();
    for (int i = 0; i < n && i < capacity; ++i) {
        if (names) names[i] = c->lane_names[i].c_str();
        if (active) active[i] = c->lane_act[i];
        if (iterations) iterations[i] = c->lane_its[i];
    }
    return n;
}

int hk_set_fsr1_sharpness(hk_ctx* c, float sharpness)
{
    if (!c) return HK_ERR_INVALID;
    if (!std::isfinite(sharpness)) return fail(c, HK_ERR_INVALID, "FSR1 sharpness must be finite");
    c->fsr_sharpness = sharpness;  // not clamped (lib.rs:507-511)
    return HK_OK;
}

int hk_set_wavefront(hk_ctx* c, int enable)
{
    if (!c) return HK_ERR_INVALID;
    c->wavefront = enable != 0;
    return HK_OK;
}

int hk_sync(hk_ctx* c, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    return c->sch.gb_join(pick(c, stream));
}

int hk_get_output(hk_ctx* c, int id, void* dst, size_t bytes, int to_host, void* stream)
{
    if (!c || !dst) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    uint32_t w, h, b;
    void* p = output_ptr(c, id, &w, &h, &b);
    if (!p) return fail(c, HK_ERR_INVALID, "unknown output id");
    size_t need = (size_t)w * h * b;
    if (bytes != need) return fail(c, HK_ERR_INVALID, "output size mismatch");
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    HK_HIP(c, hipMemcpyAsync(dst, p, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (to_host) HK_HIP(c, hipStreamSynchronize(st));
    return HK_OK;
}

// The present pass (overlay.rs, overlay.wgsl; include/hk_overlay.h).  An "other" call like hk_post_process: on the
// caller's stream after the G-buffer and tail joins, so the albedo and any input plane hold their final contents.
// The albedo slot it reads is rewritten by the k_gbuffer after the next one; the next one, pipelined on gb_stream,
// waits for ev_post (post_pending), the post-process readers' marker, and the one after follows it on that stream.
static_assert(HK_PRESENT_RGBA8_SRGB == HK_OVERLAY_RGBA8_SRGB && HK_PRESENT_BGRA8_SRGB == HK_OVERLAY_BGRA8_SRGB &&
                  HK_PRESENT_RGBA16F == HK_OVERLAY_RGBA16F, "hikari_amd.h and hk_overlay.h name the same formats");
int hk_present(hk_ctx* c, const hk_settings* st, const hk_present_target* t, void* stream)
{
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!t) return fail(c, HK_ERR_INVALID, "null present target");
    if (c->S_rows != (int32_t)c->S[1]) return fail(c, HK_ERR_STATE, "hk_present needs a whole-frame context");
    if (t->format != HK_PRESENT_RGBA8_SRGB && t->format != HK_PRESENT_BGRA8_SRGB && t->format != HK_PRESENT_RGBA16F)
        return fail(c, HK_ERR_INVALID, "unknown present format");
    const uint32_t bpp = t->format == HK_PRESENT_RGBA16F ? 8u : 4u;
    if (t->width == 0u || t->height == 0u) return fail(c, HK_ERR_INVALID, "present target with a zero dimension");
    hk_overlay_view V;
    V.format = t->format;
    V.vx = t->vp_x, V.vy = t->vp_y, V.vw = t->vp_w, V.vh = t->vp_h;
    if (t->vp_w == 0u) V.vx = V.vy = 0u, V.vw = t->width, V.vh = t->height;
    if (V.vh == 0u) return fail(c, HK_ERR_INVALID, "present viewport with a zero dimension");
    if ((uint64_t)V.vx + V.vw > t->width || (uint64_t)V.vy + V.vh > t->height)
        return fail(c, HK_ERR_INVALID, "present viewport outside the target");
    const uint64_t row_bytes = (uint64_t)t->width * bpp;
    if (row_bytes > 0xFFFFFFFFull) return fail(c, HK_ERR_INVALID, "present target row above 4 GiB");
    const uint32_t pitch = t->pitch ? t->pitch : (uint32_t)row_bytes;
    if (pitch < row_bytes || pitch % bpp != 0u)
        return fail(c, HK_ERR_INVALID, "present pitch below a row or not a multiple of the texel size");
    if (t->data && (uintptr_t)t->data % bpp != 0u) return fail(c, HK_ERR_INVALID, "present target not aligned to the texel size");
    if (!t->data && pitch != row_bytes) return fail(c, HK_ERR_INVALID, "the context's own present plane has packed rows (pitch 0)");
    // the launch's one-dimensional grid of 64 x 4 pixel workgroups
    if ((((uint64_t)V.vw + 63u) / 64u) * (((uint64_t)V.vh + 3u) / 4u) >= (1ull << 31))
        return fail(c, HK_ERR_INVALID, "present viewport too large");
    int id = t->input;
    if (id == -1) {
        // overlay.rs:227-231
        if (!st) return fail(c, HK_ERR_INVALID, "null settings (present input -1 is chosen from them)");
        id = st->upscale == 1u ? HK_OUT_FSR_RCAS : (st->taa == 0u ? HK_OUT_TAA : HK_OUT_UPSCALED);
    }
    switch (id) {
    case HK_OUT_ALBEDO: case HK_OUT_RENDER_DIRECT: case HK_OUT_RENDER_EMISSIVE: case HK_OUT_RENDER_INDIRECT:
    case HK_OUT_DENOISED_DIRECT: case HK_OUT_DENOISED_EMISSIVE: case HK_OUT_DENOISED_INDIRECT: case HK_OUT_TONE_MAPPED:
    case HK_OUT_ACCUMULATED: case HK_OUT_UPSCALED: case HK_OUT_TAA: case HK_OUT_TONE_MAPPED_PREVIOUS: case HK_OUT_FSR_EASU:
    case HK_OUT_FSR_RCAS: break;
    default: return fail(c, HK_ERR_INVALID, "present input is not an RGBA16F output plane");
    }
    uint32_t iw = 0, ih = 0;
    const void* in = output_ptr(c, id, &iw, &ih, nullptr);
    if (!in || iw == 0u || ih == 0u) return fail(c, HK_ERR_STATE, "present input plane not produced yet (hk_post_process)");
    if ((uint64_t)iw * ih >= (1ull << 31)) return fail(c, HK_ERR_INVALID, "present input above 2^31 texels");
    (void)hipSetDevice(c->device);
    hipStream_t s = pick(c, stream);
    HK_TRY(c->sch.gb_join(s));
    uint8_t* data = (uint8_t*)t->data;
    if (!data) {
        if (!c->present_buf || c->present_wh[0] != t->width || c->present_wh[1] != t->height || c->present_format != t->format) {
            release(c->present_buf);
            c->present_wh[0] = c->present_wh[1] = 0;
            HK_HIP(c, hipMalloc(&c->present_buf, (size_t)pitch * t->height));
            HK_HIP(c, hipMemset(c->present_buf, 0, (size_t)pitch * t->height));
            c->present_wh[0] = t->width, c->present_wh[1] = t->height, c->present_format = t->format;
        }
        data = c->present_buf;
    }
    OverlayArgs A;
    A.in.data = in, A.in.w = iw, A.in.h = ih, A.in.f16 = 1, A.in.comps = 4;
    A.albedo.data = c->g.albedo, A.albedo.w = c->S[0], A.albedo.h = c->S[1], A.albedo.f16 = 1, A.albedo.comps = 4;
    A.data = data, A.pitch = pitch, A.view = V, A.col0 = 0u, A.cols = V.vw;
    const bool run = c->on(OPT_PRESENT_RUN);
    timed(c, "present", s, [&] { launch_overlay(A, run, s); });
    // one marker for every post-process reader: it now also stands after the earlier ones
    if (c->sch.post_pending) HK_HIP(c, hipStreamWaitEvent(s, c->sch.ev_post, 0));
    HK_HIP(c, hipEventRecord(c->sch.ev_post, s));
    c->sch.post_pending = true;
    HK_HIP(c, hipGetLastError());
    return HK_OK;
}

int hk_present_info(const hk_ctx* c, uint32_t* w, uint32_t* h, uint32_t* bytes_per_texel, uint32_t* format)
{
    if (!c) return HK_ERR_INVALID;
    if (!c->present_buf || c->present_wh[0] == 0u) return HK_ERR_STATE;
    if (w) *w = c->present_wh[0];
    if (h) *h = c->present_wh[1];
    if (bytes_per_texel) *bytes_per_texel = c->present_format == HK_PRESENT_RGBA16F ? 8u : 4u;
    if (format) *format = c->present_format;
    return HK_OK;
}

int hk_get_present(hk_ctx* c, void* dst, size_t bytes, int to_host, void* stream)
{
    if (!c || !dst) return HK_ERR_INVALID;
    if (!c->present_buf || c->present_wh[0] == 0u)
        return fail(c, HK_ERR_STATE, "no present plane yet (hk_present with data == NULL)");
    const size_t need = (size_t)c->present_wh[0] * c->present_wh[1] * (c->present_format == HK_PRESENT_RGBA16F ? 8u : 4u);
    if (bytes != need) return fail(c, HK_ERR_INVALID, "present plane size mismatch");
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);  // the plane was written on hk_present's stream: stream order
    HK_HIP(c, hipMemcpyAsync(dst, c->present_buf, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (to_host) HK_HIP(c, hipStreamSynchronize(st));
    return HK_OK;
}

static int copy_output_rect(hk_ctx* c, int id, uint32_t row0, uint32_t rows, uint32_t col0, uint32_t cols, void* dst,
                            size_t dst_pitch, int to_host, void* stream);

int hk_copy_output_rows(hk_ctx* c, int id, uint32_t row0, uint32_t rows, void* dst, int to_host, void* stream)
{
    return copy_output_rect(c, id, row0, rows, 0u, 0u, dst, 0u, to_host, stream);
}

int hk_copy_output_rect(hk_ctx* c, int id, uint32_t row0, uint32_t rows, uint32_t col0, uint32_t cols, void* dst,
                        size_t dst_pitch, int to_host, void* stream)
{
    if (cols == 0) return HK_ERR_INVALID;
    return copy_output_rect(c, id, row0, rows, col0, cols, dst, dst_pitch, to_host, stream);
}

// cols 0: whole rows (hk_copy_output_rows); dst_pitch 0: the rectangle's own row bytes
static int copy_output_rect(hk_ctx* c, int id, uint32_t row0, uint32_t rows, uint32_t col0, uint32_t cols, void* dst,
                            size_t dst_pitch, int to_host, void* stream)
{
    if (!c || !dst) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    uint32_t w, h, b;
    void* p = output_ptr(c, id, &w, &h, &b);
    if (!p) return fail(c, HK_ERR_INVALID, "unknown output id");
    if (row0 + rows > h) return fail(c, HK_ERR_INVALID, "row range outside the plane");
    if (cols == 0) {
        col0 = 0;
        cols = w;
    }
    if (col0 + cols > w) return fail(c, HK_ERR_INVALID, "column range outside the plane");
    if (dst_pitch == 0) dst_pitch = (size_t)cols * b;
    if (dst_pitch < (size_t)cols * b) return fail(c, HK_ERR_INVALID, "destination pitch below the rectangle's row bytes");
    (void)hipSetDevice(c->device);
    // A copy on a stream other than the frame sequence's (a communication stream) enqueues nothing on the
    // frame stream but, when the plane's producer may have run there, an event marker: the frame stream
    // never waits for the copy, and the plane's next writer waits for it (ext_reads).  The tone-mapped,
    // accumulated and denoised planes of a pipelined frame come from its tail (dn_stream, ev_dn_last).
    const hipStream_t given = stream ? (hipStream_t)stream : c->stream;
    const bool foreign = c->sch.frame_st && given != c->sch.frame_st && !to_host;
    hipStream_t st = foreign ? given : pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    if (foreign) {
        const bool from_tail = c->sch.rf_swapped && c->sch.tail_open &&
                               (id == HK_OUT_TONE_MAPPED || id == HK_OUT_TONE_MAPPED_PREVIOUS || id == HK_OUT_ACCUMULATED ||
                                (id >= HK_OUT_DENOISED_DIRECT && id <= HK_OUT_DENOISED_INDIRECT));
        if (!from_tail) {
            HK_HIP(c, hipEventRecord(c->sch.ev_frame_mark, c->sch.frame_st));
            HK_HIP(c, hipStreamWaitEvent(st, c->sch.ev_frame_mark, 0));
        }
    }
    size_t pitch = (size_t)w * b;
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const char* src = (const char*)p + (size_t)row0 * pitch + (size_t)col0 * b;
    if (cols == w && dst_pitch == pitch)
        HK_HIP(c, hipMemcpyAsync(dst, src, (size_t)rows * pitch, kind, st));
    else
        HK_HIP(c, hipMemcpy2DAsync(dst, dst_pitch, src, pitch, (size_t)cols * b, rows, kind, st));
    if (to_host) HK_HIP(c, hipStreamSynchronize(st));
    if (foreign) {
        // entries whose copies have completed go back to the pool (a plane nobody rewrites would otherwise keep its
        // entries, and ext_reads would grow with every copy of it)
        for (size_t k = 0; k < c->sch.ext_reads.size();) {
            if (hipEventQuery(c->sch.ext_reads[k].second) == hipSuccess) {
                c->sch.ext_pool.push_back(c->sch.ext_reads[k].second);
                c->sch.ext_reads[k] = c->sch.ext_reads.back();
                c->sch.ext_reads.pop_back();
            } else {
                ++k;
            }
        }
        hipEvent_t e = nullptr;
        if (!c->sch.ext_pool.empty()) {
            e = c->sch.ext_pool.back();
            c->sch.ext_pool.pop_back();
        } else {
            HK_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        HK_HIP(c, hipEventRecord(e, st));
        c->sch.ext_reads.emplace_back(p, e);
    }
    return HK_OK;
}

int hk_dump_reservoirs(hk_ctx* c, int id, hk_packed_reservoir* dst, size_t count, void* stream)
{
    if (!c || !dst || id < 0 || id >= HK_RESERVOIR_BUFFERS) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    if (count != c->res_n) return fail(c, HK_ERR_INVALID, "reservoir count mismatch");
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    std::vector<uint4> planes((size_t)4 * c->res_n);
    HK_HIP(c, hipMemcpyAsync(planes.data(), c->reservoirs[id], planes.size() * sizeof(uint4), hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    const ResBuf layout{nullptr, c->res_n};
    for (size_t i = 0; i < count; ++i) {
        uint4* o = reinterpret_cast<uint4*>(dst + i);
        for (int k = 0; k < 4; ++k) o[k] = planes[res_chunk(layout, (uint32_t)k, (uint32_t)i)];
    }
    return HK_OK;
}

int hk_load_reservoirs(hk_ctx* c, int id, const hk_packed_reservoir* src, size_t count, void* stream)
{
    if (!c || !src || id < 0 || id >= HK_RESERVOIR_BUFFERS) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    if (count != c->res_n) return fail(c, HK_ERR_INVALID, "reservoir count mismatch");
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    std::vector<uint4> planes((size_t)4 * c->res_n);
    const ResBuf layout{nullptr, c->res_n};
    for (size_t i = 0; i < count; ++i) {
        const uint4* s = reinterpret_cast<const uint4*>(src + i);
        for (int k = 0; k < 4; ++k) planes[res_chunk(layout, (uint32_t)k, (uint32_t)i)] = s[k];
    }
    HK_HIP(c, hipMemcpyAsync(c->reservoirs[id], planes.data(), planes.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
    c->bg_valid[0] = c->bg_valid[1] = false;  // the elision masks no longer describe the buffers
    HK_HIP(c, hipStreamSynchronize(st));
    return HK_OK;
}

int hk_band_window_grow(hk_ctx* c, const hk_settings* settings, int32_t* ranges, int commit)
{
    if (!c || !settings || !ranges) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    const WindowGrowth G = window_growth(c, settings);
    int n = 0;
    for (int b = 0; b < HK_RESERVOIR_BUFFERS; ++b) {
        bool any = false;
        for (int side = 0; side < 2; ++side) {
            const int32_t r0 = G.rows[b][side][0], r1 = G.rows[b][side][1];
            ranges[4 * b + 2 * side] = r1 > r0 ? c->s_row0 + r0 : 0;
            ranges[4 * b + 2 * side + 1] = r1 > r0 ? r1 - r0 : 0;
            any |= r1 > r0;
        }
        n += any;
    }
    if (commit && G.grows) commit_growth(c, G);
    return n;
}

int hk_reservoir_rows(hk_ctx* c, int id, int32_t frame_row0, int32_t rows, void* data, int store, void* stream)
{
    if (!c || !data || id < 0 || id >= HK_RESERVOIR_BUFFERS || rows < 0) return HK_ERR_INVALID;
    if (!c->sized) return fail(c, HK_ERR_STATE, "hk_resize has not been called");
    if (c->stripe_n >= 2) return fail(c, HK_ERR_STATE, "hk_reservoir_rows needs a contiguous band (not stripes)");
    const int32_t r0 = frame_row0 - c->s_row0;
    if (r0 < 0 || r0 + rows > c->s_rows) return fail(c, HK_ERR_INVALID, "rows outside the context's band");
    if (rows == 0) return HK_OK;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    // after every pass the frame sequence enqueued (its side streams joined its stream before returning)
    if (c->sch.frame_st && c->sch.frame_st != st) {
        HK_HIP(c, hipEventRecord(c->sch.ev_frame_mark, c->sch.frame_st));
        HK_HIP(c, hipStreamWaitEvent(st, c->sch.ev_frame_mark, 0));
    }
    const size_t w = c->s[0], n = (size_t)rows * w;
    for (size_t k = 0; k < 4; ++k) {
        uint4* dev = c->reservoirs[id] + k * c->res_n + (size_t)r0 * w;
        uint4* ext = reinterpret_cast<uint4*>(data) + k * n;
        HK_HIP(c, hipMemcpyAsync(store ? dev : ext, store ? ext : dev, n * sizeof(uint4), hipMemcpyDefault, st));
    }
    if (store) c->bg_valid[0] = c->bg_valid[1] = false;  // the elision masks no longer describe the buffers
    HK_HIP(c, hipStreamSynchronize(st));
    return HK_OK;
}

int hk_reset_counters(hk_ctx* c, void* stream)
{
    if (!c) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    HK_TRY(c->sch.gb_join(pick(c, stream)));
    HK_HIP(c, hipMemsetAsync(c->counters, 0, COUNTER_BYTES, pick(c, stream)));
    c->primary_reused = 0;
    return HK_OK;
}

int hk_read_counters(hk_ctx* c, hk_counters* out, void* stream)
{
    if (!c || !out) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    std::vector<unsigned long long> v(3 * COUNTER_SPAN);
    HK_HIP(c, hipMemcpyAsync(v.data(), c->counters, COUNTER_BYTES, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    unsigned long long sum[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < COUNTER_SHARDS; ++i) sum[k] += v[k * COUNTER_SPAN + i * COUNTER_STRIDE];
    out->traverse_top = sum[0];
    out->traverse_emitter = sum[1];
    out->primary = sum[2] + c->primary_reused;
    out->primary_reused = c->primary_reused;
    return HK_OK;
}

int hk_enable_kernel_timing(hk_ctx* c, int enable)
{
    if (!c) return HK_ERR_INVALID;
    flush_timing(c);
    c->timing = enable != 0;
    c->timing_names.clear();
    c->timing_ms.clear();
    c->timing_n.clear();
    return HK_OK;
}

int hk_set_kernel_timing_interval(hk_ctx* c, uint32_t every)
{
    if (!c || every == 0) return HK_ERR_INVALID;
    c->timing_every = every;
    return HK_OK;
}

int hk_kernel_timing(hk_ctx* c, const char** names, float* ms, int capacity)
{
    if (!c) return HK_ERR_INVALID;
    flush_timing(c);
    int n = (int)c->timing_names.size();
    for (int i = 0; i < n && i < capacity; ++i) {
        if (names) names[i] = c->timing_names[i].c_str();
        if (ms) ms[i] = (float)(c->timing_ms[i] / (double)(c->timing_n[i] ? c->timing_n[i] : 1));
    }
    return n;
}

int hk_trace(hk_ctx* c, const float* rays, const float* max_d, const float* early_d, const uint32_t* excl, uint32_t n,
             void* hits, int device_ptrs, void* stream)
{
    if (!c || !rays || !hits) return HK_ERR_INVALID;
    if (!c->has_scene) return fail(c, HK_ERR_STATE, "no scene uploaded (hk_scene_upload)");
    if (n == 0) return HK_OK;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, stream);
    HK_TRY(c->sch.gb_join(st));
    FrameArgs A = frame_args(c, nullptr, nullptr);
    if (device_ptrs) {
        launch_trace(A.sc, rays, max_d, early_d, excl, n, (uint32_t*)hits, c->counters, st);
        HK_HIP(c, hipGetLastError());
        return HK_OK;
    }
    float *d_rays = nullptr, *d_max = nullptr, *d_early = nullptr;
    uint32_t *d_excl = nullptr, *d_hits = nullptr;
    HK_HIP(c, hipMalloc(&d_rays, (size_t)n * 24));
    HK_HIP(c, hipMalloc(&d_hits, (size_t)n * 20));
    HK_HIP(c, hipMemcpy(d_rays, rays, (size_t)n * 24, hipMemcpyHostToDevice));
    if (max_d) {
        HK_HIP(c, hipMalloc(&d_max, (size_t)n * 4));
        HK_HIP(c, hipMemcpy(d_max, max_d, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (early_d) {
        HK_HIP(c, hipMalloc(&d_early, (size_t)n * 4));
        HK_HIP(c, hipMemcpy(d_early, early_d, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (excl) {
        HK_HIP(c, hipMalloc(&d_excl, (size_t)n * 4));
        HK_HIP(c, hipMemcpy(d_excl, excl, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    launch_trace(A.sc, d_rays, d_max, d_early, d_excl, n, d_hits, c->counters, st);
    HK_HIP(c, hipGetLastError());
    HK_HIP(c, hipMemcpyAsync(hits, d_hits, (size_t)n * 20, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_rays);
    release(d_hits);
    release(d_max);
    release(d_early);
    release(d_excl);
    return HK_OK;
}

int hk_selftest_f16(hk_ctx* c, const float* in, uint32_t n, uint16_t* out)
{
    if (!c || (n && (!in || !out))) return HK_ERR_INVALID;
    if (n == 0) return HK_OK;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, nullptr);
    float* d_in = nullptr;
    uint16_t* d_out = nullptr;
    HK_HIP(c, hipMalloc(&d_in, (size_t)n * 4));
    HK_HIP(c, hipMalloc(&d_out, (size_t)n * 2));
    HK_HIP(c, hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_f16(d_in, n, d_out, st);
    HK_HIP(c, hipGetLastError());
    HK_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * 2, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_in);
    release(d_out);
    return HK_OK;
}

int hk_selftest_div(hk_ctx* c, float divisor, uint32_t lo, uint32_t hi, uint64_t* mismatches)
{
    if (!c || !mismatches || !(divisor > 0.0f)) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, nullptr);
    unsigned long long* d_bad = nullptr;
    const size_t bytes = (size_t)COUNTER_SHARDS * COUNTER_STRIDE * 8;
    HK_HIP(c, hipMalloc(&d_bad, bytes));
    HK_HIP(c, hipMemsetAsync(d_bad, 0, bytes, st));
    launch_div_check(divisor, 1.0f / divisor, lo, hi, d_bad, st);
    HK_HIP(c, hipGetLastError());
    std::vector<unsigned long long> h(bytes / 8);
    HK_HIP(c, hipMemcpyAsync(h.data(), d_bad, bytes, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_bad);
    uint64_t total = 0;
    for (size_t k = 0; k < h.size(); k += COUNTER_STRIDE) total += h[k];
    *mismatches = total;
    return HK_OK;
}

int hk_selftest_rcp(hk_ctx* c, uint32_t lo, uint32_t hi, uint64_t* mismatches)
{
    if (!c || !mismatches || lo > hi) return HK_ERR_INVALID;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, nullptr);
    unsigned long long* d_bad = nullptr;
    const size_t bytes = (size_t)COUNTER_SHARDS * COUNTER_STRIDE * 8;
    HK_HIP(c, hipMalloc(&d_bad, bytes));
    HK_HIP(c, hipMemsetAsync(d_bad, 0, bytes, st));
    launch_rcp_check(lo, hi, d_bad, st);
    HK_HIP(c, hipGetLastError());
    std::vector<unsigned long long> h(bytes / 8);
    HK_HIP(c, hipMemcpyAsync(h.data(), d_bad, bytes, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_bad);
    uint64_t total = 0;
    for (size_t k = 0; k < h.size(); k += COUNTER_STRIDE) total += h[k];
    *mismatches = total;
    return HK_OK;
}

int hk_selftest_count(hk_ctx* c, const uint32_t* values, uint32_t n, uint64_t* sum)
{
    if (!c || !sum || (n && !values)) return HK_ERR_INVALID;
    *sum = 0;
    if (n == 0) return HK_OK;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, nullptr);
    uint32_t* d_in = nullptr;
    unsigned long long* d_sum = nullptr;
    const size_t bytes = (size_t)COUNTER_SHARDS * COUNTER_STRIDE * 8;
    HK_HIP(c, hipMalloc(&d_in, (size_t)n * 4));
    HK_HIP(c, hipMalloc(&d_sum, bytes));
    HK_HIP(c, hipMemcpy(d_in, values, (size_t)n * 4, hipMemcpyHostToDevice));
    HK_HIP(c, hipMemsetAsync(d_sum, 0, bytes, st));
    launch_count_check(d_in, n, d_sum, st);
    HK_HIP(c, hipGetLastError());
    std::vector<unsigned long long> h(bytes / 8);
    HK_HIP(c, hipMemcpyAsync(h.data(), d_sum, bytes, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_in);
    release(d_sum);
    uint64_t total = 0;
    for (size_t k = 0; k < h.size(); k += COUNTER_STRIDE) total += h[k];
    *sum = total;
    return HK_OK;
}

int hk_selftest_texture(hk_ctx* c, uint32_t texture, const float* uv, uint32_t n, float* out)
{
    if (!c) return HK_ERR_INVALID;
    if (texture >= c->n_textures) return fail(c, HK_ERR_INVALID, "texture id past the uploaded textures");
    if (n && (!uv || !out)) return HK_ERR_INVALID;
    if (n == 0) return HK_OK;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, nullptr);
    FrameArgs A = frame_args(c, nullptr, nullptr);
    float *d_uv = nullptr, *d_out = nullptr;
    HK_HIP(c, hipMalloc(&d_uv, (size_t)n * 8));
    HK_HIP(c, hipMalloc(&d_out, (size_t)n * 16));
    HK_HIP(c, hipMemcpy(d_uv, uv, (size_t)n * 8, hipMemcpyHostToDevice));
    launch_texture_check(A.sc, texture, d_uv, n, d_out, st);
    HK_HIP(c, hipGetLastError());
    HK_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_uv);
    release(d_out);
    return HK_OK;
}

int hk_selftest_math(hk_ctx* c, int fn, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out0,
                     uint32_t* out1)
{
    if (!c || fn < 0 || fn >= HK_MATH_COUNT) return HK_ERR_INVALID;
    const bool two = fn == HK_MATH_POW || fn == HK_MATH_UNPACK_SNORM8_FAST || fn == HK_MATH_MINF ||
                     fn == HK_MATH_MAXF || fn == HK_MATH_DIV || fn == HK_MATH_DIV_BY;
    if (fn == HK_MATH_SINCOS && !out1) return HK_ERR_INVALID;
    if (n && (!a || !out0 || (two && !b))) return HK_ERR_INVALID;
    if (n == 0) return HK_OK;
    (void)hipSetDevice(c->device);
    hipStream_t st = pick(c, nullptr);
    const bool pair = out1 && (fn == HK_MATH_SINCOS || fn == HK_MATH_UNPACK_F16);
    const size_t bytes = (size_t)n * 4;
    uint32_t *d_a = nullptr, *d_b = nullptr, *d_out0 = nullptr, *d_out1 = nullptr;
    float* d_rb = nullptr;
    HK_HIP(c, hipMalloc(&d_a, bytes));
    HK_HIP(c, hipMalloc(&d_out0, bytes));
    HK_HIP(c, hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice));
    if (two) {
        HK_HIP(c, hipMalloc(&d_b, bytes));
        HK_HIP(c, hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice));
    }
    if (fn == HK_MATH_DIV_BY) {
        // the reciprocal as frame_args evaluates inv_s: the host's IEEE divide
        std::vector<float> rb(n);
        for (uint32_t i = 0; i < n; ++i) {
            float d;
            memcpy(&d, &b[i], 4);
            rb[i] = 1.0f / d;
        }
        HK_HIP(c, hipMalloc(&d_rb, bytes));
        HK_HIP(c, hipMemcpy(d_rb, rb.data(), bytes, hipMemcpyHostToDevice));
    }
    if (pair) HK_HIP(c, hipMalloc(&d_out1, bytes));
    if (!launch_math(fn, d_a, d_b, d_rb, n, d_out0, d_out1, st)) return HK_ERR_INVALID;
    HK_HIP(c, hipGetLastError());
    HK_HIP(c, hipMemcpyAsync(out0, d_out0, bytes, hipMemcpyDeviceToHost, st));
    if (pair) HK_HIP(c, hipMemcpyAsync(out1, d_out1, bytes, hipMemcpyDeviceToHost, st));
    HK_HIP(c, hipStreamSynchronize(st));
    release(d_a);
    release(d_b);
    release(d_rb);
    release(d_out0);
    release(d_out1);
    return HK_OK;
}

}  // extern "C"
