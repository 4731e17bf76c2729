// hk_dynamic.hip — dynamic instances, deforming meshes, changed instance sets
// (DESIGN §0 f8), appended meshes, new mesh lists, skinned meshes, the
// BLAS refit, the instance refit, the tree costs and morph targets
//  on the device.
//
// The reference re-runs `prepare_instances` on the CPU whenever a transform changes
// (instance.rs:284-437: instance records with world AABBs and inverse-transpose models, the
// TLAS built with bvh 0.7.1, emissive records with alias tables, the light BVH).  This file
// re-runs that whole derivation on the GPU from the new model matrices, with exactly the float
// (and, for the inverse, double) operations of the host builder (csrc/hk_scene.cpp), so the
// buffers are bit-identical to a host rebuild — the TLAS topology included, which the
// reference-order traversal depends on.
//
// BVH build (bvh 0.7.1 restatement, as hk_scene.cpp): every split is computed by one thread
// with the host's sequential algorithm; the segments of one tree level are split in parallel by
// the threads of one workgroup (one barrier per level).  A subtree of k shapes flattens to
// exactly 3k - 2 nodes, so each segment knows its output range without the rest of the tree.
#include "hk_device.h"
#include "hk_launch.h"
#include "../../include/hk_skin.h"
#include "../../include/hk_morph.h"
#include "../../include/hk_refit.h"
#include "../../include/hk_cost.h"

namespace hk {

struct BBox {
    float mn[3], mx[3];
};
HKD BBox bbox_empty()
{
    const float inf = __uint_as_float(0x7F800000u);
    return BBox{{inf, inf, inf}, {-inf, -inf, -inf}};
}
HKD void bbox_join(BBox& a, const BBox& b)
{
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = fminf(a.mn[k], b.mn[k]);
        a.mx[k] = fmaxf(a.mx[k], b.mx[k]);
    }
}
HKD void bbox_grow(BBox& a, const float* p)
{
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = fminf(a.mn[k], p[k]);
        a.mx[k] = fmaxf(a.mx[k], p[k]);
    }
}
// std::fmin / std::fmax as the host builder evaluates them (a NaN test, then minss / maxss): of two equal operands,
// which zeros of either sign are, the second.  fminf / fmaxf here order -0 below +0 instead, so a box that holds
// zeros of both signs would differ from the host's in the sign bit.  Every box that is written out (instance boxes,
// the child boxes of a split) gets the host's fold, in the host's order; the boxes that only steer a split
// (centroid bounds, bucket boxes, SAH areas) keep fminf / fmaxf: the sign of a zero changes no comparison there
// (an area of either zero over a non-zero one compares equal, and 0 / 0 is NaN under both signs).
HKD float host_fmin(float a, float b) { return (a < b || b != b) ? a : b; }
HKD float host_fmax(float a, float b) { return (a > b || b != b) ? a : b; }
// The box of shapes ids[first..last) as the host's fold leaves it: the value by fminf / fmaxf, and a bound of 0 with
// the sign of the last zero in index order (host_fmin keeps the second of two equal operands).
HKD BBox bbox_fold_host(const BBox* shapes, const uint32_t* ids, uint32_t first, uint32_t last)
{
    BBox a = bbox_empty();
    for (uint32_t i = first; i < last; ++i) bbox_join(a, shapes[ids[i]]);
    for (int k = 0; k < 3; ++k) {
        if (a.mn[k] == 0.0f)
            for (uint32_t i = first; i < last; ++i) {
                const float v = shapes[ids[i]].mn[k];
                if (v == 0.0f) a.mn[k] = v;
            }
        if (a.mx[k] == 0.0f)
            for (uint32_t i = first; i < last; ++i) {
                const float v = shapes[ids[i]].mx[k];
                if (v == 0.0f) a.mx[k] = v;
            }
    }
    return a;
}
HKD float bbox_center(const BBox& b, int k) { return (b.mn[k] + b.mx[k]) * 0.5f; }
HKD float bbox_area(const BBox& b)
{
    const float x = b.mx[0] - b.mn[0], y = b.mx[1] - b.mn[1], z = b.mx[2] - b.mn[2];
    return 2.0f * ((x * y + x * z) + y * z);
}
HKD int bbox_largest_axis(const BBox& b)
{
    const float x = b.mx[0] - b.mn[0], y = b.mx[1] - b.mn[1], z = b.mx[2] - b.mn[2];
    if (x > y && x > z) return 0;
    if (y > z) return 1;
    return 2;
}
HKD hk_node pack_node(const BBox& a, uint32_t entry, uint32_t exit)
{
    hk_node n;
    for (int k = 0; k < 3; ++k) {
        n.min[k] = a.mn[k];
        n.max[k] = a.mx[k];
    }
    n.entry_index = entry;
    n.exit_index = exit;
    return n;
}
HKD uint32_t flat_size(uint32_t k) { return 3u * k - 2u; }

struct Segment {
    uint32_t start, count, out;
};

constexpr int BVH_BUCKETS_MAX = 16;

// Split one segment (host BvhBuilder::build for one node) and write its two box nodes; returns
// the child segments (count 0 = none).  src/dst: the index buffers of this level / the next.
HKD void split_segment(const BBox* shapes, const uint32_t* src, uint32_t* dst, Segment s, int nb, hk_node* flat,
                       Segment& left, Segment& right)
{
    left.count = right.count = 0;
    if (s.count == 1) {
        flat[s.out] = pack_node(bbox_empty(), src[s.start] | HK_BVH_LEAF_FLAG, s.out + 1u);
        return;
    }
    BBox centroid = bbox_empty(), bounds = bbox_empty();
    for (uint32_t i = 0; i < s.count; ++i) {
        const BBox& b = shapes[src[s.start + i]];
        float c[3] = {bbox_center(b, 0), bbox_center(b, 1), bbox_center(b, 2)};
        bbox_grow(centroid, c);
        bbox_join(bounds, b);
    }
    const int axis = bbox_largest_axis(centroid);
    const float axis_size = centroid.mx[axis] - centroid.mn[axis];
    uint32_t nl = 0;
    bool halves = axis_size < HK_F32_EPSILON;
    if (!halves) {
        uint32_t bucket_n[BVH_BUCKETS_MAX];
        BBox bucket_box[BVH_BUCKETS_MAX];
        for (int b = 0; b < nb; ++b) {
            bucket_n[b] = 0;
            bucket_box[b] = bbox_empty();
        }
        auto bucket_of = [&](const BBox& b) {
            const float rel = (bbox_center(b, axis) - centroid.mn[axis]) / axis_size;
            int k = (int)(rel * ((float)nb - 0.01f));
            return k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
        };
        for (uint32_t i = 0; i < s.count; ++i) {
            const BBox& b = shapes[src[s.start + i]];
            const int k = bucket_of(b);
            bucket_n[k]++;
            bbox_join(bucket_box[k], b);
        }
        int best = 0;
        float best_cost = __uint_as_float(0x7F800000u);
        for (int sp = 0; sp < nb - 1; ++sp) {
            BBox la = bbox_empty(), ra = bbox_empty();
            uint32_t ln = 0, rn = 0;
            for (int b = 0; b <= sp; ++b) {
                bbox_join(la, bucket_box[b]);
                ln += bucket_n[b];
            }
            for (int b = sp + 1; b < nb; ++b) {
                bbox_join(ra, bucket_box[b]);
                rn += bucket_n[b];
            }
            if (ln == 0 || rn == 0) continue;
            const float cost = ((float)ln * bbox_area(la) + (float)rn * bbox_area(ra)) / bbox_area(bounds);
            if (cost < best_cost) {
                best_cost = cost;
                best = sp;
            }
        }
        for (int b = 0; b <= best; ++b) nl += bucket_n[b];
        if (nl == 0 || nl == s.count) {
            halves = true;  // degenerate (NaN areas): halves, as the host
        } else {
            // children = buckets in bucket order, each in the parent's order (a stable sort by bucket)
            uint32_t at[BVH_BUCKETS_MAX];
            uint32_t run = 0;
            for (int b = 0; b < nb; ++b) {
                at[b] = run;
                run += bucket_n[b];
            }
            for (uint32_t i = 0; i < s.count; ++i) {
                const uint32_t id = src[s.start + i];
                dst[s.start + at[bucket_of(shapes[id])]++] = id;
            }
        }
    }
    if (halves) {
        nl = s.count / 2u;
        for (uint32_t i = 0; i < s.count; ++i) dst[s.start + i] = src[s.start + i];
    }
    const uint32_t nr = s.count - nl;
    const BBox la = bbox_fold_host(shapes, dst + s.start, 0u, nl), ra = bbox_fold_host(shapes, dst + s.start, nl, s.count);
    const uint32_t q = s.out + 1u + flat_size(nl);  // box node of the right child
    flat[s.out] = pack_node(la, s.out + 1u, q);
    flat[q] = pack_node(ra, q + 1u, q + 1u + flat_size(nr));
    left = Segment{s.start, nl, s.out + 1u};
    right = Segment{s.start + nl, nr, q + 1u};
}

// ---- cooperative split: the same decisions as split_segment, by all 256 threads of the block.
// min/max reductions are exact in any order; the children are a stable sort by bucket, ranked
// with wave ballots chunk by chunk.
constexpr uint32_t COOP_MIN = 128;  // segments larger than this are split cooperatively
constexpr int COOP_BUCKETS = 6;     // bvh 0.7.1 NUM_BUCKETS
struct CoopShared {
    float red[4][48];
    float f[48];
    uint32_t wave_n[4][COOP_BUCKETS];
    uint32_t cursor[COOP_BUCKETS];
    uint32_t u[4];
};
// reduce v[0..k) over the block: op 0 = min, 1 = max, 2 = sum (integer-valued floats)
template <int K>
HKD void block_reduce(float* v, const int* op, CoopShared& sh)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            const float x = __shfl_xor(v[k], o, 64);
            v[k] = op[k] == 0 ? fminf(v[k], x) : (op[k] == 1 ? fmaxf(v[k], x) : v[k] + x);
        }
    if (lane == 0)
        for (int k = 0; k < K; ++k) sh.red[w][k] = v[k];
    __syncthreads();
    if (threadIdx.x < (uint32_t)K) {
        const int k = (int)threadIdx.x;
        float r = sh.red[0][k];
        for (int j = 1; j < 4; ++j) r = op[k] == 0 ? fminf(r, sh.red[j][k]) : (op[k] == 1 ? fmaxf(r, sh.red[j][k]) : r + sh.red[j][k]);
        sh.f[k] = r;
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) v[k] = sh.f[k];
    __syncthreads();
}
HKD int coop_bucket(const BBox& b, int axis, float cmin, float axis_size)
{
    const float rel = (bbox_center(b, axis) - cmin) / axis_size;
    int k = (int)(rel * ((float)COOP_BUCKETS - 0.01f));
    return k < 0 ? 0 : (k > COOP_BUCKETS - 1 ? COOP_BUCKETS - 1 : k);
}
HKD void coop_split(const BBox* shapes, const uint32_t* src, uint32_t* dst, Segment s, hk_node* flat, CoopShared& sh,
                    Segment& left, Segment& right)
{
    const float inf = __uint_as_float(0x7F800000u);
    // centroid bounds + bounds
    {
        float v[12];
        int op[12];
        for (int k = 0; k < 3; ++k) {
            v[k] = inf, v[3 + k] = -inf, v[6 + k] = inf, v[9 + k] = -inf;
            op[k] = 0, op[3 + k] = 1, op[6 + k] = 0, op[9 + k] = 1;
        }
        for (uint32_t i = threadIdx.x; i < s.count; i += 256u) {
            const BBox& b = shapes[src[s.start + i]];
            for (int k = 0; k < 3; ++k) {
                const float c = bbox_center(b, k);
                v[k] = fminf(v[k], c), v[3 + k] = fmaxf(v[3 + k], c);
                v[6 + k] = fminf(v[6 + k], b.mn[k]), v[9 + k] = fmaxf(v[9 + k], b.mx[k]);
            }
        }
        block_reduce<12>(v, op, sh);
        BBox centroid{{v[0], v[1], v[2]}, {v[3], v[4], v[5]}};
        BBox bounds{{v[6], v[7], v[8]}, {v[9], v[10], v[11]}};
        const int axis = bbox_largest_axis(centroid);
        const float axis_size = centroid.mx[axis] - centroid.mn[axis];
        const float cmin = centroid.mn[axis];
        bool halves = axis_size < HK_F32_EPSILON;
        uint32_t nl = 0;
        if (!halves) {
            // per-bucket counts and boxes
            float bv[COOP_BUCKETS * 7];
            int bop[COOP_BUCKETS * 7];
            for (int b = 0; b < COOP_BUCKETS; ++b) {
                bv[7 * b] = 0.0f, bop[7 * b] = 2;
                for (int k = 0; k < 3; ++k) {
                    bv[7 * b + 1 + k] = inf, bop[7 * b + 1 + k] = 0;
                    bv[7 * b + 4 + k] = -inf, bop[7 * b + 4 + k] = 1;
                }
            }
            for (uint32_t i = threadIdx.x; i < s.count; i += 256u) {
                const BBox& bb = shapes[src[s.start + i]];
                const int b = coop_bucket(bb, axis, cmin, axis_size);
#pragma unroll
                for (int q = 0; q < COOP_BUCKETS; ++q)
                    if (q == b) {
                        bv[7 * q] += 1.0f;
                        for (int k = 0; k < 3; ++k) {
                            bv[7 * q + 1 + k] = fminf(bv[7 * q + 1 + k], bb.mn[k]);
                            bv[7 * q + 4 + k] = fmaxf(bv[7 * q + 4 + k], bb.mx[k]);
                        }
                    }
            }
            block_reduce<COOP_BUCKETS * 7>(bv, bop, sh);
            uint32_t bucket_n[COOP_BUCKETS];
            BBox bucket_box[COOP_BUCKETS];
            for (int b = 0; b < COOP_BUCKETS; ++b) {
                bucket_n[b] = (uint32_t)bv[7 * b];
                bucket_box[b] = BBox{{bv[7 * b + 1], bv[7 * b + 2], bv[7 * b + 3]}, {bv[7 * b + 4], bv[7 * b + 5], bv[7 * b + 6]}};
            }
            int best = 0;
            float best_cost = inf;
            for (int sp = 0; sp < COOP_BUCKETS - 1; ++sp) {
                BBox la = bbox_empty(), ra = bbox_empty();
                uint32_t ln = 0, rn = 0;
                for (int b = 0; b <= sp; ++b) {
                    bbox_join(la, bucket_box[b]);
                    ln += bucket_n[b];
                }
                for (int b = sp + 1; b < COOP_BUCKETS; ++b) {
                    bbox_join(ra, bucket_box[b]);
                    rn += bucket_n[b];
                }
                if (ln == 0 || rn == 0) continue;
                const float cost = ((float)ln * bbox_area(la) + (float)rn * bbox_area(ra)) / bbox_area(bounds);
                if (cost < best_cost) {
                    best_cost = cost;
                    best = sp;
                }
            }
            for (int b = 0; b <= best; ++b) nl += bucket_n[b];
            if (nl == 0 || nl == s.count) {
                halves = true;
            } else {
                // stable sort by bucket: cursor[b] = start of bucket b, ranks by wave ballots
                if (threadIdx.x == 0) {
                    uint32_t run = 0;
                    for (int b = 0; b < COOP_BUCKETS; ++b) {
                        sh.cursor[b] = run;
                        run += bucket_n[b];
                    }
                }
                __syncthreads();
                const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
                for (uint32_t base = 0; base < s.count; base += 256u) {
                    const uint32_t i = base + threadIdx.x;
                    const bool valid = i < s.count;
                    const uint32_t id = valid ? src[s.start + i] : 0u;
                    const int b = valid ? coop_bucket(shapes[id], axis, cmin, axis_size) : -1;
                    unsigned long long mine = 0;
#pragma unroll
                    for (int q = 0; q < COOP_BUCKETS; ++q) {
                        const unsigned long long m = __ballot(b == q);
                        if (b == q) mine = m;
                        if (lane == 0) sh.wave_n[w][q] = (uint32_t)__popcll(m);
                    }
                    __syncthreads();
                    if (valid) {
                        uint32_t off = sh.cursor[b];
                        for (uint32_t j = 0; j < w; ++j) off += sh.wave_n[j][b];
                        off += (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
                        dst[s.start + off] = id;
                    }
                    __syncthreads();
                    if (threadIdx.x < (uint32_t)COOP_BUCKETS)
                        sh.cursor[threadIdx.x] += sh.wave_n[0][threadIdx.x] + sh.wave_n[1][threadIdx.x] +
                                                  sh.wave_n[2][threadIdx.x] + sh.wave_n[3][threadIdx.x];
                    __syncthreads();
                }
            }
        }
        if (halves) {
            nl = s.count / 2u;
            for (uint32_t i = threadIdx.x; i < s.count; i += 256u) dst[s.start + i] = src[s.start + i];
            __syncthreads();
        }
        // children boxes
        float c[12];
        int cop[12];
        for (int k = 0; k < 3; ++k) {
            c[k] = inf, c[3 + k] = -inf, c[6 + k] = inf, c[9 + k] = -inf;
            cop[k] = 0, cop[3 + k] = 1, cop[6 + k] = 0, cop[9 + k] = 1;
        }
        for (uint32_t i = threadIdx.x; i < s.count; i += 256u) {
            const BBox& b = shapes[dst[s.start + i]];
            const int o = i < nl ? 0 : 6;
            for (int k = 0; k < 3; ++k) c[o + k] = fminf(c[o + k], b.mn[k]), c[o + 3 + k] = fmaxf(c[o + 3 + k], b.mx[k]);
        }
        block_reduce<12>(c, cop, sh);
        // A bound of 0 takes its sign from the last zero of its child in index order, as the host's fold leaves it
        // (host_fmin).  c[] is the same in every thread, so the branch is block-uniform.
        for (int j = 0; j < 12; ++j) {
            if (c[j] != 0.0f) continue;
            if (threadIdx.x == 0) sh.u[0] = 0u;
            __syncthreads();
            const uint32_t first = j < 6 ? 0u : nl, last = j < 6 ? nl : s.count;
            uint32_t key = 0u;  // (index + 1) * 2 + sign bit of the thread's last zero
            for (uint32_t i = first + threadIdx.x; i < last; i += 256u) {
                const BBox& b = shapes[dst[s.start + i]];
                const float v = (j % 6) < 3 ? b.mn[j % 3] : b.mx[j % 3];
                if (v == 0.0f) key = ((i + 1u) << 1) | (__float_as_uint(v) >> 31);
            }
            if (key) atomicMax(&sh.u[0], key);
            __syncthreads();
            c[j] = (sh.u[0] & 1u) ? -0.0f : 0.0f;
            __syncthreads();
        }
        const uint32_t nr = s.count - nl;
        const uint32_t q = s.out + 1u + flat_size(nl);
        if (threadIdx.x == 0) {
            flat[s.out] = pack_node(BBox{{c[0], c[1], c[2]}, {c[3], c[4], c[5]}}, s.out + 1u, q);
            flat[q] = pack_node(BBox{{c[6], c[7], c[8]}, {c[9], c[10], c[11]}}, q + 1u, q + 1u + flat_size(nr));
        }
        left = Segment{s.start, nl, s.out + 1u};
        right = Segment{s.start + nl, nr, q + 1u};
    }
}

// One workgroup builds one flattened BVH over `n` shapes (n >= 1).  Segments of one tree level
// larger than COOP_MIN are split one after another by the whole block (coop_split), the others
// in parallel, one per thread (split_segment); one barrier per level.  idx: 2n scratch indices,
// seg: 2 x n scratch segments.  When the shapes and both index buffers fit BVH_LDS_SHAPES they
// are staged in LDS.  *levels: the number of tree levels that split (max inner nodes on a path).
constexpr uint32_t BVH_LDS_SHAPES = 1280;  // 1280 x (24 + 8) B = 40 KiB
constexpr uint32_t BIG_MAX = 64;           // big segments per level; further ones are split per thread
template <bool LDS>
HKD void build_bvh(const BBox* g_shapes, uint32_t n, int buckets, hk_node* flat, uint32_t* g_idx, Segment* seg,
                   uint32_t* levels)
{
    __shared__ uint32_t n_small, n_small_next, n_big, n_big_next;
    __shared__ Segment big[2][BIG_MAX];
    __shared__ CoopShared sh;
    __shared__ BBox s_shapes[LDS ? BVH_LDS_SHAPES : 1];
    __shared__ uint32_t s_idx[LDS ? 2 * BVH_LDS_SHAPES : 1];
    if (n == 0) return;
    const BBox* shapes = g_shapes;
    uint32_t* idx = g_idx;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) s_shapes[i] = g_shapes[i];
        shapes = s_shapes;
        idx = s_idx;
    }
    const bool coop = buckets == COOP_BUCKETS;
    uint32_t* buf[2] = {idx, idx + n};
    Segment* segs[2] = {seg, seg + n};
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) buf[0][i] = i;
    if (threadIdx.x == 0) {
        n_small = n_big = n_small_next = n_big_next = 0;
        const Segment root{0u, n, 0u};
        if (coop && n > COOP_MIN) big[0][n_big++] = root;
        else segs[0][n_small++] = root;
    }
    __syncthreads();
    uint32_t split_levels = 0;
    auto push = [&](int p, const Segment& l, const Segment& r) {  // children of a level-p split
        for (const Segment* c : {&l, &r}) {
            // Any thread may push a big segment: thread 0 after a coop_split, and every thread whose own segment
            // was a big one the full list turned away.  So the slot is claimed first and checked after; the
            // counter may pass BIG_MAX and is clamped where the level ends.
            if (coop && c->count > COOP_MIN) {
                const uint32_t k = atomicAdd(&n_big_next, 1u);
                if (k < BIG_MAX) {
                    big[p ^ 1][k] = *c;
                    continue;
                }
            }
            const uint32_t k = atomicAdd(&n_small_next, 1u);
            segs[p ^ 1][k] = *c;
        }
    };
    for (int level = 0;; ++level) {
        const int p = level & 1;
        const uint32_t nb_ = n_big, ns = n_small;
        if (nb_ + ns == 0) break;
        for (uint32_t i = 0; i < nb_; ++i) {
            Segment l, r;
            coop_split(shapes, buf[p], buf[p ^ 1], big[p][i], flat, sh, l, r);
            if (threadIdx.x == 0) push(p, l, r);
        }
        for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) {
            Segment l, r;
            split_segment(shapes, buf[p], buf[p ^ 1], segs[p][i], buckets, flat, l, r);
            if (l.count) push(p, l, r);
        }
        __syncthreads();
        if (n_small_next + n_big_next) split_levels = level + 1;
        __syncthreads();
        if (threadIdx.x == 0) {
            n_big = n_big_next < BIG_MAX ? n_big_next : BIG_MAX;
            n_small = n_small_next;
            n_big_next = n_small_next = 0;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && levels) *levels = split_levels;
}
template <bool LDS>
__global__ __launch_bounds__(256) void k_build_bvh(const BBox* g_shapes, uint32_t n, int buckets, hk_node* flat,
                                                   uint32_t* g_idx, Segment* seg, uint32_t* levels)
{
    build_bvh<LDS>(g_shapes, n, buckets, flat, g_idx, seg, levels);
}

// ---- deforming meshes (mesh.rs:77-166 prepare_mesh_assets, mod.rs:379-467 GpuMesh::try_from; hk_scene.cpp
// hks_add_mesh + hks_build "BLAS per mesh").  Topology is unchanged: the primitives keep their vertex indices.
// One thread per vertex of the listed meshes (position and normal of the hk_vertex; u, v stay), then one per
// triangle: its three positions from the new vertex data and its shape box, folded from empty in vertex order
// with the host's fmin / fmax (Aabb::grow), at the mesh's slice of the shape scratch.  The triangles read the
// uploaded positions, not the vertex array, so the two halves do not depend on each other.  Every vertex index was
// checked against vertex_count on the host (hk_update_meshes).
HKD uint32_t mesh_of(const MeshUpdate* tab, uint32_t n, uint32_t i, bool shapes)
{
    uint32_t lo = 0, hi = n;  // the last mesh whose first vertex / shape is <= i (the firsts ascend)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((shapes ? tab[mid].shape0 : tab[mid].vertex0) <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void k_update_mesh_geometry(const MeshUpdate* tab, uint32_t n_meshes,
                                                              uint32_t n_vertices, uint32_t n_shapes,
                                                              const float* positions, const float* normals,
                                                              hk_vertex* vertices, hk_primitive* prims, BBox* shapes)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_vertices) {
        const MeshUpdate& m = tab[mesh_of(tab, n_meshes, i, false)];
        const uint32_t v = i - m.vertex0;
        if (v >= m.vertex_count) return;
        hk_vertex& out = vertices[m.vertex + v];
        for (int k = 0; k < 3; ++k) out.position[k] = positions[3u * (size_t)i + k];
        if (m.has_normals)
            for (int k = 0; k < 3; ++k) out.normal[k] = normals[3u * (size_t)i + k];
        return;
    }
    const uint32_t j = i - n_vertices;
    if (j >= n_shapes) return;
    const MeshUpdate& m = tab[mesh_of(tab, n_meshes, j, true)];
    const uint32_t t = j - m.shape0;
    if (t >= m.shapes) return;
    hk_primitive& pr = prims[m.primitive + t];
    const float inf = __uint_as_float(0x7F800000u);
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (int c = 0; c < 3; ++c) {
        const uint32_t v = pr.vertices[c].index;
        if (v >= m.vertex_count) continue;  // (refused on the host; never taken)
        for (int k = 0; k < 3; ++k) {
            const float x = positions[3u * (size_t)(m.vertex0 + v) + k];
            pr.vertices[c].position[k] = x;
            mn[k] = host_fmin(mn[k], x);
            mx[k] = host_fmax(mx[k], x);
        }
    }
    shapes[j] = BBox{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}};
}
// One workgroup per listed mesh: build_bvh over the mesh's shape boxes into its own node slice (node indices
// relative to the mesh, as the host's per-mesh build leaves them), with the mesh's slices of the index and segment
// scratch.  tab: the meshes of this instantiation (LDS: at most BVH_LDS_SHAPES triangles).
template <bool LDS>
__global__ __launch_bounds__(256) void k_build_mesh_bvh(const MeshUpdate* tab, const BBox* shapes, int buckets,
                                                        hk_node* blas, uint32_t* idx, Segment* seg, uint32_t* levels)
{
    const MeshUpdate m = tab[blockIdx.x];
    build_bvh<LDS>(shapes + m.shape0, m.shapes, buckets, blas + m.node0, idx + 2u * (size_t)m.shape0,
                   seg + 2u * (size_t)m.shape0, levels + m.slot);
}

// ---- BLAS refit (include/hk_refit.h: the rule, this project's own; the host side is hk_scene.cpp
// hks_refit_nodes over the same header).  The listed slices keep their topology; every entry node's box becomes the
// hk_minf / hk_maxf fold of the shape boxes (k_update_mesh_geometry's scratch) of the leaves stored in its range
// (i, exit).  The fold has no order, so no box is derived from another: every entry node reads leaves only, nothing
// passes between workgroups inside a launch, and the two launches below are ordered by the stream alone.
//   k_refit_small  one thread per node of the listed slices.  A leaf returns.  An entry node with
//                  exit - i <= REFIT_SMALL scans its own range, folds in registers and stores its six words; a larger
//                  one appends its index to the list of large nodes (one atomicAdd on a counter the stream zeroed
//                  before; the list is read by the next launch only, in any order).
//   k_refit_large  one workgroup per listed large node (a fixed grid strides over the list, whose length it reads from
//                  the counter): a strided scan of the range by the 256 threads, block_reduce, six stores.
// exit - i is 3p - 1 for a subtree of p primitives, so the spans either side of the threshold are REFIT_SMALL (p = 11)
// and REFIT_SMALL + 3.  Work: each node is read once per entry node above it, O(n x depth) 4-byte reads out of L2.
// Every index is bounded by the slice: an exit past the slice is clamped, a payload past the mesh's primitives is
// skipped, the list takes no more entries than it has room for.  Only min / max of entry nodes are written; the words
// the scans read (entry_index, exit_index) are written by nobody.
constexpr uint32_t REFIT_SMALL = 32;
constexpr uint32_t REFIT_LARGE_GRID = 2048;  // workgroups of k_refit_large at the most (8 per CU)
// the listed mesh that holds node g of the listed slices laid end to end (mesh k starts at 3 x shape0 - 2k)
HKD uint32_t refit_mesh_of(const MeshUpdate* tab, uint32_t n, uint32_t g)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (3u * tab[mid].shape0 - 2u * mid <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the shape box of the leaf at node j of mesh m's slice joined into box (nothing for an entry node)
HKD void refit_scan(const MeshUpdate& m, const hk_node* slice, const BBox* shapes, uint32_t j, float* box)
{
    const uint32_t entry = slice[j].entry_index;
    if (!hk_refit_is_leaf(entry)) return;
    const uint32_t t = hk_refit_leaf_primitive(entry);
    if (t >= m.shapes) return;  // (a registered slice's payloads are its own primitives; never taken)
    const BBox s = shapes[m.shape0 + t];
    hk_refit_join(box, s.mn, s.mx);
}
__global__ __launch_bounds__(256) void k_refit_small(const MeshUpdate* tab, uint32_t n_meshes, uint32_t n_nodes,
                                                     const BBox* shapes, hk_node* blas, uint32_t* large,
                                                     uint32_t large_room, uint32_t* n_large)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_nodes) return;
    const uint32_t k = refit_mesh_of(tab, n_meshes, g);
    const MeshUpdate m = tab[k];
    if (m.shapes == 0u) return;  // (refused on the host; never taken)
    const uint32_t count = 3u * m.shapes - 2u, i = g - (3u * m.shape0 - 2u * k);
    if (i >= count) return;
    hk_node* slice = blas + m.node0;
    if (hk_refit_is_leaf(slice[i].entry_index)) return;
    const uint32_t exit = slice[i].exit_index, e = exit < count ? exit : count;
    if (e > i && e - i > REFIT_SMALL) {
        const uint32_t at = atomicAdd(n_large, 1u);
        if (at < large_room) large[at] = g;
        return;
    }
    float box[6];
    hk_refit_empty(box);
    for (uint32_t j = i + 1u; j < e; ++j) refit_scan(m, slice, shapes, j, box);
    for (int c = 0; c < 3; ++c) {
        slice[i].min[c] = box[c];
        slice[i].max[c] = box[3 + c];
    }
}
__global__ __launch_bounds__(256) void k_refit_large(const MeshUpdate* tab, uint32_t n_meshes, const BBox* shapes,
                                                     hk_node* blas, const uint32_t* large, uint32_t large_room,
                                                     const uint32_t* n_large)
{
    __shared__ CoopShared sh;
    const uint32_t listed = *n_large < large_room ? *n_large : large_room;
    const int op[6] = {0, 0, 0, 1, 1, 1};
    for (uint32_t w = blockIdx.x; w < listed; w += gridDim.x) {  // (block-uniform)
        const uint32_t g = large[w];
        const uint32_t k = refit_mesh_of(tab, n_meshes, g);
        const MeshUpdate m = tab[k];
        const uint32_t count = 3u * m.shapes - 2u, i = g - (3u * m.shape0 - 2u * k);
        if (m.shapes == 0u || i >= count) continue;  // (k_refit_small listed a node of the slice; never taken)
        hk_node* slice = blas + m.node0;
        const uint32_t exit = slice[i].exit_index, e = exit < count ? exit : count;
        float box[6];
        hk_refit_empty(box);
        for (uint32_t j = i + 1u + threadIdx.x; j < e; j += 256u) refit_scan(m, slice, shapes, j, box);
        block_reduce<6>(box, op, sh);
        if (threadIdx.x < 3u) slice[i].min[threadIdx.x] = box[threadIdx.x];
        else if (threadIdx.x < 6u) slice[i].max[threadIdx.x - 3u] = box[threadIdx.x];
    }
}

// ---- skinned meshes (include/hk_skin.h: Bevy 0.9's skinning.wgsl as recalled, its order pinned there;
// the host side is hk_scene.cpp hks_skin_vertices over the same header).  One thread per vertex of the posed meshes,
// found by k_update_mesh_geometry's table search: the bind pose and the rig from the context's resident streams
// (consecutive lanes read consecutive addresses: 12-byte positions and normals, one 8-byte load of the four u16 indices,
// one 16-byte load of the weights), the four joint matrices as four 16-byte loads each from the uploaded palettes, and
// the posed position and normal stored into the staged streams at the vertex's place in list order, where
// k_update_mesh_geometry and the BLAS build read them as if the host had sent them.  Every index was checked against
// the skin's joint_count on the host (hk_set_mesh_skins), and the pose's joint_count is the skin's (hk_skin_meshes).
// The skin step of one vertex, shared by k_skin_vertices and k_morph_vertices: the rig at `at` of the resident skin
// streams, the four joint matrices of the palette at joint0, and hk_skin.h's matrix applied to p (and to nr) in place.
HKD void skin_vertex(const uint2* joint_indices, const float4* joint_weights, const float4* palettes, size_t at,
                     uint32_t joint0, bool has_normals, float* p, float* nr)
{
    const uint2 ix = joint_indices[at];
    const float4 wt = joint_weights[at];
    const uint32_t joint[4] = {ix.x & 0xFFFFu, ix.x >> 16, ix.y & 0xFFFFu, ix.y >> 16};
    const float w[4] = {wt.x, wt.y, wt.z, wt.w};
    float J[4][16];
    for (int j = 0; j < 4; ++j) {
        const float4* col = palettes + 4u * ((size_t)joint0 + joint[j]);
        for (int c = 0; c < 4; ++c) {
            const float4 q = col[c];
            J[j][4 * c] = q.x, J[j][4 * c + 1] = q.y, J[j][4 * c + 2] = q.z, J[j][4 * c + 3] = q.w;
        }
    }
    float M[12], o[3];
    hk_skin_matrix(J[0], J[1], J[2], J[3], w, M);
    hk_skin_position(M, p, o);
    for (int a = 0; a < 3; ++a) p[a] = o[a];
    if (has_normals) {
        hk_skin_normal(M, nr, o);
        for (int a = 0; a < 3; ++a) nr[a] = o[a];
    }
}
__global__ __launch_bounds__(256) void k_skin_vertices(const MeshUpdate* tab, const SkinSource* sources,
                                                       uint32_t n_meshes, uint32_t n_vertices,
                                                       const float* bind_positions, const float* bind_normals,
                                                       const uint2* joint_indices, const float4* joint_weights,
                                                       const float4* palettes, float* positions, float* normals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_vertices) return;
    const uint32_t k = mesh_of(tab, n_meshes, i, false);
    const MeshUpdate& m = tab[k];
    const uint32_t v = i - m.vertex0;
    if (v >= m.vertex_count) return;
    const SkinSource s = sources[k];
    const size_t at = (size_t)s.skin0 + v;
    float p[3], nr[3] = {0.0f, 0.0f, 0.0f};
    for (int a = 0; a < 3; ++a) p[a] = bind_positions[3u * at + a];
    if (m.has_normals)
        for (int a = 0; a < 3; ++a) nr[a] = bind_normals[3u * at + a];
    skin_vertex(joint_indices, joint_weights, palettes, at, s.joint0, m.has_normals != 0u, p, nr);
    for (int a = 0; a < 3; ++a) positions[3u * (size_t)i + a] = p[a];
    if (m.has_normals)
        for (int a = 0; a < 3; ++a) normals[3u * (size_t)i + a] = nr[a];
}

// ---- morph targets (include/hk_morph.h: glTF 2.0's sum and Bevy 0.11's morph.wgsl as recalled, the
// order pinned there; the host side is hk_scene.cpp hks_morph_vertices over the same header).  One thread per vertex of
// the posed meshes, found by k_update_mesh_geometry's table search.  The base comes from the context's resident morph
// block; the fold runs over the mesh's range of the ACTIVE LIST (the targets whose weight is not zero, compacted on the
// host in ascending order), whose trip count is uniform per mesh.  Target t's delta of vertex v lies at record
// delta0 + t x V + v, so consecutive lanes read consecutive 12-byte records.  The loads of a batch of MORPH_BATCH
// targets are issued before the batch's first add (morph_batch: no condition around a load, so that the compiler need
// not wait for one before it issues the next), so that their latencies overlap instead of adding up (each add depends
// on the one before; the loads do not); whole batches first, then the rest one by one; the adds stay strictly in list
// order.  Where the source names a skin,
// skin_vertex then applies the vertex's skin matrix as k_skin_vertices does.  The results go into the staged streams at
// the vertex's place in list order.  Vertices are independent: no fence, no atomics, plain vector loads and stores.
// Every offset was checked on the host: the records against the registered set (hk_set_mesh_morphs), every list entry's
// target below the registered target_count and the skin's vertex_count equal to the morph's (hk_morph_meshes).
struct MorphFold {
    const MorphActive* list;  // the mesh's range of the active list
    const float* dp;          // its position deltas
    const float* dn;          // its normal deltas (read where NORMALS)
    uint32_t V, v;            // its vertex count, this thread's vertex
};
// N list entries from `first`: every load of the batch unconditionally and before the first add, then the adds in list
// order
template <int N, bool NORMALS>
HKD void morph_batch(const MorphFold& F, uint32_t first, float* p, float* nr)
{
    float w[N], dp[N][3], dn[N][3];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const MorphActive e = F.list[first + j];
        const size_t rec = 3u * ((size_t)e.target * F.V + F.v);
        w[j] = e.weight;
        for (int a = 0; a < 3; ++a) dp[j][a] = F.dp[rec + a];
        if (NORMALS)
            for (int a = 0; a < 3; ++a) dn[j][a] = F.dn[rec + a];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        hk_morph_add(p, w[j], dp[j]);
        if (NORMALS) hk_morph_add(nr, w[j], dn[j]);
    }
}
__global__ __launch_bounds__(256) void k_morph_vertices(const MeshUpdate* tab, const MorphSource* sources,
                                                        const MorphActive* active, uint32_t n_meshes,
                                                        uint32_t n_vertices, const float* base_positions,
                                                        const float* base_normals, const float* position_deltas,
                                                        const float* normal_deltas, const uint2* joint_indices,
                                                        const float4* joint_weights, const float4* palettes,
                                                        float* positions, float* normals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_vertices) return;
    const uint32_t k = mesh_of(tab, n_meshes, i, false);
    const MeshUpdate& m = tab[k];
    const uint32_t v = i - m.vertex0;
    if (v >= m.vertex_count) return;
    const MorphSource s = sources[k];
    const bool has_normals = m.has_normals != 0u, fold_normals = has_normals && s.normal_delta0 != MORPH_NONE;
    const size_t at = (size_t)s.base0 + v;
    float p[3], nr[3] = {0.0f, 0.0f, 0.0f};
    for (int a = 0; a < 3; ++a) p[a] = base_positions[3u * at + a];
    if (has_normals)
        for (int a = 0; a < 3; ++a) nr[a] = base_normals[3u * at + a];
    const MorphFold F{active + s.active0, position_deltas + 3u * (size_t)s.delta0,
                      fold_normals ? normal_deltas + 3u * (size_t)s.normal_delta0 : nullptr, m.vertex_count, v};
    uint32_t b = 0;
    if (fold_normals) {  // (uniform per mesh, like both trip counts)
        for (; b + (uint32_t)MORPH_BATCH <= s.active_count; b += (uint32_t)MORPH_BATCH) morph_batch<MORPH_BATCH, true>(F, b, p, nr);
        for (; b < s.active_count; ++b) morph_batch<1, true>(F, b, p, nr);
    } else {
        for (; b + (uint32_t)MORPH_BATCH <= s.active_count; b += (uint32_t)MORPH_BATCH) morph_batch<MORPH_BATCH, false>(F, b, p, nr);
        for (; b < s.active_count; ++b) morph_batch<1, false>(F, b, p, nr);
    }
    if (s.skin0 != MORPH_NONE)
        skin_vertex(joint_indices, joint_weights, palettes, (size_t)s.skin0 + v, s.joint0, has_normals, p, nr);
    for (int a = 0; a < 3; ++a) positions[3u * (size_t)i + a] = p[a];
    if (has_normals)
        for (int a = 0; a < 3; ++a) normals[3u * (size_t)i + a] = nr[a];
}
// One workgroup per posed mesh: the box of its staged (posed) positions by hk_skin.h's bounds rule, stated without an
// order: each bound's value by fminf / fmaxf (exact in any order; a NaN loses, as in the host's fold), and a bound of 0
// with the sign of the last vertex in vertex order whose component is a zero (coop_split's keyed atomicMax; the index
// is below 2^30, hk_skin_meshes' bound).  Then the Bevy Aabb (centre, half extents) over the rows of local_aabbs whose
// instance record carries this mesh's slice: one thread per instance, strided.  The records are those before the
// rebuild; k_update_instances leaves their mesh slices as they are.
// (slices: where the posed meshes' hk_mesh_index records lie, in a SkinSource or a MorphSource table)
__global__ __launch_bounds__(256) void k_skin_bounds(const MeshUpdate* tab, PosedSlices slices,
                                                     const float* positions, const hk_instance* inst, uint32_t n_inst,
                                                     float* local_aabbs)
{
    __shared__ CoopShared sh;
    const MeshUpdate m = tab[blockIdx.x];
    const hk_mesh_index mesh =
        *reinterpret_cast<const hk_mesh_index*>((const char*)slices.first + (size_t)blockIdx.x * slices.stride);
    const float* p = positions + 3u * (size_t)m.vertex0;
    const float inf = __uint_as_float(0x7F800000u);
    float b[6] = {inf, inf, inf, -inf, -inf, -inf};
    const int op[6] = {0, 0, 0, 1, 1, 1};
    for (uint32_t v = threadIdx.x; v < m.vertex_count; v += 256u)
        for (int k = 0; k < 3; ++k) {
            const float x = p[3u * (size_t)v + k];
            b[k] = fminf(b[k], x), b[3 + k] = fmaxf(b[3 + k], x);
        }
    block_reduce<6>(b, op, sh);
    for (int j = 0; j < 6; ++j) {  // (b[] is the same in every thread: the branch is block-uniform)
        if (b[j] != 0.0f) continue;
        if (threadIdx.x == 0) sh.u[0] = 0u;
        __syncthreads();
        uint32_t key = 0u;  // (index + 1) * 2 + sign bit of the thread's last zero
        for (uint32_t v = threadIdx.x; v < m.vertex_count; v += 256u) {
            const float x = p[3u * (size_t)v + j % 3];
            if (x == 0.0f) key = ((v + 1u) << 1) | (__float_as_uint(x) >> 31);
        }
        if (key) atomicMax(&sh.u[0], key);
        __syncthreads();
        b[j] = (sh.u[0] & 1u) ? -0.0f : 0.0f;
        __syncthreads();
    }
    float aabb[6];
    hk_skin_aabb(b, b + 3, aabb);
    for (uint32_t i = threadIdx.x; i < n_inst; i += 256u) {
        const hk_mesh_index& x = inst[i].mesh;
        if (x.vertex == mesh.vertex && x.primitive == mesh.primitive && x.node[0] == mesh.node[0] &&
            x.node[1] == mesh.node[1])
            for (int k = 0; k < 6; ++k) local_aabbs[6u * (size_t)i + k] = aabb[k];
    }
}

// ---- appended meshes (mesh.rs:77-166 prepare_mesh_assets on AssetEvent::Created, mod.rs:379-467 GpuMesh::try_from;
// hk_scene.cpp hks_add_mesh + hks_build "concatenate").  One thread per vertex of the new meshes: the
// whole hk_vertex (position, u | normal, v) from the three staged attribute streams, as two 16-byte stores.  Then one
// thread per triangle: its three mesh-local indices (a list: 3t, 3t + 1, 3t + 2; a strip: t, t + 1, t + 2 with the
// first two swapped for an odd mesh-local t, as hks_add_mesh winds it; no indices: the identity), the whole
// hk_primitive as three 16-byte stores (position, index per corner), and its shape box folded as
// k_update_mesh_geometry folds it.  The triangles read the staged positions, not the vertex array, so the two halves
// do not depend on each other.  Every index was checked against vertex_count on the host (hk_add_meshes).
__global__ __launch_bounds__(256) void k_assemble_meshes(const MeshUpdate* tab, const MeshSource* sources,
                                                         uint32_t n_meshes, uint32_t n_vertices, uint32_t n_shapes,
                                                         const float* positions, const float* normals, const float* uvs,
                                                         const uint32_t* indices, hk_vertex* vertices,
                                                         hk_primitive* prims, BBox* shapes)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_vertices) {
        const MeshUpdate& m = tab[mesh_of(tab, n_meshes, i, false)];
        const uint32_t v = i - m.vertex0;
        if (v >= m.vertex_count) return;
        const float* p = positions + 3u * (size_t)i;
        const float* n = normals + 3u * (size_t)i;
        const float* t = uvs + 2u * (size_t)i;
        float4* out = reinterpret_cast<float4*>(vertices + m.vertex + v);
        out[0] = make_float4(p[0], p[1], p[2], t[0]);
        out[1] = make_float4(n[0], n[1], n[2], t[1]);
        return;
    }
    const uint32_t j = i - n_vertices;
    if (j >= n_shapes) return;
    const uint32_t k = mesh_of(tab, n_meshes, j, true);
    const MeshUpdate& m = tab[k];
    const MeshSource s = sources[k];
    const uint32_t t = j - m.shape0;
    if (t >= m.shapes) return;
    const uint32_t odd = s.strip ? (t & 1u) : 0u;
    const uint32_t first = s.strip ? t : 3u * t;
    const uint32_t at[3] = {first + odd, first + 1u - odd, first + 2u};
    float4* out = reinterpret_cast<float4*>(prims + m.primitive + t);
    const float inf = __uint_as_float(0x7F800000u);
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (int c = 0; c < 3; ++c) {
        const uint32_t v = s.index0 == MESH_NO_INDICES ? at[c] : indices[(size_t)s.index0 + at[c]];
        const float* p = positions + 3u * (size_t)(m.vertex0 + v);
        const float x[3] = {p[0], p[1], p[2]};
        for (int a = 0; a < 3; ++a) {
            mn[a] = host_fmin(mn[a], x[a]);
            mx[a] = host_fmax(mx[a], x[a]);
        }
        out[c] = make_float4(x[0], x[1], x[2], __uint_as_float(v));
    }
    shapes[j] = BBox{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}};
}

// ---- a new mesh asset list (mesh.rs:89-92, 123-126 AssetEvent::Removed, mesh.rs:140-163 the three buffers rebuilt in
// the BTreeMap's order).  The kept meshes' vertices, primitives and asset nodes gathered out of place
// into their slices of the new layout: one thread per 16-byte chunk of the destination arrays (a vertex is 2 chunks, a
// primitive 3, a node 2), the vertices' chunks first, then the primitives', then the nodes'.  A thread finds its list
// entry by mesh_of's search over the destination starts, which ascend, and does one 16-byte load and one 16-byte
// store; consecutive lanes read and write consecutive addresses inside a slice.  The bytes move verbatim: vertex and
// node indices are mesh-relative.  A new mesh's chunks are left to k_assemble_meshes and k_build_mesh_bvh.  The thread
// of a node's first chunk, kept or new, also writes the node's three words of the per-node mesh tables (primitive
// offset, node base, node count) at `stride`.
HKD uint32_t move_of(const MeshMove* tab, uint32_t n, uint32_t e, int array)
{
    uint32_t lo = 0, hi = n;  // the last entry whose first destination element is <= e
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].dst[array] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void k_move_mesh_slices(const MeshMove* tab, uint32_t n_meshes, uint32_t n_vertices,
                                                          uint32_t n_prims, uint32_t n_nodes, const uint4* src_vertices,
                                                          const uint4* src_prims, const uint4* src_nodes,
                                                          uint4* vertices, uint4* prims, uint4* nodes, uint32_t* aux,
                                                          size_t stride)
{
    // (3 x 2^30 primitive chunks pass 32 bits: the chunk index is 64-bit, the table holds elements)
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t chunks[3] = {2u * (uint64_t)n_vertices, 3u * (uint64_t)n_prims, 2u * (uint64_t)n_nodes};
    int array = 0;
    while (array < 3 && i >= chunks[array]) i -= chunks[array++];
    if (array == 3) return;
    const uint32_t per = array == 1 ? 3u : 2u;
    const uint32_t e = (uint32_t)(i / per), sub = (uint32_t)(i - (uint64_t)e * per);
    const MeshMove& m = tab[move_of(tab, n_meshes, e, array)];
    const uint32_t off = e - m.dst[array];
    if (off >= m.count[array]) return;  // (the entries tile the arrays; never taken)
    if (array == 2 && sub == 0) {
        aux[e] = m.dst[1];
        aux[stride + e] = m.dst[2];
        aux[2 * stride + e] = m.count[2];
    }
    if (m.src[0] == MESH_MOVE_NEW) return;
    const uint4* from = array == 0 ? src_vertices : array == 1 ? src_prims : src_nodes;
    uint4* to = array == 0 ? vertices : array == 1 ? prims : nodes;
    to[i] = from[((uint64_t)m.src[array] + off) * per + sub];
}

// ---- instance records (instance.rs:284-330; hk_scene.cpp hks_build "instances")
HKD void transform_point(const float* m, const float* p, float* o)
{
    for (int r = 0; r < 3; ++r) o[r] = ((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r];
}
HKD void transform_vector(const float* m, const float* p, float* o)
{
    for (int r = 0; r < 3; ++r) o[r] = (m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2];
}
HKD bool inverse_transpose_d(const float* m, float* out)
{
    double a[16], inv[16];
    for (int i = 0; i < 16; ++i) a[i] = m[i];
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] +
             a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] -
             a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] +
             a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] -
              a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] -
             a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] +
             a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] -
             a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] +
              a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] +
             a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] -
             a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] +
              a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] -
              a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] -
             a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] +
             a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] -
              a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] +
              a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    if (det == 0.0) return false;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) out[c * 4 + r] = (float)(inv[r * 4 + c] / det);
    return true;
}

__global__ __launch_bounds__(256) void k_update_instances(hk_instance* inst, uint32_t n, const float* models,
                                                          const float* local_aabbs, BBox* boxes, uint32_t* singular)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    hk_instance& g = inst[i];
    const float* m = models + 16u * i;
    const float* center = local_aabbs + 6u * i;
    const float* half = center + 3;
    float c[3];
    transform_point(m, center, c);
    float mn[3] = {0.0f, 0.0f, 0.0f}, mx[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 8; ++k) {
        const float sx = (float)(2 * (k & 1) - 1), sy = (float)(2 * ((k >> 1) & 1) - 1), sz = (float)(2 * ((k >> 2) & 1) - 1);
        const float v[3] = {half[0] * sx, half[1] * sy, half[2] * sz};
        float corner[3];
        transform_vector(m, v, corner);
        for (int d = 0; d < 3; ++d) {
            mn[d] = host_fmin(mn[d], corner[d]);
            mx[d] = host_fmax(mx[d], corner[d]);
        }
    }
    BBox b;
    for (int d = 0; d < 3; ++d) {
        g.min[d] = b.mn[d] = mn[d] + c[d];
        g.max[d] = b.mx[d] = mx[d] + c[d];
    }
    for (int k = 0; k < 16; ++k) g.model[k] = m[k];
    if (!inverse_transpose_d(m, g.inverse_transpose_model)) atomicOr(singular, 1u);
    boxes[i] = b;
}

// ---- a new instance set (instance.rs:123-175 InstanceEvent, 245-444 prepare_instances)
// One thread per instance of the new set: k_update_instances' record with everything else an hk_instance holds (the
// host memsets each record, and the buffer holds the records of the set before: material, a zeroed node_index for
// k_backfill_nodes and the mesh slice are written too), the previous model gathered from the set before
// (transform.rs:8-44: a surviving entity keeps the model the last G-buffer saw, a new one starts from its own), and
// for k_compact_emitters whether the material emits (hk_scene.cpp hks_build: 255 a |rgb| > 0 in float, false for a
// NaN) and the mesh's primitive count.  Material and previous indices were checked on the host (hk_set_instances).
__global__ __launch_bounds__(256) void k_set_instances(hk_instance* inst, uint32_t n, const InstanceDesc* set,
                                                       const float* models, const float* local_aabbs,
                                                       const hk_material* mats, const float* prev_models,
                                                       uint32_t n_prev, float* new_prev, BBox* boxes, uint2* emitter,
                                                       uint32_t* singular)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const InstanceDesc d = set[i];
    const float* m = models + 16u * (size_t)i;
    const float* center = local_aabbs + 6u * (size_t)i;
    const float* half = center + 3;
    float c[3];
    transform_point(m, center, c);
    float mn[3] = {0.0f, 0.0f, 0.0f}, mx[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 8; ++k) {
        const float sx = (float)(2 * (k & 1) - 1), sy = (float)(2 * ((k >> 1) & 1) - 1), sz = (float)(2 * ((k >> 2) & 1) - 1);
        const float v[3] = {half[0] * sx, half[1] * sy, half[2] * sz};
        float corner[3];
        transform_vector(m, v, corner);
        for (int a = 0; a < 3; ++a) {
            mn[a] = host_fmin(mn[a], corner[a]);
            mx[a] = host_fmax(mx[a], corner[a]);
        }
    }
    hk_instance g;
    BBox b;
    for (int a = 0; a < 3; ++a) {
        g.min[a] = b.mn[a] = mn[a] + c[a];
        g.max[a] = b.mx[a] = mx[a] + c[a];
    }
    g.material = d.material;
    g.node_index = 0u;
    for (int k = 0; k < 16; ++k) g.model[k] = m[k];
    if (!inverse_transpose_d(m, g.inverse_transpose_model)) atomicOr(singular, 1u);
    g.mesh = d.mesh;
    inst[i] = g;
    boxes[i] = b;
    const float* pm = d.previous < n_prev ? prev_models + 16u * (size_t)d.previous : m;  // INSTANCE_NEW: its own
    for (int k = 0; k < 16; ++k) new_prev[16u * (size_t)i + k] = pm[k];
    const float* e = mats[d.material].emissive;
    const float intensity = (255.0f * e[3]) * sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    emitter[i] = make_uint2(intensity > 0.0f ? 1u : 0u, (d.mesh.node[1] + 2u) / 3u);
}

// One workgroup walks the instances in index order, 256 per chunk: the emitters' ranks from wave ballots (as
// coop_split and k_update_emissives rank), their alias offsets from an exclusive scan of the primitive counts over
// the emitters (a __shfl_up scan per wave, the waves' totals through LDS, a running carry between chunks), and each
// hk_emissive written whole: instance and alias range, everything else zero for k_update_emissives and
// k_backfill_nodes to fill.  totals[0], [1]: emitters and alias entries, for the host to compare with its own
// arithmetic; room: the records the host sized `em` for.  Integer arithmetic throughout.
__global__ __launch_bounds__(256) void k_compact_emitters(const uint2* emitter, uint32_t n, hk_emissive* em,
                                                          uint32_t room, uint32_t* totals)
{
    __shared__ uint32_t wave_n[4], wave_prims[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t rank_carry = 0, alias_carry = 0;
    for (uint32_t base = 0; base < n; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const uint2 e = i < n ? emitter[i] : make_uint2(0u, 0u);
        const bool emits = e.x != 0u;
        const uint32_t prims = emits ? e.y : 0u;
        const unsigned long long mask = __ballot(emits);
        uint32_t incl = prims;  // inclusive scan over the wave
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += t;
        }
        if (lane == 63u) {
            wave_n[w] = (uint32_t)__popcll(mask);
            wave_prims[w] = incl;
        }
        __syncthreads();
        uint32_t rank = rank_carry, offset = alias_carry;
        for (uint32_t j = 0; j < w; ++j) {
            rank += wave_n[j];
            offset += wave_prims[j];
        }
        rank += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        offset += incl - prims;
        if (emits && rank < room) {
            hk_emissive r;
            for (int k = 0; k < 4; ++k) r.emissive[k] = 0.0f;
            for (int k = 0; k < 3; ++k) r.position[k] = 0.0f;
            r.radius = 0.0f;
            r.instance = i;
            r._pad0 = 0u;
            r.alias_table[0] = offset;
            r.alias_table[1] = prims;
            r.surface_area = 0.0f;
            r.node_index = 0u;
            r._pad1[0] = r._pad1[1] = 0u;
            em[rank] = r;
        }
        rank_carry += (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
        alias_carry += (wave_prims[0] + wave_prims[1]) + (wave_prims[2] + wave_prims[3]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        totals[0] = rank_carry;
        totals[1] = alias_carry;
    }
}

// ---- emissive records + alias tables (instance.rs:377-420, mod.rs:318-376)
struct AliasWork {
    uint32_t index;
    float prob;
};
// transformed_primitive_areas (mod.rs:318-328): one thread per (emitter, primitive) = alias entry
__global__ __launch_bounds__(256) void k_emissive_areas(const hk_emissive* em, uint32_t n_em, const hk_instance* inst,
                                                        const hk_primitive* prims, uint32_t n_alias, float* areas)
{
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= n_alias) return;
    uint32_t lo = 0, hi = n_em;  // the emitter whose alias range holds a (offsets ascend)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (em[mid].alias_table[0] <= a) lo = mid;
        else hi = mid;
    }
    const hk_emissive& r = em[lo];
    if (a < r.alias_table[0] || a >= r.alias_table[0] + r.alias_table[1]) return;
    const hk_instance& in = inst[r.instance];
    const hk_primitive& pr = prims[in.mesh.primitive + (a - r.alias_table[0])];
    float w[3][3];
    for (int k = 0; k < 3; ++k) transform_point(in.model, pr.vertices[k].position, w[k]);
    const float ux = w[1][0] - w[0][0], uy = w[1][1] - w[0][1], uz = w[1][2] - w[0][2];
    const float vx = w[2][0] - w[0][0], vy = w[2][1] - w[0][1], vz = w[2][2] - w[0][2];
    // hk_scene.cpp cross(): (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)
    const float cx = uy * vz - vy * uz, cy = uz * vx - vz * ux, cz = ux * vy - vx * uy;
    areas[a] = 0.5f * fabsf(sqrtf((cx * cx + cy * cy) + cz * cz));
}

// One wave per emitter: the host's sequential surface-area sum (lane 0), the over / under lists
// by wave-ballot compaction (index order, as the host's two passes), then the alias while-loop
// on lane 0 with the stacks in LDS (global scratch beyond ALIAS_LDS entries).
constexpr uint32_t ALIAS_LDS = 3072;
__global__ __launch_bounds__(64) void k_update_emissives(hk_emissive* em, uint32_t n_em, const hk_instance* inst,
                                                         const hk_material* mats, hk_alias_entry* alias,
                                                         const float* areas, AliasWork* work, BBox* boxes)
{
    __shared__ AliasWork s_over[ALIAS_LDS], s_under[ALIAS_LDS];
    __shared__ float s_sum;
    const uint32_t e = blockIdx.x;
    if (e >= n_em) return;
    const uint32_t lane = threadIdx.x;
    hk_emissive& r = em[e];
    const hk_instance& in = inst[r.instance];
    const hk_material& mat = mats[in.material];
    const uint32_t off = r.alias_table[0], count = r.alias_table[1];
    const float* a = areas + off;  // k_emissive_areas
    if (lane == 0) {
        float sum = 0.0f;
        for (uint32_t p = 0; p < count; ++p) sum += a[p];  // the host's summation order
        s_sum = sum;
    }
    hk_alias_entry* t = alias + off;
    for (uint32_t i = lane; i < count; i += 64u) t[i] = hk_alias_entry{0.0f, i};
    __syncthreads();
    const float surface_area = s_sum;
    const float mean_area = surface_area / (float)count;
    const bool in_lds = count <= ALIAS_LDS;
    AliasWork* over = in_lds ? s_over : work + 2u * off;
    AliasWork* under = in_lds ? s_under : work + 2u * off + count;
    uint32_t n_over = 0, n_under = 0;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < count; base += 64u) {
        const uint32_t i = base + lane;
        const float prob = i < count ? a[i] / mean_area : 1.0f;
        const bool o = prob > 1.0f, u = prob < 1.0f;
        const unsigned long long mo = __ballot(o), mu = __ballot(u);
        if (o) over[n_over + (uint32_t)__popcll(mo & lt)] = AliasWork{i, prob};
        if (u) under[n_under + (uint32_t)__popcll(mu & lt)] = AliasWork{i, prob};
        n_over += (uint32_t)__popcll(mo);
        n_under += (uint32_t)__popcll(mu);
    }
    __syncthreads();
    if (lane == 0) {
        while (n_under && n_over) {
            AliasWork ob = over[--n_over];
            AliasWork ub = under[--n_under];
            const float delta = 1.0f - ub.prob;
            ob.prob -= delta;
            if (ob.prob > 1.0f) over[n_over++] = ob;
            else if (ob.prob < 1.0f) under[n_under++] = ob;
            t[ub.index] = hk_alias_entry{delta, ob.index};
        }
        const float el = sqrtf((mat.emissive[0] * mat.emissive[0] + mat.emissive[1] * mat.emissive[1]) +
                               mat.emissive[2] * mat.emissive[2]);
        const float intensity = (255.0f * mat.emissive[3]) * el;
        const float dx = in.max[0] - in.min[0], dy = in.max[1] - in.min[1], dz = in.max[2] - in.min[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        float pos[3];
        for (int k = 0; k < 3; ++k) pos[k] = (in.max[k] + in.min[k]) * 0.5f;
        const float radius = 0.5f * sqrtf(d2) + sqrtf(intensity);
        for (int k = 0; k < 4; ++k) r.emissive[k] = mat.emissive[k];
        for (int k = 0; k < 3; ++k) r.position[k] = pos[k];
        r.radius = radius;
        r.surface_area = surface_area;
        BBox b;
        for (int k = 0; k < 3; ++k) {
            b.mn[k] = pos[k] - radius;
            b.mx[k] = pos[k] + radius;
        }
        boxes[e] = b;
    }
}

// BHShape::set_bh_node_index: leaf node index back into the shape record
__global__ __launch_bounds__(256) void k_backfill_nodes(const hk_node* tlas, uint32_t n_tlas, hk_instance* inst,
                                                        const hk_node* lbvh, uint32_t n_lbvh, hk_emissive* em)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_tlas && tlas[i].entry_index >= HK_BVH_LEAF_FLAG) inst[tlas[i].entry_index - HK_BVH_LEAF_FLAG].node_index = i;
    if (i < n_lbvh && lbvh[i].entry_index >= HK_BVH_LEAF_FLAG) em[lbvh[i].entry_index - HK_BVH_LEAF_FLAG].node_index = i;
}

// ---- instance refit (include/hk_refit.h: the rule over given shape boxes, this project's own; the host
// side is hk_scene.cpp hks_refit_boxes over the same header).  The TLAS and the light BVH keep their topology, so every
// node_index in the instance and emissive records stays and nothing is backfilled; every entry node's box becomes the
// hk_minf / hk_maxf fold of the shape boxes of the leaves stored in its range (i, exit).  One launch sequence serves
// both trees: a table of at most two RefitTree records (node array, records, count), its nodes laid end to end.  The
// tiers are k_refit_small's and k_refit_large's: a thread per node, ranges up to REFIT_SMALL scanned in registers,
// larger ones listed (one atomicAdd on a counter the stream zeroed) for a workgroup each in the next launch.  Every
// box is folded from leaves alone: nothing passes between workgroups inside a launch, no fence, no spin wait; the
// stream orders the launches.
// Where the shape boxes come from: the RECORDS.  S[t] of the TLAS is the min / max k_update_instances stored in
// instance t, S[e] of the light BVH is position -+ radius of the emissive record k_update_emissives stored, the very
// f32 operations that kernel puts into boxes[e].  So the refit never reads the boxes scratch, whose head
// k_update_emissives overwrites with the emitters' boxes after k_update_instances filled it with the instances' (the
// rebuild orders the two by building the TLAS in between; the refit has nothing to order), and never a leaf's own box:
// the device TLAS carries leaf boxes from launch_fill_leaves, stale until refresh_tlas_derivatives refills them
// after these launches.  Only min / max of entry nodes are written; the words the scans read (entry_index,
// exit_index, the records) are written by nobody here.
// Hostile sizes (hk_scene_upload takes any tree of 3n - 2 nodes): an exit past the tree is clamped, a payload past
// the records is skipped, the list takes no more entries than it has room for.  Never taken on a well-formed tree.
HKD void refit_tree_scan(const RefitTree& t, uint32_t j, float* box)
{
    const uint32_t entry = t.nodes[j].entry_index;
    if (!hk_refit_is_leaf(entry)) return;
    const uint32_t s = hk_refit_leaf_primitive(entry);
    if (s >= t.shapes) return;  // (a built tree's payloads are its own shapes; never taken)
    float b[6];
    if (t.emitters) hk_refit_emitter_box((const hk_emissive*)t.records + s, b);
    else hk_refit_instance_box((const hk_instance*)t.records + s, b);
    hk_refit_join(box, b, b + 3);
}
// node g of the trees laid end to end: its tree (*i: its index there); tree 0 has 3 x shapes - 2 nodes
HKD RefitTree refit_tree_of(const RefitTrees& T, uint32_t g, uint32_t* i)
{
    const uint32_t n0 = 3u * T.tree[0].shapes - 2u;
    const uint32_t k = T.n_trees > 1u && g >= n0 ? 1u : 0u;
    *i = g - (k ? n0 : 0u);
    return k ? T.tree[1] : T.tree[0];
}
__global__ __launch_bounds__(256) void k_refit_trees_small(RefitTrees T, uint32_t* large, uint32_t large_room,
                                                           uint32_t* n_large)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= T.n_nodes) return;
    uint32_t i;
    const RefitTree t = refit_tree_of(T, g, &i);
    if (t.shapes == 0u) return;  // (no table entry without shapes; never taken)
    const uint32_t count = 3u * t.shapes - 2u;
    if (i >= count) return;
    if (hk_refit_is_leaf(t.nodes[i].entry_index)) return;
    const uint32_t exit = t.nodes[i].exit_index, e = exit < count ? exit : count;
    if (e > i && e - i > REFIT_SMALL) {
        const uint32_t at = atomicAdd(n_large, 1u);
        if (at < large_room) large[at] = g;
        return;
    }
    float box[6];
    hk_refit_empty(box);
    for (uint32_t j = i + 1u; j < e; ++j) refit_tree_scan(t, j, box);
    for (int c = 0; c < 3; ++c) {
        t.nodes[i].min[c] = box[c];
        t.nodes[i].max[c] = box[3 + c];
    }
}
__global__ __launch_bounds__(256) void k_refit_trees_large(RefitTrees T, const uint32_t* large, uint32_t large_room,
                                                           const uint32_t* n_large)
{
    __shared__ CoopShared sh;
    const uint32_t listed = *n_large < large_room ? *n_large : large_room;
    const int op[6] = {0, 0, 0, 1, 1, 1};
    for (uint32_t w = blockIdx.x; w < listed; w += gridDim.x) {  // (block-uniform)
        const uint32_t g = large[w];
        if (g >= T.n_nodes) continue;  // (k_refit_trees_small listed a node of the trees; never taken)
        uint32_t i;
        const RefitTree t = refit_tree_of(T, g, &i);
        const uint32_t count = 3u * t.shapes - 2u;
        if (t.shapes == 0u || i >= count) continue;  // (likewise)
        const uint32_t exit = t.nodes[i].exit_index, e = exit < count ? exit : count;
        float box[6];
        hk_refit_empty(box);
        for (uint32_t j = i + 1u + threadIdx.x; j < e; j += 256u) refit_tree_scan(t, j, box);
        block_reduce<6>(box, op, sh);
        if (threadIdx.x < 3u) t.nodes[i].min[threadIdx.x] = box[threadIdx.x];
        else if (threadIdx.x < 6u) t.nodes[i].max[threadIdx.x - 3u] = box[threadIdx.x];
    }
}

// the table of a refit: the TLAS over the instance records and, where there are emitters, the light BVH over theirs
static RefitTrees refit_trees(const DynamicArgs& D)
{
    RefitTrees T;
    T.tree[0] = RefitTree{D.tlas, D.instances, D.n_instances, 0u};
    T.tree[1] = RefitTree{D.lbvh, D.emissives, D.n_emissives, 1u};
    T.n_trees = D.n_emissives ? 2u : 1u;
    T.n_nodes = 3u * D.n_instances - 2u + (D.n_emissives ? 3u * D.n_emissives - 2u : 0u);
    return T;
}

// One step of what follows the uploads (hk_launch.h DynamicStep).  The list of large nodes of a refit lies in the
// builds' segments, which a refit leaves unused (2 x max(n, m) x 12 B: more words than both trees have nodes); its
// counter is flags[2], zeroed with the flags and otherwise a new instance set's.
void launch_dynamic_step(const DynamicArgs& D, DynamicStep step, hipStream_t st)
{
    const uint32_t n = D.n_instances, m = D.n_emissives;
    auto build = [&](uint32_t count, hk_node* out, uint32_t* levels) {
        if (count <= BVH_LDS_SHAPES)
            hipLaunchKernelGGL(k_build_bvh<true>, dim3(1), dim3(256), 0, st, (const BBox*)D.boxes, count, D.buckets, out,
                               D.idx, (Segment*)D.segments, levels);
        else
            hipLaunchKernelGGL(k_build_bvh<false>, dim3(1), dim3(256), 0, st, (const BBox*)D.boxes, count, D.buckets,
                               out, D.idx, (Segment*)D.segments, levels);
    };
    const uint32_t large_room = 6u * (n > m ? n : m);
    switch (step) {
    case DYN_RECORDS:
        hipLaunchKernelGGL(k_update_instances, dim3((n + 255u) / 256u), dim3(256), 0, st, D.instances, n, D.models,
                           D.local_aabbs, (BBox*)D.boxes, D.flags);
        break;
    case DYN_TLAS_BUILD:
        build(n, D.tlas, D.flags + 1);
        break;
    case DYN_EMISSIVE_AREAS:
        if (m)
            hipLaunchKernelGGL(k_emissive_areas, dim3((D.n_alias + 255u) / 256u), dim3(256), 0, st, D.emissives, m,
                               D.instances, D.primitives, D.n_alias, D.areas);
        break;
    case DYN_EMISSIVES:
        if (m)
            hipLaunchKernelGGL(k_update_emissives, dim3(m), dim3(64), 0, st, D.emissives, m, D.instances, D.materials,
                               D.alias, D.areas, (AliasWork*)D.alias_work, (BBox*)D.boxes);
        break;
    case DYN_LBVH_BUILD:
        if (m) build(m, D.lbvh, nullptr);
        break;
    case DYN_BACKFILL: {
        const uint32_t k = 3u * n - 2u > 3u * m ? 3u * n - 2u : 3u * m;
        hipLaunchKernelGGL(k_backfill_nodes, dim3((k + 255u) / 256u), dim3(256), 0, st, D.tlas, 3u * n - 2u, D.instances,
                           D.lbvh, m ? 3u * m - 2u : 0u, D.emissives);
        break;
    }
    case DYN_REFIT_SMALL: {
        const RefitTrees T = refit_trees(D);
        hipLaunchKernelGGL(k_refit_trees_small, dim3((T.n_nodes + 255u) / 256u), dim3(256), 0, st, T,
                           (uint32_t*)D.segments, large_room, D.flags + 2);
        break;
    }
    case DYN_REFIT_LARGE: {
        // (nothing where neither tree can hold a large node: the bound of a BLAS slice holds for any such flatten)
        const uint32_t bound = mesh_refit_large_bound(n) + mesh_refit_large_bound(m);
        if (bound == 0u) break;
        hipLaunchKernelGGL(k_refit_trees_large, dim3(bound < REFIT_LARGE_GRID ? bound : REFIT_LARGE_GRID), dim3(256), 0,
                           st, refit_trees(D), (const uint32_t*)D.segments, large_room, (const uint32_t*)(D.flags + 2));
        break;
    }
    }
}

// ---- tree costs (include/hk_cost.h: the rule, this project's own; the host side is hk_scene.cpp
// hks_tree_cost over the same header).  How expensive the resident trees are to walk, for a caller that refits and has
// to decide when to rebuild.  One launch serves every listed tree: a table of CostSlice records (hk_launch.h), their
// nodes laid end to end as RefitTrees lays two, a thread per node.  A thread finds its slice by bisection over the
// slices' first nodes, loads its node as two 16-byte words and, where it is an entry node, weighs its half area against
// the slice's root's (the join of the slice's two top entries, which every entry thread of the slice loads for itself:
// the same two nodes for a whole slice, out of L1/L2).  A leaf contributes nothing.
// The sums are 64-bit INTEGERS (32.32 fixed point), so they have no order and the words are the host's whatever the
// arrival order: no float atomics.  A workgroup's 256 consecutive nodes touch at most 256 consecutive slices; each has
// a row of LDS accumulators.  A wave whose 64 nodes lie in one slice (the common case) sums in registers (__shfl_xor)
// and adds once to the row, a wave that straddles slices adds lane by lane; after the barrier one thread per touched
// slice adds the row to the slice's global accumulators, which the stream zeroed before the launch: one global add per
// field per workgroup per slice it touches.  Nothing passes between workgroups inside the launch: no fence, no spin
// wait; the stream orders the zeroing, the launch and the readback.  root_half_area has one writer, node 0's thread.
// Hostile trees (hk_scene_upload takes any nodes): every index is bounded by the slice's count alone: an exit past the
// slice is clamped, a top entry's exit past the slice leaves the root node 0's box alone.  Never taken on a
// well-formed tree.
struct CostShared {
    unsigned long long inner[256], leaf[256];
    uint32_t entries[256];
};
// the slice that holds node g of the launch: the last one that starts at or before it (every slice has a node)
HKD uint32_t cost_slice_of(const CostSlice* tab, uint32_t n, uint32_t g)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].first <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
// node i of a slice as two 16-byte loads: its box (min xyz, max xyz), entry_index and exit_index
HKD void cost_load_node(const hk_node* nodes, uint32_t i, float* box, uint32_t* entry, uint32_t* exit)
{
    const float4* p = (const float4*)(nodes + i);
    const float4 a = p[0], b = p[1];
    box[0] = a.x, box[1] = a.y, box[2] = a.z;
    box[3] = b.x, box[4] = b.y, box[5] = b.z;
    *entry = __float_as_uint(a.w);
    *exit = __float_as_uint(b.w);
}
// R of a slice of count >= 2 nodes
HKD float cost_root_half_area(const hk_node* nodes, uint32_t count)
{
    float a[6], b[6], root[6];
    uint32_t entry, exit;
    cost_load_node(nodes, 0u, a, &entry, &exit);
    // (a top entry's exit past the slice: node 0's box alone, joined twice, which changes nothing; registers throughout)
    cost_load_node(nodes, exit < count ? exit : 0u, b, &entry, &exit);
    hk_cost_root(a, b, root);
    return hk_cost_half_area(root);
}
__global__ __launch_bounds__(256) void k_tree_cost(const CostSlice* tab, uint32_t n_slices, uint32_t n_nodes,
                                                   hk_tree_cost* out)
{
    __shared__ CostShared sh;
    const uint32_t g0 = blockIdx.x * 256u, g = g0 + threadIdx.x;
    sh.inner[threadIdx.x] = 0ull;
    sh.leaf[threadIdx.x] = 0ull;
    sh.entries[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t s0 = cost_slice_of(tab, n_slices, g0);  // (block-uniform: g0 < n_nodes by the grid's size)
    // a thread past the last node stands in the last slice with nothing to add, so that every lane reaches the shuffles
    const uint32_t s = g < n_nodes ? cost_slice_of(tab, n_slices, g) : n_slices - 1u;
    unsigned long long inner = 0ull, leaf = 0ull;
    uint32_t entries = 0u;
    if (g < n_nodes) {
        const CostSlice c = tab[s];
        const uint32_t i = g - c.first;
        if (c.count > 1u && i < c.count) {  // (a lone leaf has no entry node)
            float box[6];
            uint32_t entry, exit;
            cost_load_node(c.nodes, i, box, &entry, &exit);
            if (!hk_refit_is_leaf(entry)) {
                const float R = cost_root_half_area(c.nodes, c.count);
                const unsigned long long q = hk_cost_weight(hk_cost_half_area(box), R);
                if (hk_cost_over_leaf(i, exit < c.count ? exit : c.count)) leaf = q;
                else inner = q;
                entries = 1u;
                if (i == 0u) out[c.slot].root_half_area = R;
            }
        }
    }
    const uint32_t row = s - s0;  // (< 256: the slices between two nodes of one workgroup)
    if (__shfl(s, 0, 64) == __shfl(s, 63, 64)) {  // (s rises with the lane: the whole wave in one slice)
        for (int o = 32; o > 0; o >>= 1) {
            inner += __shfl_xor(inner, o, 64);
            leaf += __shfl_xor(leaf, o, 64);
            entries += __shfl_xor(entries, o, 64);
        }
        if ((threadIdx.x & 63u) != 0u) entries = 0u;  // (lane 0 adds for the wave)
    }
    if (entries && row < 256u) {
        atomicAdd(&sh.inner[row], inner);
        atomicAdd(&sh.leaf[row], leaf);
        atomicAdd(&sh.entries[row], entries);
    }
    __syncthreads();
    if (sh.entries[threadIdx.x]) {  // (a touched slice: s0 + threadIdx.x < n_slices)
        hk_tree_cost* o = out + tab[s0 + threadIdx.x].slot;
        atomicAdd((unsigned long long*)&o->inner, sh.inner[threadIdx.x]);
        atomicAdd((unsigned long long*)&o->leaf, sh.leaf[threadIdx.x]);
        atomicAdd(&o->entries, sh.entries[threadIdx.x]);
    }
}
void launch_tree_cost(const CostSlice* table, uint32_t n_slices, uint32_t n_nodes, hk_tree_cost* out, hipStream_t st)
{
    if (n_slices == 0u || n_nodes == 0u) return;
    hipLaunchKernelGGL(k_tree_cost, dim3((n_nodes + 255u) / 256u), dim3(256), 0, st, table, n_slices, n_nodes, out);
}

// what follows the instance records and their boxes: the TLAS, the emitters' areas, alias tables, records and light
// BVH, and the leaf node indices
static void launch_rebuild(const DynamicArgs& D, hipStream_t st)
{
    for (DynamicStep s : {DYN_TLAS_BUILD, DYN_EMISSIVE_AREAS, DYN_EMISSIVES, DYN_LBVH_BUILD, DYN_BACKFILL})
        launch_dynamic_step(D, s, st);
}

void launch_dynamic_update(const DynamicArgs& D, hipStream_t st)
{
    launch_dynamic_step(D, DYN_RECORDS, st);
    launch_rebuild(D, st);
}

void launch_set_instances(const DynamicArgs& D, const SetArgs& S, hipStream_t st)
{
    const uint32_t n = D.n_instances;
    hipLaunchKernelGGL(k_set_instances, dim3((n + 255u) / 256u), dim3(256), 0, st, D.instances, n, S.set, D.models,
                       D.local_aabbs, D.materials, S.prev_models, S.n_prev, S.new_prev, (BBox*)D.boxes, S.emitter,
                       D.flags);
    hipLaunchKernelGGL(k_compact_emitters, dim3(1), dim3(256), 0, st, (const uint2*)S.emitter, n, D.emissives,
                       D.n_emissives, D.flags + 2);
    launch_rebuild(D, st);
}

// tab: the LDS-sized meshes first (n_lds of them), then the others; levels[slot]: each mesh's split levels
static void launch_mesh_builds(const MeshUpdateArgs& M, hipStream_t st)
{
    if (M.n_lds)
        hipLaunchKernelGGL(k_build_mesh_bvh<true>, dim3(M.n_lds), dim3(256), 0, st, M.table_by_size, (const BBox*)M.shapes,
                           M.buckets, M.blas, M.idx, (Segment*)M.segments, M.levels);
    if (M.n_meshes > M.n_lds)
        hipLaunchKernelGGL(k_build_mesh_bvh<false>, dim3(M.n_meshes - M.n_lds), dim3(256), 0, st,
                           M.table_by_size + M.n_lds, (const BBox*)M.shapes, M.buckets, M.blas, M.idx,
                           (Segment*)M.segments, M.levels);
}
void launch_mesh_geometry(const MeshUpdateArgs& M, hipStream_t st)
{
    const uint32_t items = M.n_vertices + M.n_shapes;
    hipLaunchKernelGGL(k_update_mesh_geometry, dim3((items + 255u) / 256u), dim3(256), 0, st, M.table, M.n_meshes,
                       M.n_vertices, M.n_shapes, M.positions, M.normals, M.vertices, M.primitives, (BBox*)M.shapes);
}
void launch_mesh_update(const MeshUpdateArgs& M, hipStream_t st)
{
    launch_mesh_geometry(M, st);
    launch_mesh_builds(M, st);
}
void launch_refit_small(const MeshUpdateArgs& M, hipStream_t st)
{
    const uint32_t n_nodes = 3u * M.n_shapes - 2u * M.n_meshes;
    (void)hipMemsetAsync(M.n_large, 0, 4, st);
    hipLaunchKernelGGL(k_refit_small, dim3((n_nodes + 255u) / 256u), dim3(256), 0, st, M.table, M.n_meshes, n_nodes,
                       (const BBox*)M.shapes, M.blas, M.large, 2u * M.n_shapes, M.n_large);
}
void launch_refit_large(const MeshUpdateArgs& M, hipStream_t st)
{
    if (M.large_bound == 0) return;
    const uint32_t grid = M.large_bound < REFIT_LARGE_GRID ? M.large_bound : REFIT_LARGE_GRID;
    hipLaunchKernelGGL(k_refit_large, dim3(grid), dim3(256), 0, st, M.table, M.n_meshes, (const BBox*)M.shapes, M.blas,
                       (const uint32_t*)M.large, 2u * M.n_shapes, (const uint32_t*)M.n_large);
}
uint32_t mesh_refit_large_bound(uint32_t shapes)
{
    // the widest range below the root's, over shapes - 1 primitives, spans 3 (shapes - 1) - 1
    return shapes >= 2u && 3u * (shapes - 1u) - 1u > REFIT_SMALL ? 2u * shapes - 2u : 0u;
}
void launch_mesh_add(const MeshAddArgs& A, hipStream_t st)
{
    const MeshUpdateArgs& M = A.M;
    const uint32_t items = M.n_vertices + M.n_shapes;
    hipLaunchKernelGGL(k_assemble_meshes, dim3((items + 255u) / 256u), dim3(256), 0, st, M.table, A.sources, M.n_meshes,
                       M.n_vertices, M.n_shapes, M.positions, M.normals, A.uvs, A.indices, M.vertices, M.primitives,
                       (BBox*)M.shapes);
    launch_mesh_builds(M, st);
}
void launch_mesh_move(const MeshMoveArgs& V, hipStream_t st)
{
    const uint64_t chunks = 2u * (uint64_t)V.n_vertices + 3u * (uint64_t)V.n_prims + 2u * (uint64_t)V.n_nodes;
    hipLaunchKernelGGL(k_move_mesh_slices, dim3((uint32_t)((chunks + 255u) / 256u)), dim3(256), 0, st, V.table, V.n_meshes,
                       V.n_vertices, V.n_prims, V.n_nodes, (const uint4*)V.src[0], (const uint4*)V.src[1],
                       (const uint4*)V.src[2], (uint4*)V.dst[0], (uint4*)V.dst[1], (uint4*)V.dst[2], V.aux, V.stride);
}
void launch_skin_vertices(const SkinArgs& K, hipStream_t st)
{
    hipLaunchKernelGGL(k_skin_vertices, dim3((K.n_vertices + 255u) / 256u), dim3(256), 0, st, K.table, K.sources,
                       K.n_meshes, K.n_vertices, K.bind_positions, K.bind_normals, K.joint_indices, K.joint_weights,
                       K.palettes, K.positions, K.normals);
}
void launch_posed_bounds(const MeshUpdate* table, PosedSlices slices, uint32_t n_meshes, const float* positions,
                         const hk_instance* instances, uint32_t n_instances, float* local_aabbs, hipStream_t st)
{
    hipLaunchKernelGGL(k_skin_bounds, dim3(n_meshes), dim3(256), 0, st, table, slices, positions, instances, n_instances,
                       local_aabbs);
}
void launch_morph_vertices(const MorphArgs& K, hipStream_t st)
{
    hipLaunchKernelGGL(k_morph_vertices, dim3((K.n_vertices + 255u) / 256u), dim3(256), 0, st, K.table, K.sources,
                       K.active, K.n_meshes, K.n_vertices, K.base_positions, K.base_normals, K.position_deltas,
                       K.normal_deltas, K.joint_indices, K.joint_weights, K.palettes, K.positions, K.normals);
}
uint32_t mesh_lds_shapes() { return BVH_LDS_SHAPES; }

}  // namespace hk
