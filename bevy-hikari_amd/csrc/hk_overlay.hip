// hk_overlay.hip — the present pass (overlay.rs, overlay.wgsl): the displayed plane drawn through the linear sampler
// into the viewport of an sRGB8 or RGBA16F target.  The per-pixel steps live in include/hk_overlay.h, shared with the
// CPU side of the parity tests; here the texels come through load_rgba16f (v_cvt_f32_f16, exact) and the RGBA16F store
// through v_cvt_pk_f16_f32, as in the other image filters.  Launch shape: 256-thread workgroups of 64 columns x 4 rows
// (a wave is one row segment, so its stores are consecutive), numbered along x first in a one-dimensional grid.
// Compulsory traffic per target pixel: 8 B of input at the input's own size (less when the target is larger) and
// 4 or 8 B stored; the albedo (8 B) is read only by pixels whose sample holds a NaN.
#include "hk_launch.h"

namespace hk {

// tools/srgb_thresholds.py's table; the 8-bit kernels copy it into LDS, where the search's data-dependent reads go
__constant__ float c_srgb_t[256] = {HK_OVERLAY_SRGB_T};

template <uint32_t FMT>
struct OvFmt {
    static constexpr uint32_t bpp = FMT == HK_OVERLAY_RGBA16F ? 8u : 4u;
    static constexpr uint32_t run = 16u / bpp;  // pixels of one 16-byte store
};

// hk_pp_linear on an RGBA16F plane: the shared footprint, hardware f16 -> f32, the shared blend expression
HKD void ov_linear(const hk_pp_tex& t, float u, float v, float* o)
{
    int32_t i[2], j[2];
    float a, b;
    hk_pp_footprint(&t, u, v, i, j, &a, &b);
    const uint2* src = (const uint2*)t.data;
    const int32_t r0 = j[0] * (int32_t)t.w, r1 = j[1] * (int32_t)t.w;  // planes hold fewer than 2^31 texels (hk_present)
    const f4 t00 = load_rgba16f(src, r0 + i[0]), t10 = load_rgba16f(src, r0 + i[1]);
    const f4 t01 = load_rgba16f(src, r1 + i[0]), t11 = load_rgba16f(src, r1 + i[1]);
    const float ia = 1.0f - a, ib = 1.0f - b;
    o[0] = (t00.x * ia + t10.x * a) * ib + (t01.x * ia + t11.x * a) * b;
    o[1] = (t00.y * ia + t10.y * a) * ib + (t01.y * ia + t11.y * a) * b;
    o[2] = (t00.z * ia + t10.z * a) * ib + (t01.z * ia + t11.z * a) * b;
    o[3] = (t00.w * ia + t10.w * a) * ib + (t01.w * ia + t11.w * a) * b;
}

// hk_overlay_texel for viewport pixel (px, py) (target pixel (vx + px, vy + py)): words[0], and words[1] for RGBA16F
template <uint32_t FMT>
HKD void ov_texel(const OverlayArgs& A, const float* T, uint32_t px, uint32_t py, uint32_t* words)
{
    float uv[2], c[4];
    hk_overlay_uv(&A.view, (int32_t)(A.view.vx + px), (int32_t)(A.view.vy + py), uv);
    ov_linear(A.in, uv[0], uv[1], c);
    if (hk_overlay_any_nan(c)) ov_linear(A.albedo, uv[0], uv[1], c);
    if constexpr (FMT == HK_OVERLAY_RGBA16F) {
        hk_overlay_inverse_reinhard(c);
        words[0] = pack2x16float(c[0], c[1]);
        words[1] = pack2x16float(c[2], c[3]);
    } else {
        words[0] = hk_overlay_pack8(T, c, FMT);
    }
}

// every thread of the workgroup, before any leaves
template <uint32_t FMT>
HKD void ov_stage_table(float* T)
{
    if constexpr (FMT != HK_OVERLAY_RGBA16F) {
        T[threadIdx.x] = c_srgb_t[threadIdx.x];
        __syncthreads();
    }
}

// the address of viewport pixel (px, py) in the target
template <uint32_t FMT>
HKD uint8_t* ov_at(const OverlayArgs& A, uint32_t px, uint32_t py)
{
    return A.data + (size_t)(A.view.vy + py) * A.pitch + (size_t)(A.view.vx + px) * OvFmt<FMT>::bpp;
}

// One thread per pixel of the viewport columns [A.col0, A.col0 + A.cols): any origin, pitch and base address, and the
// columns the run kernel leaves at the end of a row.
template <uint32_t FMT>
__global__ __launch_bounds__(256) void k_overlay(OverlayArgs A)
{
    __shared__ float T[256];
    ov_stage_table<FMT>(T);
    const uint32_t bx = (A.cols + 63u) / 64u;
    const uint32_t px = (blockIdx.x % bx) * 64u + (threadIdx.x & 63u), py = (blockIdx.x / bx) * 4u + (threadIdx.x >> 6);
    if (px >= A.cols || py >= A.view.vh) return;
    uint32_t w[2];
    ov_texel<FMT>(A, T, A.col0 + px, py, w);
    uint8_t* at = ov_at<FMT>(A, A.col0 + px, py);
    if constexpr (FMT == HK_OVERLAY_RGBA16F)
        *reinterpret_cast<uint2*>(at) = make_uint2(w[0], w[1]);
    else
        *reinterpret_cast<uint32_t*>(at) = w[0];
}

// One thread per run of consecutive pixels of a row that fills one 16-byte store (4 pixels, RGBA16F 2): the viewport's
// first A.cols / run runs of every row.  The launcher sends a target here only when every run is 16-byte aligned.
template <uint32_t FMT>
__global__ __launch_bounds__(256) void k_overlay_run(OverlayArgs A)
{
    __shared__ float T[256];
    ov_stage_table<FMT>(T);
    constexpr uint32_t R = OvFmt<FMT>::run;
    const uint32_t runs = A.cols / R, bx = (runs + 63u) / 64u;
    const uint32_t r = (blockIdx.x % bx) * 64u + (threadIdx.x & 63u), py = (blockIdx.x / bx) * 4u + (threadIdx.x >> 6);
    if (r >= runs || py >= A.view.vh) return;
    uint32_t w[4];
    if constexpr (FMT == HK_OVERLAY_RGBA16F) {
        ov_texel<FMT>(A, T, r * R, py, w);
        ov_texel<FMT>(A, T, r * R + 1u, py, w + 2);
    } else {
        for (uint32_t k = 0; k < 4u; ++k) ov_texel<FMT>(A, T, r * R + k, py, w + k);
    }
    *reinterpret_cast<uint4*>(ov_at<FMT>(A, r * R, py)) = make_uint4(w[0], w[1], w[2], w[3]);
}

template <uint32_t FMT>
static void launch_overlay_fmt(OverlayArgs A, bool run, hipStream_t st)
{
    constexpr uint32_t R = OvFmt<FMT>::run;
    const uint32_t by = (A.view.vh + 3u) / 4u, vw = A.view.vw;
    // every run of every row on a 16-byte boundary: the first one is, and the pitch keeps it so
    const uintptr_t first = (uintptr_t)A.data + (size_t)A.view.vy * A.pitch + (size_t)A.view.vx * OvFmt<FMT>::bpp;
    run = run && vw >= R && first % 16u == 0u && A.pitch % 16u == 0u;
    A.col0 = 0u, A.cols = vw;
    if (run) {
        const uint32_t runs = vw / R;
        hipLaunchKernelGGL(k_overlay_run<FMT>, dim3(((runs + 63u) / 64u) * by), dim3(256), 0, st, A);
        A.col0 = runs * R, A.cols = vw - runs * R;  // the row's tail
    }
    if (A.cols > 0u) hipLaunchKernelGGL(k_overlay<FMT>, dim3(((A.cols + 63u) / 64u) * by), dim3(256), 0, st, A);
}

void launch_overlay(const OverlayArgs& A, bool run, hipStream_t st)
{
    switch (A.view.format) {
    case HK_OVERLAY_RGBA8_SRGB: launch_overlay_fmt<HK_OVERLAY_RGBA8_SRGB>(A, run, st); break;
    case HK_OVERLAY_BGRA8_SRGB: launch_overlay_fmt<HK_OVERLAY_BGRA8_SRGB>(A, run, st); break;
    default: launch_overlay_fmt<HK_OVERLAY_RGBA16F>(A, run, st); break;
    }
}

}  // namespace hk
