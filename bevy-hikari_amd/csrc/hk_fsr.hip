// hk_fsr.hip — FSR1 kernels: EASU (two variants storing the same bits) and RCAS (ffx_fsr1.h; post_process.rs:1279-1308).
// The per-pixel bodies live in include/hk_fsr.h, shared verbatim with the CPU side of the parity tests.  Launch shape:
// 256-thread workgroups over 16x16 output pixels in hk_post.hip's XCD-stripe order, each wave an 8x8 tile, ceil(S / 16)
// workgroups per axis, which covers every pixel the reference's over-sized dispatch stores.
#include "hk_launch.h"

namespace hk {

// the workgroup's 16x16 block (post_pixel's tile order) and this thread's pixel in it
HKD void fsr_block(int32_t& X0, int32_t& Y0)
{
    const uint32_t gx = gridDim.x, n = gridDim.x * gridDim.y;
    const uint32_t L = blockIdx.x + blockIdx.y * gx;
    const uint32_t xcd = L & 7u, i = L >> 3, q = n >> 3, r = n & 7u;
    const uint32_t tile = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + i;
    X0 = (int32_t)((tile % gx) * 16u);
    Y0 = (int32_t)((tile / gx) * 16u);
}
// each wave an 8x8 tile of the block: wave k at ((k & 1) * 8, (k >> 1) * 8), lane l at (l & 7, l >> 3)
HKD int32_t fsr_dx() { return (int32_t)(((threadIdx.x >> 6) & 1u) * 8u + (threadIdx.x & 7u)); }
HKD int32_t fsr_dy() { return (int32_t)((threadIdx.x >> 7) * 8u + ((threadIdx.x >> 3) & 7u)); }
static dim3 fsr_grid(uint32_t w, uint32_t h) { return dim3((w + 15u) / 16u, (h + 15u) / 16u); }

HKD hk_fsr_src plane_src(const FsrArgs& A)
{
    hk_fsr_src s;
    s.tex = A.in, s.tile = nullptr, s.x0 = s.y0 = s.tw = 0;
    return s;
}

// Plain: one thread per output pixel, the shared body on global memory (48 texel reads through the fake gather).
__global__ __launch_bounds__(256) void k_fsr_easu(FsrArgs A)
{
    int32_t X0, Y0;
    fsr_block(X0, Y0);
    const int32_t x = X0 + fsr_dx(), y = Y0 + fsr_dy();
    if ((uint32_t)x >= A.out.w || (uint32_t)y >= A.out.h) return;
    const hk_fsr_src s = plane_src(A);
    hk_fsr_easu(&A.easu, &s, &A.out, x, y);
}

// Tiled: the workgroup stages the input texels its 16x16 outputs read (hk_fsr_easu_rect: the body's own f32 expressions
// for fp at the block's first and last pixel, -2 .. +3, clamped as hk_pp_clampi clamps), decoded once from f16 to f32
// (v_cvt_f32_f16, exact), and the body's texel fetches read LDS.  22 x 22 x 16 B = 7744 B.  A block whose rectangle
// does not fit (hk_fsr.h states when: never for ratios >= 1 below 16384 texels) runs the plain body on global memory.
__global__ __launch_bounds__(256) void k_fsr_easu_tiled(FsrArgs A)
{
    __shared__ float4 tile[HK_FSR_TILE_MAX * HK_FSR_TILE_MAX];
    int32_t X0, Y0;
    fsr_block(X0, Y0);
    const int32_t X1 = min(X0 + 15, (int32_t)A.out.w - 1), Y1 = min(Y0 + 15, (int32_t)A.out.h - 1);
    int32_t r[4];
    const bool staged = hk_fsr_easu_rect(&A.easu, A.in.w, A.in.h, X0, Y0, X1, Y1, r) != 0;  // block-uniform
    hk_fsr_src s = plane_src(A);
    if (staged) {
        const uint2* src = (const uint2*)A.in.data;
        const int32_t count = r[2] * r[3];  // <= 22 * 22, inside the image by the clamps
        for (int32_t t = (int32_t)threadIdx.x; t < count; t += 256) {
            const int32_t tx = t % r[2], ty = t / r[2];
            const f4 c = load_rgba16f(src, (r[1] + ty) * (int32_t)A.in.w + (r[0] + tx));
            tile[t] = make_float4(c.x, c.y, c.z, c.w);
        }
        __syncthreads();
        s.tile = (const float*)tile, s.x0 = r[0], s.y0 = r[1], s.tw = r[2];
    }
    const int32_t x = X0 + fsr_dx(), y = Y0 + fsr_dy();
    if (x > X1 || y > Y1) return;
    float c[4];
    hk_fsr_easu_rgb(&A.easu, &s, x, y, c);
    store_rgba16f((uint2*)A.out.data, y * (int32_t)A.out.w + x, mk4(c[0], c[1], c[2], 1.0f));
}

// RCAS: five taps (out of bounds 0); 16 B/px compulsory traffic, the neighbours come from L1 / L2.  The f16 conversions
// are the hardware's (hk_device.h), the filter hk_fsr_rcas_rgb.  One thread per pixel: the kernel of odd widths.
__global__ __launch_bounds__(256) void k_fsr_rcas(FsrArgs A)
{
    int32_t X0, Y0;
    fsr_block(X0, Y0);
    const int32_t x = X0 + fsr_dx(), y = Y0 + fsr_dy();
    const int32_t w = (int32_t)A.out.w, h = (int32_t)A.out.h;
    if (x >= w || y >= h) return;
    const uint2* src = (const uint2*)A.in.data;
    const f4 zero = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    const int32_t at = y * w + x;
    const f4 b = y > 0 ? load_rgba16f(src, at - w) : zero;
    const f4 d = x > 0 ? load_rgba16f(src, at - 1) : zero;
    const f4 e = load_rgba16f(src, at);
    const f4 f = x + 1 < w ? load_rgba16f(src, at + 1) : zero;
    const f4 g = y + 1 < h ? load_rgba16f(src, at + w) : zero;
    const float bb[3] = {b.x, b.y, b.z}, dd[3] = {d.x, d.y, d.z}, ee[3] = {e.x, e.y, e.z}, ff[3] = {f.x, f.y, f.z},
                hh[3] = {g.x, g.y, g.z};
    float c[3];
    hk_fsr_rcas_rgb(A.rcas, bb, dd, ee, ff, hh, c);
    store_rgba16f((uint2*)A.out.data, at, mk4(c[0], c[1], c[2], 1.0f));
}

// RCAS on 2-pixel row runs (even widths): a thread loads its two centre texels and the two above and below as
// 16-byte vectors and the run's left and right neighbours, and stores 16 bytes.  A workgroup covers 32 x 16 pixels.
__global__ __launch_bounds__(256) void k_fsr_rcas_run(FsrArgs A)
{
    int32_t X0, Y0;
    fsr_block(X0, Y0);
    const int32_t x = 2 * (X0 + fsr_dx()), y = Y0 + fsr_dy();
    const int32_t w = (int32_t)A.out.w, h = (int32_t)A.out.h;
    if (x >= w || y >= h) return;  // w is even: x + 1 < w
    const uint2* src = (const uint2*)A.in.data;
    const int32_t at = y * w + x;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    const uint4 up = y > 0 ? *reinterpret_cast<const uint4*>(src + at - w) : z4;
    const uint4 mid = *reinterpret_cast<const uint4*>(src + at);
    const uint4 dn = y + 1 < h ? *reinterpret_cast<const uint4*>(src + at + w) : z4;
    const uint2 lf = x > 0 ? src[at - 1] : make_uint2(0u, 0u);
    const uint2 rt = x + 2 < w ? src[at + 2] : make_uint2(0u, 0u);
    auto rgb = [](uint32_t lo, uint32_t hi, float* o) {
        o[0] = unpack_lo16float(lo), o[1] = unpack_hi16float(lo), o[2] = unpack_lo16float(hi);
    };
    float b0[3], b1[3], e0[3], e1[3], h0[3], h1[3], d0[3], f1[3], c0[3], c1[3];
    rgb(up.x, up.y, b0), rgb(up.z, up.w, b1);
    rgb(mid.x, mid.y, e0), rgb(mid.z, mid.w, e1);
    rgb(dn.x, dn.y, h0), rgb(dn.z, dn.w, h1);
    rgb(lf.x, lf.y, d0), rgb(rt.x, rt.y, f1);
    hk_fsr_rcas_rgb(A.rcas, b0, d0, e0, e1, h0, c0);
    hk_fsr_rcas_rgb(A.rcas, b1, e0, e1, f1, h1, c1);
    *reinterpret_cast<uint4*>((uint2*)A.out.data + at) =
        make_uint4(pack2x16float(c0[0], c0[1]), pack2x16float(c0[2], 1.0f), pack2x16float(c1[0], c1[1]), pack2x16float(c1[2], 1.0f));
}

void launch_fsr_easu(const FsrArgs& A, bool tiled, hipStream_t st)
{
    if (tiled)
        hipLaunchKernelGGL(k_fsr_easu_tiled, fsr_grid(A.out.w, A.out.h), dim3(256), 0, st, A);
    else
        hipLaunchKernelGGL(k_fsr_easu, fsr_grid(A.out.w, A.out.h), dim3(256), 0, st, A);
}
// the row-run kernel needs 16-byte aligned pixel pairs: even widths (4K: 0.050 ms against the per-pixel kernel's 0.060)
void launch_fsr_rcas(const FsrArgs& A, hipStream_t st)
{
    if ((A.out.w & 1u) == 0u)
        hipLaunchKernelGGL(k_fsr_rcas_run, fsr_grid(A.out.w / 2u, A.out.h), dim3(256), 0, st, A);
    else
        hipLaunchKernelGGL(k_fsr_rcas, fsr_grid(A.out.w, A.out.h), dim3(256), 0, st, A);
}

}  // namespace hk
