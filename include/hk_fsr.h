/*
 * hk_fsr.h — FSR1: EASU (edge-adaptive spatial upsampling) and RCAS (robust contrast-adaptive sharpening), the two
 * compute passes the reference runs after TAA under `Upscale::Fsr1 { ratio, sharpness }` (post_process.rs:1279-1308,
 * constants post_process.rs:522-533).  Written once for both sides of the parity check, like hk_post.h: the CPU side
 * (tests/fsr_cpu.c) loops these bodies over an image, the gfx950 kernels (csrc/hk_fsr.hip) call them per thread.
 *
 * Restated is the path the reference's shaders take: the 32-bit filters (FsrEasuF / FsrRcasF) behind the
 * SAMPLE_SLOW_FALLBACK gather, hdr = 0, without the RCAS denoise and alpha pass-through variants (so RCAS's luma
 * and noise lines are dead and left out).  Every operation is an exactly rounded f32 +, -, *, /, an integer
 * operation or an f16 conversion, evaluated left to right and never fused (-ffp-contract=off).
 *
 * What GLSL leaves implementation-defined, and how both sides fix it here:
 *   filtering precision   EASU's taps come through a gather emulated by four `texture()` calls of the LINEAR
 *                         clamp-to-edge sampler at p +- half a texel.  They are not texel fetches: the coordinates
 *                         are computed in f32 and land a rounding error away from texel centres, so the weights are
 *                         near 0 or 1 but not exactly, and a weight of 0 still meets a non-finite texel (0 * inf).
 *                         Every one of them is hk_pp_linear's one fixed f32 evaluation.  The gather's samples that
 *                         no tap reads (two of (0)'s and two of (3)'s) are not taken: they have no effect.
 *   texelFetch out of bounds   RCAS's five taps return 0 outside the image (hk_pp_load), the project's rule for
 *                         textureLoad.
 *   NaN in min / max / clamp   IEEE minNum / maxNum (fminf / fmaxf): the operand that is a number wins.
 *                         RCAS depends on it: a black texel makes a limiter 0 * rcp(0) = NaN, and so does the image
 *                         border, whose out-of-bounds taps are 0; the pixel's result then rests on max(NaN, x) = x.
 *   exp2                  RCAS's constant is hk_exp2(-sharpness), the project's pinned transcendental (hk_math.h).
 *   rcp                   ARcpF1 is a correctly rounded 1 / x; the approximations (APrxLoRcpF1, APrxMedRcpF1,
 *                         APrxLoRsqF1) are integer bit tricks and are exact restatements.
 * Literal expressions of the shaders ((1.0/4.0-0.04)-0.5, 2.0/5.0) are folded in double and rounded to f32 once.
 * Parity with the reference's SPIR-V blobs themselves is unpinned, like the rest of DESIGN §3: nothing here can
 * run them.
 *
 * Input footprint of EASU (what the tiled kernel stages).  With fp = floor(ip * con0.xy + con0.zw) the twelve taps
 * are texels fp + (-1..2), and each is the near-unit-weight texel of a linear footprint sampled half a texel from a
 * texel corner n in fp .. fp + 3 (the boundary of texels n - 1 and n): ideally x = u W - 0.5 is the integer n - 1
 * or n.  u < 2 is rebuilt from fp by at most 8 rounded f32 operations (2^-24 each) and x by two more, so
 * |x - ideal| < 2^-21 W + 2^-9 <= 2^-6 for W <= 16384: floor(x) is the ideal integer or the one below, and the
 * footprint's two texels per axis lie in fp - 2 .. fp + 3 (rows too: the gather samples beyond are the ones not
 * taken).  fp is monotone in ip (f32 * and + are), so a 16 x 16
 * block of outputs reads texels fp(first) - 2 .. fp(last) + 3 per axis, clamped to the image: at most
 * floor(15 W / Wout) + 1 + 6 <= 22 for a ratio >= 1.  csrc/hk_fsr.hip derives the rectangle from these same
 * expressions (hk_fsr_easu_fp) and sends a block whose rectangle is larger, or an image above 16384 texels on an
 * axis, through the plain kernel.
 */
#ifndef HK_FSR_H
#define HK_FSR_H

#include "hk_post.h"

#define HK_FSR_TILE_MAX 22      /* staged texels per axis of one 16 x 16 output block */
#define HK_FSR_TILED_MAX_DIM 16384u

typedef struct hk_fsr_easu_con {
    float con0[4], con1[4], con2[4], con3[2];
} hk_fsr_easu_con;

/* EASU's input: the plane, or (tile != NULL) an f32 RGBA copy of its texels [x0, x0 + tw) x [y0, y0 + th) — the
 * clamped coordinates the footprints produce all lie inside (see above) */
typedef struct hk_fsr_src {
    hk_pp_tex tex;
    const float* tile;
    int32_t x0, y0, tw;
} hk_fsr_src;

/* ffx_a.h:1843-1845 */
HK_HD float hk_fsr_prx_lo_rcp(float a) { return hk_u2f(0x7ef07ebbu - hk_f2u(a)); }
HK_HD float hk_fsr_prx_med_rcp(float a)
{
    const float b = hk_u2f(0x7ef19fffu - hk_f2u(a));
    return b * ((-b) * a + 2.0f);
}
HK_HD float hk_fsr_prx_lo_rsq(float a) { return hk_u2f(0x5f347d74u - (hk_f2u(a) >> 1)); }
HK_HD float hk_fsr_rcp(float a) { return 1.0f / a; }
HK_HD float hk_fsr_min3(float x, float y, float z) { return hk_minf(x, hk_minf(y, z)); }
HK_HD float hk_fsr_max3(float x, float y, float z) { return hk_maxf(x, hk_maxf(y, z)); }

/* FsrEasuCon (ffx_fsr1.h:156-202) with input viewport = input size = (iw, ih); host, once per call */
static inline void hk_fsr_easu_constants(hk_fsr_easu_con* c, float iw, float ih, float ow, float oh)
{
    c->con0[0] = iw * hk_fsr_rcp(ow);
    c->con0[1] = ih * hk_fsr_rcp(oh);
    c->con0[2] = (0.5f * iw) * hk_fsr_rcp(ow) - 0.5f;
    c->con0[3] = (0.5f * ih) * hk_fsr_rcp(oh) - 0.5f;
    c->con1[0] = hk_fsr_rcp(iw);
    c->con1[1] = hk_fsr_rcp(ih);
    c->con1[2] = 1.0f * hk_fsr_rcp(iw);
    c->con1[3] = -1.0f * hk_fsr_rcp(ih);
    c->con2[0] = -1.0f * hk_fsr_rcp(iw);
    c->con2[1] = 2.0f * hk_fsr_rcp(ih);
    c->con2[2] = 1.0f * hk_fsr_rcp(iw);
    c->con2[3] = 2.0f * hk_fsr_rcp(ih);
    c->con3[0] = 0.0f * hk_fsr_rcp(iw);
    c->con3[1] = 4.0f * hk_fsr_rcp(ih);
}
/* FsrRcasCon (ffx_fsr1.h:662-672): stops of sharpness reduction -> linear */
static inline float hk_fsr_rcas_constant(float sharpness) { return hk_exp2(-sharpness); }

/* position of tap 'f' for output pixel (x, y): fp = floor(pp), pp the fraction left (ffx_fsr1.h:324-326) */
HK_HD void hk_fsr_easu_fp(const hk_fsr_easu_con* C, int32_t x, int32_t y, float* fp, float* pp)
{
    const float px = (float)(uint32_t)x * C->con0[0] + C->con0[2];
    const float py = (float)(uint32_t)y * C->con0[1] + C->con0[3];
    fp[0] = floorf(px), fp[1] = floorf(py);
    pp[0] = px - fp[0], pp[1] = py - fp[1];
}

/* The input texels the outputs [X0, X1] x [Y0, Y1] (inclusive) read, as the clamped rectangle
 * [r[0], r[0] + r[2]) x [r[1], r[1] + r[3]); 0 when it cannot be staged (see the top of the file) */
HK_HD int hk_fsr_easu_rect(const hk_fsr_easu_con* C, uint32_t w, uint32_t h, int32_t X0, int32_t Y0, int32_t X1,
                           int32_t Y1, int32_t* r)
{
    float lo[2], hi[2], pp[2];
    hk_fsr_easu_fp(C, X0, Y0, lo, pp);
    hk_fsr_easu_fp(C, X1, Y1, hi, pp);
    const int32_t x0 = hk_pp_clampi(hk_pp_f2i(lo[0]) - 2, (int32_t)w), x1 = hk_pp_clampi(hk_pp_f2i(hi[0]) + 3, (int32_t)w);
    const int32_t y0 = hk_pp_clampi(hk_pp_f2i(lo[1]) - 2, (int32_t)h), y1 = hk_pp_clampi(hk_pp_f2i(hi[1]) + 3, (int32_t)h);
    r[0] = x0, r[1] = y0, r[2] = x1 - x0 + 1, r[3] = y1 - y0 + 1;
    return w <= HK_FSR_TILED_MAX_DIM && h <= HK_FSR_TILED_MAX_DIM && r[2] >= 1 && r[3] >= 1 &&
           r[2] <= HK_FSR_TILE_MAX && r[3] <= HK_FSR_TILE_MAX;
}

/* `texture()` through the linear sampler: hk_pp_linear, its texels from the plane or from the staged tile */
HK_HD void hk_fsr_linear(const hk_fsr_src* s, float u, float v, float* o)
{
    if (!s->tile) {
        hk_pp_linear(&s->tex, u, v, o);
        return;
    }
    int32_t i[2], j[2];
    float a, b;
    hk_pp_footprint(&s->tex, u, v, i, j, &a, &b);
    const int32_t r0 = (j[0] - s->y0) * s->tw, r1 = (j[1] - s->y0) * s->tw, c0 = i[0] - s->x0, c1 = i[1] - s->x0;
    const float *t00 = s->tile + 4 * (r0 + c0), *t10 = s->tile + 4 * (r0 + c1);
    const float *t01 = s->tile + 4 * (r1 + c0), *t11 = s->tile + 4 * (r1 + c1);
    const float ia = 1.0f - a, ib = 1.0f - b;
    for (int k = 0; k < 4; ++k) o[k] = (t00[k] * ia + t10[k] * a) * ib + (t01[k] * ia + t11[k] * a) * b;
}

/* texture_gather.glsl: half a texel either way; the returned components are
 * x = (p.x - ps.x, p.y + ps.y), y = (p + ps), z = (p.x + ps.x, p.y - ps.y), w = (p - ps).
 * `upper` != 0: only z and w (rows p.y - ps.y), `lower` != 0: only x and y. */
HK_HD void hk_fsr_gather(const hk_fsr_src* s, const float* p, int lower, int upper, float g[4][4])
{
    const float psx = (1.0f / (float)s->tex.w) / 2.0f, psy = (1.0f / (float)s->tex.h) / 2.0f;
    if (!upper) {
        hk_fsr_linear(s, p[0] + -psx, p[1] + psy, g[0]);
        hk_fsr_linear(s, p[0] + psx, p[1] + psy, g[1]);
    }
    if (!lower) {
        hk_fsr_linear(s, p[0] + psx, p[1] + -psy, g[2]);
        hk_fsr_linear(s, p[0] - psx, p[1] - psy, g[3]);
    }
}

/* FsrEasuSetF (ffx_fsr1.h:275-313); w = the tap's bilinear weight */
HK_HD void hk_fsr_easu_set(float* dir, float* len, float w, float lA, float lB, float lC, float lD, float lE)
{
    const float dc = lD - lC, cb = lC - lB;
    float lenX = hk_maxf(hk_absf(dc), hk_absf(cb));
    lenX = hk_fsr_prx_lo_rcp(lenX);
    const float dirX = lD - lB;
    dir[0] = dir[0] + dirX * w;
    lenX = hk_saturate(hk_absf(dirX) * lenX);
    lenX = lenX * lenX;
    *len = *len + lenX * w;
    const float ec = lE - lC, ca = lC - lA;
    float lenY = hk_maxf(hk_absf(ec), hk_absf(ca));
    lenY = hk_fsr_prx_lo_rcp(lenY);
    const float dirY = lE - lA;
    dir[1] = dir[1] + dirY * w;
    lenY = hk_saturate(hk_absf(dirY) * lenY);
    lenY = lenY * lenY;
    *len = *len + lenY * w;
}

/* FsrEasuTapF (ffx_fsr1.h:239-272) */
HK_HD void hk_fsr_easu_tap(float* aC, float* aW, float offx, float offy, const float* dir, const float* len2,
                           float lob, float clp, const float* c)
{
    float vx = (offx * dir[0]) + (offy * dir[1]);
    float vy = (offx * (-dir[1])) + (offy * dir[0]);
    vx = vx * len2[0];
    vy = vy * len2[1];
    float d2 = vx * vx + vy * vy;
    d2 = hk_minf(d2, clp);
    float wB = (float)(2.0 / 5.0) * d2 + -1.0f;
    float wA = lob * d2 + -1.0f;
    wB = wB * wB;
    wA = wA * wA;
    wB = (float)(25.0 / 16.0) * wB + (float)(-(25.0 / 16.0 - 1.0));
    const float w = wB * wA;
    for (int k = 0; k < 3; ++k) aC[k] = aC[k] + c[k] * w;
    *aW = *aW + w;
}

/* FsrEasuF (ffx_fsr1.h:315-437): the colour of output pixel (x, y) */
HK_HD void hk_fsr_easu_rgb(const hk_fsr_easu_con* C, const hk_fsr_src* s, int32_t x, int32_t y, float* pix)
{
    float fp[2], pp[2];
    hk_fsr_easu_fp(C, x, y, fp, pp);
    const float p0[2] = {fp[0] * C->con1[0] + C->con1[2], fp[1] * C->con1[1] + C->con1[3]};
    const float p1[2] = {p0[0] + C->con2[0], p0[1] + C->con2[1]};
    const float p2[2] = {p0[0] + C->con2[2], p0[1] + C->con2[3]};
    const float p3[2] = {p0[0] + C->con3[0], p0[1] + C->con3[1]};
    float bczz[4][4], ijfe[4][4], klhg[4][4], zzon[4][4];
    hk_fsr_gather(s, p0, 1, 0, bczz);
    hk_fsr_gather(s, p1, 0, 0, ijfe);
    hk_fsr_gather(s, p2, 0, 0, klhg);
    hk_fsr_gather(s, p3, 0, 1, zzon);
    const float *b = bczz[0], *c = bczz[1], *i = ijfe[0], *j = ijfe[1], *f = ijfe[2], *e = ijfe[3];
    const float *k = klhg[0], *l = klhg[1], *h = klhg[2], *g = klhg[3], *o = zzon[2], *n = zzon[3];
#define HK_FSR_LUMA(t) ((t)[2] * 0.5f + ((t)[0] * 0.5f + (t)[1]))
    const float bL = HK_FSR_LUMA(b), cL = HK_FSR_LUMA(c), iL = HK_FSR_LUMA(i), jL = HK_FSR_LUMA(j);
    const float fL = HK_FSR_LUMA(f), eL = HK_FSR_LUMA(e), kL = HK_FSR_LUMA(k), lL = HK_FSR_LUMA(l);
    const float hL = HK_FSR_LUMA(h), gL = HK_FSR_LUMA(g), oL = HK_FSR_LUMA(o), nL = HK_FSR_LUMA(n);
#undef HK_FSR_LUMA
    float dir[2] = {0.0f, 0.0f}, len = 0.0f;
    hk_fsr_easu_set(dir, &len, (1.0f - pp[0]) * (1.0f - pp[1]), bL, eL, fL, gL, jL);
    hk_fsr_easu_set(dir, &len, pp[0] * (1.0f - pp[1]), cL, fL, gL, hL, kL);
    hk_fsr_easu_set(dir, &len, (1.0f - pp[0]) * pp[1], fL, iL, jL, kL, nL);
    hk_fsr_easu_set(dir, &len, pp[0] * pp[1], gL, jL, kL, lL, oL);
    float dirR = dir[0] * dir[0] + dir[1] * dir[1];
    const int zro = dirR < (float)(1.0 / 32768.0);
    dirR = hk_fsr_prx_lo_rsq(dirR);
    dirR = zro ? 1.0f : dirR;
    dir[0] = zro ? 1.0f : dir[0];
    dir[0] = dir[0] * dirR;
    dir[1] = dir[1] * dirR;
    len = len * 0.5f;
    len = len * len;
    const float stretch = (dir[0] * dir[0] + dir[1] * dir[1]) * hk_fsr_prx_lo_rcp(hk_maxf(hk_absf(dir[0]), hk_absf(dir[1])));
    const float len2[2] = {1.0f + (stretch - 1.0f) * len, 1.0f + -0.5f * len};
    const float lob = 0.5f + (float)((1.0 / 4.0 - 0.04) - 0.5) * len;
    const float clp = hk_fsr_prx_lo_rcp(lob);
    float aC[3] = {0.0f, 0.0f, 0.0f}, aW = 0.0f;
    hk_fsr_easu_tap(aC, &aW, 0.0f - pp[0], -1.0f - pp[1], dir, len2, lob, clp, b);
    hk_fsr_easu_tap(aC, &aW, 1.0f - pp[0], -1.0f - pp[1], dir, len2, lob, clp, c);
    hk_fsr_easu_tap(aC, &aW, -1.0f - pp[0], 1.0f - pp[1], dir, len2, lob, clp, i);
    hk_fsr_easu_tap(aC, &aW, 0.0f - pp[0], 1.0f - pp[1], dir, len2, lob, clp, j);
    hk_fsr_easu_tap(aC, &aW, 0.0f - pp[0], 0.0f - pp[1], dir, len2, lob, clp, f);
    hk_fsr_easu_tap(aC, &aW, -1.0f - pp[0], 0.0f - pp[1], dir, len2, lob, clp, e);
    hk_fsr_easu_tap(aC, &aW, 1.0f - pp[0], 1.0f - pp[1], dir, len2, lob, clp, k);
    hk_fsr_easu_tap(aC, &aW, 2.0f - pp[0], 1.0f - pp[1], dir, len2, lob, clp, l);
    hk_fsr_easu_tap(aC, &aW, 2.0f - pp[0], 0.0f - pp[1], dir, len2, lob, clp, h);
    hk_fsr_easu_tap(aC, &aW, 1.0f - pp[0], 0.0f - pp[1], dir, len2, lob, clp, g);
    hk_fsr_easu_tap(aC, &aW, 1.0f - pp[0], 2.0f - pp[1], dir, len2, lob, clp, o);
    hk_fsr_easu_tap(aC, &aW, 0.0f - pp[0], 2.0f - pp[1], dir, len2, lob, clp, n);
    const float rW = hk_fsr_rcp(aW);
    for (int q = 0; q < 3; ++q) {
        const float mn4 = hk_minf(hk_fsr_min3(f[q], g[q], j[q]), k[q]);
        const float mx4 = hk_maxf(hk_fsr_max3(f[q], g[q], j[q]), k[q]);
        pix[q] = hk_minf(mx4, hk_maxf(mn4, aC[q] * rW));
    }
}

/* the pass for one output pixel: imageStore(OutputTexture, pos, (c, 1)) */
HK_HD void hk_fsr_easu(const hk_fsr_easu_con* C, const hk_fsr_src* s, const hk_pp_out* out, int32_t x, int32_t y)
{
    float c[4];
    hk_fsr_easu_rgb(C, s, x, y, c);
    c[3] = 1.0f;
    hk_pp_store(out, x, y, c);
}

/* FsrRcasF (ffx_fsr1.h:684-769) on the five taps' rgb:  b above, d left, e centre, f right, h below */
HK_HD void hk_fsr_rcas_rgb(float con, const float* b, const float* d, const float* e, const float* f, const float* h,
                           float* pix)
{
    float lobe3[3];
    for (int q = 0; q < 3; ++q) {
        const float mn4 = hk_minf(hk_fsr_min3(b[q], d[q], f[q]), h[q]);
        const float mx4 = hk_maxf(hk_fsr_max3(b[q], d[q], f[q]), h[q]);
        const float hitMin = hk_minf(mn4, e[q]) * hk_fsr_rcp(4.0f * mx4);
        const float hitMax = (1.0f - hk_maxf(mx4, e[q])) * hk_fsr_rcp(4.0f * mn4 + -4.0f);
        lobe3[q] = hk_maxf(-hitMin, hitMax);
    }
    const float lobe = hk_maxf(-(float)(0.25 - (1.0 / 16.0)), hk_minf(hk_fsr_max3(lobe3[0], lobe3[1], lobe3[2]), 0.0f)) * con;
    const float rcpL = hk_fsr_prx_med_rcp(4.0f * lobe + 1.0f);
    for (int q = 0; q < 3; ++q) pix[q] = ((((lobe * b[q] + lobe * d[q]) + lobe * h[q]) + lobe * f[q]) + e[q]) * rcpL;
}

HK_HD void hk_fsr_rcas(float con, const hk_pp_out* in, const hk_pp_out* out, int32_t x, int32_t y)
{
    float b[4], d[4], e[4], f[4], h[4], c[4];
    hk_pp_load(in, x, y - 1, b);
    hk_pp_load(in, x - 1, y, d);
    hk_pp_load(in, x, y, e);
    hk_pp_load(in, x + 1, y, f);
    hk_pp_load(in, x, y + 1, h);
    hk_fsr_rcas_rgb(con, b, d, e, f, h, c);
    c[3] = 1.0f;
    hk_pp_store(out, x, y, c);
}

#endif /* HK_FSR_H */
