/*
 * hk_overlay.h — the present pass: the reference's last stage, the `Overlay` phase item's full-screen quad
 * (overlay.rs, overlay.wgsl), which draws the displayed texture into the camera's viewport of the view target.
 * Written once for both sides of the parity check, like hk_post.h / hk_fsr.h: the CPU side (tests/overlay_cpu.c)
 * loops hk_overlay_texel over a target, the gfx950 kernels (csrc/hk_overlay.hip) run the same steps per thread.  Every
 * operation is an exactly rounded f32 +, -, *, /, a comparison or an f16 conversion, evaluated left to right and never
 * fused (-ffp-contract=off).
 *
 * The steps for target pixel (x, y) inside the viewport (vx, vy, vw, vh) (overlay.rs:384-386 set_camera_viewport):
 *   fragment position   overlay.wgsl:17-22 passes the quad's vertex position (Quad 2 x 2, overlay.rs:50-53: clip
 *                       space -1 .. 1) on as `position`, interpolated by the rasteriser.  At the pixel centre it is
 *                           ndc.x = ((x - vx) + 0.5) / vw * 2 - 1,    ndc.y = 1 - ((y - vy) + 0.5) / vh * 2
 *                       (y up in clip space, down in the target).  The rasteriser's interpolation is implementation-
 *                       defined; this one f32 evaluation is the project's rule (unpinned).
 *   uv                  overlay.wgsl:37 clip_to_uv(vec4(position, 1)), as utils.wgsl:30-35 writes it: uv = clip.xy / 1,
 *                       uv = (uv + 1) * 0.5, uv.y = 1 - uv.y.  With a viewport of the input's size, uv * W - 0.5 lands
 *                       a rounding error off the texel centres, so the four-texel blend below is live (weights near 0
 *                       and 1, and a weight of 0 still meets a non-finite texel), as with EASU's gather.
 *   colour              overlay.wgsl:39-41: albedo and the input through the linear sampler (post_process.rs:703-708,
 *                       clamp-to-edge) at uv: hk_pp_linear's one fixed evaluation for both.
 *   NaN fallback        overlay.wgsl:42 select(color, albedo, any_is_nan_vec4(color)) with utils.wgsl:3-5's is_nan
 *                       !(v < 0 || 0 < v || v == 0) on all four components, alpha included; a NaN the blend itself
 *                       makes (0 * NaN, 0 * inf, inf - inf from a footprint neighbour) counts.  The whole texel is
 *                       replaced.  The albedo sample has no effect on a pixel without a NaN and is skipped there.
 *   HDR                 overlay.wgsl:28-32,44-46, only with the RGBA16F target (overlay.rs:111-116 ties the shader def
 *                       to the format): l_old = clamp(lum(rgb), 0.0005, 0.995), l_new = l_old / (1 - l_old),
 *                       rgb = rgb * (l_new / lum(rgb)) — Bevy 0.9.1 tonemapping_luminance (the Rec. 709 dot,
 *                       hk_luminance) and tonemapping_change_luminance, recalled from SURVEY App. B (unpinned).  The
 *                       divisor is the unclamped luminance: a black pixel is 0 * inf = NaN and is stored as such.
 *                       clamp is IEEE minNum / maxNum.  Alpha passes through.
 *   store               RGBA16F: f32 -> f16 round-to-nearest-even.  Rgba8UnormSrgb / Bgra8UnormSrgb (overlay.rs:112
 *                       bevy_default): per channel NaN -> 0, clamp to [0, 1]; alpha floor(a * 255 + 0.5); R, G, B the
 *                       sRGB code below; BGRA swaps R and B.  The blend state (overlay.rs:133 ALPHA_BLENDING over the
 *                       pass's clear) is not restated: the stored texel is the fragment's colour.
 * Pixels outside the viewport are not written.
 *
 * The sRGB code, without a transcendental: code(c) = #{k in 1..255 : c >= T[k]}, T[k] the smallest f32 whose exact
 * sRGB encode (12.92 c up to 0.0031308, 1.055 c^(1 / 2.4) - 0.055 above), times 255, is >= k - 0.5.  The hardware's
 * conversion is implementation-defined within 0.6 ulp of that; this rule rounds the exact encode to nearest and is
 * monotone.  T is the table below, produced and re-checked by tools/srgb_thresholds.py in exact rational arithmetic;
 * hk_overlay_srgb_code counts by a binary search of it (T is increasing), eight comparisons.
 */
#ifndef HK_OVERLAY_H
#define HK_OVERLAY_H

#include <stddef.h>

#include "hk_post.h"

#define HK_OVERLAY_RGBA8_SRGB 0u
#define HK_OVERLAY_BGRA8_SRGB 1u
#define HK_OVERLAY_RGBA16F 2u

/* T[0..255]; T[0] = 0 is never counted */
#define HK_OVERLAY_SRGB_T \
    0x0p+0f, 0x1.3e4568p-13f, 0x1.dd681cp-12f, 0x1.8dd6c2p-11f, 0x1.167cbcp-10f, 0x1.660e16p-10f, 0x1.b59f7p-10f, 0x1.029866p-9f, \
    0x1.2a6112p-9f, 0x1.5229bep-9f, 0x1.79f26cp-9f, 0x1.a1e5a2p-9f, 0x1.cbf736p-9f, 0x1.f86806p-9f, 0x1.13a0cp-8f, 0x1.2c4666p-8f, \
    0x1.46297ap-8f, 0x1.614e62p-8f, 0x1.7db96ep-8f, 0x1.9b6edap-8f, 0x1.ba72cep-8f, 0x1.dac95ep-8f, 0x1.fc768cp-8f, 0x1.0fbf22p-7f, \
    0x1.21f236p-7f, 0x1.34d664p-7f, 0x1.486d9p-7f, 0x1.5cb98ep-7f, 0x1.71bc34p-7f, 0x1.877748p-7f, 0x1.9dec9p-7f, 0x1.b51dc8p-7f, \
    0x1.cd0ca8p-7f, 0x1.e5bae2p-7f, 0x1.ff2a1ep-7f, 0x1.0cae04p-6f, 0x1.1a291ep-6f, 0x1.28072cp-6f, 0x1.3648f8p-6f, 0x1.44ef4cp-6f, \
    0x1.53fafp-6f, 0x1.636ca6p-6f, 0x1.73453p-6f, 0x1.838552p-6f, 0x1.942dc6p-6f, 0x1.a53f48p-6f, 0x1.b6ba96p-6f, 0x1.c8a064p-6f, \
    0x1.daf16ap-6f, 0x1.edae5cp-6f, 0x1.006bf8p-5f, 0x1.0a3768p-5f, 0x1.1439d8p-5f, 0x1.1e73ap-5f, 0x1.28e514p-5f, 0x1.338e8ap-5f, \
    0x1.3e7058p-5f, 0x1.498acep-5f, 0x1.54de44p-5f, 0x1.606b08p-5f, 0x1.6c316ep-5f, 0x1.7831c8p-5f, 0x1.846c64p-5f, 0x1.90e194p-5f, \
    0x1.9d91a4p-5f, 0x1.aa7ce6p-5f, 0x1.b7a3a6p-5f, 0x1.c5063p-5f, 0x1.d2a4d4p-5f, 0x1.e07fdcp-5f, 0x1.ee9794p-5f, 0x1.fcec48p-5f, \
    0x1.05bf2p-4f, 0x1.0d26e4p-4f, 0x1.14ad96p-4f, 0x1.1c5356p-4f, 0x1.24184ep-4f, 0x1.2bfc9ep-4f, 0x1.34006ap-4f, 0x1.3c23d8p-4f, \
    0x1.446708p-4f, 0x1.4cca2p-4f, 0x1.554d4p-4f, 0x1.5df08ep-4f, 0x1.66b42ap-4f, 0x1.6f9836p-4f, 0x1.789cd6p-4f, 0x1.81c228p-4f, \
    0x1.8b0852p-4f, 0x1.946f72p-4f, 0x1.9df7acp-4f, 0x1.a7a11ep-4f, 0x1.b16beap-4f, 0x1.bb5832p-4f, 0x1.c56614p-4f, 0x1.cf95b2p-4f, \
    0x1.d9e72ap-4f, 0x1.e45aap-4f, 0x1.eef02ep-4f, 0x1.f9a7f8p-4f, 0x1.02410ep-3f, 0x1.07bf5cp-3f, 0x1.0d4ef6p-3f, 0x1.12efecp-3f, \
    0x1.18a24cp-3f, 0x1.1e6628p-3f, 0x1.243b8ap-3f, 0x1.2a2286p-3f, 0x1.301b2ap-3f, 0x1.362584p-3f, 0x1.3c41a2p-3f, 0x1.426f96p-3f, \
    0x1.48af6cp-3f, 0x1.4f0132p-3f, 0x1.5564fap-3f, 0x1.5bdadp-3f, 0x1.6262c2p-3f, 0x1.68fcep-3f, 0x1.6fa938p-3f, 0x1.7667d8p-3f, \
    0x1.7d38cep-3f, 0x1.841c2ap-3f, 0x1.8b11f6p-3f, 0x1.921a44p-3f, 0x1.99352p-3f, 0x1.a06298p-3f, 0x1.a7a2bap-3f, 0x1.aef594p-3f, \
    0x1.b65b34p-3f, 0x1.bdd3a8p-3f, 0x1.c55efcp-3f, 0x1.ccfd3ep-3f, 0x1.d4ae7cp-3f, 0x1.dc72c4p-3f, 0x1.e44a22p-3f, 0x1.ec34a4p-3f, \
    0x1.f43258p-3f, 0x1.fc434ap-3f, 0x1.0233c4p-2f, 0x1.064f8ep-2f, 0x1.0a750cp-2f, 0x1.0ea444p-2f, 0x1.12dd3ap-2f, 0x1.171ff8p-2f, \
    0x1.1b6c82p-2f, 0x1.1fc2ep-2f, 0x1.242316p-2f, 0x1.288d2cp-2f, 0x1.2d012ap-2f, 0x1.317f12p-2f, 0x1.3606eep-2f, 0x1.3a98c4p-2f, \
    0x1.3f3498p-2f, 0x1.43da7p-2f, 0x1.488a56p-2f, 0x1.4d444cp-2f, 0x1.52085cp-2f, 0x1.56d688p-2f, 0x1.5baedap-2f, 0x1.609154p-2f, \
    0x1.657ep-2f, 0x1.6a74e2p-2f, 0x1.6f76p-2f, 0x1.748162p-2f, 0x1.79970ap-2f, 0x1.7eb702p-2f, 0x1.83e14ep-2f, 0x1.8915f2p-2f, \
    0x1.8e54f8p-2f, 0x1.939e64p-2f, 0x1.98f23cp-2f, 0x1.9e5084p-2f, 0x1.a3b944p-2f, 0x1.a92c82p-2f, 0x1.aeaa42p-2f, 0x1.b4328cp-2f, \
    0x1.b9c564p-2f, 0x1.bf62dp-2f, 0x1.c50ad4p-2f, 0x1.cabd7ap-2f, 0x1.d07ac6p-2f, 0x1.d642bap-2f, 0x1.dc1562p-2f, 0x1.e1f2bep-2f, \
    0x1.e7dad6p-2f, 0x1.edcdbp-2f, 0x1.f3cb5p-2f, 0x1.f9d3bcp-2f, 0x1.ffe6fcp-2f, 0x1.03028ap-1f, 0x1.061704p-1f, 0x1.0930eep-1f, \
    0x1.0c504ep-1f, 0x1.0f7524p-1f, 0x1.129f72p-1f, 0x1.15cf3ep-1f, 0x1.190488p-1f, 0x1.1c3f54p-1f, 0x1.1f7fa4p-1f, 0x1.22c57cp-1f, \
    0x1.2610dcp-1f, 0x1.2961c8p-1f, 0x1.2cb844p-1f, 0x1.301452p-1f, 0x1.3375f4p-1f, 0x1.36dd2cp-1f, 0x1.3a49fep-1f, 0x1.3dbc6cp-1f, \
    0x1.413478p-1f, 0x1.44b226p-1f, 0x1.483578p-1f, 0x1.4bbe7p-1f, 0x1.4f4d12p-1f, 0x1.52e15ep-1f, 0x1.567b5ap-1f, 0x1.5a1b06p-1f, \
    0x1.5dc064p-1f, 0x1.616b7ap-1f, 0x1.651c48p-1f, 0x1.68d2dp-1f, 0x1.6c8f16p-1f, 0x1.70511ep-1f, 0x1.7418e6p-1f, 0x1.77e674p-1f, \
    0x1.7bb9cap-1f, 0x1.7f92eap-1f, 0x1.8371d6p-1f, 0x1.87569p-1f, 0x1.8b411ep-1f, 0x1.8f317ep-1f, 0x1.9327b6p-1f, 0x1.9723c6p-1f, \
    0x1.9b25bp-1f, 0x1.9f2d7ap-1f, 0x1.a33b24p-1f, 0x1.a74ebp-1f, 0x1.ab6822p-1f, 0x1.af877cp-1f, 0x1.b3acbep-1f, 0x1.b7d7eep-1f, \
    0x1.bc090cp-1f, 0x1.c0401cp-1f, 0x1.c47d2p-1f, 0x1.c8c018p-1f, 0x1.cd090ap-1f, 0x1.d157f6p-1f, 0x1.d5acep-1f, 0x1.da07cap-1f, \
    0x1.de68b4p-1f, 0x1.e2cfa4p-1f, 0x1.e73c9ap-1f, 0x1.ebaf98p-1f, 0x1.f028a2p-1f, 0x1.f4a7bap-1f, 0x1.f92ce2p-1f, 0x1.fdb81cp-1f

/* the host's copy of the table; device code reads its own copy (LDS, filled from __constant__) through `T` */
static const float hk_overlay_srgb_t[256] = {HK_OVERLAY_SRGB_T};

/* the viewport of a present call and the target's format */
typedef struct hk_overlay_view {
    uint32_t vx, vy, vw, vh;
    uint32_t format; /* HK_OVERLAY_* */
} hk_overlay_view;

/* fragment position -> uv (overlay.wgsl:17-22,37; utils.wgsl:30-35) */
HK_HD void hk_overlay_uv(const hk_overlay_view* V, int32_t x, int32_t y, float* uv)
{
    const float nx = ((float)(x - (int32_t)V->vx) + 0.5f) / (float)V->vw * 2.0f - 1.0f;
    const float ny = 1.0f - ((float)(y - (int32_t)V->vy) + 0.5f) / (float)V->vh * 2.0f;
    uv[0] = (nx + 1.0f) * 0.5f;
    uv[1] = (ny + 1.0f) * 0.5f;
    uv[1] = 1.0f - uv[1];
}

/* utils.wgsl:3-5,11-13 */
HK_HD int hk_overlay_is_nan(float v) { return !(v < 0.0f || 0.0f < v || v == 0.0f); }
HK_HD int hk_overlay_any_nan(const float* c)
{
    return hk_overlay_is_nan(c[0]) || hk_overlay_is_nan(c[1]) || hk_overlay_is_nan(c[2]) || hk_overlay_is_nan(c[3]);
}

/* overlay.wgsl:28-32 inverse_reintard_luminance on c[0..2] */
HK_HD void hk_overlay_inverse_reinhard(float* c)
{
    const float l_in = hk_luminance(c[0], c[1], c[2]);
    const float l_old = hk_clampf(l_in, 0.0005f, 0.995f);
    const float l_new = l_old / (1.0f - l_old);
    const float scale = l_new / l_in;
    for (int k = 0; k < 3; ++k) c[k] = c[k] * scale;
}

/* NaN -> 0, then clamp to [0, 1] */
HK_HD float hk_overlay_unorm(float c)
{
    if (c != c) return 0.0f;
    return c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
}

/* #{k in 1..255 : c >= T[k]} for c in [0, 1] */
HK_HD uint32_t hk_overlay_srgb_code(const float* T, float c)
{
    uint32_t n = 0u;
    for (uint32_t step = 128u; step != 0u; step >>= 1)
        if (c >= T[n + step]) n += step;
    return n;
}

/* the 8-bit texel of colour c: R (BGRA: B) in the low byte */
HK_HD uint32_t hk_overlay_pack8(const float* T, const float* c, uint32_t format)
{
    const uint32_t r = hk_overlay_srgb_code(T, hk_overlay_unorm(c[0]));
    const uint32_t g = hk_overlay_srgb_code(T, hk_overlay_unorm(c[1]));
    const uint32_t b = hk_overlay_srgb_code(T, hk_overlay_unorm(c[2]));
    const uint32_t a = (uint32_t)floorf(hk_overlay_unorm(c[3]) * 255.0f + 0.5f);
    return format == HK_OVERLAY_BGRA8_SRGB ? (b | (g << 8) | (r << 16) | (a << 24)) : (r | (g << 8) | (b << 16) | (a << 24));
}

/* The stored texel of target pixel (x, y), which lies inside the viewport: one word for the 8-bit formats, two
 * (r | g << 16, b | a << 16 as f16) for RGBA16F.  `albedo` is sampled only when the input's sample has a NaN. */
HK_HD void hk_overlay_texel(const hk_pp_tex* input, const hk_pp_tex* albedo, const hk_overlay_view* V, const float* T,
                            int32_t x, int32_t y, uint32_t* words)
{
    float uv[2], c[4];
    hk_overlay_uv(V, x, y, uv);
    hk_pp_linear(input, uv[0], uv[1], c);
    if (hk_overlay_any_nan(c)) hk_pp_linear(albedo, uv[0], uv[1], c);
    if (V->format == HK_OVERLAY_RGBA16F) {
        hk_overlay_inverse_reinhard(c);
        words[0] = hk_pack2x16float(c[0], c[1]);
        words[1] = hk_pack2x16float(c[2], c[3]);
    } else {
        words[0] = hk_overlay_pack8(T, c, V->format);
    }
}

#endif /* HK_OVERLAY_H */
