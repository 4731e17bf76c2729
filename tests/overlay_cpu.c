/* The CPU side of the present-pass parity checks: include/hk_overlay.h's per-pixel body looped over a target.
 * TEST INFRASTRUCTURE, compiled by tests/test_overlay_independent.py and tests/test_gpu_present.py with the oracle's
 * flags (-O3 -std=gnu11 -fPIC -ffp-contract=off -fno-fast-math).  Planes are RGBA16F, row-major. */
#include "hk_overlay.h"

static hk_pp_tex plane(const uint16_t* data, uint32_t w, uint32_t h)
{
    hk_pp_tex t;
    t.data = data, t.w = w, t.h = h, t.f16 = 1, t.comps = 4;
    return t;
}

/* The viewport (vx, vy, vw, vh) of the target at `data` (row pitch in bytes); texels outside it are not touched. */
void overlay_cpu(const uint16_t* input, uint32_t iw, uint32_t ih, const uint16_t* albedo, uint32_t aw, uint32_t ah,
                 uint8_t* data, uint32_t pitch, uint32_t format, uint32_t vx, uint32_t vy, uint32_t vw, uint32_t vh)
{
    const hk_pp_tex in = plane(input, iw, ih), al = plane(albedo, aw, ah);
    const hk_overlay_view V = {vx, vy, vw, vh, format};
    const uint32_t words = format == HK_OVERLAY_RGBA16F ? 2u : 1u;
    for (uint32_t y = vy; y < vy + vh; ++y)
        for (uint32_t x = vx; x < vx + vw; ++x) {
            uint32_t* at = (uint32_t*)(data + (size_t)y * pitch) + (size_t)x * words;
            hk_overlay_texel(&in, &al, &V, hk_overlay_srgb_t, (int32_t)x, (int32_t)y, at);
        }
}

/* the header's table and the body's code of n linear values */
const float* overlay_cpu_table(void) { return hk_overlay_srgb_t; }
void overlay_cpu_codes(const float* c, uint32_t n, uint8_t* out)
{
    for (uint32_t i = 0; i < n; ++i) out[i] = (uint8_t)hk_overlay_srgb_code(hk_overlay_srgb_t, hk_overlay_unorm(c[i]));
}
