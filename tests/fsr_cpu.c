/* The CPU side of the FSR1 parity checks: include/hk_fsr.h's per-pixel bodies looped over an image.
 * TEST INFRASTRUCTURE, compiled by tests/test_fsr_independent.py and tests/test_gpu_fsr.py with the oracle's flags
 * (-O3 -std=gnu11 -fPIC -ffp-contract=off -fno-fast-math). Images are RGBA16F, row-major. */
#include <stdlib.h>

#include "hk_fsr.h"

static hk_fsr_src fsr_src(const uint16_t* in, uint32_t iw, uint32_t ih)
{
    hk_fsr_src s;
    s.tex.data = in, s.tex.w = iw, s.tex.h = ih, s.tex.f16 = 1, s.tex.comps = 4;
    s.tile = NULL, s.x0 = s.y0 = s.tw = 0;
    return s;
}

/* con: 14 floats, con0[4] con1[4] con2[4] con3[2] */
void fsr_cpu_easu_constants(float iw, float ih, float ow, float oh, float* con)
{
    hk_fsr_easu_con C;
    hk_fsr_easu_constants(&C, iw, ih, ow, oh);
    for (int k = 0; k < 4; ++k) con[k] = C.con0[k], con[4 + k] = C.con1[k], con[8 + k] = C.con2[k];
    con[12] = C.con3[0], con[13] = C.con3[1];
}

float fsr_cpu_rcas_constant(float sharpness) { return hk_fsr_rcas_constant(sharpness); }

/* EASU, one body call per output pixel on the plane itself */
void fsr_cpu_easu(const uint16_t* in, uint32_t iw, uint32_t ih, uint16_t* out, uint32_t ow, uint32_t oh)
{
    hk_fsr_easu_con C;
    hk_fsr_easu_constants(&C, (float)iw, (float)ih, (float)ow, (float)oh);
    const hk_fsr_src s = fsr_src(in, iw, ih);
    const hk_pp_out o = {out, ow, oh};
    for (int32_t y = 0; y < (int32_t)oh; ++y)
        for (int32_t x = 0; x < (int32_t)ow; ++x) hk_fsr_easu(&C, &s, &o, x, y);
}

/* EASU as the tiled kernel runs it: per 16 x 16 output block the input rectangle hk_fsr_easu_rect gives, decoded
 * to f32 in a buffer of exactly that size, and the body reading the buffer.  Returns the blocks that could not be
 * staged (they take the plane path), or -1 when out of memory. */
int fsr_cpu_easu_tiled(const uint16_t* in, uint32_t iw, uint32_t ih, uint16_t* out, uint32_t ow, uint32_t oh)
{
    hk_fsr_easu_con C;
    hk_fsr_easu_constants(&C, (float)iw, (float)ih, (float)ow, (float)oh);
    const hk_pp_out o = {out, ow, oh};
    int unstaged = 0;
    for (int32_t Y0 = 0; Y0 < (int32_t)oh; Y0 += 16)
        for (int32_t X0 = 0; X0 < (int32_t)ow; X0 += 16) {
            const int32_t X1 = X0 + 15 < (int32_t)ow ? X0 + 15 : (int32_t)ow - 1;
            const int32_t Y1 = Y0 + 15 < (int32_t)oh ? Y0 + 15 : (int32_t)oh - 1;
            hk_fsr_src s = fsr_src(in, iw, ih);
            int32_t r[4];
            float* tile = NULL;
            if (hk_fsr_easu_rect(&C, iw, ih, X0, Y0, X1, Y1, r)) {
                tile = (float*)malloc((size_t)r[2] * r[3] * 4 * sizeof(float));
                if (!tile) return -1;
                for (int32_t ty = 0; ty < r[3]; ++ty)
                    for (int32_t tx = 0; tx < r[2]; ++tx) hk_pp_texel(&s.tex, r[0] + tx, r[1] + ty, tile + 4 * (ty * r[2] + tx));
                s.tile = tile, s.x0 = r[0], s.y0 = r[1], s.tw = r[2];
            } else {
                unstaged++;
            }
            for (int32_t y = Y0; y <= Y1; ++y)
                for (int32_t x = X0; x <= X1; ++x) hk_fsr_easu(&C, &s, &o, x, y);
            free(tile);
        }
    return unstaged;
}

void fsr_cpu_rcas(const uint16_t* in, uint32_t w, uint32_t h, float con, uint16_t* out)
{
    const hk_pp_out i = {(uint16_t*)in, w, h}, o = {out, w, h};
    for (int32_t y = 0; y < (int32_t)h; ++y)
        for (int32_t x = 0; x < (int32_t)w; ++x) hk_fsr_rcas(con, &i, &o, x, y);
}
