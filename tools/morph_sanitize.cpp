// hks_morph_vertices under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program over
// csrc/hk_scene.cpp, no device and no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       tools/morph_sanitize.cpp bevy-hikari_amd/csrc/hk_scene.cpp -o /tmp/morph_sanitize && /tmp/morph_sanitize
//
// Every buffer is allocated at its exact size, so a read or a store one element past any of them is reported.  For the
// vertex counts the morph cases sit on (1, 3, 63, 64, 65, 256, 257) and target counts 1, 2, 7 and 256 it morphs seeded
// bases (with and without normals and normal deltas) and checks every stored word against the rule's fold written out
// here; then all-zero weights (the output is the base byte for byte, -0.0 included), NaN and infinite deltas under zero
// and non-zero weights, a NaN weight, and every refusal of the header's list (HK_ERR_INVALID, nothing written).  Exit
// code 0 and "ok" when all of it held.
#include "../include/hikari_scene.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static uint32_t rng_state = 0x4D4F5250u;
static float rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f - 0.5f;
}
static int failures = 0;
#define CHECK(x)                                                \
    do {                                                        \
        if (!(x)) {                                             \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__); \
            ++failures;                                         \
        }                                                       \
    } while (0)

static bool same(const std::vector<float>& a, const std::vector<float>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (std::isnan(a[i]) && std::isnan(b[i])) continue;
        if (std::memcmp(&a[i], &b[i], 4) != 0) return false;
    }
    return true;
}

// the rule, written out: ascending targets, zero weights skipped, one rounded multiply and one rounded add
static std::vector<float> fold(const std::vector<float>& base, const std::vector<float>& d, const std::vector<float>& w,
                               uint32_t nv)
{
    std::vector<float> out(base);
    for (uint32_t v = 0; v < nv; ++v)
        for (int a = 0; a < 3; ++a) {
            volatile float acc = base[3 * v + a];
            for (size_t t = 0; t < w.size(); ++t) {
                if (!(w[t] != 0.0f)) continue;
                volatile float prod = w[t] * d[3 * (t * nv + v) + a];
                acc = acc + prod;
            }
            out[3 * v + a] = acc;
        }
    return out;
}

static std::vector<float> seeded(size_t n, float scale)
{
    std::vector<float> v(n);
    for (float& x : v) x = rnd() * scale;
    return v;
}

static void run(uint32_t nv, uint32_t nt, bool normals, bool normal_deltas, int special)
{
    std::vector<float> p = seeded(3 * (size_t)nv, 4.0f), n = seeded(3 * (size_t)nv, 2.0f);
    std::vector<float> dp = seeded(3 * (size_t)nv * nt, 0.6f), dn = seeded(3 * (size_t)nv * nt, 0.4f), w(nt);
    for (uint32_t t = 0; t < nt; ++t) w[t] = (t % 3 == 1) ? (t % 2 ? -0.0f : 0.0f) : rnd() * 3.0f;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    if (special == 1) {  // all-zero weights over a base with zeros of both signs and wild deltas
        for (uint32_t t = 0; t < nt; ++t) w[t] = t % 2 ? -0.0f : 0.0f;
        for (size_t i = 0; i < p.size(); i += 2) p[i] = i % 4 ? -0.0f : 0.0f;
        for (size_t i = 0; i < dp.size(); i += 3) dp[i] = i % 2 ? inf : nan;
    }
    if (special == 2) {  // NaN and infinite deltas: target 0 skipped (weight 0), the last one taking part
        w[0] = 0.0f;
        w[nt - 1] = 0.75f;
        for (uint32_t v = 0; v < nv; ++v) {
            dp[3 * v] = inf, dp[3 * v + 1] = nan, dn[3 * v + 2] = -inf;
            dp[3 * ((size_t)(nt - 1) * nv + v) + (v % 3)] = v % 2 ? inf : nan;
        }
    }
    if (special == 3) w[nt / 2] = nan;  // a NaN weight takes part
    std::vector<float> op(p.size(), 7.0f), on(n.size(), 7.0f);
    float box[6];
    CHECK(hks_morph_vertices(p.data(), normals ? n.data() : nullptr, dp.data(), normal_deltas ? dn.data() : nullptr, nv,
                             w.data(), nt, op.data(), normals ? on.data() : nullptr, box) == 0);
    CHECK(same(op, fold(p, dp, w, nv)));
    if (normals) CHECK(same(on, normal_deltas ? fold(n, dn, w, nv) : n));
    if (special == 1) CHECK(std::memcmp(op.data(), p.data(), p.size() * 4) == 0);
    if (special == 3) CHECK(std::isnan(op[0]));
    // the box holds every finite vertex
    for (uint32_t v = 0; v < nv; ++v)
        for (int a = 0; a < 3; ++a) {
            const float x = op[3 * v + a];
            if (std::isfinite(x) && std::isfinite(box[a]) && std::isfinite(box[3 + a]))
                CHECK(std::fabs(x - box[a]) <= box[3 + a] * 1.0001f + 1e-6f);
        }
}

static void refusals()
{
    const uint32_t nv = 5, nt = 3;
    std::vector<float> p = seeded(3 * nv, 1.0f), n = seeded(3 * nv, 1.0f), dp = seeded(3 * nv * nt, 1.0f), dn = dp, w(nt, 0.5f);
    std::vector<float> op(3 * nv, 7.0f), on(3 * nv, 7.0f);
    float box[6] = {7, 7, 7, 7, 7, 7};
    auto untouched = [&] {
        for (float x : op) CHECK(x == 7.0f);
        for (float x : on) CHECK(x == 7.0f);
        for (float x : box) CHECK(x == 7.0f);
    };
    const int bad = HK_ERR_INVALID;
    CHECK(hks_morph_vertices(nullptr, n.data(), dp.data(), dn.data(), nv, w.data(), nt, op.data(), on.data(), box) == bad);
    CHECK(hks_morph_vertices(p.data(), n.data(), nullptr, dn.data(), nv, w.data(), nt, op.data(), on.data(), box) == bad);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), dn.data(), nv, nullptr, nt, op.data(), on.data(), box) == bad);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), dn.data(), nv, w.data(), nt, nullptr, on.data(), box) == bad);
    CHECK(hks_morph_vertices(p.data(), nullptr, dp.data(), nullptr, nv, w.data(), nt, op.data(), on.data(), box) == bad);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), nullptr, nv, w.data(), nt, op.data(), nullptr, box) == bad);
    CHECK(hks_morph_vertices(p.data(), nullptr, dp.data(), dn.data(), nv, w.data(), nt, op.data(), nullptr, box) == bad);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), dn.data(), nv, w.data(), 0, op.data(), on.data(), box) == bad);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), dn.data(), nv, w.data(), HK_MORPH_MAX_TARGETS + 1, op.data(),
                             on.data(), box) == bad);
    untouched();
    // what is allowed: no normals at all, no normal deltas, no box, no vertices
    CHECK(hks_morph_vertices(p.data(), nullptr, dp.data(), nullptr, nv, w.data(), nt, op.data(), nullptr, nullptr) == 0);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), nullptr, nv, w.data(), nt, op.data(), on.data(), nullptr) == 0);
    CHECK(hks_morph_vertices(p.data(), n.data(), dp.data(), dn.data(), 0, w.data(), nt, op.data(), on.data(), box) == 0);
}

int main()
{
    const uint32_t sizes[] = {1, 3, 63, 64, 65, 256, 257}, targets[] = {1, 2, 7, 256};
    for (uint32_t nv : sizes)
        for (uint32_t nt : targets) {
            run(nv, nt, true, true, 0);
            run(nv, nt, true, false, 0);
            run(nv, nt, false, false, 0);
            for (int special = 1; special <= 3; ++special) run(nv, nt, true, true, special);
        }
    refusals();
    std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
