// hks_refit_nodes under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program over
// csrc/hk_scene.cpp, no device and no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       tools/refit_sanitize.cpp bevy-hikari_amd/csrc/hk_scene.cpp -o /tmp/refit_sanitize && /tmp/refit_sanitize
//
// For triangle soups of the sizes the refit cases sit on (1, 2, either side of REFIT_SMALL's 11 / 12 primitives per
// child, 129, 1281, 2600, and a 17-level chain) it builds the BLAS with hks_build, deforms the primitives (seeded; one
// pass with NaN corners, one collapsed to a point, one scaled by 1e30), refits the slice, and checks that indices and
// leaves stayed and every entry box holds its range's corners.  Then every malformed slice of the header's list: the
// call must return HK_ERR_INVALID and leave the nodes untouched.  Exit code 0 and "ok" when all of it held.
#include "../include/hikari_scene.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static uint32_t rng_state = 0x52454654u;
static float rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f;
}
static int failures = 0;
#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            std::printf("FAILED %s (line %d)\n", #x, __LINE__);           \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct Slice {
    std::vector<hk_primitive> prims;
    std::vector<hk_node> nodes;
};

// n triangles: side by side along x, or (chain) at distances 4^i so that the SAH peels one per level
static Slice build(uint32_t n, bool chain)
{
    std::vector<float> pos, nrm, uv;
    for (uint32_t i = 0; i < n; ++i) {
        const float d = chain ? std::pow(4.0f, (float)i - 8.0f) : (float)i, h = chain ? 0.45f * d : 0.5f;
        const float c[3][3] = {{d - h, -h, 0.0f}, {d + h, -h, 0.0f}, {d, h, 0.0f}};
        for (int k = 0; k < 3; ++k) {
            pos.insert(pos.end(), c[k], c[k] + 3);
            const float up[3] = {0.0f, 0.0f, 1.0f}, t[2] = {0.5f * (float)k, (float)(k == 2)};
            nrm.insert(nrm.end(), up, up + 3);
            uv.insert(uv.end(), t, t + 2);
        }
    }
    hks_scene* s = hks_create();
    hk_material mat;
    std::memset(&mat, 0, sizeof(mat));
    const float model[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(hks_add_mesh(s, pos.data(), nrm.data(), uv.data(), 3 * n, nullptr, 0, HKS_TRIANGLE_LIST) == 0);
    CHECK(hks_add_material(s, &mat) == 0);
    CHECK(hks_add_instance(s, 0, 0, model) == 0);
    CHECK(hks_build(s, 6) == 0);
    hk_scene_desc d;
    CHECK(hks_get_desc(s, &d) == 0);
    Slice out;
    out.prims.assign((const hk_primitive*)d.primitives.data, (const hk_primitive*)d.primitives.data + d.primitives.count);
    out.nodes.assign((const hk_node*)d.asset_nodes.data, (const hk_node*)d.asset_nodes.data + d.asset_nodes.count);
    hks_destroy(s);
    CHECK(out.prims.size() == n && out.nodes.size() == 3 * (size_t)n - 2);
    return out;
}

static void refit_and_check(const Slice& s, int kind)
{
    std::vector<hk_primitive> p = s.prims;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t t = 0; t < p.size(); ++t)
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) {
                float& x = p[t].vertices[c].position[k];
                x += (rnd() - 0.5f) * (0.5f + std::fabs(x) * 0.3f);
                if (kind == 1 && rnd() < 0.05f) x = nan;
                if (kind == 2) x = (float)k - 0.75f;
                if (kind == 3) x *= 1e30f;
            }
    std::vector<hk_node> n = s.nodes;
    CHECK(hks_refit_nodes(p.data(), (uint32_t)p.size(), n.data(), (uint32_t)n.size()) == 0);
    for (size_t i = 0; i < n.size(); ++i) {
        CHECK(n[i].entry_index == s.nodes[i].entry_index && n[i].exit_index == s.nodes[i].exit_index);
        if (n[i].entry_index >= HK_BVH_LEAF_FLAG) {
            CHECK(std::memcmp(&n[i], &s.nodes[i], sizeof(hk_node)) == 0);
            continue;
        }
        for (uint32_t j = (uint32_t)i + 1; j < n[i].exit_index; ++j) {
            if (n[j].entry_index < HK_BVH_LEAF_FLAG) continue;
            const hk_primitive& t = p[n[j].entry_index - HK_BVH_LEAF_FLAG];
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < 3; ++k) {
                    const float x = t.vertices[c].position[k];
                    CHECK(x != x || (n[i].min[k] <= x && x <= n[i].max[k]));
                }
        }
    }
}

static void refuse(const Slice& s, std::vector<hk_node> bad, uint32_t prims, uint32_t nodes, const char* what)
{
    const std::vector<hk_node> before = bad;
    const int rc = hks_refit_nodes(s.prims.data(), prims, bad.data(), nodes);
    if (rc != HK_ERR_INVALID || std::memcmp(bad.data(), before.data(), before.size() * sizeof(hk_node)) != 0) {
        std::printf("FAILED refusal: %s (rc %d)\n", what, rc);
        ++failures;
    }
}

static void malformed(const Slice& s)
{
    const uint32_t k = (uint32_t)s.prims.size(), n = (uint32_t)s.nodes.size();
    uint32_t leaf = 0, inner = 0, deep = 0;  // a leaf, an entry node past the root's, an entry node over entry nodes
    for (uint32_t i = 0; i < n; ++i) {
        if (s.nodes[i].entry_index >= HK_BVH_LEAF_FLAG) leaf = i;
        else if (i) inner = i;
        if (i + 1 < n && s.nodes[i].entry_index < HK_BVH_LEAF_FLAG && s.nodes[i + 1].entry_index < HK_BVH_LEAF_FLAG) deep = i;
    }
    CHECK(hks_refit_nodes(nullptr, k, const_cast<hk_node*>(s.nodes.data()), n) == HK_ERR_INVALID);
    CHECK(hks_refit_nodes(s.prims.data(), k, nullptr, n) == HK_ERR_INVALID);
    refuse(s, s.nodes, k, n - 1, "one node short");
    refuse(s, s.nodes, k - 1, n, "one primitive short");
    refuse(s, s.nodes, 0, 0, "nothing");
    auto with = [&](uint32_t i, bool entry, uint32_t value) {
        std::vector<hk_node> b = s.nodes;
        (entry ? b[i].entry_index : b[i].exit_index) = value;
        return b;
    };
    refuse(s, with(leaf, false, leaf + 2), k, n, "leaf exit");
    refuse(s, with(leaf, true, HK_BVH_LEAF_FLAG | k), k, n, "leaf payload");
    refuse(s, with(leaf, true, 0xFFFFFFFFu), k, n, "leaf payload at the top of the range");
    refuse(s, with(leaf, true, s.nodes[leaf].entry_index ^ 1u), k, n, "primitive twice");
    refuse(s, with(inner, true, inner + 2), k, n, "entry node's entry");
    refuse(s, with(inner, false, inner + 1), k, n, "exit not past i + 1");
    refuse(s, with(inner, false, 0), k, n, "exit before the node");
    refuse(s, with(inner, false, n + 1), k, n, "exit past the slice");
    refuse(s, with(inner, false, 0xFFFFFFFFu), k, n, "exit at the top of the range");
    refuse(s, with(0, false, n), k, n, "root's children do not tile");
    refuse(s, with(deep, false, s.nodes[deep].exit_index - 1), k, n, "range one short");
    refuse(s, with(deep + 1, false, s.nodes[deep + 1].exit_index + 1), k, n, "first child runs into the second");
    refuse(s, with(s.nodes[deep + 1].exit_index, true, s.nodes[leaf].entry_index), k, n, "leaf in an entry node's place");
}

int main()
{
    const uint32_t sizes[] = {1, 2, 3, 22, 23, 129, 1281, 2600};
    for (uint32_t n : sizes) {
        const Slice s = build(n, false);
        for (int kind = 0; kind < 4; ++kind) refit_and_check(s, kind);
        if (n >= 22) malformed(s);
    }
    const Slice chain = build(18, true);
    for (int kind = 0; kind < 4; ++kind) refit_and_check(chain, kind);
    malformed(chain);
    std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
