// asan_plan3d.cpp - stand-alone host program for the sanitizer build (`make asan3d`): the host side of a d = 3 plan - a tree replayed
// on (lon, lat), the plan created with mra_topology.d = 3, the xyz gathered into leaf order (mra_plan_set_locs_rows), the knot
// coordinates and the knot chain's records filled, observations, noise vector and kernel set - in MRA_HOST_DRYRUN mode, where every
// "device" buffer is host memory under AddressSanitizer / UBSan and nothing is launched.  Three block widths, so that the level
// loops of CWT = 1, 2 and 4 are walked.  Exit status 0 and "ASAN_PLAN3D_OK" when every call returned MRA_OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mra_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != 0) { std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mra_last_error(nullptr)); return 1; } } while (0)

static void mt_seed(uint32_t s, std::vector<uint32_t>& key) {          // MT19937 init_genrand: the state numpy.random.seed(s) leaves
    key.resize(624);
    key[0] = s;
    for (int i = 1; i < 624; ++i) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + (uint32_t)i;
}

static int one_tree(int n, int r, int M) {
    const int64_t N = (int64_t)n * n;
    const double pi = 3.14159265358979323846;
    std::vector<double> ll(2 * N), xyz(3 * N), y(N), noise(N);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const int64_t k = (int64_t)j * n + i;
            const double lon = -180.0 + (i + 0.5) * 360.0 / n, lat = -80.0 + 160.0 * j / (n - 1);
            ll[2 * k] = lon; ll[2 * k + 1] = lat;
            const double a = lon * pi / 180.0, b = lat * pi / 180.0;
            xyz[3 * k] = std::cos(b) * std::cos(a); xyz[3 * k + 1] = std::cos(b) * std::sin(a); xyz[3 * k + 2] = std::sin(b);
            y[k] = (k * 2654435761u) % 5 < 2 ? std::sin(3.0 * xyz[3 * k]) : std::nan("");
            noise[k] = 1e-2 * (1.0 + 0.5 * xyz[3 * k + 2]);
        }
    std::vector<uint32_t> key;
    mt_seed(7u, key);
    int32_t pos = 624;
    int64_t cap = N;                                                     // every leaf is padded to a multiple of 16 rows: N + 15 * 4^M
    { int64_t leaves = 1; for (int m = 0; m < M; ++m) leaves *= 4; cap += 15 * leaves; }
    std::vector<int64_t> perm(cap), src(cap), knot_rows(N);
    std::vector<uint8_t> in_leaf(cap);
    mra_tree* tree = nullptr;
    CHECK(mra_tree_replay_2d_into(ll.data(), N, r, M, key.data(), &pos, cap, perm.data(), src.data(), in_leaf.data(), knot_rows.data(), &tree));
    int64_t sz[5];
    CHECK(mra_tree_sizes(tree, sz));
    const int64_t P = sz[0], nn = sz[1], nl = sz[2], nch = sz[3], nk = sz[4];
    std::vector<int64_t> level_ptr(nl + 1), row0(nn), row1(nn), knot_ptr(nn + 1);
    std::vector<int32_t> node_level(nn), parent(nn), child_ptr(nn + 1), child_list(nch), cw(nl), pre(nn);
    std::vector<uint8_t> leaf(nn);
    CHECK(mra_tree_export(tree, nullptr, nullptr, nullptr, level_ptr.data(), node_level.data(), row0.data(), row1.data(), leaf.data(), parent.data(),
                          child_ptr.data(), child_list.data(), knot_ptr.data(), nullptr, cw.data(), pre.data()));
    CHECK(mra_tree_free(tree));
    if (knot_ptr[nn] != nk) { std::fprintf(stderr, "knot count %lld != %lld\n", (long long)knot_ptr[nn], (long long)nk); return 1; }
    mra_topology t;
    t.P = P; t.d = 3; t.n_levels = (int32_t)nl; t.n_nodes = (int32_t)nn;
    t.level_ptr = level_ptr.data(); t.node_row0 = row0.data(); t.node_row1 = row1.data(); t.node_leaf = leaf.data();
    t.node_parent = parent.data(); t.child_ptr = child_ptr.data(); t.child_list = child_list.data();
    t.knot_ptr = knot_ptr.data(); t.knot_rows = knot_rows.data(); t.cw = cw.data();
    mra_plan* pl = nullptr;
    CHECK(mra_plan_create(&pl, &t, 0));
    CHECK(mra_plan_set_locs_rows(pl, xyz.data(), src.data()));
    CHECK(mra_plan_set_obs_rows(pl, y.data(), src.data(), perm.data(), 1e-2));
    CHECK(mra_plan_set_noise_rows(pl, noise.data(), src.data()));
    const double par[4] = {0.5, 1.0, 1.0, 0.0};
    CHECK(mra_plan_set_kernel(pl, 1, par, 4));
    const double circ[4] = {0.5, 1.0, 1.0, 1.0};
    if (mra_plan_set_kernel(pl, 1, circ, 4) != MRA_ERR_INVALID) { std::fprintf(stderr, "circular distances on a d = 3 plan were not refused\n"); return 1; }
    CHECK(mra_plan_set_locs_rows(pl, xyz.data(), src.data()));                  // a second upload: the staging buffer is reused
    if (mra_run(pl, MRA_RUN_LIKELIHOOD | MRA_RUN_PREDICT) != MRA_ERR_STATE) { std::fprintf(stderr, "a dry-run plan must refuse to run\n"); return 1; }
    int64_t info[8];
    mra_plan_info(pl, info, 8);
    if (info[0] != P) { std::fprintf(stderr, "plan P %lld != %lld\n", (long long)info[0], (long long)P); return 1; }
    t.d = 4;
    mra_plan* bad = nullptr;
    if (mra_plan_create(&bad, &t, 0) != MRA_ERR_INVALID || bad) { std::fprintf(stderr, "d = 4 was not refused\n"); return 1; }
    CHECK(mra_plan_destroy(pl));
    std::printf("%dx%d r0=%d M=%d: P=%lld nodes=%lld cw0=%d\n", n, n, r, M, (long long)P, (long long)nn, cw[0]);
    return 0;
}

int main() {
    const char* e = std::getenv("MRA_HOST_DRYRUN");
    if (!e || e[0] != '1') { std::fprintf(stderr, "run with MRA_HOST_DRYRUN=1 (make asan3d does)\n"); return 2; }
    if (one_tree(64, 16, 2) || one_tree(128, 32, 3) || one_tree(128, 64, 3) || one_tree(200, 16, 4)) return 1;
    CHECK(mra_release_cached_memory());
    std::printf("ASAN_PLAN3D_OK\n");
    return 0;
}
