// nuts_sanitize.cpp -- the host code of the device-resident NUTS tree (csrc/bb_nuts_host.h, csrc/bb_nuts.h in the host emulation) under a
// sanitizer, as a stand-alone program: a fitness model of 130 barcodes x 2 time points (the shape of the tests' fitness_T2), three walkers,
// the scripted tree of tests/_nuts_cases.py -- doublings of 1, 2 and 4 leaves in the directions +1, -1, +1 with the driver's ops -- with
// every kind of take, an idle walker, and the refused calls.  CPU only; it never runs on a GPU.
//   g++ -std=c++17 -O1 -g -DBB_EMU -fsanitize=address,undefined -fno-sanitize-recover=undefined -I barbay.jl_amd/csrc -I include \
//       -x c++ tools/probe/nuts_sanitize.cpp -o nuts_sanitize && ./nuts_sanitize
#include "bb_engine.hip"

#include <cstdio>

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s failed: %s\n", __LINE__, #x, bb_last_error()); return 1; } } while (0)

static void leaf_op(int i, int j, int* store, int* n_check, int* check) {
    int idx_max = 0, k = 0;
    for (int b = i >> 1; b; b >>= 1) idx_max += b & 1;
    while ((i >> k) & 1) ++k;
    *store = (i & 1) ? -1 : idx_max;
    *n_check = 0;
    if (i & 1) for (int q = 0; q < k; ++q) check[(*n_check)++] = idx_max - q;
    if (i == (1 << j) - 1) check[(*n_check)++] = BB_NUTS_EDGE_OPP;
}

int main() {
    const int B = 130, T = 2, NN = 3, W = 3, DEPTH = 3, CS = BB_NUTS_MAX_DEPTH + 1;
    std::vector<int64_t> counts((size_t)B * T), totals(T, 0);
    unsigned long long s = 12345;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            counts[(size_t)b * T + t] = 20 + (int64_t)((s >> 33) % 400);
            totals[t] += counts[(size_t)b * T + t];
        }
    const int32_t n_time = T;
    bb_model_desc m{};
    m.kind = BB_MODEL_FITNESS; m.n_rep = 1; m.n_neutral = NN; m.n_bc = B - NN;
    m.n_time = &n_time; m.counts = counts.data(); m.totals = totals.data();
    bb_advi_opts o;
    bb_default_opts(&o);
    o.seed = 11;
    bb_handle* h = nullptr;
    CHECK(bb_create(&m, &o, &h) == BB_OK);
    const size_t D = (size_t)bb_num_latents(h);
    std::vector<double> z0(W * D), lp(W), minv(D), zz(W * D), gg(W * D);
    for (size_t i = 0; i < W * D; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; z0[i] = ((double)(s >> 40) / (double)(1 << 24) - 0.5) * 0.6; }
    for (size_t i = 0; i < D; ++i) minv[i] = 0.25 + (double)(i % 16) * 0.2;

    const double eps[3] = {1e-3, 2e-3, 5e-4};
    const int32_t live[3] = {1, 1, 1}, some[3] = {1, 0, 1};
    int32_t flags[3] = {0, 0, 0};
    bb_nuts_opts no{DEPTH, 0};
    CHECK(bb_nuts_begin(h, &no) == BB_ERR_INVALID);                        // no session
    bb_hmc_opts ho{W, 0, 11, minv.data()};
    CHECK(bb_hmc_begin(h, &ho, z0.data(), lp.data()) == BB_OK);
    CHECK(bb_nuts_start(h, 5, eps, live, nullptr) == BB_ERR_INVALID);      // no bb_nuts_begin
    bb_nuts_opts big{BB_NUTS_MAX_DEPTH, 0};
    CHECK(bb_nuts_begin(h, &big) == BB_OK && bb_nuts_begin(h, &no) == BB_OK);

    std::vector<int32_t> dir(W), first(W), last(W), store(W), n_check(W), check((size_t)W * CS, 0);
    std::vector<double> lpl(W), kin(W), a((size_t)W * (DEPTH + 1)), b((size_t)W * (DEPTH + 1)), k0(W);
    bb_nuts_leaf_opts lo{dir.data(), first.data(), last.data(), store.data(), n_check.data(), check.data(), 0};
    bb_nuts_leaf_out out{lpl.data(), kin.data(), a.data(), b.data()};
    CHECK(bb_nuts_leaf(h, &lo, &out) == BB_ERR_INVALID);                   // a leaf before a start
    const int dirs[3] = {1, -1, 1};
    for (int pass = 0; pass < 2; ++pass) {                                 // all walkers, then walker 1 idle
        const int32_t* lv = pass ? some : live;
        CHECK(bb_nuts_start(h, 5 + pass, eps, lv, k0.data()) == BB_OK);
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < (1 << j); ++i) {
                for (int w = 0; w < W; ++w) {
                    dir[w] = lv[w] ? dirs[j] : 0; first[w] = i == 0; last[w] = i == (1 << j) - 1;
                    leaf_op(i, j, &store[w], &n_check[w], &check[(size_t)w * CS]);
                }
                CHECK(bb_nuts_leaf(h, &lo, &out) == BB_OK);
                for (int w = 0; w < W; ++w) CHECK(!lv[w] || (std::isfinite(lpl[w]) && std::isfinite(kin[w]) && std::isfinite(a[(size_t)w * (DEPTH + 1)])));
                if (i != (1 << j) - 1) continue;
                const int seq[3][3] = {{BB_NUTS_TAKE_LEAF, BB_NUTS_TAKE_SUB, BB_NUTS_TAKE_STATE}, {BB_NUTS_TAKE_LEAF | BB_NUTS_TAKE_SUB, BB_NUTS_TAKE_STATE, 0},
                                       {BB_NUTS_TAKE_LEAF | BB_NUTS_TAKE_SUB | BB_NUTS_TAKE_STATE, 0, 0}};
                for (int k = 0; k < 3 && seq[j][k]; ++k) {
                    for (int w = 0; w < W; ++w) flags[w] = lv[w] ? seq[j][k] : 0;
                    CHECK(bb_nuts_take(h, flags) == BB_OK);
                }
                CHECK(bb_hmc_get(h, zz.data(), lp.data(), gg.data()) == BB_OK);
                for (int w = 0; w < W; ++w) CHECK(!lv[w] || lp[w] == lpl[w]);
            }
    }
    // refused ops: nothing is launched
    dir[0] = 1; first[0] = 0; CHECK(bb_nuts_start(h, 9, eps, live, nullptr) == BB_OK && bb_nuts_leaf(h, &lo, nullptr) == BB_ERR_INVALID);
    first[0] = 1; store[0] = DEPTH; CHECK(bb_nuts_leaf(h, &lo, nullptr) == BB_ERR_INVALID);
    store[0] = 1; n_check[0] = 1; check[0] = 1; CHECK(bb_nuts_leaf(h, &lo, nullptr) == BB_ERR_INVALID);
    check[0] = DEPTH; CHECK(bb_nuts_leaf(h, &lo, nullptr) == BB_ERR_INVALID);
    n_check[0] = DEPTH + 2; CHECK(bb_nuts_leaf(h, &lo, nullptr) == BB_ERR_INVALID);
    flags[0] = BB_NUTS_TAKE_STATE; CHECK(bb_nuts_take(h, flags) == BB_ERR_INVALID);
    CHECK(bb_hmc_end(h) == BB_OK && bb_nuts_start(h, 9, eps, live, nullptr) == BB_ERR_INVALID);
    bb_destroy(h);
    std::printf("nuts_sanitize ok: D = %zu, kinetic0 %.17g %.17g\n", D, k0[0], k0[2]);
    return 0;
}
