// Stand-alone walk of the plan table (tests/_plan_cases.py) through the C ABI, for a sanitizer run of the planner on the host
// emulation: every request is created, asked for its stats and kernel name, taken through the cross-GPU attempt where the row has
// one (export, import, enable, disable -- refusals and the rollback included) and destroyed.  It asserts nothing about the plans
// (tests/test_emu_plan.py does); it must exit 0 with nothing reported.
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import _plan_cases as pc; pc.export_requests('/tmp/plan_requests.txt')"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DBB_EMU -x c++ barbay.jl_amd/csrc/bb_engine.hip \
//       -x c++ tests/plan_walk.cpp -o /tmp/plan_walk && /tmp/plan_walk /tmp/plan_requests.txt
#include "../include/barbay_hip.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: plan_walk REQUESTS\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int rows = 0, created = 0, refused = 0, enabled = 0, not_enabled = 0;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string name;
        int kind, nrep, n;
        long long nn, nb;
        f >> name >> kind >> nn >> nb >> nrep;
        std::vector<int32_t> T((size_t)nrep), geno, env;
        for (int& t : T) f >> t;
        f >> n; geno.resize((size_t)n); for (int& g : geno) f >> g;
        f >> n; env.resize((size_t)n); for (int& e : env) f >> e;
        f >> n;
        std::vector<std::string> sw((size_t)n);
        for (std::string& s : sw) { f >> s; const size_t eq = s.find('='); setenv(s.substr(0, eq).c_str(), s.substr(eq + 1).c_str(), 1); }
        int samples, elbo_every, mode, decayed, rank, world, ranks, ndev;
        f >> samples >> elbo_every >> mode >> decayed >> rank >> world >> ranks >> ndev;
        if (!f) { fprintf(stderr, "%s: malformed request\n", name.c_str()); return 2; }
        if (ranks < 0) setenv("BB_P2P_SELF", "1", 1);
        const long long B = nn + nb;
        std::vector<int64_t> counts, totals;
        for (int r = 0; r < nrep; ++r)
            for (int t = 0; t < T[(size_t)r]; ++t) totals.push_back(0);
        size_t trow = 0;
        for (int r = 0; r < nrep; ++r) {                       // counts [rep][barcode][t] = (7 (t B + b) + 11 rep) % 53 + 20, as _plan_cases.counts
            for (long long b = 0; b < B; ++b)
                for (int t = 0; t < T[(size_t)r]; ++t) {
                    const int64_t c = (7 * ((long long)t * B + b) + 11 * r) % 53 + 20;
                    counts.push_back(c);
                    totals[trow + (size_t)t] += c;
                }
            trow += (size_t)T[(size_t)r];
        }
        bb_model_desc md{};
        md.kind = kind; md.n_rep = nrep; md.n_neutral = nn; md.n_bc = nb;
        md.n_time = T.data(); md.counts = counts.data(); md.totals = totals.data();
        if (!geno.empty()) { md.geno_idx = geno.data(); for (int g : geno) if (g + 1 > md.n_geno) md.n_geno = g + 1; }
        if (!env.empty()) { md.env_idx = env.data(); for (int e : env) if (e + 1 > md.n_env) md.n_env = e + 1; }
        bb_advi_opts o;
        bb_default_opts(&o);
        o.samples_per_step = samples; o.elbo_every = elbo_every; o.launch_mode = mode; o.optimizer = decayed; o.window = 3; o.seed = 3;
        o.rank = rank; o.world_size = world;
        std::vector<int32_t> ids((size_t)ndev, 0);
        if (ndev > 1) { o.n_devices = ndev; o.device_ids = ids.data(); }
        const int nh = ranks > 0 ? ranks : 1;
        std::vector<bb_handle*> hs;
        bool ok = true;
        for (int r = 0; r < nh && ok; ++r) {
            if (ranks > 0) { o.rank = r; o.world_size = ranks; }
            bb_handle* h = nullptr;
            if (bb_create(&md, &o, &h) != BB_OK) { ok = false; ++refused; } else { hs.push_back(h); ++created; }
        }
        bb_stats st;
        char buf[128];
        auto look = [&]() { for (bb_handle* h : hs) if (bb_get_stats(h, &st) != BB_OK || bb_kernel_name(h, buf, sizeof buf) != BB_OK) { fprintf(stderr, "%s: %s\n", name.c_str(), bb_last_error()); exit(1); } };
        look();
        if (ok && ranks != 0) {
            std::vector<char> blob((size_t)nh * BB_P2P_HANDLE_BYTES);
            for (int r = 0; r < nh; ++r) if (bb_p2p_export(hs[(size_t)r], blob.data() + (size_t)r * BB_P2P_HANDLE_BYTES) != BB_OK) { fprintf(stderr, "%s: %s\n", name.c_str(), bb_last_error()); return 1; }
            for (bb_handle* h : hs) if (bb_p2p_import(h, blob.data()) != BB_OK) { fprintf(stderr, "%s: %s\n", name.c_str(), bb_last_error()); return 1; }
            for (bb_handle* h : hs) { const int rc = bb_p2p_enable(h, 1); if (rc == BB_OK) ++enabled; else if (rc == BB_ERR_UNSUPPORTED) ++not_enabled; else { fprintf(stderr, "%s: %s\n", name.c_str(), bb_last_error()); return 1; } }
            look();
            for (bb_handle* h : hs) if (bb_p2p_enable(h, 0) != BB_OK) { fprintf(stderr, "%s: %s\n", name.c_str(), bb_last_error()); return 1; }
            look();
        }
        for (bb_handle* h : hs) bb_destroy(h);
        for (const std::string& s : sw) unsetenv(s.substr(0, s.find('=')).c_str());
        unsetenv("BB_P2P_SELF");
        ++rows;
    }
    printf("plan_walk: %d rows, %d handles created, %d creates refused, %d enables taken, %d refused\n", rows, created, refused, enabled, not_enabled);
    return rows > 0 ? 0 : 2;
}
