// Host check of bb_math.h's two square roots (tests/test_opt_spec_emu.py): reads n doubles from the file argv[1] and writes, for each,
// the bits of bb_sqrt and of bb_sqrt_nonneg to the file argv[2] ([n][2] 64-bit words).  Built from the header itself, nothing restated.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bb_math.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> x;
    double v;
    while (fread(&v, sizeof v, 1, f) == 1) x.push_back(v);
    fclose(f);
    std::vector<uint64_t> out(2 * x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        const double a = bb_sqrt(x[i]), b = bb_sqrt_nonneg(x[i]);
        memcpy(&out[2 * i], &a, 8);
        memcpy(&out[2 * i + 1], &b, 8);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = fwrite(out.data(), 8, out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 5;
}
