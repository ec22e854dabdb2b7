// Stand-alone host check of znx_inter_plan / znx_normalize_inter_walk (poulpy_amd/csrc/znx_steps.hpp), the same-base normalization every
// integer kernel shares: no device, its own main.  tests/test_znx_steps_host.py writes the cases - operand, offset and the oracle's digits -
// to a text file and builds this program with the host sanitizers; every buffer is sized exactly, so a read past the operand or a store
// past res is reported, and res starts from a pattern no digit equals, so a limb the walk leaves out is reported too.
//
// File: ncases, then per case
//   n cols res_size a_size base2k res_offset
//   a: a_size * cols * n values (limb-major, then column, then coefficient)
//   want: res_size * cols * n values
#include <cstdio>
#include <fstream>
#include <vector>

#include "znx_steps.hpp"

using namespace pz;

static std::vector<long long> read_buf(std::ifstream& f, size_t count) {
    std::vector<long long> b(count);
    for (size_t i = 0; i < count; ++i) f >> b[i];
    return b;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    int ncases = 0;
    f >> ncases;
    int bad = 0;
    for (int ci = 0; ci < ncases; ++ci) {
        int n, cols, res_size, a_size, base2k;
        long long res_offset;
        f >> n >> cols >> res_size >> a_size >> base2k >> res_offset;
        if (!f || n < 1 || cols < 1 || res_size < 1 || a_size < 1 || base2k < 1 || base2k > 63) { std::fprintf(stderr, "case %d: bad header\n", ci); return 2; }
        const std::vector<long long> a = read_buf(f, (size_t)a_size * cols * n);
        const std::vector<long long> want = read_buf(f, (size_t)res_size * cols * n);
        if (!f) { std::fprintf(stderr, "case %d: truncated input\n", ci); return 2; }
        const long long untouched = 0x5A5A5A5A5A5A5A5All;   // beyond every digit: base2k <= 63 keeps them below 2^62
        std::vector<long long> res(want.size(), untouched);
        const ZnxInterPlan p = znx_inter_plan(res_size, a_size, base2k, res_offset);
        size_t stores = 0;
        for (int c = 0; c < cols; ++c)
            for (int i = 0; i < n; ++i)
                znx_normalize_inter_walk(
                    p, base2k, res_size, a_size, [&](int l) { return a.at(((size_t)l * cols + c) * n + i); },
                    [&](int j, long long v) { res.at(((size_t)j * cols + c) * n + i) = v; ++stores; });
        size_t diff = 0;
        for (size_t i = 0; i < want.size(); ++i) diff += res[i] != want[i];
        if (diff || stores != want.size()) {
            std::printf("FAIL case %d: %zu of %zu values differ, %zu stores (base2k %d, res %d limbs, a %d limbs, offset %lld)\n", ci, diff, want.size(),
                        stores, base2k, res_size, a_size, res_offset);
            ++bad;
        }
    }
    if (bad) { std::printf("%d of %d cases failed\n", bad, ncases); return 1; }
    std::printf("all znx step checks passed: %d cases\n", ncases);
    return 0;
}
