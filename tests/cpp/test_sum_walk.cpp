// Stand-alone host check of sum_plan / sum_walk (poulpy_amd/csrc/device_sum.hpp), the term planner and the per-thread walk of k_glwe_sum:
// no device, its own main.  tests/test_ckks_sum_host.py writes the cases - operands, joins and the oracle chain's digits - to a text file
// and builds this program with the host sanitizers; every buffer is sized exactly, so a read or write past an operand, res or the staging
// slice is reported.
//
// File: ncases, then per case
//   n cols res_size base2k nterms
//   per term: a_size join k neg inplace, then a: a_size * cols * n values (limb-major, then column, then coefficient); an in-place term's
//             values are the initial content of res
//   want: res_size * cols * n values
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "device_sum.hpp"

using namespace pz;

// n is even, so every container holds a whole number of 16-byte pairs
struct Buf {
    std::vector<ulonglong2> v;
    explicit Buf(size_t count = 0) : v(count / 2) {}
    long long* p() { return reinterpret_cast<long long*>(v.data()); }
};

static Buf read_buf(std::ifstream& f, size_t count) {
    Buf b(count);
    for (size_t i = 0; i < count; ++i) f >> b.p()[i];
    return b;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    int ncases = 0;
    f >> ncases;
    int bad = 0, staged = 0, dropped = 0;
    for (int ci = 0; ci < ncases; ++ci) {
        int n, cols, res_size, base2k, nterms;
        f >> n >> cols >> res_size >> base2k >> nterms;
        if (!f || n < 2 || n % 2 || nterms < 1 || nterms > kSumMaxTerms) { std::fprintf(stderr, "case %d: bad header\n", ci); return 2; }
        const size_t rcount = (size_t)res_size * cols * n;
        Buf res(rcount);
        std::vector<Buf> ops((size_t)nterms);
        std::vector<SumSpec> spec((size_t)nterms);
        for (int u = 0; u < nterms; ++u) {
            int a_size, join, neg, inplace;
            long long k;
            f >> a_size >> join >> k >> neg >> inplace;
            ops[(size_t)u] = read_buf(f, (size_t)a_size * cols * n);
            if (inplace) {
                if (u != 0 || a_size != res_size) { std::fprintf(stderr, "case %d: only term 0 may be res\n", ci); return 2; }
                res = ops[0];
            }
            spec[(size_t)u] = SumSpec{nullptr, 0, a_size, join, neg, inplace, (unsigned long long)k};
        }
        for (int u = 0; u < nterms; ++u) spec[(size_t)u].a = spec[(size_t)u].inplace ? res.p() : ops[(size_t)u].p();
        Buf want = read_buf(f, rcount);
        if (!f) { std::fprintf(stderr, "case %d: truncated input\n", ci); return 2; }
        SumArgs g;
        g.res = res.p();
        g.n = n; g.batch = 1; g.cols = cols; g.res_size = res_size; g.k = base2k; g.pad = 0;
        const int kept = sum_plan(g, spec.data(), nterms, res_size, base2k);
        if (g.stage > kSumMaxStage) { std::fprintf(stderr, "case %d: staging beyond the kernel\n", ci); return 2; }
        staged += g.stage != 0;
        dropped += kept < nterms;
        std::vector<ulonglong2> slice((size_t)g.stage);   // one thread's slice, stride 1
        for (int c = 0; c < cols; ++c)
            for (int x = 0; x < n; x += 2) sum_walk(g, 0, c, x, slice.data(), 1);
        size_t diff = 0;
        for (size_t i = 0; i < rcount; ++i) diff += res.p()[i] != want.p()[i];
        if (diff) { std::printf("FAIL case %d: %zu of %zu values differ (%d terms, %d kept, base2k %d, %d limbs)\n", ci, diff, rcount, nterms, kept, base2k, res_size); ++bad; }
    }
    if (bad) { std::printf("%d of %d cases failed\n", bad, ncases); return 1; }
    std::printf("all sum walk checks passed: %d cases, %d staged, %d with dropped terms\n", ncases, staged, dropped);
    return 0;
}
