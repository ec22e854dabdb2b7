// Stand-alone host check of lc_walk (poulpy_amd/csrc/device_lincomb.hpp), the per-coefficient walk of k_lincomb_const: no device, its own
// main.  tests/test_ckks_lincomb_host.py writes the cases - inputs, terms and the oracle's digits - to a text file and builds this program
// with the host sanitizers; every buffer is sized exactly, so a read or write past a slice, an operand or res is reported.
//
// File: ncases, then per case
//   n cols res_size base2k nterms init_res normalize
//   res: res_size * cols * n values (limb-major, then column, then coefficient), the initial content
//   per term: a_size cnv_offset has_re has_im b_size join k neg, the re digits, the im digits, then a: a_size * cols * n values
//   want: res_size * cols * n values
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "device_lincomb.hpp"

using namespace pz;

struct TermIn {
    std::vector<long long> a, re, im;
    LinTermSpec s;
};

static std::vector<long long> read_vec(std::ifstream& f, size_t count) {
    std::vector<long long> v(count);
    for (auto& x : v) f >> x;
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    int ncases = 0;
    f >> ncases;
    int bad = 0;
    for (int ci = 0; ci < ncases; ++ci) {
        int n, cols, res_size, base2k, nterms, init_res, normalize;
        f >> n >> cols >> res_size >> base2k >> nterms >> init_res >> normalize;
        const size_t rcount = (size_t)res_size * cols * n;
        std::vector<long long> res = read_vec(f, rcount);
        std::vector<TermIn> in((size_t)nterms);
        bool pair = false, has_tmp = false;
        int a_max = 1;
        for (auto& t : in) {
            int a_size, has_re, has_im, b_size, join, neg;
            long long cnv, k;
            f >> a_size >> cnv >> has_re >> has_im >> b_size >> join >> k >> neg;
            t.re = read_vec(f, has_re ? (size_t)b_size : 0);
            t.im = read_vec(f, has_im ? (size_t)b_size : 0);
            t.a = read_vec(f, (size_t)a_size * cols * n);
            t.s = LinTermSpec{t.a.data(), 0, a_size, (size_t)cnv, has_re ? (const int64_t*)t.re.data() : nullptr,
                              has_im ? (const int64_t*)t.im.data() : nullptr, b_size, join, neg, (size_t)k};
            pair = pair || has_im;
            has_tmp = has_tmp || ((&t != &in[0] || init_res) && join != 0);
            if ((has_re || has_im) && a_size > a_max) a_max = a_size;
        }
        const std::vector<long long> want = read_vec(f, rcount);
        if (!f) { std::fprintf(stderr, "case %d: truncated input\n", ci); return 2; }
        std::vector<LinTerm> terms((size_t)nterms);
        for (int u = 0; u < nterms; ++u) lc_plan_term(terms[(size_t)u], in[(size_t)u].s, res_size, base2k);
        LinArgs g;
        g.res = res.data(); g.res_bs = (long long)rcount; g.terms = terms.data();
        g.n = n; g.batch = 1; g.cols = cols; g.res_size = res_size; g.k = base2k; g.nterms = nterms;
        g.init_res = init_res; g.normalize = normalize; g.pair = pair ? 1 : 0; g.a_max = a_max; g.has_tmp = has_tmp ? 1 : 0;
        // one coefficient's slice, exactly: element e at slice[e * kMulConstBlock]
        std::vector<long long> slice((size_t)(lc_slots(a_max, res_size, g.pair, g.has_tmp) - 1) * kMulConstBlock + 1);
        const int npts = pair ? n / 2 : n;
        for (int x = 0; x < npts; ++x)
            for (int c = 0; c < cols; ++c) lc_walk(g, terms.data(), 0, c, x, slice.data());
        size_t diff = 0;
        for (size_t i = 0; i < rcount; ++i) diff += res[i] != want[i];
        if (diff) { std::printf("FAIL case %d: %zu of %zu values differ\n", ci, diff, rcount); ++bad; }
        else std::printf("ok case %d: %d terms, %s, %d -> %d limbs\n", ci, nterms, pair ? "paired" : "unpaired", a_max, res_size);
    }
    if (bad) return 1;
    std::printf("all lincomb walk checks passed: %d cases\n", ncases);
    return 0;
}
