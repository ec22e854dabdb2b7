// Host-only check of the fused tail's launch plan (poulpy_amd/csrc/tail_plan.hpp): built with -fsanitize=address,undefined and run as a child
// process by tests/test_tail_plan_host.py.
//   closure      over every call shape of the sweep that tail_plan does not refuse: at most four launches, none empty, every form with an entry
//                for the plan (tail_form_exists), every column written by exactly one launch - or by exactly one pair, the 16-bit operand on a
//                16-bit form beside the operand variant that keeps body16_wide - and no other overlap
//   equivalence  argv[1] = tests/golden/tail_plans.txt, one line per call shape: the columns of Shape below, then what launch_tail.hip did with it
//                BEFORE tail_plan.hpp (five split blocks and an if chain, tail_launch_form stubbed): per launch the form, the columns, the block order
//                and the scalar fields of TailArgs, or the refusal's code and text.  Every line is re-derived and compared as a string
//   coverage     the file holds all twelve forms, the four plain pairs, every branch of the split, both 16-bit-operand branches with and without
//                other16, and every refusal the sweep meets
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../poulpy_amd/csrc/tail_plan.hpp"

using namespace pz;

static std::atomic<int> failures{0};
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 50) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

// one call shape: the columns of the golden file, in this order
struct Shape {
    int f1a = 8, f1b = 16, cb = 16, batch = 1, ncols = 2, body_col = 0, base2k = 17, small_bits = 64, res_bits = 64, small_size = 5;
    int auto_cls = 0;   // auto_mul: 0, 1 = 2N, 2 = another value
    int gather = 0;     // gather_mul != 0
    int rowmajor = 0, small = 0, small_all = 0, small_neg = 0, small16 = 0, body_src = 0, body_only = 0, body16 = 0, other16 = 0, auto_neg = 0, post_neg = 0,
        big_neg = 0, keyauto = 0, gather_neg = 0, post_rsh = 0;
    int nz = 0, nz_lsh = 0, nz_store = 0 /* NzCombine: 0 plain, 1 mode 5, 2 another */, d16 = 0, d16_w = 0, d16_ra = 0, d16_only = 0;
};
constexpr int kShapeInts = 34;
static_assert(sizeof(Shape) == kShapeInts * sizeof(int), "Shape is its columns");

// the values the recorder gave what a shape only names: N, the strides that come with each pointer, the limbs of the 16-bit body operand
constexpr long long kN = 8192, kSmallBs = 444, kBodyBs = 111, kSmall16Cs = 222;
constexpr int kBody16Limbs = 3;
static TailFacts facts_of(const Shape& s) {
    TailFacts f;
    f.f1a = s.f1a; f.f1b = s.f1b; f.cb = s.cb; f.batch = s.batch; f.ncols = s.ncols; f.body_col = s.body_col; f.base2k = s.base2k;
    f.rowmajor = s.rowmajor; f.small = s.small; f.small_all = s.small_all; f.small_neg = s.small_neg; f.small16 = s.small16;
    f.small_bs = s.small ? kSmallBs : 0; f.small_size = s.small_size; f.small_bits = s.small_bits; f.res_bits = s.res_bits;
    f.body_src = s.body_src; f.body_only = s.body_only; f.body_bs = s.body_src ? kBodyBs : 0; f.body_ls = s.body_src ? kN : 0;
    f.body16 = s.body16; f.body16_wide = s.body16; f.other16 = s.other16; f.body16_limbs = s.body16 ? kBody16Limbs : 0;
    f.auto_mul = s.auto_cls == 0 ? 0u : s.auto_cls == 1 ? 2u * (unsigned)kN : 5u; f.gather_mul = s.gather ? 7u : 0u;
    f.auto_neg = s.auto_neg; f.post_neg = s.post_neg; f.big_neg = s.big_neg; f.keyauto = s.keyauto; f.gather_neg = s.gather_neg; f.post_rsh = s.post_rsh;
    f.nz = s.nz; f.nz_lsh = s.nz_lsh; f.nz_plain = s.nz_store == 0; f.nz_mode5 = s.nz_store == 1;
    f.d16 = s.d16; f.d16_w = s.d16 && s.d16_w; f.d16_ra = s.d16 && s.d16_ra; f.d16_only = s.d16 && s.d16_only;   // (a TailD16 counts if the call names one)
    return f;
}

static const char* kKind[] = {"PLAIN", "RSH", "SGN", "NZ1", "NZ2", "ACC32", "NZ1W", "NZ2R", "NZ1O", "NZ2O", "SGN16", "SGN16R"};
// one launch as the golden file writes it: the form, the columns, the block order, then the scalar part of tail_args (launch_tail.hip) on the
// call of the launch's role
static std::string render(const TailFacts& c, const TailLaunch& l) {
    const TailFacts d = tail_role_call(c, l.role);
    unsigned am = d.auto_mul;
    bool an = d.auto_neg, sn = d.small_neg, pb = d.body_src, b16w = false;
    long long bbs = d.body_bs;
    const char* d16a = d.nz && d.d16_ra ? "ra" : "none";
    if (d.small16) { d16a = "small16"; bbs = kSmall16Cs; }
    if (d.big_neg) { am = 2u * (unsigned)kN; an = sn = pb = true; bbs = d.small_bs; }
    if (d.body16) { d16a = l.role == TailRole::OTHER16 ? "other16" : "body16"; bbs = d.body16_limbs * kN; b16w = d.body16_wide; }
    const int acc32 = (d.small_bits == 32 ? 1 : 0) | (d.res_bits == 32 ? 2 : 0) | (d.small16 ? 4 : 0) | (d.small_bits == 16 ? 8 : 0) | (d.res_bits == 16 ? 16 : 0);
    std::ostringstream o;
    o << kKind[l.form.kind] << "(" << (int)l.form.rowmajor << "," << (int)l.form.has_small << ") cols=" << l.col_base << "+" << l.col_count << " xcd=" << (int)l.xcd;
    o << " sa=" << (int)d.small_all << " am=" << (am == 0 ? "0" : am == 2u * (unsigned)kN ? "2N" : "x") << " an=" << (int)an << " gm=" << (int)(d.gather_mul != 0)
      << " gn=" << (int)d.gather_neg << " pb=" << (int)pb << " sn=" << (int)sn << " pn=" << (int)d.post_neg << " bo=" << (int)d.body_only << " raw=0 nz=" << (int)d.nz
      << " acc32=" << acc32 << " d16a=" << d16a << " bbs=";
    if (bbs == 0) o << "zero"; else if (bbs == kBodyBs) o << "call"; else if (bbs == kSmall16Cs) o << "small16_cs"; else if (bbs == kSmallBs) o << "small_bs";
    else o << "limbs:" << bbs / kN;
    o << " b16w=" << (int)b16w << " small=" << (int)d.small << " ss=" << d.small_size;
    return o.str();
}
static std::string derive(const Shape& s) {
    const TailFacts c = facts_of(s);
    const TailPlan p = tail_plan(c);
    std::ostringstream o;
    if (p.err != PZ_OK) { o << "refuse " << p.err << " " << p.msg; return o.str(); }
    if (p.n == 0) return "nothing";
    for (int i = 0; i < p.n; ++i) o << (i ? " ; " : "") << render(c, p.launch[i]);
    return o.str();
}

// what the closure sweep and the recorded file met: forms, plain (row-major, operand) pairs and branches as bit sets, the texts of the refusals
static const char* kBranch[] = {"whole", "body / plain", "key composition", "key composition, N = 4096", "key composition, another plan without the sign-only form",
                                "plain spectral automorphism", "plain spectral automorphism, body16", "add / sub, body16", "add / sub, body16 and other16",
                                "normalizing store"};
constexpr int kBranches = sizeof(kBranch) / sizeof(kBranch[0]);
static int bits_set(unsigned v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }
struct Seen {
    unsigned kinds = 0, plain_pairs = 0, branches = 0;
    const char* refusals[32] = {nullptr};
    int nrefusals = 0;
    bool refused_with(const char* msg) const {
        for (int i = 0; i < nrefusals; ++i) if (refusals[i] == msg || std::strcmp(refusals[i], msg) == 0) return true;
        return false;
    }
    void add(const Shape& s, const TailFacts& c, const TailPlan& p) {
        if (p.err != PZ_OK) {
            if (!refused_with(p.msg) && nrefusals < 32) refusals[nrefusals++] = p.msg;
            return;
        }
        unsigned roles = 0;
        for (int i = 0; i < p.n; ++i) {
            const TailLaunch& l = p.launch[i];
            kinds |= 1u << l.form.kind;
            if (l.form.kind == TailForm::PLAIN) plain_pairs |= 1u << (2 * l.form.rowmajor + l.form.has_small);
            roles |= 1u << (int)l.role;
        }
        auto has = [&](TailRole r) { return (roles >> (int)r & 1u) != 0; };
        int b = 0;   // whole
        if (s.nz) b = 9;
        else if (c.keyauto) b = has(TailRole::SIGNS) ? 2 : (c.f1a == 4 && c.f1b == 4) ? 3 : 4;
        else if (has(TailRole::BODY)) b = 1;
        else if (has(TailRole::OTHER16)) b = 8;
        else if (has(TailRole::OPERAND)) b = 7;
        else if (has(TailRole::BODY16)) b = c.body_only ? 6 : 7;   // (add / sub with one column: nothing around it)
        else if (has(TailRole::SIGNS)) b = 5;
        if (p.n) branches |= 1u << b;
    }
    void merge(const Seen& o) {
        kinds |= o.kinds; plain_pairs |= o.plain_pairs; branches |= o.branches;
        for (int i = 0; i < o.nrefusals; ++i) if (!refused_with(o.refusals[i]) && nrefusals < 32) refusals[nrefusals++] = o.refusals[i];
    }
};

// the closure check on one shape; one of these per thread of the sweep
struct Closure {
    unsigned long long shapes = 0, planned = 0;
    Seen swept;
    void operator()(const Shape& s);
};
void Closure::operator()(const Shape& s) {
    const TailFacts c = facts_of(s);
    const TailPlan p = tail_plan(c);
    ++shapes;
    swept.add(s, c, p);
    if (p.err != PZ_OK) {
        CHECK(p.msg != nullptr && p.n == 0 && (p.err == PZ_ERR_INVALID || p.err == PZ_ERR_UNSUPPORTED), "refusal %d without a text, or with launches", p.err);
        return;
    }
    ++planned;
    CHECK(p.n >= 1 && p.n <= 4, "%d launches", p.n);
    int writers[4] = {0, 0, 0, 0}, op16[4] = {0, 0, 0, 0}, keeps_wide[4] = {0, 0, 0, 0};
    for (int i = 0; i < p.n && i < 4; ++i) {
        const TailLaunch& l = p.launch[i];
        CHECK(l.col_count > 0 && l.col_base >= 0 && l.col_base + l.col_count <= s.ncols, "launch %d: columns %d + %d of %d", i, l.col_base, l.col_count, s.ncols);
        CHECK(tail_form_exists(l.form, s.f1a, s.f1b, s.cb), "launch %d: form %s has no entry for plan (%d, %d, %d)", i, kKind[l.form.kind], s.f1a, s.f1b, s.cb);
        const TailFacts d = tail_role_call(c, l.role);
        CHECK(l.form.has_small == d.small && l.form.rowmajor == d.rowmajor, "launch %d: form (%d, %d) on a call (%d, %d)", i, (int)l.form.rowmajor, (int)l.form.has_small, (int)d.rowmajor, (int)d.small);
        const bool sixteen = (l.role == TailRole::BODY16 || l.role == TailRole::OTHER16) && (l.form.kind == TailForm::SGN16 || l.form.kind == TailForm::SGN16R);
        const bool wide = l.role == TailRole::AS_GIVEN && l.form.has_small && d.body16 && d.body16_wide;
        for (int col = l.col_base; col < l.col_base + l.col_count && col < 4 && col >= 0; ++col) { ++writers[col]; op16[col] += sixteen; keeps_wide[col] += wide; }
    }
    for (int col = 0; col < s.ncols; ++col)
        CHECK(writers[col] == 1 || (writers[col] == 2 && op16[col] == 1 && keeps_wide[col] == 1), "column %d of %d: %d launches (%d on a 16-bit form, %d keeping body16_wide)",
              col, s.ncols, writers[col], op16[col], keeps_wide[col]);
}

// the ten plans of PZ_P1F_CASES
static const int kPlans[][3] = {
#define X(A, B, C) {A, B, C},
    PZ_P1F_CASES(X)
#undef X
};
constexpr int kBits[3] = {64, 32, 16};
// Every combination of what the plan reads.  Without a normalizing store: the fourteen flags of a TailCall, auto_mul and gather_mul zero or not,
// the digit widths, the plans, 1..4 columns with every body column, base2k around the launcher's bounds 29 and 31 (gather_neg, which the plan
// does not read, is up so that a role that clears it shows).  With one: the flags the form choice reads in front of it, the three NzCombine classes,
// the four TailD16 flags, one and two columns, base2k around the bounds 14 and 16, a shift inside and on both sides of [0, base2k).
// (part, nparts): the (plan, widths) combinations this caller takes
template <class F>
static void sweep(F&& one, int part, int nparts) {
    int combination = 0;
    for (const auto& pl : kPlans)
    for (int sb = 0; sb < 3; ++sb)
    for (int rb = 0; rb < 3; ++rb) {
        if (combination++ % nparts != part) continue;
        Shape s;
        s.f1a = pl[0]; s.f1b = pl[1]; s.cb = pl[2]; s.small_bits = kBits[sb]; s.res_bits = kBits[rb]; s.gather_neg = 1;
        for (s.ncols = 1; s.ncols <= 4; ++s.ncols)
        for (s.body_col = 0; s.body_col < s.ncols; ++s.body_col)
        for (s.base2k = 29; s.base2k <= 32; ++s.base2k)
        for (int b = 0; b < (1 << 16); ++b) {
            s.rowmajor = b & 1; s.small = b >> 1 & 1; s.small_all = b >> 2 & 1; s.small_neg = b >> 3 & 1; s.small16 = b >> 4 & 1; s.body_src = b >> 5 & 1;
            s.body_only = b >> 6 & 1; s.body16 = b >> 7 & 1; s.other16 = b >> 8 & 1; s.auto_neg = b >> 9 & 1; s.post_neg = b >> 10 & 1; s.big_neg = b >> 11 & 1;
            s.keyauto = b >> 12 & 1; s.post_rsh = b >> 13 & 1; s.auto_cls = (b >> 14 & 1) * 2; s.gather = b >> 15 & 1;
            one(s);
        }
        s = Shape{};
        s.f1a = pl[0]; s.f1b = pl[1]; s.cb = pl[2]; s.small_bits = kBits[sb]; s.res_bits = kBits[rb]; s.nz = 1; s.small_size = 0;
        for (s.ncols = 1; s.ncols <= 2; ++s.ncols)
        for (s.base2k = 14; s.base2k <= 17; ++s.base2k)
        for (int sh = 0; sh < 4; ++sh)
        for (s.nz_store = 0; s.nz_store < 3; ++s.nz_store)
        for (int b = 0; b < (1 << 13); ++b) {
            s.nz_lsh = sh == 0 ? 0 : sh == 1 ? s.base2k - 1 : sh == 2 ? s.base2k : -1;
            s.rowmajor = b & 1; s.small = b >> 1 & 1; s.small_all = b >> 2 & 1; s.small16 = b >> 3 & 1; s.body_src = b >> 4 & 1; s.body16 = b >> 5 & 1;
            s.post_rsh = b >> 6 & 1; s.auto_cls = (b >> 7 & 1) * 2; s.gather = b >> 8 & 1;
            s.d16 = b >> 9 & 1; s.d16_w = b >> 10 & 1; s.d16_ra = b >> 11 & 1; s.d16_only = b >> 12 & 1;
            one(s);
        }
    }
}

int main(int argc, char** argv) {
    const int nthreads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<Closure> parts(nthreads);
    std::vector<std::thread> threads;
    for (int t = 0; t < nthreads; ++t) threads.emplace_back([&parts, t, nthreads] { sweep(parts[t], t, nthreads); });
    for (std::thread& t : threads) t.join();
    unsigned long long shapes = 0, planned = 0;
    Seen swept;
    for (const Closure& c : parts) { shapes += c.shapes; planned += c.planned; swept.merge(c.swept); }
    std::printf("closure: %llu shapes, %llu planned, %d forms, %d refusals, %d branches of the split\n", shapes, planned, bits_set(swept.kinds), swept.nrefusals,
                bits_set(swept.branches));
    CHECK(swept.kinds == (1u << 12) - 1 && swept.plain_pairs == 15u, "forms %#x, plain pairs %#x in the sweep", swept.kinds, swept.plain_pairs);
    CHECK(swept.nrefusals == 14 && swept.branches == (1u << kBranches) - 1, "%d refusals, branches %#x in the sweep", swept.nrefusals, swept.branches);

    CHECK(argc > 1, "usage: test_tail_plan tests/golden/tail_plans.txt");
    Seen recorded;
    size_t lines = 0;
    if (argc > 1) {
        std::ifstream in(argv[1]);
        CHECK(in.good(), "cannot read %s", argv[1]);
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            const size_t bar = line.find(" | ");
            CHECK(bar != std::string::npos, "line without a result: %s", line.c_str());
            if (bar == std::string::npos) continue;
            std::istringstream is(line.substr(0, bar));
            Shape s;
            int* v = &s.f1a;
            bool ok = true;
            for (int i = 0; i < kShapeInts; ++i) ok = ok && (bool)(is >> v[i]);
            CHECK(ok, "bad shape: %s", line.c_str());
            if (!ok) continue;
            const std::string want = line.substr(bar + 3), got = derive(s);
            CHECK(got == want, "%s\n    recorded %s\n    derived  %s", line.substr(0, bar).c_str(), want.c_str(), got.c_str());
            const TailFacts c = facts_of(s);
            recorded.add(s, c, tail_plan(c));
            ++lines;
        }
        CHECK(lines >= 200, "%zu recorded shapes", lines);
        CHECK(recorded.kinds == (1u << 12) - 1, "forms recorded: %#x of the twelve", recorded.kinds);
        CHECK(recorded.plain_pairs == 15u, "plain (row-major, operand) pairs recorded: %#x of the four", recorded.plain_pairs);
        for (int i = 0; i < swept.nrefusals; ++i) CHECK(recorded.refused_with(swept.refusals[i]), "no recorded shape is refused with: %s", swept.refusals[i]);
        for (int b = 0; b < kBranches; ++b) CHECK(b == 4 || (recorded.branches >> b & 1u), "no recorded shape takes the branch: %s", kBranch[b]);
    }
    std::printf("equivalence: %zu recorded shapes, %d forms, %d refusals, %d branches\n", lines, bits_set(recorded.kinds), recorded.nrefusals, bits_set(recorded.branches));

    if (failures) { std::printf("%d check(s) failed\n", failures.load()); return 1; }
    std::printf("all fused-tail plan checks passed\n");
    return 0;
}
