// Host-only check of the BDD schedule compiler (poulpy_amd/csrc/bdd_schedule.cpp): built with -fsanitize=address,undefined and run as a child
// process by tests/test_bdd_host.py.  Every circuit is compiled, its tables re-checked (bdd_check), and the schedule - all gates of a level
// reading before any of them writes, as concurrent workgroups may - is evaluated on clear bits against the two-bank walk of eval_level.
//   test_bdd_schedule [file]   file: "input_size output_size" then per output "state_size node_count" and node_count x "kind sel hi lo"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../poulpy_amd/csrc/bdd_schedule.hpp"

using namespace pz;

struct Circuit {
    size_t input_size = 0;
    std::vector<std::vector<BddNode>> nodes;
    std::vector<size_t> state;
};
static const BddNode NONE{kBddNone, 0, 0, 0}, COPY{kBddCopy, 0, 0, 0};
static BddNode cmux(uint32_t sel, uint32_t hi, uint32_t lo) { return BddNode{kBddCmux, sel, hi, lo}; }

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

static bool compile(const Circuit& c, BddSchedule* s, std::string* err) {
    std::vector<const BddNode*> ptrs;
    std::vector<size_t> counts;
    for (auto& v : c.nodes) { ptrs.push_back(v.data()); counts.push_back(v.size()); }
    return bdd_compile(ptrs.data(), counts.data(), c.state.data(), c.nodes.size(), c.input_size, s, err);
}

// eval_level on clear bits (eval.rs:241-305)
static std::vector<int> walk(const Circuit& c, const std::vector<int>& bits) {
    std::vector<int> out;
    for (size_t o = 0; o < c.nodes.size(); ++o) {
        const size_t S = c.state[o];
        if (S == 0) { out.push_back(0); continue; }
        const auto& nd = c.nodes[o];
        std::vector<int> level(2 * S, 0);
        level[1] = 1;
        size_t prev = 0, next = S;
        for (size_t at = 0; at + S < nd.size(); at += S) {
            for (size_t j = 0; j < S; ++j) {
                const BddNode& x = nd[at + j];
                if (x.kind == kBddCmux) level[next + j] = bits[x.sel] ? level[prev + x.hi] : level[prev + x.lo];
                else if (x.kind == kBddCopy) level[next + j] = level[prev + j];
            }
            std::swap(prev, next);
        }
        const BddNode& r = nd[nd.size() - S];
        out.push_back(bits[r.sel] ? level[prev + r.hi] : level[prev + r.lo]);
    }
    return out;
}

// the schedule on clear bits: per level every read first, then every write; a slot nobody wrote reads as garbage (7)
static std::vector<int> run_schedule(const BddSchedule& s, const std::vector<int>& bits) {
    std::vector<int> slot(s.slots, 7), out(s.output_size, 7);
    slot[kBddSlotZero] = 0; slot[kBddSlotOne] = 1;
    for (uint32_t o : s.zero_outputs) out[o] = 0;
    for (size_t lv = 0; lv < s.levels(); ++lv) {
        std::vector<int> res;
        for (size_t i = s.level_start[lv]; i < s.level_start[lv + 1]; ++i) res.push_back(bits[s.gates[i].sel] ? slot[s.gates[i].t] : slot[s.gates[i].f]);
        for (size_t i = s.level_start[lv]; i < s.level_start[lv + 1]; ++i) {
            const uint32_t r = s.gates[i].res;
            ((r & kBddOut) ? out[r & ~kBddOut] : slot[r]) = res[i - s.level_start[lv]];
        }
    }
    return out;
}

static void accept(const char* name, const Circuit& c, std::mt19937& rng, int trials = 64) {
    BddSchedule s;
    std::string err;
    if (!compile(c, &s, &err)) { CHECK(false, "%s: rejected: %s", name, err.c_str()); return; }
    CHECK(bdd_check(s, &err), "%s: %s", name, err.c_str());
    size_t cm = 0, cp = 0, depth = 0;
    for (size_t o = 0; o < c.nodes.size(); ++o) {
        for (auto& x : c.nodes[o]) { cm += x.kind == kBddCmux; cp += x.kind == kBddCopy; }
        if (c.state[o]) depth = std::max(depth, c.nodes[o].size() / c.state[o]);
        CHECK(s.slot_count[o] <= 2 * c.state[o], "%s: output %zu: %u slots, state %zu", name, o, s.slot_count[o], c.state[o]);
    }
    CHECK(s.gates.size() == cm && s.copies == cp && s.moved_copies == 0 && s.levels() == depth, "%s: %zu gates (%zu cmux), %zu copies (%zu), %zu levels (%zu)", name,
          s.gates.size(), cm, s.copies, cp, s.levels(), depth);
    for (int t = 0; t < trials; ++t) {
        std::vector<int> bits(c.input_size);
        for (auto& b : bits) b = (int)(rng() & 1u);
        if (t == 0) std::fill(bits.begin(), bits.end(), 0);
        if (t == 1) std::fill(bits.begin(), bits.end(), 1);
        const std::vector<int> want = walk(c, bits), got = run_schedule(s, bits);
        CHECK(want == got, "%s: trial %d: the schedule and the walk disagree", name, t);
    }
    std::printf("ok %s: %zu outputs, %zu levels, %zu gates, %zu copies renamed, %zu slots\n", name, c.nodes.size(), s.levels(), s.gates.size(), s.copies, s.slots);
}

static void reject(const char* name, const Circuit& c, const char* must_say) {
    BddSchedule s;
    std::string err;
    const bool ok = compile(c, &s, &err);
    CHECK(!ok, "%s: accepted", name);
    CHECK(err.find(must_say) != std::string::npos, "%s: message '%s' lacks '%s'", name, err.c_str(), must_say);
}

// random well-formed output: `depth` levels of state S; every kind everywhere, indices anywhere below S
static void random_output(Circuit& c, size_t S, size_t depth, std::mt19937& rng) {
    std::vector<BddNode> nd;
    for (size_t lv = 0; lv + 1 < depth; ++lv)
        for (size_t j = 0; j < S; ++j) {
            const unsigned k = rng() % 4;
            nd.push_back(k == 0 ? NONE : k == 1 ? COPY : cmux(rng() % c.input_size, rng() % S, rng() % S));
        }
    nd.push_back(cmux(rng() % c.input_size, rng() % S, rng() % S));
    for (size_t j = 1; j < S; ++j) nd.push_back(NONE);
    c.nodes.push_back(nd);
    c.state.push_back(S);
}

static bool load(const char* path, Circuit* c) {
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    size_t n_out = 0;
    bool ok = std::fscanf(f, "%zu %zu", &c->input_size, &n_out) == 2;
    for (size_t o = 0; ok && o < n_out; ++o) {
        size_t S = 0, cnt = 0;
        ok = std::fscanf(f, "%zu %zu", &S, &cnt) == 2;
        std::vector<BddNode> nd(ok ? cnt : 0);
        for (size_t i = 0; ok && i < cnt; ++i) ok = std::fscanf(f, "%u %u %u %u", &nd[i].kind, &nd[i].sel, &nd[i].hi, &nd[i].lo) == 4;
        c->nodes.push_back(nd);
        c->state.push_back(S);
    }
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    std::mt19937 rng(12345);
    if (argc > 1) {
        Circuit c;
        if (!load(argv[1], &c)) { std::printf("FAIL: cannot read %s\n", argv[1]); return 2; }
        accept("circuit from file", c, rng, 256);
    }
    {   // width 1: slot 1 of the 2 S slots is the SECOND bank - a one-level circuit reads zero, a two-level one whose first level is None reads one
        Circuit c; c.input_size = 2;
        c.nodes = {{cmux(0, 0, 0)}, {NONE, cmux(1, 0, 0)}, {cmux(0, 0, 0), cmux(1, 0, 0)}, {COPY, cmux(1, 0, 0)}};
        c.state = {1, 1, 1, 1};
        accept("width 1", c, rng);
    }
    {   // hi == lo, a gate at the position of its own source, two gates reading one slot, a stale slot read two levels later and then overwritten
        Circuit c; c.input_size = 3;
        c.nodes = {{cmux(0, 1, 1), cmux(1, 1, 0), NONE,        // B: [1, x1, 0]
                    cmux(2, 0, 1), cmux(0, 1, 1), cmux(1, 0, 1),   // A: [x2 ? B0 : B1, B1, x1 ? B0 : B1]
                    NONE, COPY, cmux(2, 2, 0),                 // B: [1 (stale), A1, x2 ? A2 : A0]
                    cmux(0, 0, 2), NONE, NONE,                 // A: [x0 ? B0 : B2, B1 (stale from two levels ago), stale]
                    cmux(1, 0, 1), NONE, NONE}};               // root
        c.state = {3};
        accept("hi == lo, stale slots", c, rng);
    }
    {   // a Copy chain from level 0 to the root's level, levels of nothing but None / Copy
        Circuit c; c.input_size = 2;
        std::vector<BddNode> nd = {cmux(0, 1, 0), cmux(1, 0, 1)};
        for (int i = 0; i < 9; ++i) { nd.push_back(COPY); nd.push_back(i % 3 == 0 ? NONE : COPY); }
        nd.push_back(NONE); nd.push_back(NONE);   // an all-None level: both banks keep what they hold
        nd.push_back(cmux(1, 0, 1)); nd.push_back(NONE);
        c.nodes = {nd};
        c.state = {2};
        accept("copy chain and empty levels", c, rng);
    }
    {   // 32 outputs of unequal depth and width, a zero output in between
        Circuit c; c.input_size = 7;
        for (size_t o = 0; o < 32; ++o) {
            if (o == 13) { c.nodes.push_back({}); c.state.push_back(0); continue; }
            random_output(c, 1 + o % 5, 1 + (o * 7) % 23, rng);
        }
        accept("32 outputs of unequal depth", c, rng, 128);
    }
    for (int rep = 0; rep < 200; ++rep) {   // random circuits of every kind
        Circuit c; c.input_size = 1 + rng() % 6;
        const size_t n_out = rng() % 5;
        for (size_t o = 0; o < n_out; ++o) {
            if (rng() % 7 == 0) { c.nodes.push_back({}); c.state.push_back(0); }
            else random_output(c, 1 + rng() % 6, 1 + rng() % 12, rng);
        }
        BddSchedule s;
        std::string err;
        CHECK(compile(c, &s, &err), "random circuit %d rejected: %s", rep, err.c_str());
        for (int t = 0; t < 16; ++t) {
            std::vector<int> bits(c.input_size);
            for (auto& b : bits) b = (int)(rng() & 1u);
            CHECK(walk(c, bits) == run_schedule(s, bits), "random circuit %d: the schedule and the walk disagree", rep);
        }
    }
    {   // every validation rule
        Circuit c; c.input_size = 2; c.state = {2};
        c.nodes = {{cmux(0, 2, 0), NONE}};       reject("hi out of range", c, "output 0 node 0: hi index 2");
        c.nodes = {{NONE, NONE, cmux(0, 0, 5), NONE}};  reject("lo out of range", c, "output 0 node 2: lo index 5");
        c.nodes = {{cmux(2, 1, 0), NONE}};       reject("selector out of range", c, "output 0 node 0: selector 2");
        c.nodes = {{cmux(0, 1, 0), NONE, NONE}}; reject("ragged", c, "output 0: 3 nodes are not whole chunks");
        c.nodes = {{COPY, NONE}};                reject("last chunk without a cmux", c, "output 0 node 0: the last chunk must start with a cmux");
        c.nodes = {{cmux(0, 1, 0), COPY}};       reject("last chunk with a second node", c, "output 0 node 1: the last chunk is [cmux, none");
        c.nodes = {{BddNode{9, 0, 0, 0}, NONE}}; reject("unknown kind", c, "output 0 node 0: unknown kind");
        c.state = {0};
        c.nodes = {{cmux(0, 0, 0)}};             reject("nodes on a zero output", c, "output 0 has state_size 0 and 1 nodes");
        c.state = {2, 2};
        c.nodes = {{cmux(0, 1, 0), NONE}, {}};   reject("no nodes", c, "output 1: 0 nodes");
    }
    {   // bdd_check itself notices a broken table
        Circuit c; c.input_size = 2; c.state = {2};
        c.nodes = {{cmux(0, 1, 0), cmux(1, 0, 1), cmux(1, 0, 1), NONE}};
        BddSchedule s;
        std::string err;
        CHECK(compile(c, &s, &err), "%s", err.c_str());
        BddSchedule t = s;
        t.gates[0].res = t.gates[2].t == t.gates[0].res ? t.gates[1].res : t.gates[0].res;   // two gates of level 0 writing one slot, or:
        t.gates[1].res = t.gates[0].res;
        CHECK(!bdd_check(t, &err), "two writers of one slot in a level went unnoticed");
        t = s; t.gates[2].t = (uint32_t)t.slots;
        CHECK(!bdd_check(t, &err), "a slot out of range went unnoticed");
        t = s; std::swap(t.gates[0], t.gates[2]); t.gates[2].res = s.gates[0].res; t.gates[0].res = s.gates[2].res;
        CHECK(!bdd_check(t, &err), "a read of an unwritten slot went unnoticed");
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all schedule checks passed\n");
    return 0;
}
