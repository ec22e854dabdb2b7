// Host-only check of the stage plan of the FheUint byte operations (poulpy_amd/csrc/word_ops.cpp): built with -fsanitize=address,undefined and
// run as a child process by tests/test_fhe_uint_bytes_host.py.  For every word width at every ring degree from word_bits to 2^16, every
// operation with every argument: the plan's traces are the traces of a walk of the reference's calls
// (poulpy-bin-fhe/src/bdd_arithmetic/ciphertexts/fhe_uint.rs:259-524) - same source, same exponent, same skip, sext's shared trace of the
// replicated sign once -, its closing steps turn back by the reference's rotations in its order, the stage counts are those of DESIGN.md
// 4.4i, the plan passes fhe_uint_word_plan_check, and damaged plans and bad arguments are refused.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../poulpy_amd/csrc/word_ops.hpp"

using namespace pz;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

// a trace: (source, version of the running word or 0, exponent, skip); sources as WordSrc
typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Trace;

struct Walk {
    size_t n, w;
    std::vector<Trace> traces;
    std::vector<uint32_t> closings;
    uint32_t c(uint32_t bit) const {   // mod.rs:97-99, fhe_uint.rs:384
        uint32_t log_bytes = 0;
        while (((size_t)8 << log_bytes) < w) ++log_bytes;
        return (uint32_t)((((bit & 7u) << log_bytes) | (bit >> 3)) * (n / w));
    }
    void zero_byte(uint32_t src, uint32_t ver, uint32_t byte) {   // :466-489
        traces.push_back(Trace{src, ver, c(byte << 3), 3});
        closings.push_back(c(byte << 3));
    }
    void splice_u8(uint32_t dst, uint32_t srcb, uint32_t a_src, uint32_t a_ver, uint32_t b_src) {   // :286-329
        zero_byte(a_src, a_ver, dst);
        traces.push_back(Trace{b_src, 0, c(srcb << 3), 3});
    }
};

static void compare(const char* what, size_t n, size_t w, uint32_t x, uint32_t y, const std::vector<WordStage>& plan, const Walk& walk, size_t want_stages,
                    size_t slots) {
    std::string err;
    CHECK(fhe_uint_word_plan_check(n, slots, plan, &err), "%s n %zu w %zu (%u, %u): %s", what, n, w, x, y, err.c_str());
    CHECK(plan.size() == want_stages, "%s n %zu w %zu (%u, %u): %zu stages, not %zu", what, n, w, x, y, plan.size(), want_stages);
    std::set<Trace> got, want(walk.traces.begin(), walk.traces.end());
    std::vector<uint32_t> closings;
    uint32_t combined = 0;
    size_t items = 0;
    for (const WordStage& st : plan) {
        for (const WordItem& it : st.items) {
            got.insert(Trace{it.src, it.src == WORD_SRC_RES ? combined : 0, it.exp, st.skip});
            ++items;
        }
        if (st.close == WORD_CLOSE_COMBINE) { closings.push_back(st.r); ++combined; }
    }
    CHECK(got == want, "%s n %zu w %zu (%u, %u): the plan's traces are not the walk's", what, n, w, x, y);
    CHECK(items == want.size(), "%s n %zu w %zu (%u, %u): %zu traced items for %zu distinct traces", what, n, w, x, y, items, want.size());
    CHECK(closings == walk.closings, "%s n %zu w %zu (%u, %u): the closing rotations differ", what, n, w, x, y);
}

int main() {
    const size_t words[] = {8, 16, 32, 64, 128};
    size_t shapes = 0, plans = 0;
    std::string err;
    for (size_t w : words)
        for (size_t n = w; n <= 65536; n *= 2) {
            const uint32_t bytes = (uint32_t)(w / 8);
            std::vector<WordStage> plan;
            // get: all bits, all bytes, in one stage each
            for (int unit = 0; unit < 2; ++unit) {
                std::vector<uint32_t> idx;
                Walk wk{n, w, {}, {}};
                for (uint32_t i = 0; i < (unit ? bytes : (uint32_t)w); ++i) {
                    idx.push_back(i);
                    wk.traces.push_back(Trace{WORD_SRC_A, 0, wk.c(unit ? i << 3 : i), unit ? 3u : 0u});
                }
                CHECK(fhe_uint_word_plan(n, w, unit ? WORD_GET_BYTE : WORD_GET_BIT, idx.data(), idx.size(), &plan, &err), "get refused: %s", err.c_str());
                compare("get", n, w, (uint32_t)unit, 0, plan, wk, 1, idx.size());
                for (size_t i = 0; i < plan[0].items.size(); ++i) CHECK(plan[0].items[i].slot == i, "get: item %zu at slot %u", i, plan[0].items[i].slot);
                CHECK(fhe_uint_word_coefficient(n, w, 0) == 0, "bit 0 is not at coefficient 0");
                ++plans;
            }
            for (uint32_t byte = 0; byte < bytes; ++byte) {
                Walk wk{n, w, {}, {}};
                wk.zero_byte(WORD_SRC_A, 0, byte);
                CHECK(fhe_uint_word_plan(n, w, WORD_ZERO_BYTE, &byte, 1, &plan, &err), "zero_byte refused: %s", err.c_str());
                compare("zero_byte", n, w, byte, 0, plan, wk, 1, kWordSlots);
                // sext :491-524
                Walk ws{n, w, {}, {}};
                ws.traces.push_back(Trace{WORD_SRC_RES, 0, ws.c((byte << 3) + 7), 0});
                for (uint32_t i = byte + 1, k = 0; i < bytes; ++i, ++k) ws.splice_u8(i, 0, WORD_SRC_RES, k, WORD_SRC_S);
                CHECK(fhe_uint_word_plan(n, w, WORD_SEXT, &byte, 1, &plan, &err), "sext refused: %s", err.c_str());
                const size_t k = bytes - 1 - byte;
                if (k == 0) CHECK(plan.empty(), "sext of the last byte has %zu stages", plan.size());
                else {
                    compare("sext", n, w, byte, 0, plan, ws, 1 + k, kWordSlots);
                    CHECK(ws.traces.size() == 1 + 2 * k, "the walk of sext has %zu traces", ws.traces.size());
                    CHECK(plan[0].close == WORD_CLOSE_REPLICATE, "sext does not replicate after its first stage");
                }
                plans += 2;
            }
            for (uint32_t dst = 0; dst < bytes; ++dst)
                for (uint32_t src = 0; src < bytes; ++src) {
                    const uint32_t args[2] = {dst, src};
                    Walk wk{n, w, {}, {}};
                    wk.splice_u8(dst, src, WORD_SRC_A, 0, WORD_SRC_B);
                    CHECK(fhe_uint_word_plan(n, w, WORD_SPLICE_U8, args, 2, &plan, &err), "splice_u8 refused: %s", err.c_str());
                    compare("splice_u8", n, w, dst, src, plan, wk, 1, kWordSlots);
                    CHECK(plan[0].plus == 1 && plan[0].minus == 0 && plan[0].base == WORD_SRC_A, "splice_u8 combines other slots");
                    ++plans;
                    if (dst < bytes / 2 && src < bytes / 2) {   // :259-282
                        Walk w16{n, w, {}, {}};
                        w16.splice_u8(dst << 1, src << 1, WORD_SRC_A, 0, WORD_SRC_B);
                        w16.splice_u8((dst << 1) + 1, (src << 1) + 1, WORD_SRC_RES, 1, WORD_SRC_B);
                        CHECK(fhe_uint_word_plan(n, w, WORD_SPLICE_U16, args, 2, &plan, &err), "splice_u16 refused: %s", err.c_str());
                        compare("splice_u16", n, w, dst, src, plan, w16, 2, kWordSlots);
                        // b is consumed by the first stage: res may be b
                        for (const WordItem& it : plan[1].items) CHECK(it.src == WORD_SRC_RES, "splice_u16 reads b in its second stage");
                        ++plans;
                    } else {
                        CHECK(!fhe_uint_word_plan(n, w, WORD_SPLICE_U16, args, 2, &plan, &err), "splice_u16 (%u, %u) of %zu bits accepted", dst, src, w);
                    }
                }
            // damaged plans are caught
            const uint32_t a01[2] = {0, bytes - 1};
            if (bytes >= 2) {
                CHECK(fhe_uint_word_plan(n, w, WORD_SPLICE_U8, a01, 2, &plan, &err), "splice_u8 refused");
                std::vector<WordStage> bad = plan;
                bad[0].items[1].exp = (uint32_t)n;
                CHECK(!fhe_uint_word_plan_check(n, kWordSlots, bad, &err), "an exponent of n passed the check");
                bad = plan;
                bad[0].items[1].slot = 3;
                CHECK(!fhe_uint_word_plan_check(n, kWordSlots, bad, &err), "items at slots apart passed the check");
                bad = plan;
                bad[0].plus = 4;
                CHECK(!fhe_uint_word_plan_check(n, kWordSlots, bad, &err), "a slot nothing traced passed the check");
                bad = plan;
                bad[0].items[0].src = WORD_SRC_S;
                CHECK(!fhe_uint_word_plan_check(n, kWordSlots, bad, &err), "s' read without a replicate passed the check");
                bad = plan;
                bad[0].items[0].slot = (uint32_t)kWordSlots - 1;
                bad[0].items[1].slot = (uint32_t)kWordSlots;
                CHECK(!fhe_uint_word_plan_check(n, kWordSlots, bad, &err), "a slot past tmp passed the check");
            }
            // arguments out of range
            const uint32_t big = bytes, bigbit = (uint32_t)w, pair_hi[2] = {0, bytes}, pair_lo[2] = {bytes, 0};
            CHECK(!fhe_uint_word_plan(n, w, WORD_ZERO_BYTE, &big, 1, &plan, &err) && !err.empty(), "zero_byte of byte %u accepted", big);
            CHECK(!fhe_uint_word_plan(n, w, WORD_SEXT, &big, 1, &plan, &err), "sext of byte %u accepted", big);
            CHECK(!fhe_uint_word_plan(n, w, WORD_GET_BYTE, &big, 1, &plan, &err), "get of byte %u accepted", big);
            CHECK(!fhe_uint_word_plan(n, w, WORD_GET_BIT, &bigbit, 1, &plan, &err), "get of bit %u accepted", bigbit);
            CHECK(!fhe_uint_word_plan(n, w, WORD_SPLICE_U8, pair_hi, 2, &plan, &err), "splice_u8 from byte %u accepted", bytes);
            CHECK(!fhe_uint_word_plan(n, w, WORD_SPLICE_U8, pair_lo, 2, &plan, &err), "splice_u8 into byte %u accepted", bytes);
            CHECK(!fhe_uint_word_plan(n, w, 6, &big, 1, &plan, &err), "operation 6 accepted");
            std::vector<uint32_t> many(kWordMaxItems + 1, 0);
            CHECK(!fhe_uint_word_plan(n, w, WORD_GET_BIT, many.data(), many.size(), &plan, &err), "a get of 129 bits accepted");
            CHECK(fhe_uint_word_plan(n, w, WORD_GET_BIT, nullptr, 0, &plan, &err) && plan.empty(), "a get of nothing is not the empty plan");
            ++shapes;
        }
    std::vector<WordStage> plan;
    const uint32_t zero = 0;
    for (size_t w : {(size_t)0, (size_t)4, (size_t)12, (size_t)24, (size_t)256}) CHECK(!fhe_uint_word_plan(1024, w, WORD_ZERO_BYTE, &zero, 1, &plan, &err) && !err.empty(), "word_bits %zu accepted", w);
    CHECK(!fhe_uint_word_plan(64, 128, WORD_ZERO_BYTE, &zero, 1, &plan, &err), "n 64 with 128-bit words accepted");
    CHECK(!fhe_uint_word_plan(96, 32, WORD_ZERO_BYTE, &zero, 1, &plan, &err), "n 96 accepted");
    CHECK(!fhe_uint_word_plan(0, 8, WORD_ZERO_BYTE, &zero, 1, &plan, &err), "n 0 accepted");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("all word plan checks passed: %zu shapes, %zu plans\n", shapes, plans);
    return 0;
}
