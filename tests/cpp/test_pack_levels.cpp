// Host-only check of the level map of FheUint::pack (poulpy_amd/csrc/pack_levels.cpp): built with -fsanitize=address,undefined and run as a
// child process by tests/test_fhe_uint_pack_host.py.  Every (n, word_bits) is compared with a walk of glwe_pack_default's loop
// (poulpy-core/src/glwe_packing.rs:147-168) over the occupied indices bit_index(s) << log_gap, the tables are re-checked (fhe_uint_pack_check),
// and damaged tables and bad shapes must be refused.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../poulpy_amd/csrc/pack_levels.hpp"

using namespace pz;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

struct Merge { uint32_t lo, hi, t; };

// the reference's loop on {index: slot}; *both_only: it met the both-present branch of pack_internal alone
static std::vector<std::vector<Merge>> walk(size_t n, size_t word_bits, bool* both_only, size_t* last) {
    size_t log_n = 0, log_bytes = 0;
    while (((size_t)1 << log_n) < n) ++log_n;
    while (((size_t)8 << log_bytes) < word_bits) ++log_bytes;
    size_t log_gap = 0;
    while ((word_bits << log_gap) < n) ++log_gap;
    std::map<size_t, uint32_t> a;
    for (uint32_t s = 0; s < word_bits; ++s) a[(size_t)fhe_uint_bit_index(s, (uint32_t)log_bytes) << log_gap] = s;
    *both_only = a.size() == word_bits;
    std::vector<std::vector<Merge>> levels;
    for (size_t i = 0; i + log_gap < log_n; ++i) {
        const size_t t = (size_t)1 << (log_n - 1 - i);
        std::vector<Merge> merges;
        for (size_t j = 0; j < t; ++j) {
            const auto lo = a.find(j), hi = a.find(j + t);
            const bool has_lo = lo != a.end(), has_hi = hi != a.end();
            if (has_lo && has_hi) merges.push_back(Merge{lo->second, hi->second, (uint32_t)t});
            else if (has_lo || has_hi) *both_only = false;
            if (!has_lo && has_hi) a[j] = hi->second;
            if (has_hi) a.erase(j + t);
        }
        levels.push_back(merges);
    }
    *last = a.size() == 1 && a.count(0) ? a[0] : (size_t)-1;
    return levels;
}

int main() {
    const size_t words[] = {8, 16, 32, 64, 128};
    size_t shapes = 0;
    for (size_t w : words)
        for (size_t n = w; n <= 65536; n *= 2) {
            std::vector<PackLevel> lv;
            std::string err;
            CHECK(fhe_uint_pack_levels(n, w, &lv, &err), "n %zu word_bits %zu refused: %s", n, w, err.c_str());
            CHECK(fhe_uint_pack_check(n, w, lv, &err), "n %zu word_bits %zu: %s", n, w, err.c_str());
            bool both_only = false;
            size_t last = 0;
            const auto want = walk(n, w, &both_only, &last);
            CHECK(both_only, "n %zu word_bits %zu: the walk met another branch of pack_internal", n, w);
            CHECK(last == 0, "n %zu word_bits %zu: the trace would read slot %zu", n, w, last);
            CHECK(want.size() == lv.size(), "n %zu word_bits %zu: %zu levels, the walk has %zu", n, w, lv.size(), want.size());
            for (size_t l = 0; l < lv.size() && l < want.size(); ++l) {
                CHECK(lv[l].pairs() == want[l].size() && lv[l].pairs() <= kPackMaxPairs, "n %zu word_bits %zu level %zu: %zu pairs, the walk has %zu", n, w, l, lv[l].pairs(), want[l].size());
                for (size_t k = 0; k < lv[l].pairs() && k < want[l].size(); ++k)
                    CHECK(lv[l].lo[k] == want[l][k].lo && lv[l].hi[k] == want[l][k].hi && lv[l].t == want[l][k].t, "n %zu word_bits %zu level %zu pair %zu: (%u, %u, %u), the walk has (%u, %u, %u)",
                          n, w, l, k, (unsigned)lv[l].lo[k], (unsigned)lv[l].hi[k], lv[l].t, want[l][k].lo, want[l][k].hi, want[l][k].t);
            }
            // the inverse of bit_index
            uint32_t log_bytes = 0;
            while (((size_t)8 << log_bytes) < w) ++log_bytes;
            for (uint32_t s = 0; s < w; ++s) CHECK(fhe_uint_slot_of_index(fhe_uint_bit_index(s, log_bytes), log_bytes) == s, "word_bits %zu: slot %u", w, s);
            // damaged tables are caught
            if (!lv.empty()) {
                std::vector<PackLevel> bad = lv;
                bad[0].lo[0] = bad[0].hi[0];
                CHECK(!fhe_uint_pack_check(n, w, bad, &err), "a slot named twice passed the check");
                bad = lv;
                bad.back().lo[0] = bad.back().hi[0];
                bad.back().hi[0] = 0;
                CHECK(!fhe_uint_pack_check(n, w, bad, &err), "a last survivor other than slot 0 passed the check");
                bad = lv;
                bad[0].t += 1;
                CHECK(!fhe_uint_pack_check(n, w, bad, &err), "a wrong rotation passed the check");
                bad = lv;
                bad[0].hi[0] = (uint8_t)w;
                CHECK(!fhe_uint_pack_check(n, w, bad, &err), "a slot out of range passed the check");
            }
            ++shapes;
        }
    std::vector<PackLevel> lv;
    std::string err;
    for (size_t w : {(size_t)0, (size_t)4, (size_t)12, (size_t)24, (size_t)256}) CHECK(!fhe_uint_pack_levels(1024, w, &lv, &err) && !err.empty(), "word_bits %zu accepted", w);
    CHECK(!fhe_uint_pack_levels(64, 128, &lv, &err), "n 64 with 128-bit words accepted");
    CHECK(!fhe_uint_pack_levels(96, 32, &lv, &err), "n 96 accepted");
    CHECK(!fhe_uint_pack_levels(0, 8, &lv, &err), "n 0 accepted");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("all pack level checks passed: %zu shapes\n", shapes);
    return 0;
}
