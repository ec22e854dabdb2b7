// pack_levels.cpp — the level map of FheUint::pack (pack_levels.hpp).  Plain C++, no HIP.
#include "pack_levels.hpp"

#include <cstdio>

namespace pz {

static bool bad(std::string* err, const char* fmt, size_t a = 0, size_t b = 0, size_t c = 0) {
    if (err) {
        char buf[200];
        std::snprintf(buf, sizeof buf, fmt, a, b, c);
        *err = buf;
    }
    return false;
}

bool fhe_uint_pack_levels(size_t n, size_t word_bits, std::vector<PackLevel>* out, std::string* err) {
    out->clear();
    if (word_bits != 8 && word_bits != 16 && word_bits != 32 && word_bits != 64 && word_bits != 128)
        return bad(err, "fhe_uint_pack: word_bits %zu is not one of 8, 16, 32, 64, 128", word_bits);
    if (n == 0 || (n & (n - 1)) != 0 || n % word_bits != 0) return bad(err, "fhe_uint_pack: n %zu is no power of two that word_bits %zu divides", n, word_bits);
    uint32_t log_bytes = 0;
    while (((size_t)8 << log_bytes) < word_bits) ++log_bytes;
    const size_t gap = n / word_bits;
    // index q << log_gap is occupied for every q < word_bits; level i pairs index j with j + t, t = n >> (i + 1), for j < t: of the occupied
    // ones q with q + h, h = word_bits >> (i + 1), for q < h - both present, the survivor stays at q
    for (size_t h = word_bits / 2; h >= 1; h /= 2) {
        PackLevel lv;
        lv.t = (uint32_t)(h * gap);
        for (size_t q = 0; q < h; ++q) {
            lv.lo.push_back((uint8_t)fhe_uint_slot_of_index((uint32_t)q, log_bytes));
            lv.hi.push_back((uint8_t)fhe_uint_slot_of_index((uint32_t)(q + h), log_bytes));
        }
        out->push_back(lv);
    }
    return true;
}

bool fhe_uint_pack_check(size_t n, size_t word_bits, const std::vector<PackLevel>& levels, std::string* err) {
    std::vector<uint8_t> live(word_bits, 1);   // slots that hold a ciphertext in front of the level
    size_t t = n / 2;
    for (size_t l = 0; l < levels.size(); ++l, t /= 2) {
        const PackLevel& lv = levels[l];
        if (lv.t != t) return bad(err, "fhe_uint_pack: level %zu turns by %zu, not %zu", l, lv.t, t);
        if (lv.lo.size() != lv.hi.size() || lv.pairs() == 0 || lv.pairs() > kPackMaxPairs) return bad(err, "fhe_uint_pack: level %zu has %zu pairs", l, lv.pairs());
        std::vector<uint8_t> named(word_bits, 0);
        for (size_t k = 0; k < lv.pairs(); ++k)
            for (const size_t s : {(size_t)lv.lo[k], (size_t)lv.hi[k]}) {
                if (s >= word_bits) return bad(err, "fhe_uint_pack: level %zu pair %zu names slot %zu", l, k, s);
                if (named[s]) return bad(err, "fhe_uint_pack: level %zu names slot %zu twice (pair %zu)", l, s, k);
                if (!live[s]) return bad(err, "fhe_uint_pack: level %zu pair %zu reads slot %zu, which holds nothing", l, k, s);
                named[s] = 1;
            }
        size_t nlive = 0;
        for (size_t s = 0; s < word_bits; ++s) nlive += live[s];
        if (nlive != 2 * lv.pairs()) return bad(err, "fhe_uint_pack: level %zu merges %zu of %zu live slots", l, 2 * lv.pairs(), nlive);
        for (size_t k = 0; k < lv.pairs(); ++k) live[lv.hi[k]] = 0;
    }
    size_t nlive = 0;
    for (size_t s = 0; s < word_bits; ++s) nlive += live[s];
    if (levels.empty() || nlive != 1 || !live[0]) return bad(err, "fhe_uint_pack: the levels leave %zu slots, slot 0 among them: %zu", nlive, word_bits ? live[0] : 0);
    return true;
}

}  // namespace pz
