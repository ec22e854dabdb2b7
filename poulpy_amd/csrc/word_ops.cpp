// word_ops.cpp — the stage plan of the FheUint byte operations (word_ops.hpp).  Plain C++, no HIP.
#include "word_ops.hpp"

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

static WordStage combine(uint32_t base, std::vector<WordItem> items, uint32_t plus, uint32_t minus, uint32_t r) {
    WordStage st;
    st.skip = 3;   // LOG_BITS - LOG_BYTES
    st.items = std::move(items);
    st.close = WORD_CLOSE_COMBINE;
    st.base = base; st.plus = plus; st.minus = minus; st.r = r;
    return st;
}

bool fhe_uint_word_plan(size_t n, size_t word_bits, uint32_t op, const uint32_t* args, size_t nargs, std::vector<WordStage>* out, std::string* err) {
    out->clear();
    if (word_bits != 8 && word_bits != 16 && word_bits != 32 && word_bits != 64 && word_bits != 128)
        return bad(err, "fhe_uint_word: word_bits %zu is not one of 8, 16, 32, 64, 128", word_bits);
    if (n == 0 || (n & (n - 1)) != 0 || n % word_bits != 0) return bad(err, "fhe_uint_word: n %zu is no power of two that word_bits %zu divides", n, word_bits);
    if (nargs != 0 && args == nullptr) return bad(err, "fhe_uint_word: null arguments");
    const uint32_t bytes = (uint32_t)(word_bits / 8);
    auto c = [&](uint32_t bit) { return fhe_uint_word_coefficient(n, word_bits, bit); };
    switch (op) {
    case WORD_GET_BIT:
    case WORD_GET_BYTE: {
        const bool bit = op == WORD_GET_BIT;
        if (nargs > kWordMaxItems) return bad(err, "fhe_uint_get: %zu indices, at most %zu", nargs, kWordMaxItems);
        if (nargs == 0) return true;
        WordStage st;
        st.skip = bit ? 0 : 3;
        for (size_t i = 0; i < nargs; ++i) {
            if (args[i] >= (bit ? (uint32_t)word_bits : bytes))
                return bad(err, bit ? "fhe_uint_get: bit %zu of a word of %zu bits" : "fhe_uint_get: byte %zu of a word of %zu bits", args[i], word_bits);
            st.items.push_back({WORD_SRC_A, c(bit ? args[i] : 8 * args[i]), (uint32_t)i});
        }
        out->push_back(st);
        return true;
    }
    case WORD_ZERO_BYTE: {
        if (nargs != 1) return bad(err, "fhe_uint_zero_byte: one argument, the byte");
        if (args[0] >= bytes) return bad(err, "fhe_uint_zero_byte: byte %zu of a word of %zu bits", args[0], word_bits);
        const uint32_t r = c(8 * args[0]);
        out->push_back(combine(WORD_SRC_A, {{WORD_SRC_A, r, 0}}, kWordNone, 0, r));
        return true;
    }
    case WORD_SPLICE_U8: {
        if (nargs != 2) return bad(err, "fhe_uint_splice: two arguments, dst and src");
        if (args[0] >= bytes || args[1] >= bytes) return bad(err, "fhe_uint_splice: u8 dst %zu / src %zu of a word of %zu bits", args[0], args[1], word_bits);
        const uint32_t rd = c(8 * args[0]), rs = c(8 * args[1]);
        out->push_back(combine(WORD_SRC_A, {{WORD_SRC_A, rd, 0}, {WORD_SRC_B, rs, 1}}, 1, 0, rd));
        return true;
    }
    case WORD_SPLICE_U16: {
        if (nargs != 2) return bad(err, "fhe_uint_splice: two arguments, dst and src");
        if (args[0] >= bytes / 2 || args[1] >= bytes / 2) return bad(err, "fhe_uint_splice: u16 dst %zu / src %zu of a word of %zu bits", args[0], args[1], word_bits);
        // tmp = splice_u8(2 dst, 2 src, a, b); res = splice_u8(2 dst + 1, 2 src + 1, tmp, b): both traces of b belong to the first stage (b is
        // consumed there: res may be b), the trace of tmp must see tmp as written
        const uint32_t rd0 = c(16 * args[0]), rd1 = c(16 * args[0] + 8), rs0 = c(16 * args[1]), rs1 = c(16 * args[1] + 8);
        out->push_back(combine(WORD_SRC_A, {{WORD_SRC_A, rd0, 0}, {WORD_SRC_B, rs0, 1}, {WORD_SRC_B, rs1, 2}}, 1, 0, rd0));
        out->push_back(combine(WORD_SRC_RES, {{WORD_SRC_RES, rd1, 0}}, 2, 0, rd1));
        return true;
    }
    case WORD_SEXT: {
        if (nargs != 1) return bad(err, "fhe_uint_sext: one argument, the byte");
        if (args[0] >= bytes) return bad(err, "fhe_uint_sext: byte %zu of a word of %zu bits", args[0], word_bits);
        const uint32_t byte = args[0];
        if (byte + 1 == bytes) return true;   // the reference's loop is empty and the word unchanged
        WordStage msb;   // s = trace_0(X^-c(8 byte + 7) word) in slot 0, s' in slot 1
        msb.skip = 0;
        msb.items.push_back({WORD_SRC_RES, c(8 * byte + 7), 0});
        msb.close = WORD_CLOSE_REPLICATE;
        out->push_back(msb);
        // splice_u8(i, 0, word, s'): trace_ts(s') is the same for every i - slot 2, traced once beside the first byte's own trace (slot 3)
        for (uint32_t i = byte + 1; i < bytes; ++i) {
            const uint32_t r = c(8 * i);
            if (i == byte + 1) out->push_back(combine(WORD_SRC_RES, {{WORD_SRC_S, 0, 2}, {WORD_SRC_RES, r, 3}}, 2, 3, r));
            else out->push_back(combine(WORD_SRC_RES, {{WORD_SRC_RES, r, 3}}, 2, 3, r));
        }
        return true;
    }
    default:
        return bad(err, "fhe_uint_word: unknown operation %zu", op);
    }
}

bool fhe_uint_word_plan_check(size_t n, size_t slots, const std::vector<WordStage>& plan, std::string* err) {
    std::vector<uint8_t> written(slots, 0);
    bool have_s = false;
    for (size_t s = 0; s < plan.size(); ++s) {
        const WordStage& st = plan[s];
        if (st.items.empty() || st.items.size() > kWordMaxItems) return bad(err, "fhe_uint_word: stage %zu has %zu items", s, st.items.size());
        if (st.skip != 0 && st.skip != 3) return bad(err, "fhe_uint_word: stage %zu skips %zu steps", s, st.skip);
        for (size_t i = 0; i < st.items.size(); ++i) {
            const WordItem& it = st.items[i];
            if (it.exp >= n) return bad(err, "fhe_uint_word: stage %zu item %zu turns by %zu", s, i, it.exp);
            if (it.slot >= slots || it.slot != st.items[0].slot + i) return bad(err, "fhe_uint_word: stage %zu item %zu at slot %zu", s, i, it.slot);
            if (it.src > WORD_SRC_S) return bad(err, "fhe_uint_word: stage %zu item %zu reads source %zu", s, i, it.src);
            if (it.src == WORD_SRC_S && (!have_s || it.slot == 1)) return bad(err, "fhe_uint_word: stage %zu item %zu reads s' before it exists, or into itself", s, i);
        }
        for (const WordItem& it : st.items) {
            if (have_s && it.slot == 1) return bad(err, "fhe_uint_word: stage %zu overwrites s'", s);
            written[it.slot] = 1;
        }
        if (st.close == WORD_CLOSE_NONE) {
            if (plan.size() != 1) return bad(err, "fhe_uint_word: stage %zu ends in nothing and is not alone", s);
        } else if (st.close == WORD_CLOSE_REPLICATE) {
            if (slots < 2 || st.items.size() != 1 || st.items[0].slot != 0) return bad(err, "fhe_uint_word: stage %zu replicates from another slot than 0", s);
            have_s = true;
            written[1] = 1;
        } else if (st.close == WORD_CLOSE_COMBINE) {
            if (st.r >= n) return bad(err, "fhe_uint_word: stage %zu turns back by %zu", s, st.r);
            if (st.base != WORD_SRC_A && st.base != WORD_SRC_RES) return bad(err, "fhe_uint_word: stage %zu adds to source %zu", s, st.base);
            if (st.plus == kWordNone && st.minus == kWordNone) return bad(err, "fhe_uint_word: stage %zu combines nothing", s);
            for (const uint32_t t : {st.plus, st.minus})
                if (t != kWordNone && (t >= slots || !written[t] || (have_s && t == 1))) return bad(err, "fhe_uint_word: stage %zu combines slot %zu, which holds no trace", s, t);
        } else {
            return bad(err, "fhe_uint_word: stage %zu closes with %zu", s, st.close);
        }
    }
    return true;
}

std::vector<uint32_t> fhe_uint_word_plan_words(const std::vector<WordStage>& plan) {
    std::vector<uint32_t> w;
    for (const WordStage& st : plan) {
        w.push_back(st.skip);
        w.push_back((uint32_t)st.items.size());
        for (const WordItem& it : st.items) { w.push_back(it.src); w.push_back(it.exp); w.push_back(it.slot); }
        w.push_back(st.close); w.push_back(st.base); w.push_back(st.plus); w.push_back(st.minus); w.push_back(st.r);
    }
    return w;
}

}  // namespace pz
