// api_fhe_uint.hip — FheUint words behind the C ABI: pack by levels and per pair, the evaluator followed by the pack in one call
// (pz_fhe_uint_execute_*), the byte operations (get, zero_byte, splice, sext) and the small host queries around them.  poulpy-bin-fhe
// bdd_arithmetic/ciphertexts/fhe_uint.rs:239-524, bdd_2w_to_1w.rs:103-136, bdd_1w_to_1w.rs:46-70; the level map and the stage plans are
// host code (pack_levels.cpp, word_ops.cpp).  DESIGN.md 4.4h, 4.4i.  (Preparing words from GLWE bits is api_lwe.hip.)
#include <algorithm>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "glwe_call.hpp"
#include "pack_levels.hpp"
#include "word_ops.hpp"

using namespace pz;

extern "C" {
// ------------------------------------------------------------------------------
// public: FheUint::pack (bdd_arithmetic/ciphertexts/fhe_uint.rs:239-255) on `batch` words.  All word_bits indices are occupied,
// so glwe_pack's tree has log2(word_bits) levels of both-present merges (pack_levels.cpp) and a trace of log_gap steps.  By levels: every
// level is k_pack_pre, ONE automorphism call on pairs * batch half-differences, k_pack_post.  tmp = [diff: word_bits / 2 slots][trace
// temporary in the keys' base].  Per pair (POULPY_DBG_PACK_LEVELS=0): glwe_pack (api_trace.hip), on the first three slots' worth of tmp.
// ------------------------------------------------------------------------------
size_t pz_fhe_uint_pack_tmp_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t word_bits, size_t trace_size, size_t batch) {
    if (!M || !p) return 0;
    const size_t ctb = batch * (size_t)M->n * (p->rank + 1) * p->res_size * 8;
    const size_t by_levels = align256(word_bits / 2 * ctb) + align256(batch * (size_t)M->n * (p->rank + 1) * trace_size * 8);
    return std::max(by_levels, pz_glwe_pack_bases_tmp_bytes(M, p, trace_size, batch));
}
size_t pz_fhe_uint_pack_level_pairs(size_t n, size_t word_bits, size_t level, uint32_t* pairs3, size_t cap) {
    std::vector<PackLevel> levels;
    if (!fhe_uint_pack_levels(n, word_bits, &levels, nullptr) || level >= levels.size()) return 0;
    const PackLevel& lv = levels[level];
    for (size_t k = 0; pairs3 && k < std::min(lv.pairs(), cap); ++k) { pairs3[3 * k] = lv.lo[k]; pairs3[3 * k + 1] = lv.hi[k]; pairs3[3 * k + 2] = lv.t; }
    return lv.pairs();
}
// every refusal of pz_fhe_uint_pack_batched, before anything is launched; *levels: the level map
static int fhe_uint_pack_refusals(pz_module* M, const int64_t* res, const int64_t* bits, size_t word_bits, const int64_t* gals, const double* const* key_pmats,
                               const pz_glwe_op_params* p, size_t trace_size, const void* tmp, size_t tmp_bytes, size_t batch,
                               std::vector<PackLevel>* levels) {
    PZ_REQUIRE(p != nullptr && gals != nullptr && key_pmats != nullptr, "fhe_uint_pack: null argument");
    PZ_REQUIRE(p->a_size == p->res_size && p->a_base2k == p->res_base2k && p->rank_out == p->rank && p->dsize == 1,
               "fhe_uint_pack: ciphertexts and result share base2k and size (dsize 1, rank_out = rank)");
    PZ_REQUIRE(p->res_size >= 1 && p->rank >= 1 && p->dnum >= 1 && p->key_size >= 1 && p->res_base2k >= 1 && p->res_base2k <= 62 && p->key_base2k >= 1,
               "fhe_uint_pack: empty shape");
    PZ_REQUIRE(p->res_base2k == p->key_base2k || trace_size >= 1, "fhe_uint_pack: keys in another base than the ciphertexts need trace_size >= 1");
    std::string err;
    if (!fhe_uint_pack_levels((size_t)M->n, word_bits, levels, &err) || !fhe_uint_pack_check((size_t)M->n, word_bits, *levels, &err))
        return fail(PZ_ERR_INVALID, "%s", err.c_str());
    PZ_REQUIRE(batch <= (1u << 24), "fhe_uint_pack: batch out of range");
    const TraceKeys tk{gals, key_pmats, log2_n(M)};
    PZ_TRY(trace_keys_check(tk, "fhe_uint_pack"));
    if (batch == 0) return PZ_OK;
    PZ_REQUIRE(res != nullptr && bits != nullptr && tmp != nullptr, "fhe_uint_pack: null argument");
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(bits) && is_device_ptr(tmp), "batched entry points take device pointers");
    const size_t need = pz_fhe_uint_pack_tmp_bytes(M, p, word_bits, p->res_base2k == p->key_base2k ? 0 : trace_size, batch);
    PZ_REQUIRE(tmp_bytes >= need, "fhe_uint_pack: tmp too small (%zu bytes, %zu needed)", tmp_bytes, need);
    const size_t cols = p->rank + 1, ctb = batch * (size_t)M->n * cols * p->res_size * 8, bits_bytes = word_bits * ctb;
    const size_t key_bytes = glwe_key_bytes(M, p);
    // (bits against tmp first: bits is the longest range - word_bits ciphertext batches - so a bits pointer that is really tmp reaches past tmp's
    // end into whatever the allocator put there, res included, and the refusal named whichever pair was tested first)
    if (ranges_overlap(bits, bits_bytes, tmp, need)) return fail(PZ_ERR_ALIAS, "fhe_uint_pack: bits overlaps tmp");
    if (ranges_overlap(res, ctb, bits, bits_bytes)) return fail(PZ_ERR_ALIAS, "fhe_uint_pack: res overlaps bits");
    if (ranges_overlap(res, ctb, tmp, need)) return fail(PZ_ERR_ALIAS, "fhe_uint_pack: res overlaps tmp");
    const size_t hit = std::min({trace_keys_overlap(tk, key_bytes, res, ctb), trace_keys_overlap(tk, key_bytes, bits, bits_bytes),
                                 trace_keys_overlap(tk, key_bytes, tmp, need)});
    if (hit < tk.nsteps) return fail(PZ_ERR_ALIAS, "fhe_uint_pack: the key of trace step %zu overlaps res, bits or tmp", hit);
    return PZ_OK;
}
// the checked call on the stream (no lock, no graph); batch >= 1
static int fhe_uint_pack_levels_run(pz_module* M, int64_t* res, int64_t* bits, const std::vector<PackLevel>& levels, const int64_t* gals,
                                    const double* const* key_pmats, const pz_glwe_op_params* p, size_t trace_size, void* tmp, size_t batch) {
    const long long n = (long long)M->n;
    const int cols = (int)p->rank + 1, size = (int)p->res_size, k = (int)p->res_base2k, B = (int)batch;
    const long long ct = n * cols * size;
    const size_t word_bits = 2 * levels[0].pairs();
    int64_t* diff = (int64_t*)tmp;
    dispatch_note(M, "fhe_uint_pack: by levels (k_pack_pre, one automorphism of pairs x batch, k_pack_post per level)");
    for (size_t l = 0; l < levels.size(); ++l) {
        const PackLevel& lv = levels[l];
        PackLevelCall pc;
        pc.bits = (long long*)bits; pc.diff = (long long*)diff;
        // the last survivor (slot 0) goes straight to res when the trace runs there (glwe_copy, glwe_packing.rs:175)
        pc.dst = (l + 1 == levels.size() && trace_size == 0) ? (long long*)res : (long long*)bits;
        pc.cols = cols; pc.size = size; pc.base2k = k; pc.batch = B; pc.pairs = (int)lv.pairs(); pc.t = lv.t;
        pc.lo = lv.lo.data(); pc.hi = lv.hi.data();
        PZ_TRY(launch_pack_level(M, false, pc));
        AutoSpec au{(long long)gals[l], 0};
        PZ_TRY(glwe_op(M, GlweKind::Automorphism, diff, diff, key_pmats[l], p, lv.pairs() * batch, &au));
        PZ_TRY(launch_pack_level(M, true, pc));
    }
    const size_t skip = levels.size(), log_n = log2_n(M);
    if (trace_size == 0) return glwe_trace(M, res, log_n - skip, gals + skip, key_pmats + skip, p, batch);
    // glwe_trace on a temporary of trace_size limbs in the keys' base (glwe_trace.rs:91-127), as glwe_pack does
    int64_t* tr = (int64_t*)((char*)tmp + align256(word_bits / 2 * (size_t)B * (size_t)ct * 8));
    return trace_in_key_base(M, res, bits, tr, trace_size, log_n - skip, gals + skip, key_pmats + skip, p, batch);
}
static int fhe_uint_pack_per_pair(pz_module* M, int64_t* res, int64_t* bits, size_t word_bits, const int64_t* gals, const double* const* key_pmats,
                                  const pz_glwe_op_params* p, size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch, const char* why) {
    dispatch_note(M, "fhe_uint_pack: per pair (%s)", why);
    size_t log_bytes = 0, log_gap = 0;
    while (((size_t)8 << log_bytes) < word_bits) ++log_bytes;
    while ((word_bits << log_gap) < (size_t)M->n) ++log_gap;
    const size_t ct = (size_t)M->n * (p->rank + 1) * p->res_size;
    std::vector<uint64_t> indices(word_bits);
    std::vector<int64_t*> cts(word_bits);
    for (size_t s = 0; s < word_bits; ++s) { indices[s] = (uint64_t)fhe_uint_bit_index((uint32_t)s, (uint32_t)log_bytes) << log_gap; cts[s] = bits + s * batch * ct; }
    return glwe_pack(M, res, word_bits, indices.data(), cts.data(), log_gap, gals, key_pmats, p, tmp, tmp_bytes, batch, trace_size);
}
// both routes for a caller that holds the module lock and has run fhe_uint_pack_refusals; the level route replays as a graph
static int fhe_uint_pack(pz_module* M, int64_t* res, int64_t* bits, size_t word_bits, const std::vector<PackLevel>& levels, const int64_t* gals,
                         const double* const* key_pmats, const pz_glwe_op_params* p, size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch) {
    if (batch == 0) return PZ_OK;
    if (p->res_base2k == p->key_base2k) trace_size = 0;
    if (rt_knob("POULPY_DBG_PACK_LEVELS", 1) == 0)   // (read per call: tests flip it)
        return fhe_uint_pack_per_pair(M, res, bits, word_bits, gals, key_pmats, p, trace_size, tmp, tmp_bytes, batch, "POULPY_DBG_PACK_LEVELS=0");
    KeyHash k = graph_key(M, GRAPH_FHE_UINT_PACK, res, bits, word_bits, tmp, batch, trace_size, *p);
    for (size_t s = 0, log_n = log2_n(M); s < log_n; ++s) { k.add(gals[s]); k.add(key_pmats[s]); }
    return with_graph(M, k.h, [&]() { return fhe_uint_pack_levels_run(M, res, bits, levels, gals, key_pmats, p, trace_size, tmp, batch); });
}
int pz_fhe_uint_pack_batched(pz_module* M, int64_t* res, int64_t* bits, size_t word_bits, const int64_t* gals, const double* const* key_pmats,
                             const pz_glwe_op_params* p, size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    std::vector<PackLevel> levels;
    PZ_TRY(fhe_uint_pack_refusals(M, res, bits, word_bits, gals, key_pmats, p, trace_size, tmp, tmp_bytes, batch, &levels));
    return fhe_uint_pack(M, res, bits, word_bits, levels, gals, key_pmats, p, trace_size, tmp, tmp_bytes, batch);
}

// ------------------------------------------------------------------------------
// public: execute_bdd_circuit_2w_to_1w / _1w_to_1w (bdd_2w_to_1w.rs:103-136, bdd_1w_to_1w.rs:46-70): the evaluator into the slot buffer at the
// head of tmp, then the pack above into res, both behind every refusal of either.  tmp = [slot buffer][max(evaluator, pack)] (:70-74).
// The halves keep their own graphs (the evaluator's gathered route writes the call's keys to tmp outside its graph).
// ------------------------------------------------------------------------------
size_t pz_fhe_uint_execute_tmp_bytes(const pz_module* M, const pz_bdd_circuit* c, const pz_glwe_op_params* gate_p, const pz_glwe_op_params* pack_p,
                                     size_t word_bits, size_t trace_size, size_t batch) {
    if (!M || !c || !gate_p || !pack_p) return 0;
    const size_t slots = align256(word_bits * batch * (size_t)M->n * (gate_p->rank + 1) * gate_p->res_size * 8);
    return slots + std::max(align256(pz_bdd_circuit_execute_tmp_bytes(M, c, gate_p, batch)), pz_fhe_uint_pack_tmp_bytes(M, pack_p, word_bits, trace_size, batch));
}
int pz_fhe_uint_execute_batched(pz_module* M, const pz_bdd_circuit* c, int64_t* res, size_t word_bits, const double* const* bits, size_t nbits,
                                const pz_glwe_op_params* gate_p, const int64_t* gals, const double* const* atk_pmats, const pz_glwe_op_params* pack_p,
                                size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_REQUIRE(gate_p != nullptr && pack_p != nullptr && c != nullptr, "fhe_uint_execute: null argument");
    PZ_REQUIRE(gate_p->res_size == pack_p->res_size && gate_p->res_base2k == pack_p->res_base2k && gate_p->rank == pack_p->rank,
               "fhe_uint_execute: the evaluator's result is the pack's ciphertext (res_size, res_base2k, rank of gate_p and pack_p)");
    PZ_REQUIRE(pz_bdd_circuit_output_size(c) <= word_bits, "fhe_uint_execute: output_size %zu > word_bits %zu", pz_bdd_circuit_output_size(c), word_bits);
    PZ_REQUIRE(batch == 0 || tmp != nullptr, "fhe_uint_execute: null argument");
    bool nothing = false;
    PZ_TRY(bdd_circuit_execute_precheck(M, c, (const int64_t*)tmp, word_bits, bits, nbits, gate_p, batch, &nothing));
    PZ_ENTER(M);
    const size_t slot_bytes = align256(word_bits * batch * (size_t)M->n * (gate_p->rank + 1) * gate_p->res_size * 8);
    const size_t need = pz_fhe_uint_execute_tmp_bytes(M, c, gate_p, pack_p, word_bits, trace_size, batch);
    PZ_REQUIRE(tmp_bytes >= need, "fhe_uint_execute: tmp too small (%zu bytes, %zu needed)", tmp_bytes, need);
    int64_t* slots = (int64_t*)tmp;
    void* rest = (char*)tmp + slot_bytes;
    std::vector<PackLevel> levels;
    PZ_TRY(fhe_uint_pack_refusals(M, res, slots, word_bits, gals, atk_pmats, pack_p, trace_size, rest, tmp_bytes - slot_bytes, batch, &levels));
    if (batch == 0 || nothing) return PZ_OK;
    PZ_TRY(bdd_circuit_execute(M, c, slots, word_bits, bits, nbits, gate_p, rest, tmp_bytes - slot_bytes, batch));
    PZ_TRY(fhe_uint_pack(M, res, slots, word_bits, levels, gals, atk_pmats, pack_p, trace_size, rest, tmp_bytes - slot_bytes, batch));
    return finish_call(M, false);
}

// ------------------------------------------------------------------------------
// public: the FheUint byte operations (bdd_arithmetic/ciphertexts/fhe_uint.rs:259-524): get_bit_glwe / get_byte, zero_byte,
// splice_u8 / splice_u16 and sext on `batch` words.  By stages (word_ops.cpp): every stage is k_word_pre (the rotated items into a dense array
// [item][batch], with the first one-bit shift of the trace where the word is in the keys' base), ONE glwe_trace on items * batch ciphertexts,
// and a closing k_word_post / k_word_replicate.  tmp = kWordSlots ciphertext arrays [batch].  Literal (POULPY_DBG_WORD_STAGES=0): the
// reference's calls in its order - one rotation launch, one glwe_trace per trace, launch_ew adds and subs.
// ------------------------------------------------------------------------------
size_t pz_fhe_uint_bit_coefficient(size_t n, size_t word_bits, size_t bit) {
    if ((word_bits != 8 && word_bits != 16 && word_bits != 32 && word_bits != 64 && word_bits != 128) || n == 0 || (n & (n - 1)) != 0 || n % word_bits != 0 ||
        bit >= word_bits)
        return (size_t)-1;
    return fhe_uint_word_coefficient(n, word_bits, (uint32_t)bit);
}
size_t pz_fhe_uint_word_plan(size_t n, size_t word_bits, uint32_t op, const uint32_t* args, size_t nargs, uint32_t* words, size_t cap, int* status) {
    std::vector<WordStage> plan;
    std::string err;
    const bool ok = fhe_uint_word_plan(n, word_bits, op, args, nargs, &plan, &err) &&
                    fhe_uint_word_plan_check(n, op <= WORD_GET_BYTE ? std::max<size_t>(nargs, 1) : kWordSlots, plan, &err);
    if (status) *status = ok ? PZ_OK : PZ_ERR_INVALID;
    if (!ok) { fail(PZ_ERR_INVALID, "%s", err.c_str()); return 0; }
    const std::vector<uint32_t> w = fhe_uint_word_plan_words(plan);
    for (size_t i = 0; words && i < std::min(w.size(), cap); ++i) words[i] = w[i];
    return w.size();
}
size_t pz_fhe_uint_word_op_tmp_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t word_bits, size_t max_items, size_t batch) {
    if (!M || !p || max_items > kWordMaxItems) return 0;
    if (word_bits != 8 && word_bits != 16 && word_bits != 32 && word_bits != 64 && word_bits != 128) return 0;
    // (a get traces its items in res itself: whatever max_items, the six arrays of the other operations)
    return align256(kWordSlots * batch * (size_t)M->n * (p->rank + 1) * p->res_size * 8);
}

namespace {
struct WordCall {
    pz_module* M;
    const char* what;
    int64_t* res;           // get: [nitems][batch]; else `batch` words
    const int64_t* a;       // get: the words; sext: the word itself (= res)
    const int64_t* b;       // splice only
    const int64_t* gals;
    const double* const* key_pmats;
    const pz_glwe_op_params* p;
    void* tmp;
    size_t tmp_bytes, batch, res_items;
    bool is_get;
};
}  // namespace
// every refusal of the four calls, after the plan's own and before anything is launched
static int fhe_uint_word_refusals(const WordCall& c, size_t word_bits) {
    pz_module* M = c.M;
    const pz_glwe_op_params* p = c.p;
    PZ_REQUIRE(p != nullptr && c.gals != nullptr && c.key_pmats != nullptr, "%s: null argument", c.what);
    PZ_REQUIRE(p->rank_out == p->rank && p->dsize == 1, "%s: dsize 1, rank_out = rank", c.what);
    PZ_REQUIRE(p->res_size >= 1 && p->rank >= 1 && p->dnum >= 1 && p->key_size >= 1 && p->res_base2k >= 1 && p->res_base2k <= 62 && p->key_base2k >= 1,
               "%s: empty shape", c.what);
    if (p->res_base2k == p->key_base2k)
        PZ_REQUIRE(p->a_size == p->res_size && p->a_base2k == p->res_base2k, "%s: a and res describe the same words when they are in the keys' base", c.what);
    else
        PZ_REQUIRE(p->a_base2k == p->key_base2k && p->a_size >= 1, "%s: with the words in another base than the keys, (a_size, a_base2k) is their layout in the keys' base", c.what);
    PZ_REQUIRE(c.batch <= (1u << 20), "%s: batch out of range", c.what);
    const TraceKeys tk{c.gals, c.key_pmats, log2_n(M)};
    PZ_TRY(trace_keys_check(tk, c.what));
    if (c.batch == 0 || c.res_items == 0) return PZ_OK;
    PZ_REQUIRE(c.res != nullptr && c.a != nullptr && c.tmp != nullptr, "%s: null argument", c.what);
    PZ_REQUIRE(is_device_ptr(c.res) && is_device_ptr(c.a) && is_device_ptr(c.tmp) && (c.b == nullptr || is_device_ptr(c.b)), "batched entry points take device pointers");
    const size_t need = pz_fhe_uint_word_op_tmp_bytes(M, p, word_bits, c.is_get ? c.res_items : 0, c.batch);
    PZ_REQUIRE(c.tmp_bytes >= need, "%s: tmp too small (%zu bytes, %zu needed)", c.what, c.tmp_bytes, need);
    const size_t cols = p->rank + 1, ctb = c.batch * (size_t)M->n * cols * p->res_size * 8, res_bytes = c.res_items * ctb;
    const size_t key_bytes = glwe_key_bytes(M, p);
    // res == a, res == b (whole) and a == b are allowed for everything but a get
    if (ranges_overlap(c.res, res_bytes, c.a, ctb) && (c.is_get || (const void*)c.res != (const void*)c.a)) return fail(PZ_ERR_ALIAS, "%s: res overlaps a", c.what);
    if (c.b && ranges_overlap(c.res, res_bytes, c.b, ctb) && (const void*)c.res != (const void*)c.b) return fail(PZ_ERR_ALIAS, "%s: res overlaps b", c.what);
    if (c.b && ranges_overlap(c.a, ctb, c.b, ctb) && (const void*)c.a != (const void*)c.b) return fail(PZ_ERR_ALIAS, "%s: a overlaps b", c.what);
    if (ranges_overlap(c.res, res_bytes, c.tmp, need)) return fail(PZ_ERR_ALIAS, "%s: res overlaps tmp", c.what);
    if (ranges_overlap(c.a, ctb, c.tmp, need)) return fail(PZ_ERR_ALIAS, "%s: a overlaps tmp", c.what);
    if (c.b && ranges_overlap(c.b, ctb, c.tmp, need)) return fail(PZ_ERR_ALIAS, "%s: b overlaps tmp", c.what);
    const size_t hit = std::min({trace_keys_overlap(tk, key_bytes, c.res, res_bytes), trace_keys_overlap(tk, key_bytes, c.a, ctb),
                                 c.b ? trace_keys_overlap(tk, key_bytes, c.b, ctb) : tk.nsteps, trace_keys_overlap(tk, key_bytes, c.tmp, need)});
    if (hit < tk.nsteps) return fail(PZ_ERR_ALIAS, "%s: the key of trace step %zu overlaps res, a, b or tmp", c.what, hit);
    return PZ_OK;
}
// the checked call by stages on the stream (no lock, no graph); batch >= 1
static int fhe_uint_word_stages_run(const WordCall& c, const std::vector<WordStage>& plan) {
    pz_module* M = c.M;
    const pz_glwe_op_params* p = c.p;
    const long long n = (long long)M->n;
    const int cols = (int)p->rank + 1, size = (int)p->res_size, B = (int)c.batch;
    const long long ct = n * cols * size;
    const size_t log_n = log2_n(M);
    const bool same = p->res_base2k == p->key_base2k;
    dispatch_note(M, "fhe_uint_word: by stages (%zu: k_word_pre%s, one trace of items x batch, one closing kernel)", plan.size(),
                  same ? " with the trace's first shift" : "");
    long long* dense = c.is_get ? (long long*)c.res : (long long*)c.tmp;
    auto slot = [&](uint32_t s) { return dense + (long long)s * B * ct; };
    for (const WordStage& st : plan) {
        const size_t nsteps = log_n - st.skip;
        const int items = (int)st.items.size();
        unsigned exp[kWordMaxItems];
        unsigned char sel[kWordMaxItems];
        for (int i = 0; i < items; ++i) { exp[i] = st.items[i].exp; sel[i] = (unsigned char)st.items[i].src; }
        WordPreCall pc;
        pc.src[WORD_SRC_A] = (const long long*)c.a; pc.src[WORD_SRC_B] = (const long long*)c.b; pc.src[WORD_SRC_RES] = (const long long*)c.res;
        pc.src[WORD_SRC_S] = c.is_get ? nullptr : slot(1);
        pc.out = slot(st.items[0].slot);
        pc.cols = cols; pc.size = size; pc.base2k = (int)p->res_base2k; pc.batch = B; pc.items = items;
        pc.shift = same && nsteps >= 1;
        pc.exp = exp; pc.sel = sel;
        PZ_TRY(launch_word_pre(M, pc));
        PZ_TRY(glwe_trace(M, (int64_t*)pc.out, nsteps, c.gals + st.skip, c.key_pmats + st.skip, p, (size_t)items * c.batch, pc.shift));
        if (st.close == WORD_CLOSE_REPLICATE) {
            PZ_TRY(launch_word_replicate(M, slot(1), slot(0), cols, size, B));
        } else if (st.close == WORD_CLOSE_COMBINE) {
            const long long* base = st.base == WORD_SRC_A ? (const long long*)c.a : (const long long*)c.res;
            PZ_TRY(launch_word_post(M, (long long*)c.res, base, st.plus == kWordNone ? nullptr : slot(st.plus), st.minus == kWordNone ? nullptr : slot(st.minus),
                                    st.r, cols, size, B));
        }
    }
    return PZ_OK;
}
// the reference's calls in its order on today's launchers: the byte-for-byte twin of the staged route
namespace {
struct WordLiteral {
    pz_module* M;
    const WordCall& c;
    long long n, ct;
    int cols, size, B;
    size_t log_n;
    int64_t* slot(int s) const { return (int64_t*)c.tmp + (long long)s * B * ct; }
    int rot(int64_t* dst, const int64_t* src, long long k) const {
        const PolyMap pm{1, 1, n, 0, 0, 0};
        return launch_rotate(M, B * size * cols, (const long long*)src, pm, (long long*)dst, pm, k);
    }
    int trace(int64_t* x, size_t skip) const { return glwe_trace(M, x, log_n - skip, c.gals + skip, c.key_pmats + skip, c.p, (size_t)B); }
    int ew(int op, int64_t* r, const int64_t* x, const int64_t* y) const { return launch_ew(M, op, r, ct, n, x, ct, n, y, ct, n, size * cols, B); }
    int get(int64_t* res, const int64_t* a, uint32_t exp, size_t skip) const {   // fhe_uint.rs:401-430
        PZ_TRY(rot(res, a, -(long long)exp));
        return trace(res, skip);
    }
    int zero_byte(int64_t* res, const int64_t* a, uint32_t r) const {   // :466-489 on a copy of a; glwe_trace = glwe_trace_assign on a copy
        PZ_TRY(rot(slot(0), a, -(long long)r));
        PZ_TRY(ew(EW_COPY, slot(1), slot(0), nullptr));
        PZ_TRY(trace(slot(1), 3));
        PZ_TRY(ew(EW_SUB_I64, slot(0), slot(0), slot(1)));
        return rot(res, slot(0), (long long)r);
    }
    int splice_u8(int64_t* res, const int64_t* a, const int64_t* b, uint32_t rd, uint32_t rs) const {   // :286-329; b's side first: res may be b
        PZ_TRY(rot(slot(2), b, -(long long)rs));
        PZ_TRY(trace(slot(2), 3));
        PZ_TRY(rot(slot(3), slot(2), (long long)rd));
        PZ_TRY(zero_byte(res, a, rd));
        return ew(EW_ADD_I64, res, res, slot(3));
    }
};
}  // namespace
static int fhe_uint_word_literal_run(const WordCall& c, size_t word_bits, uint32_t op, const uint32_t* args, size_t nargs) {
    pz_module* M = c.M;
    dispatch_note(M, "fhe_uint_word: literal (POULPY_DBG_WORD_STAGES=0: one rotation, one trace, one add or sub at a time)");
    WordLiteral w{M, c, (long long)M->n, (long long)M->n * (long long)(c.p->rank + 1) * (long long)c.p->res_size, (int)c.p->rank + 1, (int)c.p->res_size,
                  (int)c.batch, log2_n(M)};
    const size_t n = (size_t)M->n;
    auto cf = [&](uint32_t bit) { return fhe_uint_word_coefficient(n, word_bits, bit); };
    switch (op) {
    case WORD_GET_BIT:
    case WORD_GET_BYTE:
        for (size_t i = 0; i < nargs; ++i)
            PZ_TRY(w.get(c.res + (long long)i * w.B * w.ct, c.a, cf(op == WORD_GET_BIT ? args[i] : 8 * args[i]), op == WORD_GET_BIT ? 0 : 3));
        return PZ_OK;
    case WORD_ZERO_BYTE:
        return w.zero_byte(c.res, c.a, cf(8 * args[0]));
    case WORD_SPLICE_U8:
        return w.splice_u8(c.res, c.a, c.b, cf(8 * args[0]), cf(8 * args[1]));
    case WORD_SPLICE_U16:   // :259-282
        PZ_TRY(w.splice_u8(w.slot(4), c.a, c.b, cf(16 * args[0]), cf(16 * args[1])));
        return w.splice_u8(c.res, w.slot(4), c.b, cf(16 * args[0] + 8), cf(16 * args[1] + 8));
    default: {   // WORD_SEXT, :491-524
        const uint32_t byte = args[0], bytes = (uint32_t)(word_bits / 8);
        if (byte + 1 == bytes) return PZ_OK;
        PZ_TRY(w.get(w.slot(4), c.res, cf(8 * byte + 7), 0));
        for (int i = 0; i < 3; ++i) {
            PZ_TRY(w.rot(w.slot(5), w.slot(4), (long long)((n / 8) << i)));
            PZ_TRY(w.ew(EW_ADD_I64, w.slot(4), w.slot(4), w.slot(5)));
        }
        for (uint32_t i = byte + 1; i < bytes; ++i) PZ_TRY(w.splice_u8(c.res, c.res, w.slot(4), cf(8 * i), 0));
        return PZ_OK;
    }
    }
}
// plan, refusals, route, graph: the body of the four calls under the module lock
static int fhe_uint_word_call(const WordCall& c, size_t word_bits, uint32_t op, const uint32_t* args, size_t nargs) {
    pz_module* M = c.M;
    std::vector<WordStage> plan;
    std::string err;
    if (!fhe_uint_word_plan((size_t)M->n, word_bits, op, args, nargs, &plan, &err) ||
        !fhe_uint_word_plan_check((size_t)M->n, c.is_get ? std::max<size_t>(nargs, 1) : kWordSlots, plan, &err))
        return fail(PZ_ERR_INVALID, "%s", err.c_str());
    PZ_TRY(fhe_uint_word_refusals(c, word_bits));
    if (c.batch == 0 || plan.empty()) return PZ_OK;
    if (rt_knob("POULPY_DBG_WORD_STAGES", 1) == 0) return fhe_uint_word_literal_run(c, word_bits, op, args, nargs);   // (read per call: tests flip it)
    KeyHash k = graph_key(M, GRAPH_FHE_UINT_WORD, c.res, c.a, c.b, word_bits, op, nargs, c.tmp, c.batch, *c.p);
    for (size_t i = 0; i < nargs; ++i) k.add(args[i]);
    for (size_t s = 0, log_n = log2_n(M); s < log_n; ++s) { k.add(c.gals[s]); k.add(c.key_pmats[s]); }
    return with_graph(M, k.h, [&]() { return fhe_uint_word_stages_run(c, plan); });
}
int pz_fhe_uint_get_batched(pz_module* M, int64_t* res, const int64_t* words, size_t word_bits, int unit, size_t nidx, const uint32_t* idx,
                            const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(unit == PZ_WORD_BIT || unit == PZ_WORD_BYTE, "fhe_uint_get: unit %d is neither PZ_WORD_BIT nor PZ_WORD_BYTE", unit);
    PZ_REQUIRE(nidx == 0 || idx != nullptr, "fhe_uint_get: null argument");
    const WordCall c{M, "fhe_uint_get", res, words, nullptr, gals, key_pmats, p, tmp, tmp_bytes, batch, nidx, true};
    return fhe_uint_word_call(c, word_bits, unit == PZ_WORD_BIT ? WORD_GET_BIT : WORD_GET_BYTE, idx, nidx);
}
int pz_fhe_uint_zero_byte_batched(pz_module* M, int64_t* res, const int64_t* a, size_t word_bits, size_t byte, const int64_t* gals,
                                  const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    const uint32_t args[1] = {(uint32_t)std::min<size_t>(byte, 0xFFFFu)};
    const WordCall c{M, "fhe_uint_zero_byte", res, a, nullptr, gals, key_pmats, p, tmp, tmp_bytes, batch, 1, false};
    return fhe_uint_word_call(c, word_bits, WORD_ZERO_BYTE, args, 1);
}
int pz_fhe_uint_splice_batched(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, size_t word_bits, size_t width, size_t dst, size_t src,
                               const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(width == 8 || width == 16, "fhe_uint_splice: width %zu is neither 8 nor 16", width);
    PZ_REQUIRE(batch == 0 || b != nullptr, "fhe_uint_splice: null argument");
    const uint32_t args[2] = {(uint32_t)std::min<size_t>(dst, 0xFFFFu), (uint32_t)std::min<size_t>(src, 0xFFFFu)};
    const WordCall c{M, "fhe_uint_splice", res, a, b, gals, key_pmats, p, tmp, tmp_bytes, batch, 1, false};
    return fhe_uint_word_call(c, word_bits, width == 8 ? WORD_SPLICE_U8 : WORD_SPLICE_U16, args, 2);
}
int pz_fhe_uint_sext_batched(pz_module* M, int64_t* word, size_t word_bits, size_t byte, const int64_t* gals, const double* const* key_pmats,
                             const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    const uint32_t args[1] = {(uint32_t)std::min<size_t>(byte, 0xFFFFu)};
    const WordCall c{M, "fhe_uint_sext", word, word, nullptr, gals, key_pmats, p, tmp, tmp_bytes, batch, 1, false};
    return fhe_uint_word_call(c, word_bits, WORD_SEXT, args, 1);
}

}  // extern "C"
