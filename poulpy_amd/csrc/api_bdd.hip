// api_bdd.hip — BDD circuits behind the C ABI: the circuit object and its accessors, the device copies of its level tables, and the executor with
// its gathered and per-gate routes over the CMUX of api_gates.hip.  poulpy-bin-fhe bdd_arithmetic/eval.rs:104-305 (ExecuteBDDCircuit); the
// schedule itself is compiled on the host by bdd_schedule.cpp.  DESIGN.md 4.4f.
#include <algorithm>
#include <atomic>
#include <string>
#include <unordered_map>
#include <vector>

#include "api_common.hpp"
#include "bdd_schedule.hpp"
#include "glwe_call.hpp"

using namespace pz;

// ------------------------------------------------------------------------------
// BDD circuits: ExecuteBDDCircuit (eval.rs:104-305).  pz_bdd_circuit_new compiles the node lists on the host (bdd_schedule.cpp) into
// level tables of gates over physical slots; pz_bdd_circuit_execute_batched runs them on `batch` inputs.  tmp = [state pool, slot-major
// [slots][batch]][gather table][key pointers][row-sliced copies of the selected keys that are not pinned].  Routes:
//   gathered   N = 1024 / 2048 / 4096 where the small-ring kernels serve the CMUX: per call one table kernel turns (slot, slot, slot, selector) of
//              every gate and input into (t, f, res, key) addresses, then every level is ONE launch (or one per wave of the module's chunk) of the
//              gathered kernels - blocks input-major, the gates of an input sorted by selector, so the ciphertexts of one key sit side by side
//   per-gate   every other shape, and POULPY_DBG_BDD_GATHER=0: the same schedule, one glwe_cmux per (gate, input)
// What depends on the call's keys reaches the gathered kernels through tmp, written outside the graph (the slices, the pointer array); the graph
// itself holds kernel nodes only and is keyed by the circuit, out, tmp and the shape.  The per-gate route bakes key pointers into kernel arguments,
// so there the resolved keys are part of the key.
// ------------------------------------------------------------------------------
struct pz_bdd_circuit {
    BddSchedule s;
    uint64_t uid;
};
static std::atomic<uint64_t> g_bdd_uid{1};

struct BddWs { size_t state, tab, ptrs, slice, nsel, total; };
static BddWs bdd_ws(const pz_module* M, const BddSchedule& s, const pz_glwe_op_params* p, size_t batch, size_t nbits) {
    BddWs w;
    w.state = align256(s.slots * batch * (size_t)M->n * 8 * (p->rank + 1) * p->res_size);
    w.tab = align256(s.gates.size() * batch * sizeof(SmallGather));
    w.ptrs = align256(batch * nbits * sizeof(void*));
    w.slice = align256(ggsw_key_bytes(M, p));
    w.nsel = 0;
    for (uint8_t u : s.selected) w.nsel += u;
    w.total = w.state + w.tab + w.ptrs + batch * w.nsel * w.slice;
    return w;
}
// the module's device copy of the circuit's level tables (uploaded once per module and circuit, with a blocking copy: the handle may be freed
// as soon as the call returns)
static int bdd_device_tables(pz_module* M, const pz_bdd_circuit* c, const BddGate** gates, const uint32_t** level_start) {
    for (auto& bt : M->bdd_tables)
        if (bt.uid == c->uid) { bt.stamp = ++M->mirror_clock; *gates = (const BddGate*)bt.gates; *level_start = (const uint32_t*)bt.level_start; return PZ_OK; }
    if (M->bdd_tables.size() >= 16) {   // (a captured graph may hold the evicted tables: it goes with them)
        size_t lru = 0;
        for (size_t i = 1; i < M->bdd_tables.size(); ++i) if (M->bdd_tables[i].stamp < M->bdd_tables[lru].stamp) lru = i;
        PZ_HIP(hipStreamSynchronize(M->stream));
        M->graph_epoch++;
        (void)hipFree(M->bdd_tables[lru].gates); (void)hipFree(M->bdd_tables[lru].level_start);
        M->bdd_tables.erase(M->bdd_tables.begin() + (long)lru);
    }
    void *dg = nullptr, *dl = nullptr;
    const size_t gb = std::max<size_t>(c->s.gates.size(), 1) * sizeof(BddGate), lb = c->s.level_start.size() * sizeof(uint32_t);
    PZ_TRY(device_malloc_retry(M, &dg, gb));
    if (device_malloc_retry(M, &dl, lb) != PZ_OK) { (void)hipFree(dg); return PZ_ERR_HIP; }
    if ((c->s.gates.empty() ? hipSuccess : hipMemcpy(dg, c->s.gates.data(), c->s.gates.size() * sizeof(BddGate), hipMemcpyHostToDevice)) != hipSuccess ||
        hipMemcpy(dl, c->s.level_start.data(), lb, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dg); (void)hipFree(dl);
        return fail(PZ_ERR_HIP, "bdd_circuit_execute: upload of the level tables failed");
    }
    M->bdd_tables.push_back({c->uid, dg, dl, ++M->mirror_clock});
    *gates = (const BddGate*)dg; *level_start = (const uint32_t*)dl;
    return PZ_OK;
}
// the initial state and the outputs no gate writes: slots 0 / 1 of the pool (zero, one), the zero outputs, the slots beyond output_size
static int bdd_init(pz_module* M, const BddSchedule& s, int64_t* state, int64_t* out, size_t n_out, const pz_glwe_op_params* p, size_t batch) {
    const long long n = (long long)M->n, cols = (long long)p->rank + 1, ct = n * cols * (long long)p->res_size;
    const size_t slot_bytes = batch * (size_t)ct * 8;
    PZ_TRY(launch_zero_bytes(M, state, 2 * slot_bytes));
    // encode_coeff_i64(base2k, col 0, k = 2, idx 0, 1) (encoding.rs:116-155): 1 << (bits of limb `used - 1` below 2^-2), normalized
    const int k = (int)p->res_base2k, used = (2 + k - 1) / k;
    long long d[2] = {0, 0};
    d[used - 1] = 1ll << (used * k - 2);
    long long carry = 0;
    for (int j = used - 1; j >= 0; --j) {
        const long long v = d[j] + carry, half = 1ll << (k - 1), dg = ((v + half) & ((1ll << k) - 1)) - half;
        carry = (v - dg) >> k;
        d[j] = dg;
    }
    PZ_TRY(launch_bdd_one(M, (long long*)state + (long long)batch * ct, ct, (int)batch, cols * n, d[0], d[1], used));
    for (uint32_t o : s.zero_outputs) PZ_TRY(launch_zero_bytes(M, out + (size_t)o * batch * (size_t)ct, slot_bytes));
    if (n_out > s.output_size) PZ_TRY(launch_zero_bytes(M, out + s.output_size * batch * (size_t)ct, (n_out - s.output_size) * slot_bytes));
    return PZ_OK;
}

extern "C" {
pz_bdd_circuit* pz_bdd_circuit_new(const pz_bdd_node* const* nodes, const size_t* node_count, const size_t* state_size, size_t output_size,
                                   size_t input_size) {
    static_assert(sizeof(pz_bdd_node) == sizeof(BddNode) && (int)PZ_BDD_NONE == (int)kBddNone && (int)PZ_BDD_COPY == (int)kBddCopy && (int)PZ_BDD_CMUX == (int)kBddCmux,
                  "pz_bdd_node is the compiler's node");
    pz_bdd_circuit* c = new pz_bdd_circuit();
    std::string err;
    if (!bdd_compile(reinterpret_cast<const BddNode* const*>(nodes), node_count, state_size, output_size, input_size, &c->s, &err)) {
        delete c;
        (void)fail(PZ_ERR_INVALID, "%s", err.c_str());
        return nullptr;
    }
    c->uid = g_bdd_uid.fetch_add(1);
    return c;
}
void pz_bdd_circuit_free(pz_bdd_circuit* c) { delete c; }
size_t pz_bdd_circuit_input_size(const pz_bdd_circuit* c) { return c ? c->s.input_size : 0; }
size_t pz_bdd_circuit_output_size(const pz_bdd_circuit* c) { return c ? c->s.output_size : 0; }
size_t pz_bdd_circuit_max_state_size(const pz_bdd_circuit* c) { return c ? c->s.max_state_size : 0; }
size_t pz_bdd_circuit_levels(const pz_bdd_circuit* c) { return c ? c->s.levels() : 0; }
size_t pz_bdd_circuit_gates(const pz_bdd_circuit* c) { return c ? c->s.gates.size() : 0; }
size_t pz_bdd_circuit_moved_copies(const pz_bdd_circuit* c) { return c ? c->s.moved_copies : 0; }
size_t pz_bdd_circuit_slots(const pz_bdd_circuit* c) { return c ? c->s.slots : 0; }
int pz_bdd_circuit_output_slots(const pz_bdd_circuit* c, size_t o, size_t* first, size_t* count) {
    if (!c || o >= c->s.output_size) return -1;
    if (first) *first = c->s.slot_first[o];
    if (count) *count = c->s.slot_count[o];
    return 0;
}
size_t pz_bdd_circuit_level_gates(const pz_bdd_circuit* c, size_t level, uint32_t* gates4, size_t cap) {
    if (!c || level >= c->s.levels()) return 0;
    const size_t a = c->s.level_start[level], cnt = c->s.level_start[level + 1] - a;
    for (size_t i = 0; gates4 && i < std::min(cnt, cap); ++i) {
        const BddGate& g = c->s.gates[a + i];
        gates4[4 * i] = g.t; gates4[4 * i + 1] = g.f; gates4[4 * i + 2] = g.res; gates4[4 * i + 3] = g.sel;
    }
    return cnt;
}
size_t pz_bdd_circuit_execute_tmp_bytes(const pz_module* M, const pz_bdd_circuit* c, const pz_glwe_op_params* p, size_t batch) {
    if (!M || !c || !p) return 0;
    return bdd_ws(M, c->s, p, batch, c->s.input_size).total;
}
}  // extern "C"

// which route a call takes: null = gathered (*one: the one-kernel form), else why it walks gate by gate
static const char* bdd_per_gate_reason(pz_module* M, const GlweCall& c, const SmallGatherShape& sh, bool* one) {
    *one = false;
    if (rt_knob("POULPY_DBG_BDD_GATHER", 1) == 0) return "POULPY_DBG_BDD_GATHER=0";   // (read per call: tests flip it)
    if (c.digits) return "dsize > 1";
    if (!cmux_fused_route(c)) return "no small-ring kernels for this shape";
    *one = !fused_applies(M, c.p, c.s, c.kind) && small_one_gather_supported(M, sh);
    return nullptr;
}
static int bdd_levels_gathered(pz_module* M, const BddSchedule& s, const SmallGatherShape& sh, bool one, const SmallGather* tab, cplx* S, size_t chunk, size_t batch) {
    dispatch_note(M, one ? "bdd: gathered small-one (k_small_one_gather, one launch per level)" : "bdd: gathered small two-kernel (k_small_fwd_gather -> k_small_inv_gather per level)");
    for (size_t lv = 0; lv < s.levels(); ++lv) {
        const size_t first = (size_t)s.level_start[lv] * batch, total = (size_t)(s.level_start[lv + 1] - s.level_start[lv]) * batch;
        for (size_t c0 = 0; c0 < total; c0 += chunk) {
            const int nb = (int)std::min(chunk, total - c0);
            if (one) { PZ_TRY(launch_small_one_gather(M, nb, sh, tab + first + c0)); continue; }
            PZ_TRY(launch_small_fwd_gather(M, nb, sh, tab + first + c0, S));
            PZ_TRY(launch_small_inv_gather(M, nb, sh, tab + first + c0, S));
        }
    }
    return PZ_OK;
}
static int bdd_levels_per_gate(pz_module* M, const BddSchedule& s, int64_t* state, int64_t* out, const double* const* keys, size_t nbits,
                               const pz_glwe_op_params* p, size_t batch) {
    const size_t ct = (size_t)M->n * (p->rank + 1) * p->res_size;
    const CmuxOperands ops{p->res_size, p->res_size, 0};
    for (const BddGate& g : s.gates)   // (level-major: every gate of a level before any of the next)
        for (size_t b = 0; b < batch; ++b) {
            int64_t* res = (g.res & kBddOut) ? out + ((size_t)(g.res & ~kBddOut) * batch + b) * ct : state + ((size_t)g.res * batch + b) * ct;
            PZ_TRY(glwe_cmux(M, res, state + ((size_t)g.t * batch + b) * ct, state + ((size_t)g.f * batch + b) * ct, keys[b * nbits + g.sel], p, &ops, 1));
        }
    return PZ_OK;
}

namespace pz {
int bdd_circuit_execute_precheck(const pz_module* M, const pz_bdd_circuit* c, const int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                                 const pz_glwe_op_params* p, size_t batch, bool* nothing) {
    *nothing = false;
    PZ_REQUIRE(p != nullptr, "bdd_circuit_execute: null params");
    PZ_REQUIRE(c != nullptr, "bdd_circuit_execute: null circuit");
    const BddSchedule& s = c->s;
    PZ_REQUIRE(p->dsize >= 1 && p->dnum >= 1 && p->key_size >= 1 && p->a_size >= 1 && p->res_size >= 1 && p->res_base2k >= 1 && p->res_base2k <= 62, "bdd_circuit_execute: empty shape");
    PZ_REQUIRE(p->a_base2k == p->key_base2k && p->res_base2k == p->key_base2k, "bdd_circuit_execute: the state, the result and the GGSWs share one base2k (%llu / %llu / %llu)",
               (unsigned long long)p->a_base2k, (unsigned long long)p->res_base2k, (unsigned long long)p->key_base2k);
    PZ_REQUIRE(p->a_size == p->res_size, "bdd_circuit_execute: the state has the layout of the result (p->a_size == p->res_size)");
    PZ_REQUIRE(p->res_size * p->res_base2k >= 2, "bdd_circuit_execute: the result cannot hold the constant 2^-2");
    PZ_REQUIRE(n_out >= s.output_size, "bdd_circuit_execute: n_out %zu < output_size %zu", n_out, s.output_size);
    PZ_REQUIRE(batch <= (1u << 24) && n_out < kBddOut, "bdd_circuit_execute: batch or n_out out of range");
    if (batch == 0 || n_out == 0) { *nothing = true; return M ? PZ_OK : fail(PZ_ERR_INVALID, "null module"); }   // no ciphertext to write
    PZ_REQUIRE(nbits >= s.input_size, "bdd_circuit_execute: nbits %zu < input_size %zu", nbits, s.input_size);
    PZ_REQUIRE(out != nullptr, "bdd_circuit_execute: null argument");
    if (!s.gates.empty()) {
        PZ_REQUIRE(bits != nullptr, "bdd_circuit_execute: null argument");
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < s.input_size; ++i)
                PZ_REQUIRE(!s.selected[i] || bits[b * nbits + i] != nullptr, "bdd_circuit_execute: the GGSW of input bit %zu of input %zu is null and the circuit selects it", i, b);
    }
    return PZ_OK;
}
int bdd_circuit_execute(pz_module* M, const pz_bdd_circuit* c, int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                        const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    const BddSchedule& s = c->s;
    PZ_REQUIRE(is_device_ptr(out), "batched entry points take device pointers");
    const size_t cols = p->rank + 1, ct = (size_t)M->n * cols * p->res_size;
    const size_t out_bytes = n_out * batch * ct * 8, key_bytes = ggsw_key_bytes(M, p);
    if (s.gates.empty()) return launch_zero_bytes(M, out, out_bytes);   // nothing but zero outputs
    const BddWs w = bdd_ws(M, s, p, batch, nbits);
    PZ_REQUIRE(tmp != nullptr && is_device_ptr(tmp) && tmp_bytes >= w.total, "bdd_circuit_execute: tmp too small (%zu bytes, %zu needed)", tmp_bytes, w.total);
    if (ranges_overlap(out, out_bytes, tmp, w.total)) return fail(PZ_ERR_ALIAS, "bdd_circuit_execute: out overlaps tmp");
    // Every selected entry resolves as every GLWE key does - and all of them must stay resolved until the call has been issued.  A module mirrors at
    // most kKeyMirrorMax host keys (kKeyMirrorBytes) and frees the least recently used one beyond that: a call whose distinct host-resident keys
    // do not fit at once is refused here, before the first of them is resolved (each distinct pointer is resolved once)
    std::unordered_map<const double*, const double*> resolved;
    size_t nhost = 0;
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < s.input_size; ++i)
            if (s.selected[i] && resolved.emplace(bits[b * nbits + i], nullptr).second && !is_device_ptr(bits[b * nbits + i])) ++nhost;
    if (nhost > kKeyMirrorMax || nhost * key_bytes > kKeyMirrorBytes)
        return fail(PZ_ERR_UNSUPPORTED, "bdd_circuit_execute: %zu distinct host-resident GGSWs of %zu bytes in one call; a module mirrors at most %zu (%zu GiB) at a time - "
                    "keep them on the device (pz_device_alloc, pz_memcpy_h2d)", nhost, key_bytes, kKeyMirrorMax, kKeyMirrorBytes >> 30);
    for (auto& kv : resolved) PZ_TRY(resolve_key(M, kv.first, key_bytes, &kv.second));
    std::vector<const double*> keys(batch * nbits, nullptr);
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < s.input_size; ++i) {
            if (!s.selected[i]) continue;
            keys[b * nbits + i] = resolved[bits[b * nbits + i]];
            if (ranges_overlap(out, out_bytes, keys[b * nbits + i], key_bytes)) return fail(PZ_ERR_ALIAS, "bdd_circuit_execute: out overlaps the GGSW of input bit %zu of input %zu", i, b);
            if (ranges_overlap(tmp, w.total, keys[b * nbits + i], key_bytes)) return fail(PZ_ERR_ALIAS, "bdd_circuit_execute: tmp overlaps the GGSW of input bit %zu of input %zu", i, b);
        }
    char* base = (char*)tmp;
    int64_t* state = (int64_t*)base;
    SmallGather* tab = (SmallGather*)(base + w.state);
    const cplx** dptrs = (const cplx**)(base + w.state + w.tab);
    char* slices = base + w.state + w.tab + w.ptrs;
    GlweCall gc;
    const double* any_key = nullptr;
    for (const double* k : keys) if (k) { any_key = k; break; }
    PZ_TRY(glwe_call_init(gc, M, GlweKind::ExternalProduct, out, state, any_key, p, batch, nullptr, nullptr, nullptr));
    gc.add = state;   // (the CMUX's every-column operand: part of what cmux_fused_route looks at)
    const SmallGatherShape sh{(int)cols, (int)p->res_size, (int)p->key_size, (int)p->dnum, (int)p->res_base2k};
    bool one = false;
    const char* why = bdd_per_gate_reason(M, gc, sh, &one);
    // (the module's state enters the key when it is built: on the gathered route behind ws_reserve, which may move the workspace)
    auto route_key = [&]() { return graph_key(M, GRAPH_BDD_EXECUTE, c->uid, out, n_out, tmp, nbits, batch, *p, why != nullptr, rt_knob("POULPY_DBG_CMUX_FUSED", 1)); };
    if (why) {
        KeyHash k = route_key();
        for (const double* key : keys) k.add(key);
        PZ_TRY(with_graph(M, k.h, [&]() {
            dispatch_note(M, "bdd: per-gate (%s)", why);
            PZ_TRY(bdd_init(M, s, state, out, n_out, p, batch));
            return bdd_levels_per_gate(M, s, state, out, keys.data(), nbits, p, batch);
        }));
        return PZ_OK;
    }
    // ---- gathered: everything that depends on the keys is written to tmp here, outside the graph ----
    const BddGate* d_gates; const uint32_t* d_levels;
    PZ_TRY(bdd_device_tables(M, c, &d_gates, &d_levels));
    const bool pipeline = fused_applies(M, p, gc.s, gc.kind);   // N = 4096: the key layout of the three-kernel pipeline's plan
    // the pointer array goes through page-locked staging: the previous call's copy out of it has finished before it is rewritten
    if (M->bdd_stage_ev) PZ_HIP(hipEventSynchronize(M->bdd_stage_ev));
    else PZ_HIP(hipEventCreateWithFlags(&M->bdd_stage_ev, hipEventDisableTiming));
    if (M->bdd_stage_count < batch * nbits) {
        if (M->bdd_stage) PZ_HIP(hipHostFree(M->bdd_stage));
        M->bdd_stage = nullptr; M->bdd_stage_count = 0;
        PZ_HIP(hipHostMalloc((void**)&M->bdd_stage, batch * nbits * sizeof(void*), hipHostMallocDefault));
        M->bdd_stage_count = batch * nbits;
    }
    std::fill(M->bdd_stage, M->bdd_stage + batch * nbits, nullptr);
    // (hash maps: a batch of 64 additions brings 4096 keys, every one of them pinned)
    std::unordered_map<const void*, const cplx*> sliced;   // the distinct keys of this call -> their row-sliced copies
    std::unordered_map<const void*, const cplx*> pinned;
    for (auto& pk : M->pinned)
        if (pk.sliced && pk.bytes == key_bytes) pinned.emplace(pk.key, pk.sliced);   // (pinned_slices' test, api_glwe.hip)
    size_t nsliced = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        if (!keys[i]) continue;
        auto it = sliced.find(keys[i]);
        if (it == sliced.end()) {
            const auto pin = pinned.find(keys[i]);
            const cplx* Pp = pin != pinned.end() ? pin->second : nullptr;
            if (!Pp) {
                cplx* dst = (cplx*)(slices + (nsliced++) * w.slice);
                if (pipeline) PZ_TRY(launch_permute_pmat(M, keys[i], dst, gc.nrows * gc.ncols));
                else PZ_TRY(launch_small_permute(M, keys[i], dst, gc.nrows * gc.ncols));
                Pp = dst;
            }
            it = sliced.emplace(keys[i], Pp).first;
        }
        M->bdd_stage[i] = it->second;
    }
    PZ_HIP(hipMemcpyAsync(dptrs, M->bdd_stage, batch * nbits * sizeof(void*), hipMemcpyHostToDevice, M->stream));
    PZ_HIP(hipEventRecord(M->bdd_stage_ev, M->stream));
    size_t widest = 0;
    for (size_t lv = 0; lv < s.levels(); ++lv) widest = std::max<size_t>(widest, s.level_start[lv + 1] - s.level_start[lv]);
    const size_t chunk = pick_chunk(M, p, gc.s, widest * batch);
    const size_t s_bytes = one ? 0 : align256(chunk * (size_t)gc.npi * (size_t)M->m * sizeof(cplx));
    PZ_TRY(ws_reserve(M, s_bytes));
    char* wsb = (char*)M->ws;
    cplx* S = nullptr;
    PZ_TRY(ws_take(M, wsb, s_bytes, &S));
    KeyHash k = route_key();
    k.add(one);
    PZ_TRY(with_graph(M, k.h, [&]() {
        PZ_TRY(bdd_init(M, s, state, out, n_out, p, batch));
        BddTableCall tc;
        tc.gates = d_gates; tc.level_start = d_levels; tc.levels = (int)s.levels(); tc.total = (uint32_t)s.gates.size(); tc.batch = (int)batch; tc.nbits = (int)nbits;
        tc.state = (long long*)state; tc.out = (long long*)out; tc.ct = (long long)ct; tc.keys = dptrs; tc.tab = tab;
        PZ_TRY(launch_bdd_table(M, tc));
        return bdd_levels_gathered(M, s, sh, one, tab, S, chunk, batch);
    }));
    return PZ_OK;
}
}  // namespace pz

extern "C" {
int pz_bdd_circuit_execute_batched(pz_module* M, const pz_bdd_circuit* c, int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                                   const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    bool nothing = false;
    PZ_TRY(bdd_circuit_execute_precheck(M, c, out, n_out, bits, nbits, p, batch, &nothing));
    if (nothing) return PZ_OK;
    PZ_ENTER(M);
    PZ_TRY(bdd_circuit_execute(M, c, out, n_out, bits, nbits, p, tmp, tmp_bytes, batch));
    return finish_call(M, false);
}
}  // extern "C"
