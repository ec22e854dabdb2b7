// api_trace.hip — glwe_trace and glwe_pack behind the C ABI: chains of the automorphism family of glwe_op (api_glwe.hip), one prepared key per
// step, and the one place where a trace runs in the keys' base on a temporary (trace_in_key_base).  poulpy-core glwe_trace.rs:91-176,
// glwe_packing.rs:15-176.
#include <algorithm>
#include <vector>

#include "api_common.hpp"
#include "glwe_call.hpp"

using namespace pz;

// src (res_size limbs, res_base2k) -> tmp (tmp_size limbs in the keys' base: glwe_normalize), glwe_trace there, tmp -> res (glwe_trace.rs:91-127,
// :153-163)
int trace_in_key_base(pz_module* M, int64_t* res, const int64_t* src, int64_t* tmp, size_t tmp_size, size_t nsteps, const int64_t* gals,
                      const double* const* key_pmats, const pz_glwe_op_params* p, size_t batch) {
    const long long n = (long long)M->n;
    const int cols = (int)p->rank + 1, size = (int)p->res_size, k = (int)p->res_base2k, kk = (int)p->key_base2k, tsz = (int)tmp_size, B = (int)batch;
    const long long ct = n * cols * size;
    DV tv{tmp, n * cols * tsz, cols, tsz}, sv{(void*)src, ct, cols, size}, rv{res, ct, cols, size};
    for (int c = 0; c < cols; ++c) PZ_TRY(dev_normalize(M, B, tv, kk, 0, c, sv, k, c));
    pz_glwe_op_params q = *p;
    q.a_size = q.res_size = (uint64_t)tsz; q.a_base2k = q.res_base2k = p->key_base2k;
    PZ_TRY(glwe_trace(M, tmp, nsteps, gals, key_pmats, &q, batch));
    for (int c = 0; c < cols; ++c) PZ_TRY(dev_normalize(M, B, rv, k, 0, c, tv, kk, c));
    return PZ_OK;
}

namespace pz {
// glwe_trace_assign (poulpy-core/src/glwe_trace.rs:129-176) on `batch` ciphertexts:
//   for every step s:  res = rsh(res, 1 bit) on every column (operations/glwe.rs:1096-1112);  res = glwe_automorphism_add_assign(res, key_s)
// res in another base than the keys (:153-163; test_suite/trace.rs:36-39): (a_size, a_base2k = key_base2k) describe res re-expressed in
// the keys' base (a_size = ceil(res.max_k / key_base2k)); normalize into a temporary of that layout, trace there, normalize back.
int glwe_trace(pz_module* M, int64_t* res, size_t nsteps, const int64_t* gals, const double* const* key_pmats,
                      const pz_glwe_op_params* p, size_t batch, bool first_shifted) {
    PZ_REQUIRE(p != nullptr && (nsteps == 0 || (gals != nullptr && key_pmats != nullptr)), "glwe_trace: null argument");
    PZ_REQUIRE(!first_shifted || (p->res_base2k == p->key_base2k && nsteps >= 1), "glwe_trace: the first shift can only be the caller's in the keys' base");
    PZ_REQUIRE(p->rank_out == p->rank, "glwe_trace: rank_out != rank");
    PZ_REQUIRE(is_device_ptr(res), "batched entry points take device pointers");
    if (p->res_base2k != p->key_base2k) {
        PZ_REQUIRE(p->a_base2k == p->key_base2k && p->a_size >= 1 && p->res_size >= 1,
                   "glwe_trace: with res in another base than the keys, (a_size, a_base2k) is its layout in the keys' base");
        if (batch == 0) return PZ_OK;
        PZ_TRY(ws2_reserve(M, batch * (size_t)M->n * (p->rank + 1) * p->a_size * 8));
        return trace_in_key_base(M, res, res, (int64_t*)M->ws2, p->a_size, nsteps, gals, key_pmats, p, batch);
    }
    PZ_REQUIRE(p->a_size == p->res_size && p->a_base2k == p->res_base2k,
               "glwe_trace: a and res describe the same ciphertexts when res is in the keys' base");
    if (batch == 0) return PZ_OK;
    const long long n = (long long)M->n;
    const int cols = (int)p->rank + 1;
    const long long ct = n * cols * (long long)p->res_size;
    // the one-bit shift in front of step s + 1 rides on the tail of step s where that path has the shifted-store variant
    bool shifted = first_shifted;   // (the FheUint byte operations' pre-kernel shifts on its way out: k_word_pre)
    for (size_t s = 0; s < nsteps; ++s) {
        PZ_REQUIRE((gals[s] & 1) != 0, "glwe_trace: Galois elements must be odd");
        if (!shifted) PZ_TRY(launch_rsh(M, (int)batch, (long long*)res, ct, cols, (int)p->res_size, 0, cols, (int)p->res_base2k, 1));
        AutoSpec au{(long long)gals[s], 1};
        bool rsh = s + 1 < nsteps;
        PZ_TRY(glwe_op(M, GlweKind::Automorphism, res, res, key_pmats[s], p, batch, &au, nullptr, &rsh));
        shifted = rsh;
    }
    return PZ_OK;
}
}  // namespace pz

extern "C" {
int pz_glwe_trace_batched(pz_module* M, int64_t* res, size_t nsteps, const int64_t* gals, const double* const* key_pmats,
                          const pz_glwe_op_params* p, size_t batch) {
    PZ_ENTER(M);
    KeyHash k = graph_key(M, GRAPH_GLWE_TRACE, res, nsteps, batch);
    if (p) k.add(*p);
    for (size_t s = 0; s < nsteps && gals && key_pmats; ++s) { k.add(gals[s]); k.add(key_pmats[s]); }
    return with_graph(M, k.h, [&]() { return glwe_trace(M, res, nsteps, gals, key_pmats, p, batch, false); });
}

// ------------------------------------------------------------------------------
// public: GLWEPacking::glwe_pack (poulpy-core/src/glwe_packing.rs:122-176, pack_internal :15-87) on `batch` independent packing
// problems with the same occupancy pattern, one base2k / size for ciphertexts, keys and result.  cts[s] points to the `batch`
// contiguous GLWEs of index indices[s] (the reference's HashMap entry); they are clobbered, as the reference's `&mut` entries.
// The tree is walked on the host exactly as the reference does; every step is a batched launch of the i64 kernels
// (rotate, add / sub, rsh, normalize) or of the fused automorphism pipeline.
// ------------------------------------------------------------------------------
size_t pz_glwe_pack_tmp_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t batch) {
    if (!M || !p) return 0;
    return 3 * align256(batch * (size_t)M->n * (p->rank + 1) * p->res_size * 8);
}
size_t pz_glwe_pack_bases_tmp_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t trace_size, size_t batch) {
    if (!M || !p) return 0;
    return pz_glwe_pack_tmp_bytes(M, p, batch) + align256(batch * (size_t)M->n * (p->rank + 1) * trace_size * 8);
}
}  // extern "C"

// trace_size = 0: ciphertexts, keys and result share one base2k.  Otherwise the keys have their own (test_suite/glwe_packing.rs:40-42):
// pack_internal's arithmetic stays in the ciphertexts' base, the automorphisms convert, and the closing glwe_trace (glwe_trace.rs:91-127)
// runs on a temporary of trace_size limbs in the keys' base (behind the three ciphertext arrays of tmp).
// The limb-wise steps of glwe_pack on `B` ciphertexts at a time (poulpy-core glwe_packing.rs:41-86), and one merge of two slots
struct PackStep {
    pz_module* M;
    const pz_glwe_op_params* p;
    size_t batch;
    long long n, ct;
    int cols, size, k, B;
    int64_t *tmp_b, *t1, *t2;
    PolyMap pm() const { return PolyMap{size, cols, ct, (long long)cols * n, n, 0}; }
    int rotate_to(long long kk, int64_t* dst, const int64_t* src) {
        return launch_rotate(M, B * size * cols, (const long long*)src, pm(), (long long*)dst, pm(), kk);
    }
    int rotate_assign(long long kk, int64_t* x) {
        PZ_TRY(rotate_to(kk, t1, x));
        return launch_ew(M, EW_COPY, x, ct, n, t1, ct, n, nullptr, 0, 0, cols * size, B);
    }
    int ew3(int op, int64_t* r, const int64_t* x, const int64_t* y) {   // limb-wise over whole ciphertexts (equal sizes)
        return launch_ew(M, op, r, ct, n, x, ct, n, y, ct, n, cols * size, B);
    }
    int rsh1(int64_t* x) { return launch_rsh(M, B, (long long*)x, ct, cols, size, 0, cols, k, 1); }
    int normalize_assign(int64_t* x) {
        PZ_TRY(launch_ew(M, EW_COPY, t2, ct, n, x, ct, n, nullptr, 0, 0, cols * size, B));
        DV xv{x, ct, cols, size}, tv{t2, ct, cols, size};
        for (int c = 0; c < cols; ++c) PZ_TRY(dev_normalize(M, B, xv, k, 0, c, tv, k, c));
        return PZ_OK;
    }
    // slots j (a) and j + tt (b) of one level -> *out (null when both are empty)
    int merge(int64_t* a, int64_t* b, size_t tt, int64_t gal, const double* key, int64_t** out) {
        *out = nullptr;
        if (a && b) {                                                       // :41-70
            PZ_TRY(rotate_assign(-(long long)tt, a));
            PZ_TRY(ew3(EW_SUB_I64, tmp_b, a, b));
            PZ_TRY(rsh1(tmp_b));
            PZ_TRY(ew3(EW_ADD_I64, a, a, b));
            PZ_TRY(rsh1(a));
            PZ_TRY(normalize_assign(tmp_b));
            AutoSpec au{(long long)gal, 0};
            PZ_TRY(glwe_op(M, GlweKind::Automorphism, tmp_b, tmp_b, key, p, batch, &au));
            PZ_TRY(ew3(EW_SUB_I64, a, a, tmp_b));
            PZ_TRY(normalize_assign(a));
            PZ_TRY(rotate_assign((long long)tt, a));
            *out = a;
        } else if (a) {                                                     // :71-75
            PZ_TRY(rsh1(a));
            AutoSpec au{(long long)gal, 1};
            PZ_TRY(glwe_op(M, GlweKind::Automorphism, a, a, key, p, batch, &au));
            *out = a;
        } else if (b) {                                                     // :76-86
            PZ_TRY(rotate_to((long long)tt, tmp_b, b));
            PZ_TRY(rsh1(tmp_b));
            AutoSpec au{(long long)gal, 3};
            PZ_TRY(glwe_op(M, GlweKind::Automorphism, b, tmp_b, key, p, batch, &au));
            *out = b;
        }
        return PZ_OK;
    }
};
namespace pz {
int glwe_pack(pz_module* M, int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts, size_t log_gap_out,
              const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes,
              size_t batch, size_t trace_size) {
    PZ_REQUIRE(p != nullptr && indices != nullptr && cts != nullptr && gals != nullptr && key_pmats != nullptr, "glwe_pack: null argument");
    PZ_REQUIRE(p->a_size == p->res_size && p->a_base2k == p->res_base2k && p->rank_out == p->rank && p->dsize == 1,
               "glwe_pack: ciphertexts and result share base2k and size");
    PZ_REQUIRE(p->res_base2k == p->key_base2k || trace_size >= 1,
               "glwe_pack: keys in another base than the ciphertexts need pz_glwe_pack_bases_batched (trace_size)");
    if (p->res_base2k == p->key_base2k) trace_size = 0;
    const size_t log_n = log2_n(M);
    PZ_REQUIRE(log_gap_out <= log_n && nslots >= 1, "glwe_pack: bad shape");
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(tmp), "batched entry points take device pointers");
    PZ_REQUIRE(tmp_bytes >= pz_glwe_pack_bases_tmp_bytes(M, p, trace_size, batch), "glwe_pack: tmp is smaller than pz_glwe_pack[_bases]_tmp_bytes");
    if (batch == 0) return PZ_OK;
    PackStep st;
    st.M = M; st.p = p; st.batch = batch; st.n = (long long)M->n;
    st.cols = (int)p->rank + 1; st.size = (int)p->res_size; st.k = (int)p->res_base2k; st.B = (int)batch;
    st.ct = st.n * st.cols * st.size;
    const long long n = st.n, ct = st.ct;
    const int cols = st.cols, size = st.size, B = st.B;
    const size_t ctb = align256((size_t)B * ct * 8);
    st.tmp_b = (int64_t*)tmp;
    st.t1 = (int64_t*)((char*)tmp + ctb);
    st.t2 = (int64_t*)((char*)tmp + 2 * ctb);
    std::vector<int64_t*> slots((size_t)M->n, nullptr);
    for (size_t s_ = 0; s_ < nslots; ++s_) {
        PZ_REQUIRE(indices[s_] < (uint64_t)M->n, "glwe_pack: index out of range");   // glwe_packing.rs:138
        PZ_REQUIRE(cts[s_] != nullptr && is_device_ptr(cts[s_]) && slots[indices[s_]] == nullptr, "glwe_pack: bad or duplicate entry");
        slots[indices[s_]] = cts[s_];
    }
    for (size_t i = 0; i + log_gap_out < log_n; ++i) {
        const size_t tt = (size_t)1 << (log_n - 1 - i);
        PZ_REQUIRE((gals[i] & 1) != 0 && key_pmats[i] != nullptr, "glwe_pack: bad automorphism key");
        for (size_t j = 0; j < tt; ++j) {
            int64_t* a = slots[j];
            int64_t* b = slots[j + tt];
            slots[j + tt] = nullptr;
            PZ_TRY(st.merge(a, b, tt, gals[i], key_pmats[i], &slots[j]));
        }
    }
    PZ_REQUIRE(slots[0] != nullptr, "glwe_pack: no ciphertext ends at index 0");   // :175 a.get(&0).unwrap()
    const size_t skip = log_n - log_gap_out;
    if (trace_size == 0) {   // glwe_copy both ways
        PZ_TRY(launch_ew(M, EW_COPY, res, ct, n, slots[0], ct, n, nullptr, 0, 0, cols * size, B));
        return glwe_trace(M, res, log_n - skip, gals + skip, key_pmats + skip, p, batch);
    }
    return trace_in_key_base(M, res, slots[0], (int64_t*)((char*)tmp + 3 * ctb), trace_size, log_n - skip, gals + skip, key_pmats + skip, p, batch);
}
}  // namespace pz

extern "C" {
int pz_glwe_pack_batched(pz_module* M, int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts, size_t log_gap_out,
                         const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes,
                         size_t batch) {
    PZ_ENTER(M);
    return glwe_pack(M, res, nslots, indices, cts, log_gap_out, gals, key_pmats, p, tmp, tmp_bytes, batch, 0);
}
int pz_glwe_pack_bases_batched(pz_module* M, int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts, size_t log_gap_out,
                               const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, size_t trace_size, void* tmp,
                               size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(trace_size >= 1, "glwe_pack: trace_size = 0");
    return glwe_pack(M, res, nslots, indices, cts, log_gap_out, gals, key_pmats, p, tmp, tmp_bytes, batch, trace_size);
}
}  // extern "C"
