// api_lwe.hip — the LWE glue of the gate bootstrap (BASELINE configs[3]: blind rotation + key switch) on device-resident batches:
//   mod_switch_2n        poulpy-bin-fhe/src/blind_rotation/algorithms/mod.rs:136-176
//   lwe_sample_extract   poulpy-core/src/api/conversion.rs:15-40
//   lwe_keyswitch        poulpy-core/src/keyswitching/lwe.rs:49-94
//   glwe_from_lwe        poulpy-core/src/conversion/lwe_to_glwe.rs:46-121
//   lwe_from_glwe        poulpy-core/src/conversion/glwe_to_lwe.rs:42-90 (one coefficient, and many coefficients in one launch chain)
// and what feeds poulpy-bin-fhe's bdd_arithmetic from FheUint words:
//   ggsw_prepare         on contiguous device GGSWs, one grid
//   fhe_uint_prepare     bdd_arithmetic/ciphertexts/fhe_uint_prepared.rs:399-460
// An LWE is the reference's container: VecZnx(n = n_lwe + 1, one column, `size` limbs), limb i = [b, a_0 .. a_{n_lwe-1}]; a batch is
// `batch` of them back to back.  The embeddings / extractions are index kernels, everything else is the batched key switch.
#include "api_common.hpp"

namespace pz {

struct LweIdx {
    const long long* src;
    long long* dst;
    long long total;        // elements (or element pairs) this launch covers
    int n;                  // ring degree of the GLWE side
    int len;                // n_lwe + 1
    int lwe_size, glwe_size, glwe_cols;
    int min_size;           // limbs that carry data (the rest is zero)
    int base2k, log2n, negate;
};

// mod.rs:136-171: limb 0 (negated for rot_dir = Left), then either rounded down to log2n - 1 bits (base2k > log2n) or extended by
// the following limbs to log2n bits (the low limbs are appended unsigned-shifted and NOT negated, as in the reference)
__global__ void __launch_bounds__(256) k_lwe_mod_switch(LweIdx g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const long long b = idx / g.len;
    const int j = (int)(idx % g.len);
    const long long* lwe = g.src + b * (long long)g.lwe_size * g.len;
    unsigned long long y = (unsigned long long)lwe[j];
    if (g.negate) y = 0ull - y;
    if (g.base2k > g.log2n) {
        const int diff = g.base2k - (g.log2n - 1);
        y = (unsigned long long)((long long)(y + (1ull << (diff - 1))) >> diff);
    } else {
        const int rem = g.base2k - (g.log2n % g.base2k);
        const int size = (g.log2n + g.base2k - 1) / g.base2k;
        for (int i = 1; i < size; ++i) {
            const long long x = lwe[(long long)i * g.len + j];
            if (i == size - 1 && rem != g.base2k) y = (y << (g.base2k - rem)) + (unsigned long long)(x >> rem);
            else y = (y << g.base2k) + (unsigned long long)x;
        }
    }
    g.dst[idx] = (long long)y;
}

// lwe.rs:69-80 / lwe_to_glwe.rs:71-80: a zeroed two-column container of glwe_size limbs; limb i < min_size: b -> X^0 of column 0,
// a_0.. -> the first n_lwe coefficients of column 1.  Two coefficients per thread.
__global__ void __launch_bounds__(256) k_lwe_embed(LweIdx g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // pair index
    if (idx >= g.total) return;
    const int half = g.n >> 1;
    const int jp = (int)(idx % half);
    long long t = idx / half;
    const int col = (int)(t % 2); t /= 2;
    const int limb = (int)(t % g.glwe_size);
    const long long b = t / g.glwe_size;
    long long v0 = 0, v1 = 0;
    if (limb < g.min_size) {
        const long long* lwe = g.src + (b * g.lwe_size + limb) * (long long)g.len;
        const int j = 2 * jp;
        if (col == 0) { if (j == 0) v0 = lwe[0]; }
        else {
            if (j < g.len - 1) v0 = lwe[1 + j];
            if (j + 1 < g.len - 1) v1 = lwe[2 + j];
        }
    }
    *reinterpret_cast<longlong2*>(g.dst + 2 * idx) = make_longlong2(v0, v1);
}

// conversion.rs:28-39: limb i < min_size of the LWE = [X^0 of column 0, the first n_lwe coefficients of column 1]; the other limbs zero
__global__ void __launch_bounds__(256) k_lwe_extract(LweIdx g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const int j = (int)(idx % g.len);
    long long t = idx / g.len;
    const int limb = (int)(t % g.lwe_size);
    const long long b = t / g.lwe_size;
    long long v = 0;
    if (limb < g.min_size) {
        const long long* glwe = g.src + (b * g.glwe_size + limb) * (long long)g.glwe_cols * g.n;
        v = j == 0 ? glwe[0] : glwe[(long long)g.n + (j - 1)];
    }
    g.dst[idx] = v;
}

static int launch_lwe_embed(pz_module* M, long long* dst, int glwe_size, const long long* lwe, int n_lwe, int lwe_size, int min_size, size_t batch) {
    LweIdx g{};
    g.src = lwe; g.dst = dst; g.n = (int)M->n; g.len = n_lwe + 1; g.lwe_size = lwe_size; g.glwe_size = glwe_size; g.glwe_cols = 2;
    g.min_size = min_size;
    g.total = (long long)batch * glwe_size * 2 * (M->n / 2);
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_lwe_embed, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, M->stream, g);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}
static int launch_lwe_extract(pz_module* M, long long* res, int res_n_lwe, int res_size, const long long* glwe, int glwe_cols, int glwe_size,
                              size_t batch) {
    LweIdx g{};
    g.src = glwe; g.dst = res; g.n = (int)M->n; g.len = res_n_lwe + 1; g.lwe_size = res_size; g.glwe_size = glwe_size; g.glwe_cols = glwe_cols;
    g.min_size = std::min(res_size, glwe_size);
    g.total = (long long)batch * res_size * g.len;
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_lwe_extract, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, M->stream, g);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

// api.hip: the batched key switch without taking the module lock (the caller holds it)
int glwe_keyswitch_nolock(pz_module* M, int64_t* res, const int64_t* a, const double* key_pmat, const pz_glwe_op_params* p, size_t batch);
// api_glwe.hip: the key switch of rotated ciphertexts with the rotation applied where the source is read, and the shapes it serves
bool glwe_keyswitch_rot_applies(const pz_module* M, const pz_glwe_op_params* p);
int glwe_keyswitch_rot_nolock(pz_module* M, int64_t* res, const int64_t* a, const RotSrc* rot_tab, const double* key_pmat, const pz_glwe_op_params* p,
                              size_t batch);
// api_br.hip: the constant-mode circuit bootstrapping on plain stream launches, the caller holding the lock
int circuit_bootstrapping_nolock(pz_module* M, int64_t* ggsw, const int64_t* lwe_2n, const int64_t* lut, const double* brk, size_t nsteps,
                                 const int64_t* gals, const double* const* atk_pmats, const double* const* tsk_pmats,
                                 const pz_circuit_bootstrapping_params* p, void* tmp, size_t tmp_bytes, size_t batch);

// ---- lwe_from_glwe at many coefficients ----------------------------------------------------------------------------
// The tail of that call: sample extraction (k_lwe_extract on a two-column GLWE with the LWE's own limb count) and mod_switch_2n
// (k_lwe_mod_switch) in one pass over the key-switched GLWEs - every limb is read once, written to the LWE when the caller wants it, and
// folded into the [b, a_1 .. a_n_lwe] vector the blind rotation reads.
struct LweTail {
    const long long* glwe;   // ciphertext c: `size` limbs x 2 columns x n
    long long* lwe;          // null: the LWE limbs are not written
    long long* lwe_2n;       // null: no mod switch; else dense, ciphertext c at c * len
    long long total;         // ciphertexts * len
    long long row_stride;    // the LWE of ciphertext c lies at LWE slot (c / row_len) * row_stride + c % row_len
    int row_len;
    int n, len, size;
    int base2k, log2n, negate;
};
__global__ void __launch_bounds__(256) k_lwe_extract_switch(LweTail g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.total) return;
    const long long c = idx / g.len;
    const int j = (int)(idx % g.len);
    const long long* src = g.glwe + c * 2ll * g.size * g.n + (j == 0 ? 0 : (long long)g.n + (j - 1));
    long long* out = g.lwe ? g.lwe + ((c / g.row_len) * g.row_stride + c % g.row_len) * (long long)g.size * g.len + j : nullptr;
    // mod.rs:136-171 as k_lwe_mod_switch has it: `ext` limbs take part (one, rounded, when base2k > log2n)
    const int ext = !g.lwe_2n ? 0 : (g.base2k > g.log2n ? 1 : (g.log2n + g.base2k - 1) / g.base2k);
    const int rem = g.base2k - (g.log2n % g.base2k);
    unsigned long long y = 0ull;
    for (int limb = 0; limb < g.size; ++limb) {
        const long long x = src[(long long)limb * 2 * g.n];
        if (out) out[(long long)limb * g.len] = x;
        if (limb >= ext) continue;
        if (limb == 0) {
            y = (unsigned long long)x;
            if (g.negate) y = 0ull - y;
            if (g.base2k > g.log2n) {
                const int diff = g.base2k - (g.log2n - 1);
                y = (unsigned long long)((long long)(y + (1ull << (diff - 1))) >> diff);
            }
        } else if (limb == ext - 1 && rem != g.base2k) y = (y << (g.base2k - rem)) + (unsigned long long)(x >> rem);
        else y = (y << g.base2k) + (unsigned long long)x;
    }
    if (g.lwe_2n) g.lwe_2n[idx] = (long long)y;
}

// the exponent table of the rotation launch: entry c = vals[(c / div) % period] (the values travel as a kernel argument: no host buffer
// has to outlive the call)
constexpr int kRotVals = 128;
struct RotVals { long long v[kRotVals]; };
__global__ void __launch_bounds__(256) k_fill_rot_table(long long* tab, RotVals vals, long long total, int div, int period) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) tab[i] = vals.v[(i / div) % period];
}

// the same for the rotation on load: entry c = (the word ciphertext c rotates, the exponent mod 2n)
__global__ void __launch_bounds__(256) k_fill_rot_src(RotSrc* tab, RotVals vals, long long total, int div, int period, int word_div, int word_mod,
                                                      unsigned mask2n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) tab[i] = RotSrc{(unsigned)((i / word_div) % word_mod), (unsigned)((unsigned long long)vals.v[(i / div) % period]) & mask2n};
}

// usize::BITS - (n2 - 1).leading_zeros() + 1 (mod.rs:139)
static int mod_switch_log2n(size_t n2) {
    int bits = 0;
    for (size_t v = n2 - 1; v; v >>= 1) ++bits;
    return bits + 1;
}
static bool mod_switch_reaches(size_t base2k, size_t lwe_size, size_t n2) {
    const int log2n = mod_switch_log2n(n2);
    return (int)base2k > log2n || lwe_size >= (size_t)((log2n + base2k - 1) / base2k);
}

struct LweManyWs { size_t table, rot, glwe1, total; };
static LweManyWs lwe_many_ws(const pz_module* M, const pz_glwe_op_params* p, size_t ncts) {
    LweManyWs w;
    const size_t n8 = (size_t)M->n * 8;
    w.table = align256(ncts * 8);
    w.rot = align256(ncts * n8 * (p->rank + 1) * p->a_size);
    w.glwe1 = align256(ncts * n8 * 2 * p->res_size);
    w.total = w.table + w.rot + w.glwe1;
    return w;
}

// Where the LWEs and the mod-switched vectors of a pass go.  lwe / lwe_2n may each be null.
struct LweManyOut {
    int64_t* lwe; long long row_len, row_stride;
    int64_t* lwe_2n; size_t n2; int negate;
};
// lwe_from_glwe of `nwords` GLWEs at `nidx` coefficients each, nwords * nidx ciphertexts in one launch chain: the rotated copies (one k_rotate
// whose exponent comes from a device table), one batched key switch, the fused tail.  Ciphertext c of the chain is (word c / nidx, index
// c % nidx) when word_major, (index c / nwords, word c % nwords) otherwise.  Arguments are checked by the callers; tmp holds lwe_many_ws.
static int lwe_from_glwe_rect(pz_module* M, const int64_t* a, size_t nwords, size_t nidx, const size_t* idx, bool word_major, const double* ksk,
                              const pz_glwe_op_params* p, int n_lwe, const LweManyOut& o, void* tmp) {
    const size_t ncts = nwords * nidx;
    if (ncts == 0) return PZ_OK;
    if (word_major && nidx > (size_t)kRotVals) return fail(PZ_ERR_UNSUPPORTED, "lwe_from_glwe_many: more than %d indices per word", kRotVals);
    const long long n = (long long)M->n;
    const int cols = (int)p->rank + 1, ctp = cols * (int)p->a_size;
    const long long ct = n * ctp;
    const LweManyWs w = lwe_many_ws(M, p, ncts);
    char* base = (char*)tmp;
    long long* table = (long long*)base;
    long long* rot = (long long*)(base + w.table);
    long long* glwe1 = (long long*)(base + w.table + w.rot);
    const bool on_load = glwe_keyswitch_rot_applies(M, p);
    if (on_load) {
        // the key switch reads the words through the monomial's index and sign map, in its forward column pass and in its operand load: no rotated copy
        dispatch_note(M, "lwe_from_glwe_many: rotation on load (k_small_one<.., rotated source>, k_lwe_extract_switch)");
        RotSrc* tab = (RotSrc*)base;
        KTimer kt(M, PZ_K_ELEMENTWISE);
        for (size_t j0 = 0; j0 < nidx; j0 += kRotVals) {
            const size_t nj = std::min<size_t>(kRotVals, nidx - j0);
            RotVals vals{};
            for (size_t j = 0; j < nj; ++j) vals.v[j] = -(long long)idx[j0 + j];
            const long long total = (long long)(word_major ? ncts : nj * nwords);
            RotSrc* dst = tab + (word_major ? 0 : (long long)(j0 * nwords));
            // word-major: ciphertext c = (word c / nidx, index c % nidx); index-major: (index c / nwords, word c % nwords)
            hipLaunchKernelGGL(k_fill_rot_src, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, M->stream, dst, vals, total,
                               word_major ? 1 : (int)nwords, word_major ? (int)nidx : kRotVals, word_major ? (int)nidx : 1,
                               word_major ? (int)nwords : (int)nwords, (unsigned)(2 * n - 1));
        }
        PZ_HIP(hipGetLastError());
    } else {
    dispatch_note(M, "lwe_from_glwe_many: materialised rotation (one table-driven k_rotate, one key switch, k_lwe_extract_switch)");
    {
        KTimer kt(M, PZ_K_ELEMENTWISE);
        for (size_t j0 = 0; j0 < nidx; j0 += kRotVals) {
            const size_t nj = std::min<size_t>(kRotVals, nidx - j0);
            RotVals vals{};
            for (size_t j = 0; j < nj; ++j) vals.v[j] = -(long long)idx[j0 + j];
            const long long total = (long long)(word_major ? ncts : nj * nwords);
            long long* dst = table + (word_major ? 0 : (long long)(j0 * nwords));
            hipLaunchKernelGGL(k_fill_rot_table, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, M->stream, dst, vals, total,
                               word_major ? 1 : (int)nwords, word_major ? (int)nidx : kRotVals);
        }
        PZ_HIP(hipGetLastError());
    }
    // polynomial p of the launch = (ciphertext c, polynomial i of it): the source is its word, whatever the index
    const PolyMap sm = word_major ? PolyMap{(int)nidx, ctp, ct, 0, n, 0} : PolyMap{(int)nwords, ctp, 0, ct, n, 0};
    const PolyMap dm{1, 1, n, 0, 0, 0};
    PZ_TRY(launch_rotate(M, (int)(ncts * ctp), (const long long*)a, sm, rot, dm, 0, ctp, table, 1, 0, 0));
    PZ_TRY(glwe_keyswitch_nolock(M, (int64_t*)glwe1, (const int64_t*)rot, ksk, p, ncts));
    }
    if (on_load) PZ_TRY(glwe_keyswitch_rot_nolock(M, (int64_t*)glwe1, a, (const RotSrc*)base, ksk, p, ncts));
    LweTail g{};
    g.glwe = glwe1; g.lwe = (long long*)o.lwe; g.lwe_2n = (long long*)o.lwe_2n; g.n = (int)n; g.len = n_lwe + 1; g.size = (int)p->res_size;
    g.row_len = (int)std::max<long long>(o.row_len, 1); g.row_stride = o.row_stride;
    g.base2k = (int)p->res_base2k; g.log2n = o.lwe_2n ? mod_switch_log2n(o.n2) : 0; g.negate = o.negate ? 1 : 0;
    g.total = (long long)ncts * g.len;
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_lwe_extract_switch, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, M->stream, g);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}
static int lwe_many_checks(pz_module* M, const pz_glwe_op_params* p, size_t res_n_lwe, size_t ncts) {
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(res_n_lwe >= 1 && res_n_lwe <= M->n, "LWE dimension %zu must be in [1, n = %llu]", res_n_lwe, (unsigned long long)M->n);
    PZ_REQUIRE(p->rank >= 1 && p->rank_out == 1, "lwe_from_glwe: the key maps rank -> 1");
    PZ_REQUIRE(p->dsize >= 1 && p->dnum >= 1 && p->key_size >= 1 && p->a_size >= 1 && p->res_size >= 1, "lwe_from_glwe: empty shape");
    PZ_REQUIRE(ncts <= 0x7fffffffull / ((p->rank + 1) * p->a_size), "lwe_from_glwe_many: %zu ciphertexts exceed one launch", ncts);
    return PZ_OK;
}

// ---- ggsw_prepare on a grid ----------------------------------------------------------------------------------------------
// The transform of pz_vmp_prepare (one forward FFT per matrix entry, MatZnx order kept) on `npolys` polynomials: polynomial q is read at
// src + map_off(sm, q) and its spectrum written at dst + map_off(dm, q).  One launch pair per `group` polynomials of pass-1 scratch.
// (POULPY_DBG_PREPARE_GROUP, read per call: a smaller group, so that tests reach the launch pairs per chunk)
static size_t prepare_group(const pz_module* M) {
    const int knob = rt_knob("POULPY_DBG_PREPARE_GROUP", 0);
    if (knob > 0) return (size_t)knob;
    return std::max<size_t>(256, ((size_t)64 << 20) / ((size_t)M->m * sizeof(cplx)));
}
static int ggsw_prepare_polys(pz_module* M, size_t npolys, const int64_t* src, long long src_row, double* dst, long long dst_row, size_t row_polys) {
    // rows of row_polys contiguous polynomials, src_row / dst_row elements between rows
    const long long n = (long long)M->n;
    const size_t group = prepare_group(M);
    cplx* T;
    PZ_TRY(need_T(M, std::min(npolys, group), &T));
    const size_t rows = npolys / row_polys;
    const size_t rows_per = std::max<size_t>(1, group / row_polys);
    if (row_polys > group) {   // (a row wider than the scratch: polynomial ranges of each row)
        for (size_t r = 0; r < rows; ++r)
            for (size_t q0 = 0; q0 < row_polys; q0 += group) {
                const int cnt = (int)std::min(group, row_polys - q0);
                PolyMap sm{cnt, 1, 0, n, 0, (long long)r * src_row + (long long)q0 * n}, dm{cnt, 1, 0, n, 0, (long long)r * dst_row + (long long)q0 * n};
                PZ_TRY(launch_fwd_pass1(M, cnt, (const long long*)src, sm, T));
                PZ_TRY(launch_fwd_pass2(M, cnt, T, dst, dm, nullptr));
            }
        return PZ_OK;
    }
    for (size_t r0 = 0; r0 < rows; r0 += rows_per) {
        const size_t nr = std::min(rows_per, rows - r0);
        const int cnt = (int)(nr * row_polys);
        PolyMap sm{(int)row_polys, 1, src_row, n, 0, (long long)r0 * src_row}, dm{(int)row_polys, 1, dst_row, n, 0, (long long)r0 * dst_row};
        PZ_TRY(launch_fwd_pass1(M, cnt, (const long long*)src, sm, T));
        PZ_TRY(launch_fwd_pass2(M, cnt, T, dst, dm, nullptr));
    }
    return PZ_OK;
}

}  // namespace pz

static int lwe_ptr_checks(pz_module* M, const void* a, const void* b, size_t n_lwe) {
    PZ_REQUIRE(is_device_ptr(a) && is_device_ptr(b), "batched entry points take device pointers");
    PZ_REQUIRE(n_lwe >= 1 && n_lwe <= M->n, "LWE dimension %zu must be in [1, n = %llu]", n_lwe, (unsigned long long)M->n);
    return PZ_OK;
}

extern "C" {

int pz_lwe_mod_switch_2n_batched(pz_module* M, int64_t* res, const int64_t* lwe, size_t n_lwe, size_t lwe_size, size_t base2k, size_t n2,
                                 int negate, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(lwe), "batched entry points take device pointers");
    PZ_REQUIRE(n_lwe >= 1 && lwe_size >= 1, "mod_switch_2n: empty LWE");
    PZ_REQUIRE(base2k >= 1 && base2k <= 62, "base2k %zu out of range", base2k);
    PZ_REQUIRE(n2 >= 2 && n2 <= ((size_t)1 << 40), "mod_switch_2n: n = %zu out of range", n2);
    int bits = 0;
    for (size_t v = n2 - 1; v; v >>= 1) ++bits;
    const int log2n = bits + 1;   // usize::BITS - (n - 1).leading_zeros() + 1  (mod.rs:139)
    if ((int)base2k <= log2n)
        PZ_REQUIRE(lwe_size >= (size_t)((log2n + base2k - 1) / base2k), "mod_switch_2n: %zu limbs of %zu bits do not reach %d bits", lwe_size,
                   base2k, log2n);
    if (batch == 0) return PZ_OK;
    LweIdx g{};
    g.src = (const long long*)lwe; g.dst = (long long*)res; g.len = (int)n_lwe + 1; g.lwe_size = (int)lwe_size;
    g.base2k = (int)base2k; g.log2n = log2n; g.negate = negate ? 1 : 0;
    g.total = (long long)batch * g.len;
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_lwe_mod_switch, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, M->stream, g);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

int pz_lwe_sample_extract_batched(pz_module* M, int64_t* res, size_t res_n_lwe, size_t res_size, const int64_t* a, size_t a_cols,
                                  size_t a_size, size_t batch) {
    PZ_ENTER(M);
    PZ_TRY(lwe_ptr_checks(M, res, a, res_n_lwe));
    PZ_REQUIRE(a_cols >= 2 && res_size >= 1 && a_size >= 1, "lwe_sample_extract: the GLWE needs a mask column and both sides a limb");
    if (batch == 0) return PZ_OK;
    return launch_lwe_extract(M, (long long*)res, (int)res_n_lwe, (int)res_size, (const long long*)a, (int)a_cols, (int)a_size, batch);
}

// lwe.rs:49-94.  p: the rank-1 -> rank-1 key switch (rank = rank_out = 1; a_size / a_base2k = the input LWE's, res_size / res_base2k =
// the output LWE's).  The two intermediate GLWEs live in the module's second workspace.
int pz_lwe_keyswitch_batched(pz_module* M, int64_t* res, size_t res_n_lwe, const int64_t* a, size_t a_n_lwe, const double* ksk_pmat,
                             const pz_glwe_op_params* p, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_TRY(lwe_ptr_checks(M, res, a, res_n_lwe));
    PZ_REQUIRE(a_n_lwe >= 1 && a_n_lwe <= M->n, "LWE dimension %zu must be in [1, n]", a_n_lwe);
    PZ_REQUIRE(p->rank == 1 && p->rank_out == 1, "lwe_keyswitch: the key maps rank 1 -> rank 1 (lwe.rs:70-92)");
    PZ_REQUIRE(p->a_size >= 1 && p->res_size >= 1, "lwe_keyswitch: empty shape");
    if (batch == 0) return PZ_OK;
    const size_t n = M->n;
    const size_t in_b = align256(batch * n * 2 * p->a_size * 8), out_b = align256(batch * n * 2 * p->res_size * 8);
    PZ_TRY(ws2_reserve(M, in_b + out_b));
    char* wbase = (char*)M->ws2;
    long long* glwe_in; long long* glwe_out;
    PZ_TRY(ws_take(M, wbase, in_b, &glwe_in));
    PZ_TRY(ws_take(M, wbase, out_b, &glwe_out));
    PZ_TRY(launch_lwe_embed(M, glwe_in, (int)p->a_size, (const long long*)a, (int)a_n_lwe, (int)p->a_size, (int)p->a_size, batch));
    PZ_TRY(glwe_keyswitch_nolock(M, (int64_t*)glwe_out, (const int64_t*)glwe_in, ksk_pmat, p, batch));
    return launch_lwe_extract(M, (long long*)res, (int)res_n_lwe, (int)p->res_size, glwe_out, 2, (int)p->res_size, batch);
}

// lwe_to_glwe.rs:46-121.  p: the rank 1 -> rank_out key switch; p->a_size = limbs of the intermediate GLWE = ceil(lwe_size * lwe_base2k /
// key_base2k), p->a_base2k must be the key's base (the reference builds it so, :65-70).
int pz_glwe_from_lwe_batched(pz_module* M, int64_t* res, const int64_t* lwe, size_t n_lwe, size_t lwe_size, size_t lwe_base2k,
                             const double* ksk_pmat, const pz_glwe_op_params* p, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_TRY(lwe_ptr_checks(M, res, lwe, n_lwe));
    PZ_REQUIRE(p->rank == 1, "glwe_from_lwe: the key's input rank is 1");
    PZ_REQUIRE(p->a_base2k == p->key_base2k, "glwe_from_lwe: the embedded GLWE has the key's base (lwe_to_glwe.rs:65-70)");
    PZ_REQUIRE(lwe_size >= 1 && lwe_base2k >= 1 && lwe_base2k <= 62, "glwe_from_lwe: bad LWE shape");
    if (batch == 0) return PZ_OK;
    const size_t n = M->n, gsz = p->a_size;
    const bool same = lwe_base2k == p->key_base2k;
    PZ_REQUIRE(!same || lwe_size <= gsz, "glwe_from_lwe: %zu LWE limbs do not fit the %zu limbs of the embedded GLWE", lwe_size, gsz);
    const size_t g_b = align256(batch * n * 2 * gsz * 8), c_b = same ? 0 : align256(batch * n * 2 * lwe_size * 8);
    PZ_TRY(ws2_reserve(M, g_b + c_b));
    char* wbase = (char*)M->ws2;
    long long* glwe; long long* conv;
    PZ_TRY(ws_take(M, wbase, g_b, &glwe));
    PZ_TRY(ws_take(M, wbase, c_b, &conv));
    if (same) {
        PZ_TRY(launch_lwe_embed(M, glwe, (int)gsz, (const long long*)lwe, (int)n_lwe, (int)lwe_size, (int)lwe_size, batch));
    } else {
        // :82-116: each column embedded in the LWE's base, then vec_znx_normalize into the key's base
        PZ_TRY(launch_lwe_embed(M, conv, (int)lwe_size, (const long long*)lwe, (int)n_lwe, (int)lwe_size, (int)lwe_size, batch));
        DV dg{glwe, (long long)(n * 2 * gsz), 2, (int)gsz}, dc{conv, (long long)(n * 2 * lwe_size), 2, (int)lwe_size};
        for (int c = 0; c < 2; ++c) PZ_TRY(dev_normalize(M, (int)batch, dg, (int)p->key_base2k, 0, c, dc, (int)lwe_base2k, c));
    }
    return glwe_keyswitch_nolock(M, res, (const int64_t*)glwe, ksk_pmat, p, batch);
}

// glwe_to_lwe.rs:42-90.  p: the rank -> 1 key switch (rank_out = 1; res_size / res_base2k = the LWE's); a_idx: the coefficient to
// extract (the GLWE is multiplied by X^-a_idx first)
int pz_lwe_from_glwe_batched(pz_module* M, int64_t* res, size_t res_n_lwe, const int64_t* a, size_t a_idx, const double* ksk_pmat,
                             const pz_glwe_op_params* p, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_TRY(lwe_ptr_checks(M, res, a, res_n_lwe));
    PZ_REQUIRE(p->rank >= 1 && p->rank_out == 1, "lwe_from_glwe: the key maps rank -> 1");
    PZ_REQUIRE(a_idx < M->n, "lwe_from_glwe: coefficient index %zu >= n", a_idx);
    if (batch == 0) return PZ_OK;
    const size_t n = M->n, cols = p->rank + 1;
    const size_t in_b = a_idx ? align256(batch * n * cols * p->a_size * 8) : 0, out_b = align256(batch * n * 2 * p->res_size * 8);
    PZ_TRY(ws2_reserve(M, in_b + out_b));
    const long long* src = (const long long*)a;
    char* wbase = (char*)M->ws2;
    long long* rot; long long* glwe1;
    PZ_TRY(ws_take(M, wbase, in_b, &rot));
    PZ_TRY(ws_take(M, wbase, out_b, &glwe1));
    if (a_idx) {
        const int npolys = (int)(batch * cols * p->a_size);
        PolyMap mp{1, 1, (long long)n, 0, 0, 0};
        PZ_TRY(launch_rotate(M, npolys, src, mp, rot, mp, -(long long)a_idx));
        src = rot;
    }
    PZ_TRY(glwe_keyswitch_nolock(M, (int64_t*)glwe1, (const int64_t*)src, ksk_pmat, p, batch));
    return launch_lwe_extract(M, (long long*)res, (int)res_n_lwe, (int)p->res_size, glwe1, 2, (int)p->res_size, batch);
}

// glwe_to_lwe.rs:42-90 at nidx coefficients of each of `batch` GLWEs, index-major
size_t pz_lwe_from_glwe_many_tmp_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t nidx, size_t batch) {
    if (!M || !p) return 0;
    return lwe_many_ws(M, p, nidx * batch).total;
}
int pz_lwe_from_glwe_many_batched(pz_module* M, int64_t* res, size_t res_n_lwe, const int64_t* a, size_t nidx, const size_t* idx,
                                  const double* ksk_pmat, const pz_glwe_op_params* p, int64_t* lwe_2n, size_t n2, int negate, void* tmp,
                                  size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    PZ_TRY(lwe_many_checks(M, p, res_n_lwe, nidx * batch));
    PZ_REQUIRE(ksk_pmat != nullptr && (nidx == 0 || idx != nullptr), "lwe_from_glwe_many: null argument");
    PZ_REQUIRE(res != nullptr || lwe_2n != nullptr, "lwe_from_glwe_many: neither the LWEs nor their mod-switched vectors are asked for");
    PZ_REQUIRE(is_device_ptr(a) && (res == nullptr || is_device_ptr(res)) && (lwe_2n == nullptr || is_device_ptr(lwe_2n)),
               "batched entry points take device pointers");
    for (size_t j = 0; j < nidx; ++j) PZ_REQUIRE(idx[j] < M->n, "lwe_from_glwe_many: coefficient index %zu >= n", idx[j]);
    if (lwe_2n) {
        PZ_REQUIRE(p->res_base2k >= 1 && p->res_base2k <= 62 && n2 >= 2 && n2 <= ((size_t)1 << 40), "lwe_from_glwe_many: mod switch out of range");
        PZ_REQUIRE(mod_switch_reaches(p->res_base2k, p->res_size, n2), "mod_switch_2n: %zu limbs of %zu bits do not reach n2 = %zu",
                   (size_t)p->res_size, (size_t)p->res_base2k, n2);
    }
    if (nidx == 0 || batch == 0) return PZ_OK;
    PZ_REQUIRE(is_device_ptr(tmp) && tmp_bytes >= lwe_many_ws(M, p, nidx * batch).total, "lwe_from_glwe_many: tmp is smaller than pz_lwe_from_glwe_many_tmp_bytes");
    const LweManyOut o{res, 1, 1, lwe_2n, n2, negate};
    return lwe_from_glwe_rect(M, a, batch, nidx, idx, false, ksk_pmat, p, (int)res_n_lwe, o, tmp);
}

int pz_ggsw_prepare_batched(pz_module* M, double* pmat, const int64_t* ggsw, size_t count, size_t dnum, size_t rank, size_t size) {
    PZ_ENTER(M);
    PZ_REQUIRE(dnum >= 1 && rank >= 1 && size >= 1, "ggsw_prepare: empty shape");
    PZ_REQUIRE(is_device_ptr(pmat) && is_device_ptr(ggsw), "batched entry points take device pointers");
    const size_t per = dnum * (rank + 1) * (rank + 1) * size;
    PZ_REQUIRE(count <= 0x7fffffffull / per, "ggsw_prepare: %zu matrices exceed one call", count);
    const size_t bytes = count * per * (size_t)M->n * 8;
    if ((const char*)pmat < (const char*)ggsw + bytes && (const char*)ggsw < (const char*)pmat + bytes)
        return fail(PZ_ERR_ALIAS, "ggsw_prepare: pmat overlaps ggsw");
    if (count == 0) return PZ_OK;
    return ggsw_prepare_polys(M, count * per, ggsw, 0, pmat, 0, count * per);
}

// ---- FheUintPrepared::prepare (fhe_uint_prepared.rs:399-460) on `batch` words; DESIGN.md 4.4g -------------------------------------------------
// tmp = [ks: the words after the ks_glwe key switch, once per word][per pass of `cap` (word, bit) pairs: lwe_many_ws | lwe_2n | GGSWs | the circuit
// bootstrapping's scratch]
struct FheUintWs { size_t ks, many, lwe_2n, ggsw, cbt; size_t fixed() const { return ks; } size_t pass() const { return many + lwe_2n + ggsw + cbt; } };
static FheUintWs fhe_uint_ws(const pz_module* M, const pz_fhe_uint_prepare_params* p, bool with_ks, size_t batch, size_t cap) {
    FheUintWs w;
    const size_t n8 = (size_t)M->n * 8, cols = p->cbt.br.rank + 1;
    w.ks = with_ks ? align256(batch * n8 * (p->ks_glwe.rank_out + 1) * p->ks_glwe.res_size) : 0;
    w.many = lwe_many_ws(M, &p->ks_lwe, cap).total;
    w.lwe_2n = align256(cap * (p->n_lwe + 1) * 8);
    w.ggsw = align256(cap * p->cbt.res_dnum * cols * cols * p->cbt.res_size * n8);
    w.cbt = align256(pz_circuit_bootstrapping_tmp_bytes(M, &p->cbt, cap));
    return w;
}
static bool fhe_uint_word_bits_ok(uint64_t w) { return w == 8 || w == 16 || w == 32 || w == 64 || w == 128; }
// (the query cannot know whether ks_glwe is used: it counts its intermediate whenever the params describe one)
size_t pz_fhe_uint_prepare_tmp_bytes(const pz_module* M, const pz_fhe_uint_prepare_params* p, size_t batch, size_t chunk_bits) {
    if (!M || !p) return 0;
    const size_t pairs = std::min<size_t>(batch * p->bit_count, 65535);
    const size_t cap = chunk_bits ? std::min(chunk_bits, pairs) : pairs;
    const FheUintWs w = fhe_uint_ws(M, p, p->ks_glwe.res_size != 0, batch, cap);
    return w.fixed() + w.pass();
}
int pz_fhe_uint_prepare_batched(pz_module* M, double* res_pmat, int64_t* ggsw_out, int64_t* lwe_out, const int64_t* words,
                                const double* ks_glwe_pmat, const double* ks_lwe_pmat, const int64_t* lut, const double* brk, size_t nsteps,
                                const int64_t* gals, const double* const* atk_pmats, const double* const* tsk_pmats,
                                const pz_fhe_uint_prepare_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(fhe_uint_word_bits_ok(p->word_bits), "fhe_uint_prepare: word_bits = %llu is not one of 8 / 16 / 32 / 64 / 128", (unsigned long long)p->word_bits);
    PZ_REQUIRE(M->n % p->word_bits == 0, "fhe_uint_prepare: n = %llu is no multiple of word_bits = %llu", (unsigned long long)M->n, (unsigned long long)p->word_bits);
    PZ_REQUIRE(p->bit_start <= p->word_bits && p->bit_count <= p->word_bits - p->bit_start, "fhe_uint_prepare: bits [%llu, %llu) leave the word",
               (unsigned long long)p->bit_start, (unsigned long long)(p->bit_start + p->bit_count));
    PZ_REQUIRE(res_pmat != nullptr && words != nullptr && ks_lwe_pmat != nullptr && lut != nullptr && brk != nullptr && atk_pmats != nullptr &&
                   tsk_pmats != nullptr && (nsteps == 0 || gals != nullptr),
               "fhe_uint_prepare: null argument");
    for (size_t s = 0; s < nsteps; ++s) PZ_REQUIRE(atk_pmats[s] != nullptr, "fhe_uint_prepare: null automorphism key");
    for (size_t c = 0; c < p->cbt.br.rank; ++c) PZ_REQUIRE(tsk_pmats[c] != nullptr, "fhe_uint_prepare: null tensor key");
    PZ_REQUIRE(is_device_ptr(res_pmat) && is_device_ptr(words) && (ggsw_out == nullptr || is_device_ptr(ggsw_out)) &&
                   (lwe_out == nullptr || is_device_ptr(lwe_out)),
               "batched entry points take device pointers");
    const bool with_ks = ks_glwe_pmat != nullptr;
    const pz_glwe_op_params* kl = &p->ks_lwe;
    PZ_REQUIRE(p->n_lwe == p->cbt.br.n_lwe && p->lwe_size >= 1 && p->lwe_base2k >= 1 && p->lwe_base2k <= 62, "fhe_uint_prepare: bad LWE shape");
    PZ_TRY(lwe_many_checks(M, kl, p->n_lwe, 1));
    PZ_REQUIRE(kl->res_size == p->lwe_size && kl->res_base2k == p->lwe_base2k, "fhe_uint_prepare: ks_lwe's result is the LWE (size, base2k)");
    if (with_ks) {
        const pz_glwe_op_params* kg = &p->ks_glwe;
        PZ_REQUIRE(kg->dsize >= 1 && kg->dnum >= 1 && kg->key_size >= 1 && kg->a_size >= 1 && kg->res_size >= 1 && kg->rank >= 1 && kg->rank_out >= 1,
                   "fhe_uint_prepare: empty ks_glwe shape");
        PZ_REQUIRE(kl->rank == kg->rank_out && kl->a_size == kg->res_size && kl->a_base2k == kg->res_base2k,
                   "fhe_uint_prepare: ks_lwe reads what ks_glwe writes (rank, size, base2k)");
    }
    PZ_REQUIRE(p->cbt.extension_factor <= 1, "fhe_uint_prepare: extension_factor = 1 (fhe_uint_prepared.rs:431)");
    PZ_REQUIRE(p->cbt.res_dnum >= 1 && p->cbt.res_size >= 1 && p->cbt.br.rank >= 1, "fhe_uint_prepare: empty GGSW shape");
    const size_t n2 = 2 * (size_t)M->n;
    PZ_REQUIRE(mod_switch_reaches(p->lwe_base2k, p->lwe_size, n2), "mod_switch_2n: %llu limbs of %llu bits do not reach n2 = %zu",
               (unsigned long long)p->lwe_size, (unsigned long long)p->lwe_base2k, n2);
    if (batch == 0) return PZ_OK;
    const long long n = (long long)M->n;
    const size_t cols = p->cbt.br.rank + 1, wb = p->word_bits, nb = p->bit_count, b0 = p->bit_start;
    const size_t gpolys = p->cbt.res_dnum * cols * cols * p->cbt.res_size;   // polynomials of one GGSW
    PZ_REQUIRE(batch <= 0x7fffffffull / (wb * gpolys), "fhe_uint_prepare: %zu words exceed one call", batch);
    // the largest pass that fits tmp (at most 65535 pairs: the blind rotation's limit)
    size_t cap = 0;
    if (nb > 0) {
        PZ_REQUIRE(is_device_ptr(tmp), "batched entry points take device pointers");
        size_t lo = 0, hi = std::min<size_t>(batch * nb, 65535);
        auto fits = [&](size_t c) { const FheUintWs w = fhe_uint_ws(M, p, with_ks, batch, c); return w.fixed() + w.pass() <= tmp_bytes; };
        while (lo < hi) {
            const size_t mid = (lo + hi + 1) / 2;
            if (fits(mid)) lo = mid; else hi = mid - 1;
        }
        cap = lo;
        PZ_REQUIRE(cap >= 1, "fhe_uint_prepare: tmp holds no (word, bit) pair (pz_fhe_uint_prepare_tmp_bytes)");
    }
    // ggsw_zero on the bits outside [bit_start, bit_start + bit_count) (fhe_uint_prepared.rs:453-459)
    const long long gsw = (long long)gpolys * n, word_gsw = (long long)wb * gsw;
    auto zero_bits = [&](void* basep, size_t first, size_t count) -> int {
        if (!basep || count == 0) return PZ_OK;
        return launch_ew(M, EW_ZERO, (long long*)basep + (long long)first * gsw, word_gsw, n, nullptr, 0, 0, nullptr, 0, 0, (int)(count * gpolys), (int)batch);
    };
    PZ_TRY(zero_bits(res_pmat, 0, b0));
    PZ_TRY(zero_bits(res_pmat, b0 + nb, wb - b0 - nb));
    PZ_TRY(zero_bits(ggsw_out, 0, b0));
    PZ_TRY(zero_bits(ggsw_out, b0 + nb, wb - b0 - nb));
    if (nb == 0) return PZ_OK;
    // bit i lives at coefficient bit_index(i) << log_gap (bdd_arithmetic/mod.rs:97-99, fhe_uint.rs:384)
    int log_bytes = 0;
    while (((size_t)8 << log_bytes) < wb) ++log_bytes;
    const size_t gap = (size_t)M->n / wb;
    std::vector<size_t> coef(nb);
    for (size_t i = 0; i < nb; ++i) {
        const size_t bit = b0 + i;
        coef[i] = ((((bit & 7) << log_bytes) | (bit >> 3))) * gap;
    }
    const FheUintWs w = fhe_uint_ws(M, p, with_ks, batch, cap);
    char* base = (char*)tmp;
    int64_t* ks = (int64_t*)base;
    void* many_tmp = base + w.ks;
    int64_t* lwe_2n = (int64_t*)(base + w.ks + w.many);
    int64_t* gg = (int64_t*)(base + w.ks + w.many + w.lwe_2n);
    void* cbt_tmp = base + w.ks + w.many + w.lwe_2n + w.ggsw;
    // get_bit_lwe's first key switch (fhe_uint.rs:385-394) does not depend on the bit: once per word
    const int64_t* src = words;
    if (with_ks) {
        PZ_TRY(glwe_keyswitch_nolock(M, ks, words, ks_glwe_pmat, &p->ks_glwe, batch));
        src = ks;
    }
    const long long src_ct = n * (long long)(kl->rank + 1) * (long long)kl->a_size;
    const long long lwe_len = (long long)(p->n_lwe + 1) * (long long)p->lwe_size;
    // passes: whole words while a word fits, else bit ranges of one word
    const size_t words_per = cap >= nb ? cap / nb : 1, bits_per = cap >= nb ? nb : cap;
    for (size_t w0 = 0; w0 < batch; w0 += words_per) {
        const size_t nw = std::min(words_per, batch - w0);
        for (size_t i0 = 0; i0 < nb; i0 += bits_per) {
            const size_t ni = std::min(bits_per, nb - i0), np = nw * ni;
            LweManyOut o{lwe_out ? lwe_out + ((long long)(w0 * nb + i0)) * lwe_len : nullptr, (long long)ni, (long long)nb, lwe_2n, n2, 1};
            PZ_TRY(lwe_from_glwe_rect(M, src + (long long)w0 * src_ct, nw, ni, coef.data() + i0, true, ks_lwe_pmat, kl, (int)p->n_lwe, o, many_tmp));
            PZ_TRY(circuit_bootstrapping_nolock(M, gg, lwe_2n, lut, brk, nsteps, gals, atk_pmats, tsk_pmats, &p->cbt, cbt_tmp, w.cbt, np));
            const long long first = ((long long)w0 * (long long)wb + (long long)(b0 + i0)) * gsw;
            if (ggsw_out)
                PZ_TRY(launch_ew(M, EW_COPY, ggsw_out + first, word_gsw, n, gg, (long long)ni * gsw, n, nullptr, 0, 0, (int)(ni * gpolys), (int)nw));
            PZ_TRY(ggsw_prepare_polys(M, np * gpolys, gg, (long long)ni * gsw, res_pmat + first, word_gsw, ni * gpolys));
        }
    }
    return finish_call(M, false);
}

}  // extern "C"
