// api_glwe.hip — the batched GLWE product behind the C ABI: GLWE (x) GGSW external product, GLWE key switch, the glwe_automorphism family,
// tensor relinearization.  The engine (shapes, workspace models, GlweCall, the three pipelines, glwe_op), the host-container path of the four GLWE
// entry points, and the hoisted rotations (pz_glwe_automorphism_many_batched), which drive the fused pipeline's pieces directly.  The composites
// live in their own units: api_ggsw.hip, api_gates.hip, api_bdd.hip, api_trace.hip, api_br.hip, api_fhe_uint.hip; glwe_call.hpp is what they see.
// Reference call stacks: poulpy-core/src/external_product/glwe.rs:99-271, keyswitching/glwe.rs:53-380, automorphism/glwe_ct.rs:51-275,
// operations/glwe.rs:541-607.
//
// glwe_op = validate -> pick the pipeline for the shape -> per wave of ciphertexts, the launch sequence of that pipeline:
//   fused      pass 1 | row pass + VMP + inverse row pass | tail         (plans with 128 / 256-point rows; the measured path)
//                per family: plain / spectral automorphism / cross-base output / digits (dsize > 1, a table for the middle kernel) / N = 4096 two-kernel
//   small ring whole forward transform | product + whole inverse + carry chain   (N = 1024 / 2048)
//   five-kernel the reference's op sequence, one kernel per HAL op                (every other shape; fusion switched off)
// One definition of "which pipeline" serves the call and the workspace query (pz_glwe_op_workspace_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "api_common.hpp"
#include "glwe_call.hpp"

using namespace pz;

// ------------------------------------------------------------------------------
// host containers at the batched GLWE entry points (what the Rust shim's CoreImpl overrides pass: poulpy-hal buffers are host
// addressable by contract).  Ciphertexts are staged like any per-op argument; prepared keys get a device mirror (api.hip).
// ------------------------------------------------------------------------------
struct GlweArgs {
    Stage sa, sr;
    int64_t* res = nullptr;
    const int64_t* a = nullptr;
    const double* key = nullptr;
    bool host = false;
};
static int glwe_args_in(pz_module* M, GlweArgs& g, int64_t* res, const int64_t* a, const double* pmat, size_t res_bytes, size_t a_bytes,
                        size_t key_bytes) {
    PZ_REQUIRE(res != nullptr && a != nullptr && pmat != nullptr, "null argument");
    PZ_TRY(resolve_key(M, pmat, key_bytes, &g.key));
    PZ_TRY(g.sa.in(a, a_bytes, true, false, M));
    if ((const void*)res == (const void*)a) {   // *_assign forms
        PZ_REQUIRE(res_bytes == a_bytes, "in-place call with different layouts for a and res");
        g.sr.M = M; g.sr.dev = g.sa.dev; g.sa.out = true;
    } else {
        PZ_TRY(g.sr.in(res, res_bytes, false, true, M));
    }
    g.res = (int64_t*)g.sr.dev; g.a = (const int64_t*)g.sa.dev;
    g.host = g.sa.owned || g.sr.owned;
    return PZ_OK;
}
static int glwe_args_out(pz_module* M, GlweArgs& g) {
    PZ_TRY(g.sr.finish());
    PZ_TRY(g.sa.finish());
    return finish_call(M, g.host);
}

// ------------------------------------------------------------------------------
// shapes, workspaces, pipeline choice
// ------------------------------------------------------------------------------
// (OpShape: glwe_call.hpp)
// external product; key switch / automorphism (mask columns 1.. of a GLWE); tensor relinearization (operations/glwe.rs:541-607: `a` is
// a GLWETensor of cols + pairs columns, the pairs = rank (rank + 1) / 2 columns behind the first cols = rank + 1 are key-switched
// and the first cols are added to every column of the big value)
static inline bool kind_ks(GlweKind k) { return k != GlweKind::ExternalProduct; }   // the product is gglwe_product_dft, as for a key switch
OpShape op_shape(const pz_glwe_op_params* p, GlweKind kind) {
    OpShape s;
    const bool ks = kind_ks(kind);
    if (kind == GlweKind::TensorRelin) {
        const int cols = (int)p->rank + 1, pairs = (int)(p->rank * (p->rank + 1) / 2);
        s.cols_a = cols + pairs; s.cols_in = pairs; s.cols_out = cols; s.a_col0 = cols;
        s.convert = p->a_base2k != p->key_base2k;
        s.a_size_eff = s.convert ? (int)((p->a_size * p->a_base2k + p->key_base2k - 1) / p->key_base2k) : (int)p->a_size;
        return s;
    }
    s.a_col0 = ks ? 1 : 0;
    s.cols_a = (int)p->rank + 1;
    s.cols_in = ks ? (int)p->rank : (int)p->rank + 1;
    s.cols_out = ks ? (int)p->rank_out + 1 : (int)p->rank + 1;
    s.convert = p->a_base2k != p->key_base2k;
    s.a_size_eff = s.convert ? (int)((p->a_size * p->a_base2k + p->key_base2k - 1) / p->key_base2k) : (int)p->a_size;
    return s;
}

struct OpWs {
    size_t a_conv, a_dft, res_dft, tmp_dft, T, res_tmp, total;
};
static OpWs op_ws(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, size_t chunk, GlweKind kind) {
    OpWs w;
    const bool ks = kind_ks(kind), au = kind == GlweKind::Automorphism;
    const size_t n8 = (size_t)M->n * 8;
    const size_t dsz = p->dsize;
    w.a_conv = s.convert ? align256(chunk * n8 * s.cols_a * s.a_size_eff) : 0;
    w.a_dft = align256(chunk * n8 * s.cols_in * (size_t)s.a_size_eff);
    w.res_dft = align256(chunk * n8 * s.cols_out * p->key_size);
    w.tmp_dft = dsz > 1 ? align256(chunk * n8 * (s.cols_out * p->key_size + (ks ? s.cols_in * (size_t)s.a_size_eff : 0))) : 0;
    const size_t tp = std::max((size_t)s.cols_in * s.a_size_eff, (size_t)s.cols_out * p->key_size);
    w.T = align256(chunk * tp * (size_t)M->m * sizeof(cplx));
    w.res_tmp = au ? align256(chunk * n8 * s.cols_out * p->res_size) : 0;  // normalized result before the final permutation
    w.total = w.a_conv + w.a_dft + w.res_dft + w.tmp_dft + w.T + w.res_tmp;
    return w;
}
size_t pick_chunk(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, size_t batch) {
    if (M->chunk) return std::min(M->chunk, batch);
    // Measured on MI355X (profiles/r01_chunk_sweep.txt, r01_batch_sweep.txt): the intermediates do not stay in the Infinity
    // Cache anyway and every wave re-streams the key and pays the pipeline fill of the persistent middle kernel, so larger
    // waves win (128 -> 1024 ciphertexts per wave: +13 %); cap the workspace at ~24 GiB of the 288 GB.
    const size_t per_ct = (size_t)M->n * 8 * ((size_t)s.cols_in * s.a_size_eff + 2 * (size_t)s.cols_out * p->key_size);
    size_t c = ((size_t)24 << 30) / std::max<size_t>(per_ct, 1);
    c = std::max<size_t>(c & ~(size_t)7, 8);
    return std::min(c, batch);
}

// which pipeline glwe_op takes for a shape, and what it reserves there (one definition for the call and for the workspace query)
bool fused_applies(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, GlweKind kind) {
    const bool tensor = kind == GlweKind::TensorRelin, au = kind == GlweKind::Automorphism;
    const int npi = s.cols_in * s.a_size_eff, npo = s.cols_out * (int)p->key_size;
    const bool digits = p->dsize > 1, cross_out = p->res_base2k != p->key_base2k;
    return M->fuse_mid && M->fuse_tail && tail_supported(M) && mid_supported(M, npi, npo) && !(tensor && s.convert) &&
           (!(digits || cross_out) || (M->plan.m2 == 128 && !au && (int)p->dnum * s.cols_in <= 255 && npo <= 255));
}
struct FusedWs {
    size_t key, conv, t, t2, rtmp, small2, total;
};
// Placement of T2' relative to the result: the tail of ciphertext b reads T2' + X and writes res + X and res + X + N*4 bytes (the two
// coefficient halves), the same X for every workgroup; with both buffers on the same 1 MiB phase (large allocations are 2 MiB aligned)
// the read and the two write streams of every workgroup meet on the same HBM channels: tail 3.55 ms per 1024 ciphertexts in most
// processes, 3.14 in some, depending on the physical pages (profiles/r02_t2_placement.txt).  T2' therefore sits 768 KiB out of phase
// with the result (mod 4 MiB).  Rounds 2-3 MEASURED the phase per call shape (eight candidates, an event pair each); on every box of
// round 3 and round 4 the tuned and the fixed placement measured the same (99 952 vs 99 181/s, 99 142 vs 98 445/s: noise), so the tuner,
// its shape cache and its two ABI functions were removed in round 4 (ABI version 4).
static constexpr size_t kT2Phase = 0xC0000, kT2PhaseMask = 0x3FFFFF;
static FusedWs fused_ws(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, size_t chunk, bool au) {
    FusedWs w;
    const size_t n8 = (size_t)M->n * 8, ksz = p->key_size;
    const size_t npi = (size_t)s.cols_in * s.a_size_eff, npo = (size_t)s.cols_out * ksz;
    w.key = align256((size_t)p->dnum * s.cols_in * npo * n8);
    w.conv = s.convert ? align256(chunk * n8 * s.cols_a * s.a_size_eff) : 0;
    w.t = align256(chunk * npi * M->m * sizeof(cplx));
    w.t2 = align256(chunk * npo * M->m * sizeof(cplx));
    // res_tmp holds the normalized result before the final permutation (mode 0 / gather scheme) OR, in the spectral form, the
    // body-column operand (min(a_size, key_size) limbs of one column): sized for the larger of the two
    const size_t body_limbs = std::min<size_t>((size_t)s.a_size_eff, ksz);
    w.rtmp = au ? align256(chunk * n8 * std::max((size_t)s.cols_out * p->res_size, body_limbs)) : 0;
    // cross-base output: the tail's key-base digits (cols_out x key_size limbs per ciphertext) before the cross-base pass
    w.small2 = p->res_base2k != p->key_base2k ? align256(chunk * n8 * s.cols_out * ksz) : 0;
    w.total = w.key + w.conv + w.t + w.t2 + w.rtmp + w.small2 + kMidDummyBytes + (kT2PhaseMask + 1);
    return w;
}
// N = 1024 / 2048: the two-kernel pipeline of device_small.hpp (plain products, key switches and the automorphism family; dsize 1, one
// base2k, <= 4 key limbs); `packed` = no OpLayout (the automorphism family needs it)
bool small_ring_applies(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, GlweKind kind, bool packed) {
    const bool ks = kind_ks(kind), tensor = kind == GlweKind::TensorRelin, au = kind == GlweKind::Automorphism;
    const bool cross_out = p->res_base2k != p->key_base2k;   // (with an automorphism: phi and the cross-base pass do not commute)
    return M->small_path && M->fuse_mid && M->fuse_tail && M->n < 4096 && (!au || (ks && packed && !cross_out)) &&
           !tensor && p->dsize == 1 && M->dbg_stages == 7 && small_supported(M, s.cols_in * s.a_size_eff, (int)p->key_size);
}
struct SmallWs {
    size_t key, spectra, conv, digits, total;
};
static SmallWs small_ws(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, size_t chunk) {
    SmallWs w;
    const size_t n8 = (size_t)M->n * 8;
    w.key = align256((size_t)p->dnum * s.cols_in * s.cols_out * p->key_size * n8);                       // the key re-sliced
    w.spectra = align256(chunk * (size_t)(s.cols_in * s.a_size_eff) * (size_t)M->m * sizeof(cplx));      // the spectra of one wave
    w.conv = s.convert ? align256(chunk * n8 * s.cols_a * s.a_size_eff) : 0;
    w.digits = p->res_base2k != p->key_base2k ? align256(chunk * n8 * s.cols_out * p->key_size) : 0;    // key-base digits before the cross-base pass
    w.total = w.key + w.spectra + w.conv + w.digits;
    return w;
}

// (GlweCall, everything a call of glwe_op derives from its arguments before it launches anything: glwe_call.hpp)

extern "C" {
// keyswitch: 0 external product, 1 key switch, 2 automorphism family, 3 tensor relinearization.  The figure is what the call reserves
// in the module's grow-only workspace (+ the 12.5 % growth slack of its first allocation); a key that is neither pinned nor mirrored
// costs its row-sliced copy, which is included.
size_t pz_glwe_op_workspace_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t batch, int keyswitch) {
    if (!M || !p || p->key_size == 0 || p->a_size == 0) return 0;
    if (keyswitch < 0 || keyswitch > 3) return 0;
    const GlweKind kind = (GlweKind)keyswitch;
    const OpShape s = op_shape(p, kind);
    const size_t chunk = pick_chunk(M, p, s, batch);
    size_t bytes;
    if (fused_applies(M, p, s, kind)) bytes = fused_ws(M, p, s, chunk, kind == GlweKind::Automorphism).total;
    else if (small_ring_applies(M, p, s, kind, true)) bytes = small_ws(M, p, s, chunk).total;
    else bytes = op_ws(M, p, s, chunk, kind).total;
    return bytes + (bytes >> 3);
}
}

// ------------------------------------------------------------------------------
// pieces shared by the pipelines
// ------------------------------------------------------------------------------
// the wave's input in the key's base: `a` itself, or glwe_normalize into a_conv (external_product/glwe.rs:124-132)
static int wave_input(const GlweCall& c, size_t b0, int nb, int64_t* a_conv, DV* av) {
    if (c.diff) { *av = DV{nullptr, c.a_bs, c.s.cols_a, (int)c.p->a_size}; return PZ_OK; }   // (CMUX, fused routes: the forward stage reads c.diff)
    if (c.rot_tab) { *av = DV{(void*)c.a, c.a_bs, c.s.cols_a, (int)c.p->a_size}; return PZ_OK; }   // (the table names the source ciphertext: no wave offset)
    *av = DV{(void*)(c.a + (long long)b0 * c.a_bs), c.a_bs, c.s.cols_a, (int)c.p->a_size};
    if (!c.s.convert) return PZ_OK;
    DV cv{a_conv, c.n * c.s.cols_a * c.s.a_size_eff, c.s.cols_a, c.s.a_size_eff};
    for (int col = 0; col < c.s.cols_a; ++col)
        PZ_TRY(dev_normalize(c.M, nb, cv, (int)c.p->key_base2k, 0, col, *av, (int)c.p->a_base2k, col));
    *av = cv;
    return PZ_OK;
}
// the permuted copy of the key a pipeline reads: the pinned / mirrored one if the caller declared the key immutable, else built now
// the cached row-sliced copy of `key` if the caller pinned it with this call's key shape, else null
static const cplx* pinned_slices(const GlweCall& c, const double* key) {
    const size_t bytes = (size_t)c.nrows * c.ncols * (size_t)c.M->n * 8;
    for (auto& pk : c.M->pinned)
        if (pk.key == (const void*)key && pk.sliced && pk.bytes == bytes) return pk.sliced;
    return nullptr;
}
static int wave_key(const GlweCall& c, cplx* scratch, bool small_ring, const cplx** out) {
    // (key composition: the slices of phi_g(key), built per call in the call's own scratch - never a pinned key's cached copy, and never into it)
    if (c.keyauto) { PZ_TRY(launch_permute_pmat_gal(c.M, c.pmat, scratch, c.nrows * c.ncols, c.ka_perm)); *out = scratch; return PZ_OK; }
    if (const cplx* pinned = pinned_slices(c, c.pmat)) { *out = pinned; return PZ_OK; }
    // the key arrives in the standard device layout; its row-sliced copy is rebuilt per call (2 x 128 MiB of traffic at the metric
    // shape, ~4 % of a 128-ciphertext call) so that no stale copy can ever be used
    if (small_ring) PZ_TRY(launch_small_permute(c.M, c.pmat, scratch, c.nrows * c.ncols));
    else if (c.M->dbg_stages & 2) PZ_TRY(launch_permute_pmat(c.M, c.pmat, scratch, c.nrows * c.ncols));
    *out = scratch;
    return PZ_OK;
}
// the tail of a wave with everything at its defaults for this call (row-major T2', key-base limbs in, res out)
static TailCall wave_tail(const GlweCall& c, int nb, const cplx* T2, size_t b0) {
    TailCall t;
    t.batch = nb; t.T = T2; t.rowmajor = true; t.nlimbs = c.ksz; t.ncols = c.s.cols_out;
    t.res = (long long*)c.res_at(b0); t.res_bs = c.res_bs; t.res_cols = c.s.cols_out; t.res_size = (int)c.p->res_size;
    t.base2k = (int)c.p->res_base2k;
    t.body_col = c.body_col;
    return t;
}
static void tail_operand(TailCall& t, const DV& av, bool every_column) {
    t.small = (const long long*)av.p; t.small_bs = av.bs; t.small_cols = av.cols; t.small_size = av.size; t.small_all = every_column;
}
// the same for a wave on the small-ring kernels: the key and shape, the result at its defaults (res, in its own base), the key switch's operand
static SmallKey small_key(const GlweCall& c, const cplx* Pp) { return SmallKey{Pp, c.npi, c.nrows, c.ncols, c.s.cols_out, c.ksz}; }
static SmallRes small_res(const GlweCall& c, size_t b0) {
    return SmallRes{(long long*)c.res_at(b0), c.res_bs, c.s.cols_out, (int)c.p->res_size, (int)c.p->res_base2k};
}
static SmallOperand small_operand(const GlweCall& c, const DV& av, size_t b0) {
    if (c.add) return SmallOperand{(const long long*)(c.add + (long long)b0 * c.add_bs), c.add_bs, c.s.cols_out, c.add_size, -1};   // CMUX: + f on every column
    return SmallOperand{c.ks ? (const long long*)av.p : nullptr, av.bs, c.s.cols_a, av.size, c.body_col};
}
// conditional swap: the wave's part of the second result, which is its own operand
static SmallRes small_res2(const GlweCall& c, size_t b0) {
    if (!c.res2) return SmallRes{};
    return SmallRes{(long long*)c.res2_at(b0), c.res2_bs, c.s.cols_out, c.res2_size, (int)c.p->res_base2k};
}
static SmallOperand small_operand2(const GlweCall& c, size_t b0) {
    if (!c.res2) return SmallOperand{};
    return SmallOperand{(const long long*)c.res2_at(b0), c.res2_bs, c.s.cols_out, c.res2_size, -1};
}
// CMUX: the wave's part of the every-column operand f, and of the two sources of the fused forward stage
static DV wave_add(const GlweCall& c, size_t b0) { return DV{(void*)(c.add + (long long)b0 * c.add_bs), c.add_bs, c.s.cols_out, c.add_size}; }
static SmallDiff wave_diff(const GlweCall& c, size_t b0) {
    SmallDiff d = *c.diff;
    if (d.t) d.t += (long long)b0 * d.tmap.sb;
    d.f += (long long)b0 * d.fmap.sb;
    return d;
}
// ... and the automorphism form of the inverse kernel, with glwe_trace's shifted store where asked for
static void small_inv_auto(SmallInvCall& sc, const GlweCall& c, bool rsh) {
    sc.au = c.au != nullptr; sc.au_p = c.au_p; sc.au_mode = c.au ? c.au->mode : 0; sc.post_rsh = rsh;
}

// dsize > 1 (external_product/glwe.rs:235-267, keyswitching/glwe.rs:332-379) as a table for the middle kernel: limb l of `a` is digit
// di = (dsize - 1 - l) mod dsize, element k = (l - (dsize - 1 - di)) / dsize of that digit's vector (vec_znx_dft_apply with step dsize,
// offset dsize - 1 - di); the vector has (a_size + di) / dsize elements (at most dnum for a key switch) and multiplies key rows k (all
// input columns) with limb_offset di, into a result of key_size - max(dsize - di - 2, 0) limbs (zero-tail semantics of SURVEY.md A.2)
static MidDigits digit_terms(const GlweCall& c) {
    MidDigits dg;
    const int dsize = c.dsize;
    for (int l = 0; l < c.s.a_size_eff; ++l) {
        const int di = ((dsize - 1 - l) % dsize + dsize) % dsize;
        const int k = (l - (dsize - 1 - di)) / dsize;
        int a_sz = (c.s.a_size_eff + di) / dsize;
        if (c.ks) a_sz = std::min(a_sz, c.dnum);
        if (k < 0 || k >= a_sz || k >= c.dnum) continue;
        const int r_sz = c.ksz - std::max(dsize - di - 2, 0);
        const int off = di * c.s.cols_out;
        const int cb = off < c.ncols ? std::min(c.s.cols_out * r_sz, c.ncols - off) : 0;
        if (cb <= 0) continue;
        for (int col = 0; col < c.s.cols_in; ++col) {
            dg.in[dg.n] = (unsigned char)(l * c.s.cols_in + col);
            dg.row[dg.n] = (unsigned char)(k * c.s.cols_in + col);
            dg.coff[dg.n] = (unsigned char)off;
            dg.cb[dg.n] = (unsigned char)cb;
            ++dg.n;
        }
    }
    return dg;
}

// ------------------------------------------------------------------------------
// fused pipeline
// ------------------------------------------------------------------------------
struct FusedBufs {
    cplx* key_scratch; int64_t* a_conv; cplx* T; cplx* T2; int64_t* res_tmp; int64_t* key_digits; cplx* mid_dummy;
    const cplx* Pp;
    short* side16 = nullptr;   // this wave's 16-bit side copy of pass 1's input (add / sub automorphism forms at rank 1: wave_spectral_tail), or null
    const short* body16_pre = nullptr;   // plain form, hoisted rotations (glwe_rotations_hoisted): this rotation's 16-bit body operand, already written
};
static int fused_carve(const GlweCall& c, FusedBufs* f) {
    pz_module* M = c.M;
    const FusedWs fw = fused_ws(M, c.p, c.s, c.chunk, c.au != nullptr);
    PZ_TRY(ws_reserve(M, fw.total));
    char* base = (char*)M->ws;
    PZ_TRY(ws_take(M, base, fw.key, &f->key_scratch));
    PZ_TRY(ws_take(M, base, fw.conv, &f->a_conv));
    PZ_TRY(ws_take(M, base, fw.t, &f->T));
    base += (kT2Phase - (size_t)(((uintptr_t)base - (uintptr_t)c.res) & kT2PhaseMask)) & kT2PhaseMask;   // see kT2Phase
    PZ_TRY(ws_take(M, base, fw.t2, &f->T2));
    PZ_TRY(ws_take(M, base, fw.rtmp, &f->res_tmp));
    PZ_TRY(ws_take(M, base, fw.small2, &f->key_digits));
    PZ_TRY(ws_take(M, base, kMidDummyBytes, &f->mid_dummy));
    return PZ_OK;
}

// N = 4096, plain external product / key switch / automorphism with <= 4 key limbs: two kernels, the spectra cross HBM once
// (device_small.hpp).  (round 3: the 8-slot tile of k_mid128r - 8 polynomials in, 8 out, 8 product rows: the external product with 4
// limbs, BASELINE configs[1] - beats the two-kernel form, 3.25 vs 3.16 M/s, profiles/r03_ab_small_vs_pipeline.txt)
bool n4096_two_kernel(const GlweCall& c) {
    const pz_module* M = c.M;
    // (CMUX at that shape stays on the two kernels: their forward stage forms the difference itself, where the pipeline needs it written out first
    //  and its tail takes the every-column operand - 2.51 against 2.05 M gates / s at batch 4096, profiles/cmux_lines.txt)
    const bool mid8 = !c.ks && !c.au && !c.add && c.npi == 8 && c.npo == 8 && std::min(c.nrows, c.npi) == 8;
    return M->small_path && (!c.au || (c.ks && !c.lay)) && !c.tensor && !c.digits && !c.cross_out &&
           M->dbg_stages == 7 && small_supported(M, c.npi, c.ksz) && !mid8;
}
// which pipeline serves the product of a CMUX, and whether its forward stage can take the two sources
bool cmux_fused_route(const GlweCall& c) {
    if (fused_applies(c.M, c.p, c.s, c.kind)) return n4096_two_kernel(c);
    return small_ring_applies(c.M, c.p, c.s, c.kind, true);
}
static int wave_n4096_two_kernel(const GlweCall& c, const FusedBufs& f, size_t b0, int nb, const DV& av, const PolyMap& sm) {
    const bool rsh = c.want_rsh && c.au && c.au->mode != 0 && c.p->res_base2k <= 29;
    if (c.diff) {
        dispatch_note(c.M, "%s: fused small two-kernel (k_small_fwd<.., difference> -> k_small_inv)", gate_name(c));
        PZ_TRY(launch_small_fwd_diff(c.M, nb * c.npi, wave_diff(c, b0), f.T));
    } else PZ_TRY(launch_small_fwd(c.M, nb * c.npi, (const long long*)av.p, sm, f.T));
    SmallInvCall sc;
    sc.S = f.T; sc.key = small_key(c, f.Pp); sc.res = small_res(c, b0); sc.small = small_operand(c, av, b0);
    sc.res2 = small_res2(c, b0); sc.small2 = small_operand2(c, b0);
    small_inv_auto(sc, c, rsh);
    PZ_TRY(launch_small_inv(c.M, nb, sc));
    if (rsh) *c.post_rsh = true;
    return PZ_OK;
}

// Spectral form of the automorphism family (m2 = 128 plans).  X -> X^p with p = 1 mod 4: DFT(phi(a))[q] = DFT(a)[p q + (p-1)/4 mod m] is an
// affine map of the spectrum index that sends rows of the four-step layout to rows, so the middle kernel writes its product at the
// permuted position (k_mid128<.., PERM>) and the tail's inverse transform is phi(big) itself.  p = 3 mod 4 (X -> X^-1, the first step of
// every trace, among them): the spectrum of phi(a) is the CONJUGATE of a permuted spectrum (MidArgs::perm_ysign).  (SpectralPerm: internal.hpp)
static SpectralPerm spectral_perm(const GlweCall& c) {
    SpectralPerm sp;
    sp.on = c.au && c.M->plan.m2 == 128 && c.M->dbg_stages == 7;
    if (!sp.on) return sp;
    const unsigned mm = (unsigned)c.M->m;
    if ((c.au_p & 3u) == 1u) {
        sp.mul = c.au_g & (mm - 1u);
        const unsigned long long c0 = (unsigned long long)(((c.au_p - 1u) >> 2) & (mm - 1u));
        sp.add = (unsigned)((mm - (unsigned)(((unsigned long long)sp.mul * c0) & (unsigned long long)(mm - 1u))) & (mm - 1u));
    } else {
        sp.conj = true;
        sp.mul = (mm - (c.au_g & (mm - 1u))) & (mm - 1u);                                            // (-p)^-1 mod m
        const unsigned long long c0 = (unsigned long long)((((unsigned long long)c.au_p + 1ull) >> 2) & (unsigned long long)(mm - 1u));
        sp.add = (unsigned)(((unsigned long long)sp.mul * c0) & (unsigned long long)(mm - 1u));      // (-p)^-1 (p + 1)/4
    }
    return sp;
}
// The tail of the spectral form adds ONE operand stream per column at the natural index: +-a[col] and, on the body column, the stream
// prepared here by one k_automorphism pass over that column into the (cache-resident) workspace - phi(body) for the plain form,
// +-phi(body) + a0 for add / sub / sub_negate.  No permutation pass over the result, no gathers in the tail, in-place forms safe.
// whether the spectral tail takes its body-column operand as 16-bit copies (see wave_spectral_tail)
static bool spectral_body16(const GlweCall& c) {
    pz_module* M = c.M;
    const long long n = c.n;
    return !M->probe && (!c.want_rsh || (c.au_big && (int)c.p->key_base2k <= 14 && (int)c.p->res_base2k <= 29)) &&
           n >= 4096 && n <= 65536 && (int)c.p->key_base2k <= (c.au_big ? 15 : 16) && (int)c.p->res_base2k <= 31 && tail_rsh_supported(M);
}
static int wave_spectral_tail(const GlweCall& c, const FusedBufs& f, size_t b0, int nb, const DV& av) {
    pz_module* M = c.M;
    const long long n = c.n;
    const int bl = std::min(av.size, c.ksz);   // the tail reads operand limbs j < min(key_size, a_size) only: the pre-pass covers exactly those
    PolyMap bsm{bl, 1, av.bs, (long long)av.cols * n, 0, 0}, bdm{bl, 1, (long long)bl * n, n, 0, 0};
    TailCall t = wave_tail(c, nb, f.T2, b0);
    tail_operand(t, av, true);
    // phi(body): prepared by a pre-pass in the workspace.  (Gathering it in the tail itself is bit-exact and saves a kernel, but the tail goes
    // from 5.05 to 8.3 - 8.8 ms against 1.8 - 3.0 for the pre-pass: 16 dependent 8-byte gathers per thread and limb in front of the carry chain,
    // profiles/r04_ab_auto_fold.txt.)
    // Round 6, plain form: the pre-pass leaves phi(body) as 16-bit values in the tail's own tile order (2 B written and 2 B read per coefficient
    // instead of 8) where the digits are expected to fit - a key base of at most 16 bits - and the body column then rides on the f64 chain of the
    // sign-only tail with that operand (k_inv_tail<.., NZF = 7, SGN>) instead of the operand variant's integer chain.  A value that does not fit
    // (un-normalized input) raises a device flag, and the wave then runs exactly the i64 scheme: a second, CONDITIONAL pre-pass writes the i64 operand
    // over the copies (its blocks return at once while the flag is down), the 16-bit form of the tail returns at once and the operand variant, launched
    // beside it and returning at once while the flag is down, does the column.  In-place calls included (both pre-passes read the input before any
    // tail writes); with the shifted store of glwe_trace too (k_inv_tail<..,RSH,7,SGN>: the one-bit shift behind the f64 chain).
    // (not under the rounding-margin probe: its instantiation of the tail keeps the i64 operand - the values that are rounded are the same)
    // (add / sub forms: the operand phi(body) +- a0 is a sum of two digits - a key base of at most 15 bits; the other columns keep their 8-byte operand)
    // (glwe_trace's steps, want_rsh: their input is the previous step's - or the initial shift's - normalized output, so with a base of at most 14 bits
    //  the operand always fits and the flag-up launches of the shifted-store forms stay what they are there: never taken)
    const bool body16 = spectral_body16(c);   // (glwe_fused zeroed the flag word in front of pass 1: that kernel may raise it too, f.side16)
    if (body16) dispatch_note(M, "spectral tail: 16-bit body operand (%s form)", c.au_big ? "add / sub" : "plain");
    // (hoisted rotations: the copy of this Galois element was made from the one read of the body column all rotations share - the i64 fallback keeps
    //  its own segment, res_tmp, so that it never lands on the copy of a rotation whose tail has not run yet)
    short* b16 = body16 ? (f.body16_pre ? const_cast<short*>(f.body16_pre) : (short*)f.res_tmp) : nullptr;
    if (body16) {
        t.body16 = b16; t.body16_limbs = bl; t.body16_wide = M->wide16();
        if (f.side16 && c.au_big) t.other16 = f.side16;
    }
    t.body_src = (const long long*)f.res_tmp; t.body_bs = (long long)bl * n; t.body_ls = n;
    const int cond = body16 ? AUTO_IF_WIDE : 0;   // (the i64 pre-pass only if the flag is up)
    if (!c.au_big) {
        // plain form, res = phi(normalize(big)) (glwe_ct.rs:65-71): the inverse transform is phi(big) with phi's signs; the tail undoes
        // them in front of the carry chain (auto_mul) and puts them back on the digits (post_neg); only the body column has an operand
        if (body16 && !f.body16_pre) PZ_TRY(launch_automorphism(M, nb * bl, (const long long*)av.p, bsm, nullptr, bdm, c.au_g, AUTO_SIGN, nullptr, PolyMap{1, 1, 0, 0, 0, 0}, b16));
        PZ_TRY(launch_automorphism(M, nb * bl, (const long long*)av.p, bsm, (long long*)f.res_tmp, bdm, c.au_g, AUTO_SIGN | cond));
        t.auto_mul = c.au_g; t.post_neg = true; t.body_only = true;
        return launch_inv_tail(M, t);
    }
    // operand of the body column, one stream: phi(body) + a0 (add) or -phi(body) + a0 (sub forms: the tail negates every operand)
    const bool rsh = c.want_rsh && tail_rsh_supported(M) && !c.cross_out && c.p->res_base2k <= 29;   // (32-bit shift steps: device_fft.hpp)
    // (16-bit scheme: the pre-pass writes the operand the chain adds - phi(body) + a0 (add), phi(body) - a0 (sub forms; the i64 scheme stores
    //  -phi(body) + a0 and lets the tail negate it))
    if (body16) PZ_TRY(launch_automorphism(M, nb * bl, (const long long*)av.p, bsm, nullptr, bdm, c.au_g, c.au->mode == 1 ? AUTO_SIGN : (AUTO_SIGN | AUTO_SUB16), (const long long*)av.p, bsm, b16));
    PZ_TRY(launch_automorphism(M, nb * bl, (const long long*)av.p, bsm, (long long*)f.res_tmp, bdm, c.au_g, (c.au->mode == 1 ? AUTO_SIGN : (AUTO_SIGN | AUTO_NEGATE)) | cond,
                               (const long long*)av.p, bsm));
    if (c.au->mode == 3) { t.auto_mul = 2u * (unsigned)n; t.auto_neg = true; }   // a - phi(big): every sign flipped
    t.small_neg = c.au->mode != 1;
    t.post_rsh = rsh;
    PZ_TRY(launch_inv_tail(M, t));
    if (rsh) *c.post_rsh = true;
    return PZ_OK;
}
// res_base2k != key_base2k: vec_znx_big_normalize(res_base2k <- key_base2k) in two exact steps - the tail's carry chain writes balanced
// key-base digits (all key_size limbs: nothing is dropped), the cross-base kernel converts them.  Both steps are functions of the torus
// value only, so the result equals the reference's single cross-base pass over the big value (checked on the oracle over thousands of
// random shapes / edge digits, and by the parity tests).
static int wave_cross_base_tail(const GlweCall& c, const FusedBufs& f, size_t b0, int nb, const DV& av) {
    const long long tmp_ct = c.n * c.s.cols_out * (long long)c.ksz;
    TailCall t = wave_tail(c, nb, f.T2, b0);
    t.res = (long long*)f.key_digits; t.res_bs = tmp_ct; t.res_size = c.ksz; t.base2k = (int)c.p->key_base2k;
    if (c.ks) tail_operand(t, av, c.tensor);
    PZ_TRY(launch_inv_tail(c.M, t));
    DV tv{f.key_digits, tmp_ct, c.s.cols_out, c.ksz}, rv{c.res_at(b0), c.res_bs, c.s.cols_out, (int)c.p->res_size};
    for (int col = 0; col < c.s.cols_out; ++col)
        PZ_TRY(dev_normalize(c.M, nb, rv, (int)c.p->res_base2k, 0, col, tv, (int)c.p->key_base2k, col));
    return PZ_OK;
}
// plain product / key switch / relinearization, and the automorphism family where the spectral form does not apply (m2 = 256 plan, or
// dbg_stages != 7): the tail gathers -+phi^-1(a) (+ body) itself, writes into res_tmp, one permutation pass follows
static int wave_plain_tail(const GlweCall& c, const FusedBufs& f, size_t b0, int nb, const DV& av) {
    pz_module* M = c.M;
    if (M->dbg_stages & 4) {
        TailCall t = wave_tail(c, nb, f.T2, b0);
        if (c.au) { t.res = (long long*)f.res_tmp; t.res_bs = c.res_ct; }
        if (c.ks) tail_operand(t, av, c.au_big || c.tensor);
        else if (c.add) tail_operand(t, wave_add(c, b0), true);   // CMUX: + f on every column
        if (c.a16) { t.small16 = c.a16 + (long long)b0 * av.size * c.n; t.small16_cs = c.a16_cs; t.small_bs = 0; }
        if (c.au_big) { t.auto_mul = c.au_p; t.gather_mul = c.au_p; t.gather_neg = c.au->mode != 1; }
        t.auto_neg = c.au && c.au->mode == 3;
        PZ_TRY(launch_inv_tail(M, t));
        if (c.res2) {   // conditional swap: the big value in T2' (the tail only reads it) once more - negated in front of the chain, operand res2
            TailCall t2 = wave_tail(c, nb, f.T2, b0);
            t2.res = (long long*)c.res2_at(b0); t2.res_bs = c.res2_bs; t2.res_size = c.res2_size;
            tail_operand(t2, DV{(void*)c.res2_at(b0), c.res2_bs, c.s.cols_out, c.res2_size}, true);
            t2.big_neg = true;
            PZ_TRY(launch_inv_tail(M, t2));
        }
    }
    if (c.au) {
        PolyMap tm{(int)c.p->res_size, c.s.cols_out, c.res_ct, (long long)c.s.cols_out * c.n, c.n, 0};
        PZ_TRY(launch_automorphism(M, nb * (int)c.p->res_size * c.s.cols_out, (const long long*)f.res_tmp, tm, (long long*)c.res_at(b0), tm, c.au_g,
                                   c.au->mode == 0 ? AUTO_SIGN : AUTO_PLAIN));
    }
    return PZ_OK;
}

// Key composition, fast form.  For one entry the reference computes phi_g(normalize(KS_K(phi_p(a)))), g = p^-1 (gglwe_atk.rs:77-107).  phi is a
// ring automorphism, so with the limbs of `a` entering the product as they are (dsize 1, one base2k)
//   phi_g(sum_j phi_p(a_j) K_j + phi_p(a_0)) = sum_j a_j phi_g(K_j) + a_0 :
// the big value at the NATURAL index is a plain key switch of the unpermuted `a` by phi_g(K) (wave_key / KeyPerm), body operand a_0 as it is.
// The carry chain does not commute with phi's signs (normalize(-x) != -normalize(x) on the tie 2^(base2k-1)): the reference normalizes
// phi_p(B) and permutes back, i.e. s .* normalize(s .* B) per coefficient with s(i) the sign phi_p gives source index i - auto_mul = p in
// front of the chain, post_neg behind it, no index map anywhere.
static int wave_keyauto_tail(const GlweCall& c, const FusedBufs& f, size_t b0, int nb, const DV& av) {
    TailCall t = wave_tail(c, nb, f.T2, b0);
    tail_operand(t, av, false);
    t.auto_mul = c.ka_p; t.post_neg = true; t.keyauto = true;
    return launch_inv_tail(c.M, t);
}

int glwe_fused(const GlweCall& c) {
    pz_module* M = c.M;
    FusedBufs f;
    PZ_TRY(fused_carve(c, &f));
    PZ_TRY(wave_key(c, f.key_scratch, false, &f.Pp));
    const MidDigits dg = c.digits ? digit_terms(c) : MidDigits{};
    const SpectralPerm sp = spectral_perm(c);
    const bool two_kernel = n4096_two_kernel(c);
    for (size_t b0 = 0; b0 < c.batch; b0 += c.chunk) {
        const int nb = (int)std::min(c.chunk, c.batch - b0);
        DV av;
        PZ_TRY(wave_input(c, b0, nb, f.a_conv, &av));
        PolyMap sm{av.size, c.s.cols_in, av.bs, (long long)av.cols * c.n, c.n, c.n * c.s.a_col0};
        if (two_kernel) { PZ_TRY(wave_n4096_two_kernel(c, f, b0, nb, av, sm)); continue; }
        f.side16 = nullptr;
        if (sp.on && spectral_body16(c)) {
            PZ_TRY(launch_zero_bytes(M, M->margin + 1, 8));   // the wide flag (module.hpp: wide16), in front of everything that may raise it
            // add / sub forms at rank 1 (one mask column = the key switch's input): pass 1 also leaves its input as 16-bit values for the tail's other
            // column, behind the body operand's segment of res_tmp when there is room (16 res_size - 8 bl >= 2 a_size limbs' worth per ciphertext)
            const int bl_ = std::min(av.size, c.ksz);
            if (c.au_big && c.s.cols_in == 1 && c.s.cols_out == 2 && !c.digits && !c.a16 && (M->dbg_stages & 1) &&
                16 * (long long)c.p->res_size - 8 * (long long)bl_ >= 2 * (long long)av.size)
                f.side16 = (short*)((char*)f.res_tmp + (size_t)nb * bl_ * c.n * 8);
        }
        if (c.a16) {
            PolyMap s16{av.size, c.s.cols_in, (long long)av.size * c.n, c.n, c.a16_cs, c.a16_cs * c.s.a_col0};
            PZ_TRY(launch_fwd_pass1_t16(M, nb * c.npi, c.a16 + (long long)b0 * av.size * c.n, s16, f.T));
        } else if (f.side16) {
            PZ_TRY(launch_fwd_pass1_w16(M, nb * c.npi, (const long long*)av.p, sm, f.T, f.side16));
        } else if (M->dbg_stages & 1) {
            PZ_TRY(launch_fwd_pass1(M, nb * c.npi, (const long long*)av.p, sm, f.T, true));
        }
        if (c.digits && dg.n == 0) {   // nothing reaches the product (e.g. dsize > a.size): the big value is the body alone
            PZ_TRY(launch_zero_bytes(M, f.T2, (size_t)nb * c.npo * M->m * sizeof(cplx)));
        } else if (M->dbg_stages & 2) {
            MidCall mc;
            mc.T = f.T; mc.T2 = f.T2; mc.Pp = f.Pp; mc.dummy = f.mid_dummy; mc.npi = c.npi; mc.npo = c.npo; mc.nrows = c.nrows; mc.ncols = c.ncols;
            mc.perm = sp; mc.digits = c.digits ? &dg : nullptr;
            PZ_TRY(launch_mid(M, nb, mc));
        }
        if (c.keyauto) PZ_TRY(wave_keyauto_tail(c, f, b0, nb, av));
        else if (sp.on) PZ_TRY(wave_spectral_tail(c, f, b0, nb, av));
        else if (c.cross_out) PZ_TRY(wave_cross_base_tail(c, f, b0, nb, av));
        else PZ_TRY(wave_plain_tail(c, f, b0, nb, av));
    }
    return PZ_OK;
}

// ------------------------------------------------------------------------------
// N = 1024 / 2048: no pipeline plan (their per-op split is 16 x 32 / 32 x 32), but whole polynomials fit LDS: the two-kernel pipeline of
// device_small.hpp with its own m = M1 x 128 tables.  Mixed bases as in the fused pipeline: `a` re-expressed in the key's base first; a
// result in another base = balanced key-base digits from the inverse kernel (all key limbs), then one cross-base pass.  The automorphism
// family rides along: phi is an index / sign map inside the inverse kernel's carry-chain stage.
// ------------------------------------------------------------------------------
int glwe_small_ring(const GlweCall& c) {
    pz_module* M = c.M;
    const SmallWs w = small_ws(M, c.p, c.s, c.chunk);
    PZ_TRY(ws_reserve(M, w.total));
    char* base = (char*)M->ws;
    cplx* key_scratch; cplx* S; int64_t* a_conv; int64_t* key_digits;
    PZ_TRY(ws_take(M, base, w.key, &key_scratch));
    PZ_TRY(ws_take(M, base, w.spectra, &S));
    PZ_TRY(ws_take(M, base, w.conv, &a_conv));
    PZ_TRY(ws_take(M, base, w.digits, &key_digits));
    const cplx* Pp;
    PZ_TRY(wave_key(c, key_scratch, true, &Pp));
    const bool rsh = c.want_rsh && c.au && c.au->mode != 0 && !c.cross_out && c.p->res_base2k <= 29;
    for (size_t b0 = 0; b0 < c.batch; b0 += c.chunk) {
        const int nb = (int)std::min(c.chunk, c.batch - b0);
        DV av;
        PZ_TRY(wave_input(c, b0, nb, a_conv, &av));
        PolyMap sm{av.size, c.s.cols_in, av.bs, (long long)av.cols * c.n, c.n, c.n * c.s.a_col0};
        const SmallKey key = small_key(c, Pp);
        const SmallOperand body = small_operand(c, av, b0);
        const SmallDiff wd = c.diff ? wave_diff(c, b0) : SmallDiff{};
        // plain product / key switch of a rank-1 ciphertext: one kernel, the spectra never leave the CU (round 6, device_small_one.hpp)
        if (!c.au && !c.cross_out && small_one_supported(M, c.npi, c.nrows, c.ncols, c.s.cols_out, c.ksz, nb)) {
            if (c.diff) dispatch_note(M, "%s: fused small-one (k_small_one<.., difference>)", gate_name(c));
            PZ_TRY(launch_small_one(M, nb, SmallOneCall{(const long long*)av.p, sm, key, small_res(c, b0), body, c.diff ? &wd : nullptr,
                                                        small_res2(c, b0), small_operand2(c, b0), c.rot_tab ? c.rot_tab + b0 : nullptr}));
            continue;
        }
        if (c.rot_tab) return fail(PZ_ERR_UNSUPPORTED, "rotated-source key switch: the one-kernel small-ring form only");
        if (c.diff) {
            dispatch_note(M, "%s: fused small two-kernel (k_small_fwd<.., difference> -> k_small_inv)", gate_name(c));
            PZ_TRY(launch_small_fwd_diff(M, nb * c.npi, wd, S));
        } else PZ_TRY(launch_small_fwd(M, nb * c.npi, (const long long*)av.p, sm, S));
        SmallInvCall sc;
        sc.S = S; sc.key = key; sc.res = small_res(c, b0); sc.small = body;
        sc.res2 = small_res2(c, b0); sc.small2 = small_operand2(c, b0);
        if (c.cross_out) {
            const long long tmp_ct = c.n * c.s.cols_out * (long long)c.ksz;
            sc.res = SmallRes{(long long*)key_digits, tmp_ct, c.s.cols_out, c.ksz, (int)c.p->key_base2k};
            PZ_TRY(launch_small_inv(M, nb, sc));
            DV tv{key_digits, tmp_ct, c.s.cols_out, c.ksz}, rv{c.res_at(b0), c.res_bs, c.s.cols_out, (int)c.p->res_size};
            for (int col = 0; col < c.s.cols_out; ++col)
                PZ_TRY(dev_normalize(M, nb, rv, (int)c.p->res_base2k, 0, col, tv, (int)c.p->key_base2k, col));
            continue;
        }
        small_inv_auto(sc, c, rsh);
        PZ_TRY(launch_small_inv(M, nb, sc));
    }
    if (rsh) *c.post_rsh = true;
    return PZ_OK;
}

// ------------------------------------------------------------------------------
// five-kernel path: the reference's op sequence, one batched kernel per HAL op (every shape; what the fused pipelines are tested against)
// ------------------------------------------------------------------------------
struct UnfusedBufs {
    int64_t* a_conv; double* a_dft; double* res_dft; double* tmp_dft; cplx* T; int64_t* res_tmp;
};
// a_dft <- DFT of the input limbs, res_dft <- VMP; returns the limbs of res_dft that carry the result
static int wave_unfused_product(const GlweCall& c, const UnfusedBufs& u, int nb, const DV& av, DV rd, int* res_dft_size) {
    pz_module* M = c.M;
    const long long n = c.n;
    const int a_size = av.size, a_col0 = c.s.a_col0;   // key-switch transforms the mask columns only (keyswitching/glwe.rs:231-234)
    *res_dft_size = c.ksz;
    if (c.dsize == 1) {
        DV ad{u.a_dft, n * c.s.cols_in * a_size, c.s.cols_in, a_size};
        PZ_TRY(dev_dft_apply(M, nb, 1, 0, ad, 0, av, a_col0, c.s.cols_in, nullptr, u.T));
        return dev_vmp(M, nb, rd, ad, c.pmat, c.dnum, c.s.cols_in, c.s.cols_out, c.ksz, 0);
    }
    // external_product/glwe.rs:235-267 ; keyswitching/glwe.rs:332-379
    // res_dft starts zeroed (glwe.rs:122): limbs skipped by the first iterations are only ever added to
    PZ_TRY(launch_zero_bytes(M, u.res_dft, (size_t)nb * rd.bs * 8));
    DV td{u.tmp_dft, n * c.s.cols_out * c.ksz, c.s.cols_out, c.ksz};
    for (int di = 0; di < c.dsize; ++di) {
        int a_sz = (a_size + di) / c.dsize;
        if (c.ks) a_sz = std::min(a_sz, c.dnum);
        const int drop = std::max(c.dsize - di - 2, 0);
        *res_dft_size = c.ksz - drop;
        DV ad{u.a_dft, n * c.s.cols_in * a_sz, c.s.cols_in, a_sz};
        PZ_TRY(dev_dft_apply(M, nb, c.dsize, c.dsize - 1 - di, ad, 0, av, a_col0, c.s.cols_in, nullptr, u.T));
        DV rdi{u.res_dft, rd.bs, c.s.cols_out, *res_dft_size};
        if (di == 0) {
            PZ_TRY(dev_vmp(M, nb, rdi, ad, c.pmat, c.dnum, c.s.cols_in, c.s.cols_out, c.ksz, 0));
        } else {
            DV tdi{u.tmp_dft, td.bs, c.s.cols_out, *res_dft_size};
            PZ_TRY(dev_vmp(M, nb, tdi, ad, c.pmat, c.dnum, c.s.cols_in, c.s.cols_out, c.ksz, di));
            PZ_TRY(launch_ew(M, EW_ADD, u.res_dft, rd.bs, n, u.res_dft, rd.bs, n, u.tmp_dft, td.bs, n, c.s.cols_out * *res_dft_size, nb));
        }
    }
    // keyswitching/glwe.rs:378 res.set_size(res.max_size()): limbs dropped by the last iterations keep the value of the earlier ones
    if (c.ks) *res_dft_size = c.ksz;
    return PZ_OK;
}
// automorphism family, op by op as the reference: big value, body, [automorphism of the big value, +- a], normalize, [automorphism]
static int wave_unfused_auto(const GlweCall& c, const UnfusedBufs& u, int nb, const DV& av, DV rb, DV rv) {
    pz_module* M = c.M;
    const long long n = c.n;
    const int a_size = av.size, L = rb.size;
    PZ_TRY(dev_idft(M, nb, rb, 0, rb, 0, c.s.cols_out, L, u.T));
    const long long big_ls = (long long)c.s.cols_out * n, a_ls = (long long)av.cols * n;
    PZ_TRY(launch_ew(M, EW_ADD_I64, u.res_dft, rb.bs, big_ls, u.res_dft, rb.bs, big_ls, av.p, av.bs, a_ls, std::min(L, a_size), nb));
    DV nsrc = rb;
    if (c.au_big) {
        int64_t* big2 = (int64_t*)u.T;  // free again: same bytes as the big value
        PolyMap bm{L, c.s.cols_out, rb.bs, big_ls, n, 0};
        PZ_TRY(launch_automorphism(M, nb * L * c.s.cols_out, (const long long*)u.res_dft, bm, (long long*)big2, bm, c.au_g, AUTO_SIGN));
        const int sum = std::min(L, a_size);
        for (int col = 0; col < c.s.cols_out; ++col) {
            int64_t* bc = big2 + (long long)col * n;
            const int64_t* ac = (const int64_t*)av.p + (long long)col * n;
            if (c.au->mode == 1) PZ_TRY(launch_ew(M, EW_ADD_I64, bc, rb.bs, big_ls, bc, rb.bs, big_ls, ac, av.bs, a_ls, sum, nb));
            else if (c.au->mode == 2) PZ_TRY(launch_ew(M, EW_SUB_I64, bc, rb.bs, big_ls, bc, rb.bs, big_ls, ac, av.bs, a_ls, sum, nb));
            else {  // a - big, and -big where a has no limb (vec_znx/sub.rs:84-110)
                PZ_TRY(launch_ew(M, EW_SUB_I64, bc, rb.bs, big_ls, ac, av.bs, a_ls, bc, rb.bs, big_ls, sum, nb));
                PZ_TRY(launch_ew(M, EW_NEG_I64, bc + (long long)sum * big_ls, rb.bs, big_ls, bc + (long long)sum * big_ls, rb.bs, big_ls,
                                 nullptr, 0, 0, L - sum, nb));
            }
        }
        nsrc = DV{big2, rb.bs, c.s.cols_out, L};
    }
    DV nd = c.au->mode == 0 ? DV{u.res_tmp, c.res_ct, c.s.cols_out, (int)c.p->res_size} : rv;
    for (int col = 0; col < c.s.cols_out; ++col)
        PZ_TRY(dev_normalize(M, nb, nd, (int)c.p->res_base2k, 0, col, nsrc, (int)c.p->key_base2k, col));
    if (c.au->mode == 0) {
        PolyMap tm{(int)c.p->res_size, c.s.cols_out, c.res_ct, (long long)c.s.cols_out * n, n, 0};
        PZ_TRY(launch_automorphism(M, nb * (int)c.p->res_size * c.s.cols_out, (const long long*)u.res_tmp, tm, (long long*)rv.p, tm, c.au_g, AUTO_SIGN));
    }
    return PZ_OK;
}
int glwe_unfused(const GlweCall& c) {
    pz_module* M = c.M;
    const long long n = c.n;
    const OpWs w = op_ws(M, c.p, c.s, c.chunk, c.kind);
    PZ_TRY(ws_reserve(M, w.total));
    char* base = (char*)M->ws;
    UnfusedBufs u;
    PZ_TRY(ws_take(M, base, w.a_conv, &u.a_conv));
    PZ_TRY(ws_take(M, base, w.a_dft, &u.a_dft));
    PZ_TRY(ws_take(M, base, w.res_dft, &u.res_dft));
    PZ_TRY(ws_take(M, base, w.tmp_dft, &u.tmp_dft));
    PZ_TRY(ws_take(M, base, w.T, &u.T));
    PZ_TRY(ws_take(M, base, w.res_tmp, &u.res_tmp));
    for (size_t b0 = 0; b0 < c.batch; b0 += c.chunk) {
        const int nb = (int)std::min(c.chunk, c.batch - b0);
        const DV raw_av{(void*)(c.a + (long long)b0 * c.a_bs), c.a_bs, c.s.cols_a, (int)c.p->a_size};
        DV av;
        PZ_TRY(wave_input(c, b0, nb, u.a_conv, &av));
        DV rd{u.res_dft, n * c.s.cols_out * c.ksz, c.s.cols_out, c.ksz};
        int res_dft_size = c.ksz;
        PZ_TRY(wave_unfused_product(c, u, nb, av, rd, &res_dft_size));
        DV rb{u.res_dft, rd.bs, c.s.cols_out, res_dft_size};
        DV rv{(void*)c.res_at(b0), c.res_bs, c.s.cols_out, (int)c.p->res_size};
        if (c.au) {
            PZ_TRY(wave_unfused_auto(c, u, nb, av, rb, rv));
        } else if (!c.res2 && c.p->res_base2k == c.p->key_base2k && M->fuse_tail && tail_supported(M)) {
            // inverse pass 2, then the fused tail: inverse pass 1 + body add + carry chain, no VecZnxBig in HBM
            PolyMap sm{res_dft_size, c.s.cols_out, rb.bs, (long long)c.s.cols_out * n, n, 0};
            PZ_TRY(launch_inv_pass2(M, nb * res_dft_size * c.s.cols_out, u.res_dft, sm, u.T));
            // (tensor: every column receives its operand; with a conversion the reference still adds the UN-normalized a when
            //  res_base2k == key_base2k, operations/glwe.rs:588-592)
            TailCall t;
            t.batch = nb; t.T = u.T; t.rowmajor = false; t.nlimbs = res_dft_size; t.ncols = c.s.cols_out;
            t.res = (long long*)rv.p; t.res_bs = rv.bs; t.res_cols = rv.cols; t.res_size = rv.size; t.base2k = (int)c.p->res_base2k;
            t.body_col = c.body_col;
            if (c.ks) tail_operand(t, c.tensor ? raw_av : av, c.tensor);
            else if (c.add) tail_operand(t, wave_add(c, b0), true);
            PZ_TRY(launch_inv_tail(M, t));
        } else {
            PZ_TRY(dev_idft(M, nb, rb, 0, rb, 0, c.s.cols_out, res_dft_size, u.T));
            const long long big_ls = (long long)c.s.cols_out * n;
            if (c.res2) {   // conditional swap, eval.rs:455-459: the i64 big value feeds both normalizations - first b - big (limbs of big beyond b:
                            // negated, vec_znx_big_sub_small_a) into the transform scratch (free again: the bytes of the big value) and from there into res2
                int64_t* big2 = (int64_t*)u.T;
                const int sum = std::min(res_dft_size, c.res2_size);
                for (int col = 0; col < c.s.cols_out; ++col) {
                    int64_t* bc = big2 + (long long)col * n;
                    const int64_t* xc = (const int64_t*)u.res_dft + (long long)col * n;
                    const int64_t* oc = c.res2_at(b0) + (long long)col * n;
                    PZ_TRY(launch_ew(M, EW_SUB_I64, bc, rb.bs, big_ls, oc, c.res2_bs, big_ls, xc, rb.bs, big_ls, sum, nb));
                    PZ_TRY(launch_ew(M, EW_NEG_I64, bc + (long long)sum * big_ls, rb.bs, big_ls, xc + (long long)sum * big_ls, rb.bs, big_ls, nullptr, 0, 0,
                                     res_dft_size - sum, nb));
                }
                DV r2{(void*)c.res2_at(b0), c.res2_bs, c.s.cols_out, c.res2_size}, b2{big2, rb.bs, c.s.cols_out, res_dft_size};
                for (int col = 0; col < c.s.cols_out; ++col)
                    PZ_TRY(dev_normalize(M, nb, r2, (int)c.p->res_base2k, 0, col, b2, (int)c.p->key_base2k, col));
            }
            if (c.tensor) {  // operations/glwe.rs:588-598: + a[col] on every column (raw a when res_base2k == key_base2k, else the converted one)
                const DV& sv = c.p->res_base2k == c.p->key_base2k ? raw_av : av;
                for (int col = 0; col < c.s.cols_out; ++col)
                    PZ_TRY(launch_ew(M, EW_ADD_I64, u.res_dft + (long long)col * n, rb.bs, big_ls, u.res_dft + (long long)col * n, rb.bs, big_ls,
                                     (const int64_t*)sv.p + (long long)col * n, sv.bs, (long long)sv.cols * n, std::min(res_dft_size, sv.size), nb));
            } else if (c.add) {  // CMUX, eval.rs:568-569: + f[col] on every column
                const DV fv = wave_add(c, b0);
                for (int col = 0; col < c.s.cols_out; ++col)
                    PZ_TRY(launch_ew(M, EW_ADD_I64, u.res_dft + (long long)col * n, rb.bs, big_ls, u.res_dft + (long long)col * n, rb.bs, big_ls,
                                     (const int64_t*)fv.p + (long long)col * n, fv.bs, (long long)fv.cols * n, std::min(res_dft_size, fv.size), nb));
            } else if (c.ks) {  // body column added after the inverse transform (keyswitching/glwe.rs:237)
                PZ_TRY(launch_ew(M, EW_ADD_I64, u.res_dft + (long long)c.body_col * n, rb.bs, big_ls, u.res_dft + (long long)c.body_col * n, rb.bs,
                                 big_ls, av.p, av.bs, (long long)av.cols * n, std::min(res_dft_size, av.size), nb));
            }
            for (int col = 0; col < c.s.cols_out; ++col)
                PZ_TRY(dev_normalize(M, nb, rv, (int)c.p->res_base2k, 0, col, rb, (int)c.p->key_base2k, col));
        }
    }
    return PZ_OK;
}

// ------------------------------------------------------------------------------
// glwe_op
// ------------------------------------------------------------------------------
// Automorphism family on top of the key switch (poulpy-core automorphism/glwe_ct.rs:51-275).  With phi = X -> X^p:
//   mode 0  res = phi(normalize(big))                       (:65-71)
//   mode 1  res = normalize(phi(big) + a)   (add, :133-138)   2: phi(big) - a (:222-227)   3: a - phi(big) (:268-273)
// where big is the key-switch value including the body (keyswitching/glwe.rs:236-237).  Normalization acts per
// coefficient, so modes 1-3 are computed as  phi(normalize'(s .* (big + small)))  with small = -+phi^-1(a) (+ body), s(n) the sign phi
// gives coefficient n (applied inside the tail before the carry chain; flipped for mode 3); mode 0 is the plain key switch followed by
// the signed permutation - or, in the spectral form, all of it inside the three kernels (spectral_perm above).
// (Round 2 experiment, removed — git history has it: a CU-partitioned, overlapped form of the fused pipeline.  With a CU mask spread
//  over the 8 XCDs pass 1 and the tail keep their full rate down to 64 CUs while the middle kernel scales with its CU count
//  (profiles/r02_cu_mask_scaling.txt), so chunk c+1's pass 1, chunk c's middle kernel and chunk c-1's tail were run concurrently on
//  disjoint CU sets, chained by events.  Bit-exact, but slower in every split tried (best 73 500/s against 88 700/s back to back,
//  profiles/r02_overlap_sweep.txt): under concurrency the three kernels share HBM at ~4.7 TB/s aggregate.)
// the Galois element of a call: au, p mod 2N and its inverse (glwe_call_init; glwe_rotations_hoisted per rotation)
static void call_set_galois(GlweCall& c, const AutoSpec* au) {
    c.au = au;
    c.au_p = (unsigned)((unsigned long long)au->p & (2ull * (unsigned long long)c.n - 1ull));
    c.au_g = inv_mod_2n(au->p, c.n);
}
int glwe_call_init(GlweCall& c, pz_module* M, GlweKind kind, int64_t* res, const int64_t* a, const double* pmat, const pz_glwe_op_params* p,
                          size_t batch, const AutoSpec* au, const OpLayout* lay, bool* post_rsh) {
    const bool ks = kind_ks(kind), tensor = kind == GlweKind::TensorRelin;
    c.want_rsh = post_rsh && *post_rsh;
    c.post_rsh = post_rsh;
    if (post_rsh) *post_rsh = false;
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_TRY(require_op_shape(p, "glwe op"));
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && is_device_ptr(pmat), "batched entry points take device pointers");
    PZ_REQUIRE(!(tensor && (au || lay)), "glwe_tensor_relinearize: packed tensors, no automorphism");
    PZ_REQUIRE((kind == GlweKind::Automorphism) == (au != nullptr), "glwe op: the automorphism family and its Galois element go together");
    c.M = M; c.p = p; c.kind = kind; c.ks = ks; c.tensor = tensor; c.au = au; c.lay = lay; c.res = res; c.a = a; c.pmat = pmat; c.batch = batch;
    c.s = op_shape(p, kind);
    c.chunk = pick_chunk(M, p, c.s, std::max<size_t>(batch, 1));
    c.n = (long long)M->n;
    c.dsize = (int)p->dsize; c.dnum = (int)p->dnum; c.ksz = (int)p->key_size;
    c.a_ct = c.n * c.s.cols_a * (long long)p->a_size;
    c.res_ct = c.n * c.s.cols_out * (long long)p->res_size;
    c.npi = c.s.cols_in * c.s.a_size_eff; c.npo = c.s.cols_out * c.ksz;
    c.nrows = c.dnum * c.s.cols_in; c.ncols = c.s.cols_out * c.ksz;
    c.au_big = au && au->mode != 0;
    c.au_p = c.au_g = 0u;
    if (au) call_set_galois(c, au);
    c.a_bs = lay ? lay->a_stride : c.a_ct; c.res_bs = lay ? lay->res_stride : c.res_ct;
    c.body_col = lay ? lay->body_col : 0;
    c.digits = c.dsize > 1; c.cross_out = p->res_base2k != p->key_base2k;
    PZ_REQUIRE(!(au && lay), "glwe_automorphism: packed ciphertexts only");
    PZ_REQUIRE(c.body_col >= 0 && c.body_col < c.s.cols_out, "body column out of range");
    if (au) {
        PZ_REQUIRE(ks && c.s.cols_a == c.s.cols_out, "glwe_automorphism: the key must map rank -> rank");
        PZ_REQUIRE((au->p & 1) != 0, "glwe_automorphism: the Galois element must be odd");
        PZ_REQUIRE(au->mode >= 0 && au->mode <= 3, "glwe_automorphism: unknown mode");
    }
    return PZ_OK;
}

namespace pz {
int glwe_op(pz_module* M, GlweKind kind, int64_t* res, const int64_t* a, const double* pmat, const pz_glwe_op_params* p, size_t batch,
            const AutoSpec* au, const OpLayout* lay, bool* post_rsh) {
    GlweCall c;
    PZ_TRY(glwe_call_init(c, M, kind, res, a, pmat, p, batch, au, lay, post_rsh));
    if (batch == 0) return PZ_OK;
    // dsize > 1 (digit-selected product inside the middle kernel) and res_base2k != key_base2k (the tail normalizes into the key's base,
    // one cross-base pass follows) ride on the fused pipeline too; both need the 128-point-row plans and no automorphism (fused_applies)
    // (keyauto_entries, api_ggsw.hip, enters glwe_fused directly, with GlweCall::keyauto set, where keyauto_fast_applies says this line would take it)
    if (fused_applies(M, p, c.s, kind)) return glwe_fused(c);
    if (small_ring_applies(M, p, c.s, kind, lay == nullptr)) return glwe_small_ring(c);
    return glwe_unfused(c);
}

// glwe_tensor_relinearize on a GLWETensor kept as 16-bit digits (the fused multiply + relinearize, api_cnv.hip): forward pass 1 reads the pair
// columns, the tail adds the first rank + 1 columns - both from a16 (GlweCall::a16)
bool glwe_relin_t16_supported(const pz_module* M, const pz_glwe_op_params* p) {
    if (!p || p->dsize != 1 || p->a_base2k != p->key_base2k || p->res_base2k != p->key_base2k || p->rank_out != p->rank || p->rank < 1) return false;
    const OpShape s = op_shape(p, GlweKind::TensorRelin);
    return fused_applies(M, p, s, GlweKind::TensorRelin) && tail_d16_only_supported(M) && M->dbg_stages == 7;
}
size_t glwe_relin_chunk(const pz_module* M, const pz_glwe_op_params* p, size_t batch) { return pick_chunk(M, p, op_shape(p, GlweKind::TensorRelin), std::max<size_t>(batch, 1)); }
int glwe_relin_t16(pz_module* M, int64_t* res, const short* a16, long long a16_cs, const double* pmat, const pz_glwe_op_params* p, size_t batch) {
    GlweCall c;
    PZ_TRY(glwe_call_init(c, M, GlweKind::TensorRelin, res, reinterpret_cast<const int64_t*>(a16), pmat, p, batch, nullptr, nullptr, nullptr));
    PZ_REQUIRE(glwe_relin_t16_supported(M, p) && !n4096_two_kernel(c), "glwe_relin_t16: the pipeline path only");
    if (batch == 0) return PZ_OK;
    c.a16 = a16; c.a16_cs = a16_cs;
    return glwe_fused(c);
}
}  // namespace pz

extern "C" {
// The four GLWE-level entry points accept device pointers (batched, device-resident: the measured path) or HOST containers
// (what a CoreImpl override of the Rust shim passes): host ciphertexts are staged, a host-resident prepared key is mirrored on
// the device (resolve_key); the call is then logically synchronous like every host-pointer call.
// Pinned (page-locked: pz_alloc_bytes, hipHostMalloc, hipHostRegister) host memory - the only kind a copy engine reads and writes on its own
static bool is_pinned_host(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}
// Host containers, several ciphertexts per call, pinned memory (round 5): the call as waves of ciphertexts on three streams - wave k + 1 travels to
// the device (stream2) while wave k runs on the module stream and wave k - 1 travels back (stream_out).  PCIe is full duplex: the serial form
// (everything up, kernels, everything down) used one direction at a time - 3 200 external products/s at 16 ciphertexts per call at the metric
// shape, 53 GB/s summed over both directions.  Logically synchronous like every host-pointer call: returns when the last wave is back.
static int glwe_entry_duplex(pz_module* M, GlweKind kind, int64_t* res, const int64_t* a, const double* key, const pz_glwe_op_params* p,
                             size_t batch, const AutoSpec* au, size_t res_ct_bytes, size_t a_ct_bytes) {
    if (!M->stream2) {
        SideStream probe(M);   // (creates the side stream and its events)
        PZ_TRY(probe.fork());
    }
    if (!M->stream_out && hipStreamCreateWithFlags(&M->stream_out, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return fail(PZ_ERR_HIP, "stream create failed"); }
    const bool in_place = (const void*)res == (const void*)a;
    void *a_dev = nullptr, *r_dev = nullptr;
    PZ_TRY(arena_alloc(M, batch * a_ct_bytes, &a_dev));
    if (in_place) r_dev = a_dev; else PZ_TRY(arena_alloc(M, batch * res_ct_bytes, &r_dev));
    // 8 equal waves (measured at 16 ciphertexts per call at the metric shape: 4 waves 4 700/s, 8 waves 4 960/s, 16 waves 4 850/s; a half-size first
    // and last wave - shorter fill and drain, one wave more - 4 610/s; profiles/r05_host_duplex.txt)
    const size_t per = (batch + 7) / 8;
    std::vector<size_t> waves;
    for (size_t left = batch; left > 0; left -= waves.back()) waves.push_back(std::min(per, left));
    std::vector<hipEvent_t> up, done;
    auto ev = [&](std::vector<hipEvent_t>& v) -> hipEvent_t {
        hipEvent_t e = KTimer::get(M);
        if (e) v.push_back(e);
        return e;
    };
    int rc = PZ_OK;
    // (no HIP-graph capture of the waves' launch sequences: one graph per wave - keyed by its pointers - would fill the module's 16-entry cache,
    //  and instantiating them costs more than the three launches per wave they would save)
    const bool graphs_were_on = M->graphs_on;
    M->graphs_on = false;
    // everything issued on the module stream so far (key mirror upload, earlier calls) precedes the first copies
    hipEvent_t e0 = ev(up);
    if (!e0 || hipEventRecord(e0, M->stream) != hipSuccess || hipStreamWaitEvent(M->stream2, e0, 0) != hipSuccess ||
        hipStreamWaitEvent(M->stream_out, e0, 0) != hipSuccess) rc = fail(PZ_ERR_HIP, "duplex host path: event set-up failed");
    size_t b0 = 0;
    for (size_t wi = 0; rc == PZ_OK && wi < waves.size(); b0 += waves[wi], ++wi) {
        const size_t nb = waves[wi];
        hipEvent_t eu = ev(up), ed = ev(done);
        if (!eu || !ed) { rc = fail(PZ_ERR_HIP, "duplex host path: no event"); break; }
        char* ad = (char*)a_dev + b0 * a_ct_bytes;
        char* rd = (char*)r_dev + b0 * res_ct_bytes;
        if (hipMemcpyAsync(ad, (const char*)a + b0 * a_ct_bytes, nb * a_ct_bytes, hipMemcpyHostToDevice, M->stream2) != hipSuccess ||
            hipEventRecord(eu, M->stream2) != hipSuccess || hipStreamWaitEvent(M->stream, eu, 0) != hipSuccess) { rc = fail(PZ_ERR_HIP, "duplex host path: upload failed"); break; }
        rc = glwe_op(M, kind, (int64_t*)rd, (const int64_t*)ad, key, p, nb, au);
        if (rc != PZ_OK) break;
        if (hipEventRecord(ed, M->stream) != hipSuccess || hipStreamWaitEvent(M->stream_out, ed, 0) != hipSuccess ||
            hipMemcpyAsync((char*)res + b0 * res_ct_bytes, rd, nb * res_ct_bytes, hipMemcpyDeviceToHost, M->stream_out) != hipSuccess) { rc = fail(PZ_ERR_HIP, "duplex host path: download failed"); break; }
    }
    M->graphs_on = graphs_were_on;
    // the call returns when every wave is back (and nothing of it is still in flight on an error path)
    const hipError_t s1 = hipStreamSynchronize(M->stream2), s2 = hipStreamSynchronize(M->stream), s3 = hipStreamSynchronize(M->stream_out);
    for (hipEvent_t e : up) M->event_pool.push_back(e);
    for (hipEvent_t e : done) M->event_pool.push_back(e);
    if (rc == PZ_OK && (s1 != hipSuccess || s2 != hipSuccess || s3 != hipSuccess)) { (void)hipGetLastError(); rc = fail(PZ_ERR_HIP, "duplex host path: a stream failed"); }
    return rc;
}
static int glwe_entry(pz_module* M, GlweKind kind, int64_t* res, const int64_t* a, const double* pmat, const pz_glwe_op_params* p,
                      size_t batch, const AutoSpec* au) {
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_TRY(require_op_shape(p, "glwe op"));
    const OpShape s = op_shape(p, kind);
    const size_t n8 = (size_t)M->n * 8;
    // in place (*_assign forms): one layout for a and res - checked HERE, in front of both host paths (the duplex path below does not go through
    // glwe_args_in: with res == a and a larger res every wave's kernels would write past the a-sized arena block).  Host ranges that overlap
    // without being equal take the serial path: there the whole input is on the device before the first result travels back
    const size_t res_ct_bytes = n8 * s.cols_out * p->res_size, a_ct_bytes = n8 * s.cols_a * p->a_size;
    if (res != nullptr && (const void*)res == (const void*)a) PZ_REQUIRE(res_ct_bytes == a_ct_bytes, "in-place call with different layouts for a and res");
    const bool partial_overlap = res != nullptr && a != nullptr && (const void*)res != (const void*)a &&
                                 ranges_overlap(res, batch * res_ct_bytes, a, batch * a_ct_bytes);
    if (batch >= 2 && res != nullptr && a != nullptr && pmat != nullptr && !partial_overlap && !M->timing && !canary_mode() && is_pinned_host(a) && is_pinned_host(res)) {
        const double* key = nullptr;
        PZ_TRY(resolve_key(M, pmat, prepared_key_bytes(M, p, s.cols_in, s.cols_out), &key));
        return glwe_entry_duplex(M, kind, res, a, key, p, batch, au, res_ct_bytes, a_ct_bytes);
    }
    GlweArgs g;
    PZ_TRY(glwe_args_in(M, g, res, a, pmat, batch * res_ct_bytes, batch * a_ct_bytes, prepared_key_bytes(M, p, s.cols_in, s.cols_out)));
    PZ_TRY(glwe_op(M, kind, g.res, g.a, g.key, p, batch, au));
    return glwe_args_out(M, g);
}
int pz_glwe_external_product_batched(pz_module* M, int64_t* res, const int64_t* a, const double* ggsw_pmat,
                                     const pz_glwe_op_params* p, size_t batch) {
    PZ_ENTER(M);
    return glwe_entry(M, GlweKind::ExternalProduct, res, a, ggsw_pmat, p, batch, nullptr);
}
int pz_glwe_keyswitch_batched(pz_module* M, int64_t* res, const int64_t* a, const double* key_pmat, const pz_glwe_op_params* p,
                              size_t batch) {
    PZ_ENTER(M);
    return glwe_entry(M, GlweKind::KeySwitch, res, a, key_pmat, p, batch, nullptr);
}
int pz_glwe_automorphism_batched(pz_module* M, int64_t* res, const int64_t* a, const double* key_pmat, const pz_glwe_op_params* p,
                                 int64_t gal, int mode, size_t batch) {
    PZ_ENTER(M);
    AutoSpec au{(long long)gal, mode};
    return glwe_entry(M, GlweKind::Automorphism, res, a, key_pmat, p, batch, &au);
}
// glwe_tensor_relinearize (poulpy-core/src/operations/glwe.rs:541-607) on `batch` GLWETensors sharing one prepared tensor key
int pz_glwe_tensor_relinearize_batched(pz_module* M, int64_t* res, const int64_t* a, const double* tsk_pmat, const pz_glwe_op_params* p,
                                       size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(p->rank >= 1 && p->rank_out == p->rank, "glwe_tensor_relinearize: the tensor key maps rank (rank + 1) / 2 -> rank");
    return glwe_entry(M, GlweKind::TensorRelin, res, a, tsk_pmat, p, batch, nullptr);
}
}  // extern "C"

// ------------------------------------------------------------------------------
// One ciphertext batch rotated by many Galois elements (pz_glwe_automorphism_many_batched).  res[r] = phi_r(normalize(KS_{K_r}(a))):
// the key switch decomposes the unpermuted `a`, and in the spectral form phi_r only reaches the middle kernel's store position and the tail's
// signs - so pass 1's output T and the body column's 16-bit image are the same for every rotation ("hoisted rotations").  Per wave:
//   wave_input, pass 1                      once
//   k_automorphism_t16_many                 once per kAutoManyCap rotations: one read of the body column, one 16-bit copy per rotation
//   middle kernel (key r, perm r), tail r   per rotation - the launches of the single call, on copy r
// Workspace: [row-sliced keys that are not pinned][a_conv][T][T2'][res_tmp: the i64 fallback's operand, one rotation at a time][copies, nrot x]
// [middle kernel's scratch].  Each rotation's arithmetic is the single call's: the result is bit-identical to nrot calls.
// ------------------------------------------------------------------------------
static size_t rot_copy_bytes(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, size_t chunk) {
    return align256(chunk * std::min<size_t>((size_t)s.a_size_eff, p->key_size) * (size_t)M->n * sizeof(short));
}
// why a call takes one glwe_op per rotation instead of the hoisted route; null: it takes the hoisted route
static const char* rot_loop_reason(const GlweCall& c, size_t nrot) {
    const pz_module* M = c.M;
    // (measured at N = 2^16, 16 limbs, 512 ciphertexts: 49 850 against 50 235 rotations/s - nothing is shared, and the copy in a segment of its own costs 0.7 %)
    if (nrot == 1) return "one rotation: nothing to share";
    if (rt_knob("POULPY_DBG_ROT_HOIST", 1) == 0) return "POULPY_DBG_ROT_HOIST=0";   // (read per call: tests flip it)
    if (c.digits) return "dsize > 1";
    if (c.cross_out) return "res_base2k != key_base2k";
    if (!fused_applies(M, c.p, c.s, GlweKind::Automorphism)) return "no three-kernel pipeline for this shape";
    if (!spectral_perm(c).on) return "no spectral form on this plan";
    if (n4096_two_kernel(c)) return "N = 4096 two-kernel path";
    if (M->probe) return "rounding-margin probe";
    if ((int)c.p->key_base2k > 16) return "digits beyond the 16-bit copies";   // (res_base2k == key_base2k here)
    return nullptr;
}
static int glwe_rotations_hoisted(const GlweCall& c0, size_t nrot, const int64_t* gals, const double* const* keys) {
    pz_module* M = c0.M;
    const long long n = c0.n;
    const bool copies = spectral_body16(c0);   // (false: the plans without the 16-bit-operand tail, N = 4096 - pass 1 is shared, the i64 pre-pass runs per rotation)
    std::vector<const cplx*> Pp(nrot);
    size_t nslice = 0;
    for (size_t r = 0; r < nrot; ++r) { Pp[r] = pinned_slices(c0, keys[r]); nslice += Pp[r] == nullptr; }
    const FusedWs fw = fused_ws(M, c0.p, c0.s, c0.chunk, true);
    const size_t copy_bytes = copies ? rot_copy_bytes(M, c0.p, c0.s, c0.chunk) : 0;
    PZ_TRY(ws_reserve(M, fw.total - fw.key + nslice * fw.key + nrot * copy_bytes));
    char* base = (char*)M->ws;
    FusedBufs f;
    char* key_area; char* copy_area;
    PZ_TRY(ws_take(M, base, nslice * fw.key, &key_area));
    PZ_TRY(ws_take(M, base, fw.conv, &f.a_conv));
    PZ_TRY(ws_take(M, base, fw.t, &f.T));
    base += (kT2Phase - (size_t)(((uintptr_t)base - (uintptr_t)c0.res) & kT2PhaseMask)) & kT2PhaseMask;   // see kT2Phase
    PZ_TRY(ws_take(M, base, fw.t2, &f.T2));
    PZ_TRY(ws_take(M, base, fw.rtmp, &f.res_tmp));
    PZ_TRY(ws_take(M, base, nrot * copy_bytes, &copy_area));
    PZ_TRY(ws_take(M, base, kMidDummyBytes, &f.mid_dummy));
    f.key_scratch = nullptr; f.key_digits = nullptr;
    // every key row-sliced at most once per call
    for (size_t r = 0, k = 0; r < nrot; ++r) {
        if (Pp[r]) continue;
        cplx* dst = (cplx*)(key_area + (k++) * fw.key);
        PZ_TRY(launch_permute_pmat(M, keys[r], dst, c0.nrows * c0.ncols));
        Pp[r] = dst;
    }
    std::vector<unsigned> muls(nrot);
    for (size_t r = 0; r < nrot; ++r) muls[r] = inv_mod_2n((long long)gals[r], n);
    dispatch_note(M, "rotations: hoisted, %d per forward pass%s", (int)nrot, copies ? "" : " (i64 body operand per rotation)");
    for (size_t b0 = 0; b0 < c0.batch; b0 += c0.chunk) {
        const int nb = (int)std::min(c0.chunk, c0.batch - b0);
        DV av;
        PZ_TRY(wave_input(c0, b0, nb, f.a_conv, &av));
        PolyMap sm{av.size, c0.s.cols_in, av.bs, (long long)av.cols * n, n, n * c0.s.a_col0};
        if (copies) PZ_TRY(launch_zero_bytes(M, M->margin + 1, 8));   // the wide flag: one for all rotations, it depends on the body's digits alone
        PZ_TRY(launch_fwd_pass1(M, nb * c0.npi, (const long long*)av.p, sm, f.T, true));
        if (copies) {
            const int bl = std::min(av.size, c0.ksz);
            PolyMap bsm{bl, 1, av.bs, (long long)av.cols * n, 0, 0}, bdm{bl, 1, (long long)bl * n, n, 0, 0};
            PZ_TRY(launch_automorphism_t16_many(M, nb * bl, (const long long*)av.p, bsm, (short*)copy_area, bdm, (long long)(copy_bytes / sizeof(short)),
                                                muls.data(), (int)nrot));
        }
        for (size_t r = 0; r < nrot; ++r) {
            AutoSpec au{(long long)gals[r], 0};
            GlweCall c = c0;
            call_set_galois(c, &au);   // (c.au_g == muls[r]: the pre-pass's gather multiplier is the tail's)
            c.pmat = keys[r];
            c.res = c0.res + (long long)r * (long long)c0.batch * c0.res_ct;   // rotation-major
            MidCall mc;
            mc.T = f.T; mc.T2 = f.T2; mc.Pp = Pp[r]; mc.dummy = f.mid_dummy; mc.npi = c.npi; mc.npo = c.npo; mc.nrows = c.nrows; mc.ncols = c.ncols;
            mc.perm = spectral_perm(c);
            PZ_TRY(launch_mid(M, nb, mc));
            f.body16_pre = copies ? (const short*)(copy_area + r * copy_bytes) : nullptr;
            PZ_TRY(wave_spectral_tail(c, f, b0, nb, av));
        }
    }
    return PZ_OK;
}

extern "C" {
size_t pz_glwe_automorphism_many_workspace_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t nrot, size_t batch) {
    if (!M || !p || p->key_size == 0 || p->a_size == 0 || nrot == 0) return 0;
    // the per-rotation calls' reservation; where the three-kernel pipeline serves the shape, the hoisted layout on top of it: a row-sliced copy
    // per key (none of them pinned) and a 16-bit copy of the body operand per rotation
    // (+ the room ws_reserve adds for the guards of POULPY_DBG_CANARY: the figure bounds the allocation itself, pz_module_workspace_bytes)
    const size_t loop = pz_glwe_op_workspace_bytes(M, p, batch, (int)GlweKind::Automorphism) + kGuardSlack + (kGuardSlack >> 3);
    const OpShape s = op_shape(p, GlweKind::Automorphism);
    if (!fused_applies(M, p, s, GlweKind::Automorphism) || M->plan.m2 != 128) return loop;
    const size_t chunk = pick_chunk(M, p, s, std::max<size_t>(batch, 1));
    const FusedWs fw = fused_ws(M, p, s, chunk, true);
    const size_t bytes = fw.total + (nrot - 1) * fw.key + nrot * rot_copy_bytes(M, p, s, chunk) + kGuardSlack;
    return std::max(loop, bytes + (bytes >> 3));
}

int pz_glwe_automorphism_many_batched(pz_module* M, int64_t* res, const int64_t* a, size_t nrot, const int64_t* gals, const double* const* key_pmats,
                                      const pz_glwe_op_params* p, size_t batch) {
    // (the argument checks that need no module come first; nothing is launched when one fails)
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(nrot >= 1, "glwe_automorphism_many: no rotation asked for");
    PZ_REQUIRE(res != nullptr && a != nullptr && gals != nullptr && key_pmats != nullptr, "glwe_automorphism_many: null argument");
    for (size_t r = 0; r < nrot; ++r) {
        PZ_REQUIRE((gals[r] & 1) != 0, "glwe_automorphism_many: Galois element %zu is even", r);
        PZ_REQUIRE(key_pmats[r] != nullptr, "glwe_automorphism_many: key %zu is null", r);
    }
    PZ_ENTER(M);
    PZ_TRY(require_op_shape(p, "glwe op"));
    PZ_REQUIRE(p->rank >= 1 && p->rank_out == p->rank, "glwe_automorphism_many: the keys map rank -> rank");
    const size_t cols = p->rank + 1, n8 = (size_t)M->n * 8;
    const size_t a_bytes = batch * n8 * cols * p->a_size, res_bytes = nrot * batch * n8 * cols * p->res_size;
    // every rotation reads `a` after the first one has written: no in-place form
    PZ_REQUIRE(!ranges_overlap(res, res_bytes, a, a_bytes) && (const void*)res != (const void*)a, "glwe_automorphism_many: res overlaps a");
    for (size_t r = 0; r < nrot; ++r) PZ_REQUIRE(is_device_ptr(key_pmats[r]), "batched entry points take device pointers");
    AutoSpec au0{(long long)gals[0], 0};
    GlweCall c;
    PZ_TRY(glwe_call_init(c, M, GlweKind::Automorphism, res, a, key_pmats[0], p, batch, &au0, nullptr, nullptr));
    if (batch == 0) return PZ_OK;
    const char* why = rot_loop_reason(c, nrot);
    if (!why) {
        PZ_TRY(glwe_rotations_hoisted(c, nrot, gals, key_pmats));
        return finish_call(M, false);
    }
    dispatch_note(M, "rotations: per-rotation calls (%s)", why);
    for (size_t r = 0; r < nrot; ++r) {
        AutoSpec au{(long long)gals[r], 0};
        PZ_TRY(glwe_op(M, GlweKind::Automorphism, res + (long long)(r * batch) * c.res_ct, a, key_pmats[r], p, batch, &au));
    }
    return finish_call(M, false);
}
}  // extern "C"


// api_lwe.hip composes the LWE <-> GLWE conversions around the batched key switch while holding the module lock
namespace pz {
// Key switch of `batch` ciphertexts that are rotations of the ciphertexts of `a`: ciphertext b = X^rot a[word], (word, rot mod 2n) = rot_tab[b] (device).
// Served where the one-kernel small-ring form takes the key switch with every object in the key's base (N = 1024, and the N = 2048 shapes
// small_one_supported names): its forward column pass and its operand load read `a` through the monomial's index and sign map, so the rotated
// ciphertexts are never written.  glwe_keyswitch_rot_applies says whether a shape is served; the caller materialises the rotation otherwise.
bool glwe_keyswitch_rot_applies(const pz_module* M, const pz_glwe_op_params* p) {
    if (!p || p->dsize < 1 || p->dnum < 1 || p->key_size < 1 || p->a_size < 1 || p->res_size < 1 || p->rank < 1) return false;
    if (rt_knob("POULPY_DBG_LWE_ROT_ON_LOAD", 1) == 0) return false;   // (read per call: tests flip it)
    const OpShape s = op_shape(p, GlweKind::KeySwitch);
    if (s.convert || p->res_base2k != p->key_base2k) return false;     // the first reader is a cross-base pass / the digits leave through one
    if (fused_applies(M, p, s, GlweKind::KeySwitch) || !small_ring_applies(M, p, s, GlweKind::KeySwitch, true)) return false;
    return small_one_supported(M, s.cols_in * s.a_size_eff, (int)p->dnum * s.cols_in, s.cols_out * (int)p->key_size, s.cols_out, (int)p->key_size, 1);
}
int glwe_keyswitch_rot_nolock(pz_module* M, int64_t* res, const int64_t* a, const RotSrc* rot_tab, const double* key_pmat, const pz_glwe_op_params* p,
                              size_t batch) {
    PZ_REQUIRE(glwe_keyswitch_rot_applies(M, p) && rot_tab != nullptr, "rotated-source key switch: shape not served");
    const OpShape s = op_shape(p, GlweKind::KeySwitch);
    const double* key = nullptr;
    PZ_TRY(resolve_key(M, key_pmat, prepared_key_bytes(M, p, s.cols_in, s.cols_out), &key));
    GlweCall c;
    PZ_TRY(glwe_call_init(c, M, GlweKind::KeySwitch, res, a, key, p, batch, nullptr, nullptr, nullptr));
    if (batch == 0) return PZ_OK;
    c.rot_tab = rot_tab;
    return glwe_small_ring(c);
}
int glwe_keyswitch_nolock(pz_module* M, int64_t* res, const int64_t* a, const double* key_pmat, const pz_glwe_op_params* p, size_t batch) {
    return glwe_entry(M, GlweKind::KeySwitch, res, a, key_pmat, p, batch, nullptr);
}
}  // namespace pz
