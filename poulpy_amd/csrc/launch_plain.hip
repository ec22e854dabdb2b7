// launch_plain.hip — GLWE x constant (device_plain.hpp) and sums of such products (device_lincomb.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.hpp"
#include "device_plain.hpp"
#include "device_lincomb.hpp"

namespace pz {

bool mul_const_nz_supported(const pz_module* M, int a_size, int b_size) {
    return M->n >= 2 && a_size >= 1 && a_size <= kMulConstMaxA && b_size >= 1 && b_size <= kMulConstMaxB;
}

int launch_mul_const_nz(pz_module* M, int batch, long long* res, long long res_bs, const long long* a, long long a_bs, int cols, int a_size,
                        int res_size, int base2k, long long res_offset, int form, const MulConstArmSpec* arms) {
    if (batch <= 0) return PZ_OK;
    if (!mul_const_nz_supported(M, a_size, arms[0].b_size) || (form == 2 && !mul_const_nz_supported(M, a_size, arms[1].b_size)))
        return fail(PZ_ERR_INVALID, "k_mul_const_nz: shape outside the kernel (a_size %d, b_size %d)", a_size, arms[0].b_size);
    MulConstArgs g;
    g.res = res; g.a = a; g.res_bs = res_bs; g.a_bs = a_bs;
    g.n = (int)M->n; g.batch = batch; g.cols = cols;
    mul_const_plan(g, a_size, res_size, base2k, res_offset, form, arms);
    const long long npts = form == 0 ? M->n : M->n / 2;
    const long long threads = (long long)batch * npts;
    const size_t lds = (size_t)a_size * (form == 0 ? 1 : 2) * kMulConstBlock * sizeof(long long);
    KTimer kt(M, PZ_K_NORMALIZE);
    PZ_TRY(launch_k(k_mul_const_nz, dim3((unsigned)((threads + kMulConstBlock - 1) / kMulConstBlock)), dim3(kMulConstBlock), lds, M->stream, g));
    dispatch_note(M, "k_mul_const_nz (form %d, a %d limbs x %d digits -> %d, lds=%zu)", form, a_size, arms[0].b_size, res_size, lds);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

static_assert(kLinMaxTerms == kLincombMaxTerms, "the device table holds every term of a call");
size_t lincomb_lds_bytes(int a_max, int res_size, bool pair, bool has_tmp) {
    return (size_t)lc_slots(a_max, res_size, pair ? 1 : 0, has_tmp ? 1 : 0) * kMulConstBlock * sizeof(long long);
}

int lincomb_stage(pz_module* M, const LinTermSpec* terms, int nterms, int res_size, int base2k) {
    if (nterms < 1 || nterms > kLinMaxTerms) return fail(PZ_ERR_INVALID, "k_lincomb_const: %d terms (1 to %d)", nterms, kLinMaxTerms);
    const size_t bytes = sizeof(LinTerm) * kLinMaxTerms;
    if (!M->lin_tab) PZ_HIP(hipMalloc(&M->lin_tab, bytes));
    if (!M->lin_stage) PZ_HIP(hipHostMalloc(&M->lin_stage, bytes, hipHostMallocDefault));
    // the previous call's copy out of the staging has finished before it is rewritten
    if (M->lin_stage_ev) PZ_HIP(hipEventSynchronize(M->lin_stage_ev));
    else PZ_HIP(hipEventCreateWithFlags(&M->lin_stage_ev, hipEventDisableTiming));
    LinTerm* st = (LinTerm*)M->lin_stage;
    for (int u = 0; u < nterms; ++u) lc_plan_term(st[u], terms[u], res_size, base2k);
    PZ_HIP(hipMemcpyAsync(M->lin_tab, M->lin_stage, sizeof(LinTerm) * (size_t)nterms, hipMemcpyHostToDevice, M->stream));
    PZ_HIP(hipEventRecord(M->lin_stage_ev, M->stream));
    return PZ_OK;
}

int launch_lincomb(pz_module* M, int batch, long long* res, long long res_bs, int cols, int res_size, int base2k, int nterms, int init_res,
                   int normalize, bool pair, int a_max, bool has_tmp) {
    if (batch <= 0) return PZ_OK;
    const size_t lds = lincomb_lds_bytes(a_max, res_size, pair, has_tmp);
    if (lds > kLincombMaxLds || !M->lin_tab || M->n < 2) return fail(PZ_ERR_INVALID, "k_lincomb_const: shape outside the kernel (lds %zu)", lds);
    LinArgs g;
    g.res = res; g.res_bs = res_bs; g.terms = (const LinTerm*)M->lin_tab;
    g.n = (int)M->n; g.batch = batch; g.cols = cols; g.res_size = res_size; g.k = base2k; g.nterms = nterms;
    g.init_res = init_res; g.normalize = normalize; g.pair = pair ? 1 : 0; g.a_max = a_max; g.has_tmp = has_tmp ? 1 : 0;
    const long long threads = (long long)batch * (pair ? M->n / 2 : M->n);
    KTimer kt(M, PZ_K_NORMALIZE);
    PZ_TRY(launch_k(k_lincomb_const, dim3((unsigned)((threads + kMulConstBlock - 1) / kMulConstBlock)), dim3(kMulConstBlock), lds, M->stream, g));
    dispatch_note(M, "k_lincomb_const (%d terms, %s, %d operand limbs -> %d, normalize %d, lds=%zu)", nterms, pair ? "paired" : "unpaired", a_max,
                  res_size, normalize, lds);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

bool mid_cnv_pt_supported(const pz_module* M, int cols, int a_size, int b_size, int min_size) {
    // measured slower than per-column k_mid_cnv: built, tested, selected only with POULPY_DBG_MULPLAIN_FUSED=1
    static const bool on = (rt_knob("POULPY_DBG_MULPLAIN_FUSED", 0) != 0);
    const bool bs_ok = b_size == a_size || (b_size >= 1 && b_size <= 4);
    return on && (a_size == 8 || a_size == 16) && bs_ok && cols >= 2 && cols <= 3 && mid_cnv_supported(M, a_size, b_size, min_size) && min_size <= 32 &&
           ((size_t)mid_pt_rows(a_size, b_size, cols, min_size) * kMidPtRS + 256) * sizeof(cplx) <= (size_t)160 * 1024;
}
int launch_mid_cnv_pt(pz_module* M, int batch, const MidCnvCall& c) {
    const int cols = c.cols, a_size = c.a_size, b_size = c.b_size, min_size = c.min_size, offset = c.offset;
    const bool b_shared = c.b_shared;
    if (batch <= 0 || min_size <= 0) return PZ_OK;
    if (!mid_cnv_pt_supported(M, cols, a_size, b_size, min_size)) return fail(PZ_ERR_INVALID, "k_mid_cnv_pt: shape outside the kernel");
    MidCnvPtArgs g;
    g.a_main = c.a_main; g.a_last = c.a_last; g.b_main = c.b_main; g.b_last = c.b_last;
    g.b_main_bs = b_shared ? 0 : (long long)(b_size - 1) * M->m;
    g.b_last_bs = b_shared ? 0 : (long long)M->m;
    g.T2 = c.T2; g.cols = cols; g.min_size = min_size; g.offset = offset; g.m1 = M->plan.m1; g.batch = batch; g.wL2 = M->wL2; g.tw12t = M->tw12t;
    const size_t lds = ((size_t)mid_pt_rows(a_size, b_size, cols, min_size) * kMidPtRS + 256) * sizeof(cplx);
    const dim3 grid((unsigned)((long long)batch * g.m1));
    KTimer kt(M, PZ_K_FUSED_MID);
#define PZ_PT_LAUNCH(AS_, BS_) { PZ_TRY(launch_k((k_mid_cnv_pt<AS_, BS_>), grid, dim3(256), lds, M->stream, g)); }
#define PZ_PT_FORMS(AS_)                                                                                                          \
    {                                                                                                                             \
        if (b_size == AS_) PZ_PT_LAUNCH(AS_, AS_)                                                                                 \
        else if (b_size == 1) PZ_PT_LAUNCH(AS_, 1)                                                                                \
        else if (b_size == 2) PZ_PT_LAUNCH(AS_, 2)                                                                                \
        else if (b_size == 3) PZ_PT_LAUNCH(AS_, 3)                                                                                \
        else PZ_PT_LAUNCH(AS_, 4)                                                                                                 \
    }
    if (a_size == 16) PZ_PT_FORMS(16) else PZ_PT_FORMS(8)
#undef PZ_PT_FORMS
#undef PZ_PT_LAUNCH
    dispatch_note(M, "k_mid_cnv_pt<%d,%d> (%d columns, %d limbs each, product limbs [%d, %d), %s plaintext, lds=%zu)", a_size, b_size, cols, min_size,
                  offset, offset + min_size, b_shared ? "shared" : "per-ciphertext", lds);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

int launch_cnv_by_const_batched(pz_module* M, int batch, long long* res, long long res_bs, int res_size, int min_size, int offset, const long long* a,
                                long long a_bs, int cols, int a_size, const long long* bconst, int b_size) {
    if (batch <= 0 || min_size <= 0) return PZ_OK;
    CnvConstBatchArgs g;
    g.res = res; g.a = a; g.b = bconst; g.res_bs = res_bs; g.a_bs = a_bs;
    g.cols = cols; g.res_size = res_size; g.a_size = a_size; g.b_size = b_size; g.offset = offset; g.n = (int)M->n;
    KTimer kt(M, PZ_K_ELEMENTWISE);
    for (int b0 = 0; b0 < batch; b0 += 65535 / cols) {   // gridDim.z limit
        CnvConstBatchArgs gb = g;
        gb.res = res + (long long)b0 * res_bs;
        gb.a = a + (long long)b0 * a_bs;
        const int nb = std::min(65535 / cols, batch - b0);
        hipLaunchKernelGGL(k_cnv_by_const_batched, dim3((unsigned)((M->n + 255) / 256), (unsigned)min_size, (unsigned)(nb * cols)), dim3(256), 0, M->stream, gb);
    }
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

}  // namespace pz
