// launch_mid.hip — dispatch of the fused middle kernels and the key re-slicing (device_mid.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "device_mid.hpp"
#include "mid_forms.hpp"

namespace pz {

bool mid_supported(const pz_module* M, int npi, int npo) {
    const int np_max = M->plan.m2 == 128 ? 32 : 16;  // 128-point rows: up to 32 polynomial slots (two ciphertexts per tile)
    return (M->plan.m2 == 256 || M->plan.m2 == 128) && (M->plan.m1 % 16) == 0 && npi >= 1 && npi <= np_max && npo >= 1 && npo <= np_max;
}
int launch_permute_pmat(pz_module* M, const double* P, cplx* Pp, int npolys) {
    const FftPlan& pl = M->plan;
    const int blocks = npolys * (pl.m1 / 16) * (pl.m2 / 16);
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_permute_pmat, dim3(blocks), dim3(256), 0, M->stream, reinterpret_cast<const cplx*>(P), Pp, npolys, pl.m1, pl.m2);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}
// the row-sliced copy of phi_g(key) (k_permute_pmat_gal; 128-point-row plans)
int launch_permute_pmat_gal(pz_module* M, const double* P, cplx* Pp, int npolys, const KeyPerm& kp) {
    const FftPlan& pl = M->plan;
    if (pl.m2 != 128 || (pl.m1 % 16) != 0) return fail(PZ_ERR_UNSUPPORTED, "permuted key slicing: 128-point-row plans only");
    const unsigned m = (unsigned)pl.m1 * 128u;
    if (!(kp.mul & 1u) || kp.mul >= m || kp.add >= m) return fail(PZ_ERR_INVALID, "permuted key slicing: not an index map of this ring");
    unsigned inv = kp.mul;   // Newton steps for mul^-1 mod 2^32 (mul odd: 3 correct bits to start with)
    for (int i = 0; i < 5; ++i) inv *= 2u - kp.mul * inv;
    const int blocks = npolys * (pl.m1 / 16);
    KTimer kt(M, PZ_K_ELEMENTWISE);
    if (kp.conj) hipLaunchKernelGGL(k_permute_pmat_gal<true>, dim3(blocks), dim3(256), 0, M->stream, reinterpret_cast<const cplx*>(P), Pp, npolys, pl.m1, kp.mul, kp.add, inv);
    else hipLaunchKernelGGL(k_permute_pmat_gal<false>, dim3(blocks), dim3(256), 0, M->stream, reinterpret_cast<const cplx*>(P), Pp, npolys, pl.m1, kp.mul, kp.add, inv);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}
// m2 = 256 plans: k_mid, two ciphertexts per tile (one ciphertext per tile, two workgroups per CU, measured slower: NOTEBOOK.md section 4)
static int launch_mid256(pz_module* M, MidArgs g, int batch) {
    constexpr int CT = 2;
    g.n_ct = (batch + CT - 1) / CT;
    const size_t lds = ((size_t)CT * 16 * 17 * 16 + 512) * sizeof(cplx);
    KTimer kt(M, PZ_K_FUSED_MID);
    // persistent: as many workgroups as fit (LDS-bound: 144 KiB -> 1 per CU)
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, M->device);
    const int grid = std::min(ncu, g.m1 * g.n_ct);
    PZ_TRY(launch_k(k_mid<CT>, dim3(grid), dim3(CT * 256), lds, M->stream, g));
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}
// one launch of the instantiation `f` names (mid_forms.hpp): tile count, LDS bytes and grid follow from its (ct, np)
static int mid128_launch_form(pz_module* M, MidArgs& g, int batch, int ncu, const Mid128Form& f) {
    g.n_ct = (batch + f.ct - 1) / f.ct;
    const size_t lds = ((size_t)f.ct * f.np * kMidRS + 384 + 32) * sizeof(cplx);   // tile | wL2 | two twiddle rows | exponents
    const dim3 grid(std::min({ncu, 256, g.m1 * g.n_ct}));   // <= 256: one scratch tile per workgroup (kMidDummyBytes)
    char note[160];
    mid128_note(f, PZ_MIDR_KR, note, sizeof note);
    if (f.ring) {
#define X(CT_, NP_, PERM_, NR_, HALFIN_, DS_, C2_)                                                                           \
    if (f.ct == CT_ && f.np == NP_ && f.perm == PERM_ && f.nr == NR_ && f.halfin == HALFIN_ && f.ds == DS_ && f.c2 == C2_) {  \
        PZ_TRY(launch_k((k_mid128r<CT_, NP_, PERM_, NR_, HALFIN_, (NP_ == 32 ? 3 : PZ_MIDR_KR), DS_, C2_>), grid, dim3(512), lds, M->stream, g)); \
        dispatch_note(M, "%s", note);                                                                                        \
        return PZ_OK;                                                                                                        \
    }
        PZ_MID128R_FORMS(X)
#undef X
    } else {
#define X(CT_, NP_, PERM_, DS_, BR_, SKIPW_, BRNEST_, NCO_)                                                                  \
    if (f.ct == CT_ && f.np == NP_ && f.perm == PERM_ && f.ds == DS_ && f.br == BR_ && f.skipw == SKIPW_ && f.brnest == BRNEST_ && f.nco == NCO_) { \
        PZ_TRY(launch_k((k_mid128<CT_, NP_, PERM_, DS_, BR_, SKIPW_, BRNEST_, NCO_>), grid, dim3(512), lds, M->stream, g));   \
        dispatch_note(M, "%s", note);                                                                                        \
        return PZ_OK;                                                                                                        \
    }
        PZ_MID128_FORMS(X)
#undef X
    }
    return fail(PZ_ERR_UNSUPPORTED, "launch_mid: no instantiation of %s", note);
}
// m2 = 128 plans: the persistent tile kernels k_mid128 / k_mid128r, in the instantiation mid128_form chooses for this shape
static int launch_mid128(pz_module* M, MidArgs& g, int batch, int npi, int npo, bool perm, bool ds, bool br) {
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, M->device);
    static const bool mid_r = (rt_knob("POULPY_DBG_MID_R", 1) != 0);   // 0: k_mid128 (the kernel of rounds 1-2) instead of k_mid128r (A/B)
    Mid128Shape s;
    s.npi = npi; s.npo = npo; s.row_max = g.row_max; s.ncols = g.ncols; s.ncomp = g.ncomp; s.ds_n = g.ds_n; s.br_rm = g.br_rm;
    s.perm = perm; s.ds = ds; s.br = br; s.mid_r = mid_r;
    KTimer kt(M, PZ_K_FUSED_MID);
    PZ_TRY(mid128_launch_form(M, g, batch, ncu, mid128_form(s)));
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}
int launch_mid(pz_module* M, int batch, const MidCall& c) {
    const MidDigits* dg = c.digits;
    const MidBr* br = c.br;
    const int npi = c.npi, npo = c.npo, ncols = c.ncols;
    int nrows = c.nrows;
    MidArgs g;
    g.br_lwe = nullptr; g.br_lwe_bs = 0; g.br_i0 = 0; g.br_blk = 0; g.br_rm = 0; g.w2n = M->w2n;
    if (br) {
        // nrows = the key rows of ONE GGSW (= npi here); Pp holds br->blk of them per frequency row
        g.br_lwe = br->lwe; g.br_lwe_bs = br->lwe_bs; g.br_i0 = br->i0; g.br_blk = br->blk; g.br_rm = nrows;
        nrows *= br->blk;
    }
    g.ds_n = 0;
    const bool ds = dg != nullptr && dg->n > 0;
    if (ds) {
        g.ds_n = dg->n;
        for (int t = 0; t < dg->n; ++t) { g.ds_in[t] = dg->in[t]; g.ds_row[t] = dg->row[t]; g.ds_coff[t] = dg->coff[t]; g.ds_cb[t] = dg->cb[t]; }
    }
    g.perm_mul = c.perm.mul; g.perm_add = c.perm.add; g.perm_ysign = c.perm.conj ? -1.0 : 1.0; g.log_m1 = 0;
    g.dbg = 0;
    while ((1 << g.log_m1) < M->plan.m1) ++g.log_m1;
    const bool perm = c.perm.mul != 0;
    g.T = c.T; g.T2 = c.T2; g.P = c.Pp; g.npi = npi; g.npo = npo; g.nrows = nrows; g.ncols = ncols;
    g.row_max = br ? nrows : std::min(nrows, npi);
    g.ncomp = std::min(npo, ncols);
    if ((ds ? g.ds_n : g.row_max) < 1)   // k_mid128 assumes at least one product term
        return fail(PZ_ERR_INVALID, "launch_mid: no product term (rows %d, npi %d, ds_n %d)", nrows, npi, g.ds_n);
    g.batch = batch; g.m1 = M->plan.m1; g.n_ct = 0;
    g.wL2 = M->wL2; g.tw12t = M->tw12t; g.dummy = c.dummy;
    g.groups = 1; g.stagger = 0; g.stagger_mod = 0;
    if (M->plan.m2 == 128) return launch_mid128(M, g, batch, npi, npo, perm, ds, br != nullptr);
    return launch_mid256(M, g, batch);
}


}  // namespace pz
