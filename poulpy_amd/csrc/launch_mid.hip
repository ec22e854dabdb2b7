// launch_mid.hip — dispatch of the fused middle kernels and the key re-slicing (device_mid.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "device_mid.hpp"

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
// m2 = 128 plans: the persistent tile kernels k_mid128 / k_mid128r - which instantiation for this shape (tile geometry by the polynomials in and
// out, the product form: plain / permuted / digit-selected / CGGI block step)
static int launch_mid128(pz_module* M, MidArgs& g, int batch, int npi, int npo, bool perm, bool ds, bool br) {
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, M->device);
    static const bool mid_r = (rt_knob("POULPY_DBG_MID_R", 1) != 0);   // 0: k_mid128 (the kernel of rounds 1-2) instead of k_mid128r (A/B)
    KTimer kt(M, PZ_K_FUSED_MID);
#define PZ_MID128_GO(CT_, NP_, PERM_, SKIPW_)                                                                              \
{                                                                                                                      \
    PZ_TRY(launch_k((k_mid128<CT_, NP_, PERM_, false, false, ((SKIPW_) && (NP_ > 8))>), grid_, dim3(512), lds, M->stream, g)); \
    dispatch_note(M, "k_mid128<CT=%d,NP=%d,PERM=%d,DS=0,BR=0,SKIPW=%d>", CT_, NP_, (int)(PERM_), (int)((SKIPW_) && (NP_ > 8))); \
}
#define PZ_MID128_GOR1(CT_, NP_, PERM_, NR_, HALF_)                                                                        \
{                                                                                                                      \
    PZ_TRY(launch_k((k_mid128r<CT_, NP_, PERM_, NR_, ((HALF_) && (NP_ >= 16))>), grid_, dim3(512), lds, M->stream, g)); \
    dispatch_note(M, "k_mid128r<CT=%d,NP=%d,PERM=%d,NR=%d,HALFIN=%d,KR=%d>", CT_, NP_, (int)(PERM_), NR_, (int)((HALF_) && (NP_ >= 16)), NP_ == 32 ? 3 : PZ_MIDR_KR); \
}
/* k_mid128r: product rows = NP (no idle waves) or NP / 2 with the upper half of the slots without input (key switch) */ \
/* or, 8-slot tile, 8 rows                                                                                             */
#define PZ_MID128_GOR(CT_, NP_, PERM_)                                                                                     \
{                                                                                                                      \
    if (g.row_max == NP_) PZ_MID128_GOR1(CT_, NP_, PERM_, NP_, false)                                                  \
    else if (NP_ >= 16 && npi <= NP_ / 2) PZ_MID128_GOR1(CT_, NP_, PERM_, ((NP_ >= 16) ? NP_ / 2 : NP_), true)          \
    else PZ_MID128_GOR1(CT_, NP_, PERM_, ((NP_ >= 16) ? NP_ / 2 : NP_), false)                                         \
}
/* plain product: the interleaved kernel k_mid128r where it applies — 8 or 16 product rows, no idle waves or exactly the upper half */ \
/* of a 16-slot tile without input (key switch) — k_mid128 otherwise                                                            */
#define PZ_MID128_PICK(CT_, NP_, perm_, skipw_, ring_)                                                                     \
if (ring_ && (!(skipw_) || (NP_ >= 16 && npi <= NP_ / 2 && npo > NP_ / 2))) {                                                      \
    if (perm_) PZ_MID128_GOR(CT_, NP_, true) else PZ_MID128_GOR(CT_, NP_, false)                                       \
} else {                                                                                                               \
    if (perm_) { if (skipw_) PZ_MID128_GO(CT_, NP_, true, true) else PZ_MID128_GO(CT_, NP_, true, false) }             \
    else       { if (skipw_) PZ_MID128_GO(CT_, NP_, false, true) else PZ_MID128_GO(CT_, NP_, false, false) }           \
}
#define PZ_MID128_LAUNCH(CT_, NP_)                                                                                         \
{                                                                                                                      \
    g.n_ct = (batch + CT_ - 1) / CT_;                                                                                  \
    const size_t lds = ((size_t)CT_ * NP_ * kMidRS + 384 + 32) * sizeof(cplx);   /* tile | wL2 | two twiddle rows | exponents */                                         \
    const dim3 grid_(std::min({ncu, 256, g.m1 * g.n_ct}));   /* <= 256: one scratch tile per workgroup (kMidDummyBytes) */ \
    if (br && NP_ == 8 && (g.br_rm & 1) == 0 && g.ncomp == 6 && npi <= 6) {   /* six output columns in an 8-slot tile: 2 x 3 per thread */ \
        PZ_TRY(launch_k((k_mid128<CT_, NP_, false, false, true, false, (NP_ == 8 ? 2 : 0), (NP_ == 8 ? 3 : 0)>), grid_, dim3(512), lds, M->stream, g)); \
        dispatch_note(M, "k_mid128<CT=%d,NP=%d,BR=1,BRNEST=2,NCO=3> (%d ciphertexts per key value)", CT_, NP_, CT_);   \
    } else if (br && NP_ < 32 && (g.br_rm & 1) == 0) {   /* an even number of key rows per coefficient: the nested form of the product loop */ \
        PZ_TRY(launch_k((k_mid128<CT_, NP_, false, false, true, false, (NP_ < 32 ? 2 : 0)>), grid_, dim3(512), lds, M->stream, g)); \
        dispatch_note(M, "k_mid128<CT=%d,NP=%d,BR=1,BRNEST=2> (%d ciphertexts per key value)", CT_, NP_, CT_);         \
    } else if (br) {                                                                                                   \
        PZ_TRY(launch_k((k_mid128<CT_, NP_, false, false, true>), grid_, dim3(512), lds, M->stream, g)); \
        dispatch_note(M, "k_mid128<CT=%d,NP=%d,BR=1> (%d ciphertexts per key value)", CT_, NP_, CT_);                  \
    } else if (ds) {                                                                                                          \
        /* 16-slot tile with 16 terms on 16 inputs (external product) or 8 terms on <= 8 inputs (key switch): k_mid128r */     \
        bool done_ = false;                                                                                            \
        if constexpr (CT_ == 4 && NP_ == 16) {                                                                         \
            if (mid_r && g.ds_n == 16 && npi == 16) {                                                                  \
                PZ_TRY(launch_k((k_mid128r<4, 16, false, 16, false, PZ_MIDR_KR, true>), grid_, dim3(512), lds, M->stream, g)); \
                dispatch_note(M, "k_mid128r<CT=4,NP=16,NR=16,HALFIN=0,KR=%d,DS=1>", PZ_MIDR_KR);                       \
                done_ = true;                                                                                          \
            } else if (mid_r && g.ds_n == 8 && npi <= 8 && npo > 8) {                                                  \
                PZ_TRY(launch_k((k_mid128r<4, 16, false, 8, true, PZ_MIDR_KR, true>), grid_, dim3(512), lds, M->stream, g)); \
                dispatch_note(M, "k_mid128r<CT=4,NP=16,NR=8,HALFIN=1,KR=%d,DS=1>", PZ_MIDR_KR);                        \
                done_ = true;                                                                                          \
            }                                                                                                          \
        }                                                                                                              \
        if (!done_) {                                                                                                  \
            PZ_TRY(launch_k((k_mid128<CT_, NP_, false, true>), grid_, dim3(512), lds, M->stream, g)); \
            dispatch_note(M, "k_mid128<CT=%d,NP=%d,DS=1>", CT_, NP_);                                                  \
        }                                                                                                              \
    } else {                                                                                                           \
        const bool skipw_ = NP_ > 8 && (npi <= NP_ - 8 || npo <= NP_ - 8);   /* shapes with idle waves */              \
        const bool ring_ = mid_r && (g.row_max == NP_ || (NP_ >= 16 && g.row_max == NP_ / 2));   /* product rows k_mid128r is built for */                      \
        PZ_MID128_PICK(CT_, NP_, perm, skipw_, ring_)                                                                  \
    }                                                                                                                  \
}
    // 16 polynomials in, 32 = 16 limbs x 2 columns out, 16 key rows of 32 columns (rank-1 key switch / automorphism / relinearization at 16 limbs:
    // BASELINE configs[4]): 4 ciphertexts per tile and the two output columns as two passes over the same inputs - every key value serves 4
    // ciphertexts instead of the 32-slot tile's 2 (k_mid128r<.., C2>; profiles/r06_ab_mid_c2.txt)
    if (mid_r && !br && !ds && npi == 16 && npo == 32 && g.row_max == 16 && g.ncols == 32 && g.ncomp == 32) {
        g.n_ct = (batch + 3) / 4;
        const size_t lds = ((size_t)4 * 16 * kMidRS + 384 + 32) * sizeof(cplx);
        const dim3 grid_(std::min({ncu, 256, g.m1 * g.n_ct}));
        if (perm) {
            PZ_TRY(launch_k((k_mid128r<4, 16, true, 16, false, PZ_MIDR_KR, false, true>), grid_, dim3(512), lds, M->stream, g));
        } else {
            PZ_TRY(launch_k((k_mid128r<4, 16, false, 16, false, PZ_MIDR_KR, false, true>), grid_, dim3(512), lds, M->stream, g));
        }
        dispatch_note(M, "k_mid128r<CT=4,NP=16,PERM=%d,NR=16,HALFIN=0,KR=%d,C2=1> (two output-column passes per tile of 4 ciphertexts)", (int)perm, PZ_MIDR_KR);
        PZ_HIP(hipGetLastError());
        return PZ_OK;
    }
    if (npi <= 8 && npo <= 8) {
        // <= 8 polynomials in and out (e.g. rank 1 with 4 limbs, BASELINE configs[1]): 8 ciphertexts x 8 slots per tile
        PZ_MID128_LAUNCH(8, 8)
    } else if (npi > 16 || npo > 16) {
        // 17..32 polynomials in or out (rank 2-3 with 8 limbs, rank 1 with 16 limbs): 2 ciphertexts x 32 slots per tile
        PZ_MID128_LAUNCH(2, 32)
    } else {
        PZ_MID128_LAUNCH(4, 16)
    }
#undef PZ_MID128_LAUNCH
#undef PZ_MID128_PICK
#undef PZ_MID128_GO
#undef PZ_MID128_GOR
#undef PZ_MID128_GOR1
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
