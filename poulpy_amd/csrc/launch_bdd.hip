// launch_bdd.hip — kernels of the BDD circuit evaluator (pz_bdd_circuit_execute_batched): the per-call gather table and the gathered
// instantiations of the small-ring CMUX kernels (device_small.hpp, device_small_one.hpp), one launch per circuit level.
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "bdd_schedule.hpp"
#include "device_small.hpp"
#include "device_small_one.hpp"

namespace pz {

static inline int small_m1(const pz_module* M) { return (int)(M->m / kSmallM2); }

struct BddTableArgs {
    const BddGate* gates;
    const uint32_t* level_start;
    int levels;
    uint32_t total;
    int batch, nbits;
    long long* state;
    long long* out;
    long long ct;
    const cplx* const* keys;
    SmallGather* tab;
};
// one thread per (gate, input): slot indices and the selector of the immutable level table -> addresses of this call.  All levels at once, in front of
// the first level's launch.  Every index was checked on the host (bdd_check); the key pointers are the call's own array.
__global__ void __launch_bounds__(256) k_bdd_table(BddTableArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.total * a.batch) return;
    const uint32_t gi = (uint32_t)(idx / a.batch);
    const int b = (int)(idx % a.batch);
    int lo = 0, hi = a.levels;   // the level of gate gi: the last one that starts at or before it
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.level_start[mid] <= gi) lo = mid; else hi = mid;
    }
    const uint32_t first = a.level_start[lo], count = a.level_start[lo + 1] - first;
    const BddGate g = a.gates[gi];
    SmallGather e;
    e.t = a.state + ((long long)g.t * a.batch + b) * a.ct;
    e.f = a.state + ((long long)g.f * a.batch + b) * a.ct;
    e.res = (g.res & kBddOut) ? a.out + ((long long)(g.res & ~kBddOut) * a.batch + b) * a.ct : a.state + ((long long)g.res * a.batch + b) * a.ct;
    e.Pp = a.keys[(long long)b * a.nbits + g.sel];
    a.tab[(long long)first * a.batch + (long long)b * count + (gi - first)] = e;   // input-major inside the level: one key's ciphertexts side by side
}
int launch_bdd_table(pz_module* M, const BddTableCall& c) {
    const long long n = (long long)c.total * c.batch;
    if (n <= 0) return PZ_OK;
    BddTableArgs a{c.gates, c.level_start, c.levels, c.total, c.batch, c.nbits, c.state, c.out, c.ct, c.keys, c.tab};
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_bdd_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, M->stream, a);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

__global__ void __launch_bounds__(256) k_bdd_one(long long* slot, long long ct, int batch, long long limb_stride, long long d0, long long d1, int used) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    long long* p = slot + (long long)b * ct;
    p[0] = d0;
    if (used > 1) p[limb_stride] = d1;
}
int launch_bdd_one(pz_module* M, long long* slot, long long ct, int batch, long long limb_stride, long long d0, long long d1, int used) {
    if (batch <= 0) return PZ_OK;
    KTimer kt(M, PZ_K_ELEMENTWISE);
    hipLaunchKernelGGL(k_bdd_one, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, M->stream, slot, ct, batch, limb_stride, d0, d1, used);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

// ---- the gathered CMUX: t, f, res of one layout (`size` limbs), the difference of `size` limbs, f the operand of every column ----
static SmallDiff gather_diff(const pz_module* M, const SmallGatherShape& s) {
    const long long n = (long long)M->n;
    const PolyMap map{s.size, s.cols, n * s.cols * s.size, (long long)s.cols * n, n, 0};
    return SmallDiff{nullptr, nullptr, map, map, s.size, s.size, 0u};
}
bool small_one_gather_supported(const pz_module* M, const SmallGatherShape& s) {
    const int m1 = small_m1(M);
    return (M->m % kSmallM2) == 0 && (m1 == 4 || m1 == 8) && s.cols == 2 && s.ksz >= 1 && s.ksz <= 4 && s.size >= 1 && s.cols * s.size <= 8 && s.dnum >= 1;
}
int launch_small_one_gather(pz_module* M, int batch, const SmallGatherShape& s, const SmallGather* tab) {
    if (batch <= 0) return PZ_OK;
    if (!small_one_gather_supported(M, s)) return fail(PZ_ERR_UNSUPPORTED, "gathered one-kernel product: unsupported shape");
    PZ_TRY(ensure_small_tables(M));
    const long long n = (long long)M->n;
    SmallOneArgs g;
    g.diff = gather_diff(M, s);
    g.src = nullptr; g.smap = g.diff.fmap; g.Pp = nullptr; g.res = nullptr; g.small = nullptr;   // (t, f, res, Pp: tab[c])
    g.rot_tab = nullptr;
    g.res_bs = g.small_bs = n * s.cols * s.size;
    g.batch = batch; g.npi = s.cols * s.size; g.nrows = s.dnum * s.cols; g.ncols = s.cols * s.ksz; g.ksz = s.ksz;
    g.res_cols = s.cols; g.res_size = s.size; g.small_cols = s.cols; g.small_size = s.size; g.base2k = s.base2k; g.body_col = -1;
    g.tw1 = M->s_tw1; g.tw12t = M->s_tw12t; g.wL2 = M->s_wL2; g.tw1inv = M->s_tw1inv; g.margin = M->probe ? M->margin : nullptr;
    g.res2 = nullptr; g.small2 = nullptr; g.res2_bs = g.small2_bs = 0; g.res2_size = g.small2_size = 0;
    const int m1 = small_m1(M);
    const size_t lds = ((size_t)8 * m1 * kSmallRS + kSmallM2 + m1) * sizeof(cplx);
    KTimer kt(M, PZ_K_FUSED_TAIL);
#define X(M1_, KS_)                                                                                                        \
    if (m1 == M1_ && s.ksz == KS_) {                                                                                       \
        PZ_TRY(launch_k((k_small_one_gather<M1_, KS_>), dim3(batch), dim3(512), lds, M->stream, g, tab));                  \
        PZ_HIP(hipGetLastError());                                                                                         \
        return PZ_OK;                                                                                                      \
    }
    X(4, 1) X(4, 2) X(4, 3) X(4, 4) X(8, 1) X(8, 2) X(8, 3) X(8, 4)
#undef X
    return fail(PZ_ERR_UNSUPPORTED, "gathered one-kernel product: m1 = %d, %d key limbs", m1, s.ksz);
}
int launch_small_fwd_gather(pz_module* M, int batch, const SmallGatherShape& s, const SmallGather* tab, cplx* S) {
    if (batch <= 0) return PZ_OK;
    PZ_TRY(ensure_small_tables(M));
    const int npolys = batch * s.cols * s.size;
    SmallFwdArgs g;
    g.diff = gather_diff(M, s);
    g.src = nullptr; g.smap = g.diff.fmap; g.S = S; g.npolys = npolys; g.tw1 = M->s_tw1; g.tw12t = M->s_tw12t; g.wL2 = M->s_wL2; g.natural = 0;
    g.use_dmap = 0; g.dmap = g.diff.fmap; g.mul = nullptr;
    const int m1 = small_m1(M);
    const size_t lds = ((size_t)2 * m1 * kSmallRS + kSmallM2) * sizeof(cplx);
    KTimer kt(M, PZ_K_FWD_PASS1);
    const dim3 grid((unsigned)((npolys + 1) / 2));
#define X(M1_)                                                                                      \
    if (m1 == M1_) {                                                                                \
        PZ_TRY(launch_k((k_small_fwd_gather<M1_>), grid, dim3(256), lds, M->stream, g, tab));       \
        PZ_HIP(hipGetLastError());                                                                  \
        return PZ_OK;                                                                               \
    }
    X(4) X(8) X(16)
#undef X
    return fail(PZ_ERR_UNSUPPORTED, "gathered small-ring pipeline: m1 = %d", m1);
}
int launch_small_inv_gather(pz_module* M, int batch, const SmallGatherShape& s, const SmallGather* tab, const cplx* S) {
    if (batch <= 0) return PZ_OK;
    PZ_TRY(ensure_small_tables(M));
    const long long n = (long long)M->n;
    SmallInvArgs g;
    g.S = S; g.Pp = nullptr; g.res = nullptr; g.small = nullptr;   // (f, res, Pp: tab[c])
    g.res_bs = g.small_bs = n * s.cols * s.size;
    g.batch = batch; g.npi = s.cols * s.size; g.nrows = s.dnum * s.cols; g.ncols = s.cols * s.ksz; g.cols_out = s.cols; g.ksz = s.ksz;
    g.res_cols = s.cols; g.res_size = s.size; g.small_cols = s.cols; g.small_size = s.size; g.base2k = s.base2k; g.body_col = -1;
    g.tw12t = M->s_tw12t; g.wL2 = M->s_wL2; g.tw1inv = M->s_tw1inv;
    g.post_rsh = 0; g.au_p = 1; g.au_pinv = 1; g.au_mode = 0;
    g.S_out = nullptr; g.tw1 = M->s_tw1; g.fwd_limbs = 0;
    g.margin = M->probe ? M->margin : nullptr;
    g.acc32 = 0;
    g.res2 = nullptr; g.small2 = nullptr; g.res2_bs = g.small2_bs = 0; g.res2_size = g.small2_size = 0;
    const int m1 = small_m1(M);
    const size_t lds = ((size_t)s.ksz * m1 * small_inv_rs(m1, false) + kSmallM2 + m1) * sizeof(cplx);
    const int grid = ((batch + 7) / 8) * 8 * s.cols;   // workgroup id -> ciphertext and column as in launch_small_inv
    KTimer kt(M, PZ_K_FUSED_TAIL);
#define X(M1_, KS_)                                                                                                        \
    if (m1 == M1_ && s.ksz == KS_) {                                                                                       \
        PZ_TRY(launch_k((k_small_inv_gather<M1_, KS_>), dim3(grid), dim3(64 * m1), lds, M->stream, g, tab));               \
        PZ_HIP(hipGetLastError());                                                                                         \
        return PZ_OK;                                                                                                      \
    }
    X(4, 1) X(4, 2) X(4, 3) X(4, 4) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4)
#undef X
    return fail(PZ_ERR_UNSUPPORTED, "gathered small-ring pipeline: m1 = %d, %d key limbs", m1, s.ksz);
}

}  // namespace pz
