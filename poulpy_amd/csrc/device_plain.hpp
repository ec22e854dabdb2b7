// device_plain.hpp — GLWE x constant on the device (poulpy-core operations/glwe.rs:66-131 glwe_mul_const / _assign and poulpy-ckks
// leveled/default/mul.rs:342-415, the complex constant re + i im).
//
// k_mul_const_nz: one thread per coefficient (per coefficient pair (x, x + N/2) in the complex forms, so that the X^{N/2} rotation of the
// imaginary part stays inside the thread) walks every column.  A column's limbs at the thread's coefficients are read ONCE into the
// thread's own LDS slice (the reference reads the whole column into res_big before it normalizes, so the assign forms may overwrite it
// afterwards); the product limbs sum_j a[k + offset - j] * b[j] (wrapping i64, convolution.rs:147-203) are formed from that slice as the
// carry chain of vec_znx_big_normalize asks for them (znx_normalize_inter_walk of znx_steps.hpp: same base2k, any res_offset) and never stored.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "device_fft.hpp"

namespace pz {

constexpr int kMulConstMaxB = 32;       // constant digits carried in the kernel arguments
constexpr int kMulConstMaxA = 64;       // operand limbs staged in LDS
constexpr int kMulConstBlock = 128;

// the normalization plan of one arm (ZnxInterPlan without lsh, which the arms share) and its product (convolution.rs:160-165)
struct MulConstArm {
    long long b[kMulConstMaxB];
    int b_size, big_size, min_size, offset;
    int res_end, res_start, a_end, a_start;
};
struct MulConstArgs {
    long long* res;
    const long long* a;
    long long res_bs, a_bs;   // scalars between ciphertexts
    int n, batch, cols, a_size, res_size, k, lsh;
    // form 0: arm 0 alone; 1: arm 0 then X^{N/2}; 2: arm 0 + X^{N/2} arm 1 (vec_znx_add_assign, no renormalization)
    int form;
    MulConstArm arm[2];
};

// product limb kk of res_big (convolution.rs:395-421; limbs >= min_size are the zeroed tail, :199-202); `la` = the operand limbs of
// this thread's coefficient, limb l at la[l * kMulConstBlock]
__host__ __device__ __forceinline__ long long mc_big(const MulConstArm& w, const long long* la, int a_size, int kk) {
    if (kk >= w.min_size) return 0;
    const int k = kk + w.offset;
    unsigned long long acc = 0;
    if (k < a_size + w.b_size) {
        const int j_min = k >= a_size - 1 ? k - (a_size - 1) : 0;
        const int j_max = k + 1 < w.b_size ? k + 1 : w.b_size;
        for (int j = j_min; j < j_max; ++j) acc += (unsigned long long)la[(k - j) * kMulConstBlock] * (unsigned long long)w.b[j];
    }
    return (long long)acc;
}
// res limb j at `r` (limb stride rls): mode 1 = v, 2 = -v, 3 += v, 4 -= v (wrapping)
__host__ __device__ __forceinline__ void mc_put(long long* r, int mode, long long v) {
    if (mode == 1) *r = v;
    else if (mode == 2) *r = (long long)(0ull - (unsigned long long)v);
    else if (mode == 3) *r = wadd(*r, v);
    else *r = (long long)((unsigned long long)*r - (unsigned long long)v);
}
// vec_znx_normalize_inter_base2k on the product limbs, which are formed as the walk asks for them
__host__ __device__ __forceinline__ void mc_walk(const MulConstArgs& g, const MulConstArm& w, const long long* la, long long* r, long long rls, int mode) {
    const ZnxInterPlan plan{g.lsh, w.res_end, w.res_start, w.a_end, w.a_start};
    znx_normalize_inter_walk(
        plan, g.k, g.res_size, w.big_size, [&](int l) { return mc_big(w, la, g.a_size, l); },
        [&](int j, long long v) { mc_put(r + (long long)j * rls, mode, v); });
}

// the normalization plan of a product and of its arms (convolution.rs:160-162) into g: everything but the pointers, the strides and the grid
inline void mul_const_plan(MulConstArgs& g, int a_size, int res_size, int base2k, long long res_offset, int form, const MulConstArmSpec* arms) {
    g.a_size = a_size; g.res_size = res_size; g.k = base2k; g.form = form;
    for (int u = 0; u < (form == 2 ? 2 : 1); ++u) {
        const MulConstArmSpec& s = arms[u];
        MulConstArm& w = g.arm[u];
        for (int j = 0; j < kMulConstMaxB; ++j) w.b[j] = j < s.b_size ? (long long)s.b[j] : 0;
        const int bound = a_size + s.b_size - 1;   // convolution.rs:160-162
        w.b_size = s.b_size; w.big_size = s.big_size; w.min_size = (s.big_size < bound ? s.big_size : bound); w.offset = (s.hi < bound ? s.hi : bound);
        const ZnxInterPlan p = znx_inter_plan(res_size, s.big_size, base2k, res_offset);
        g.lsh = p.lsh;
        w.res_end = p.res_end; w.res_start = p.res_start; w.a_end = p.a_end; w.a_start = p.a_start;
    }
    if (form != 2) g.arm[1] = g.arm[0];
}

// grid: ceil(batch * npts / kMulConstBlock) workgroups, npts = n (form 0) or n / 2; dynamic LDS = a_size x (2 if paired, else 1) x kMulConstBlock i64
__global__ void __launch_bounds__(kMulConstBlock) k_mul_const_nz(MulConstArgs g) {
    extern __shared__ long long mc_lds[];
    const bool pair = g.form != 0;
    const int npts = pair ? g.n / 2 : g.n;
    const long long t = (long long)blockIdx.x * kMulConstBlock + threadIdx.x;
    if (t >= (long long)g.batch * npts) return;
    const int x = (int)(t % npts);
    const long long bt = t / npts;
    const long long rls = (long long)g.cols * g.n;
    long long* l0 = mc_lds + threadIdx.x;                                   // limbs at x
    long long* l1 = mc_lds + (long long)g.a_size * kMulConstBlock + threadIdx.x;   // limbs at x + N/2
    for (int c = 0; c < g.cols; ++c) {
        const long long* a = g.a + bt * g.a_bs + (long long)c * g.n + x;
        long long* r = g.res + bt * g.res_bs + (long long)c * g.n + x;
        for (int l = 0; l < g.a_size; ++l) l0[l * kMulConstBlock] = __builtin_nontemporal_load(a + (long long)l * rls);
        if (pair)
            for (int l = 0; l < g.a_size; ++l) l1[l * kMulConstBlock] = __builtin_nontemporal_load(a + (long long)l * rls + g.n / 2);
        // (every read of the column precedes the first write: the assign forms read and write the same column)
        if (g.form == 0) {
            mc_walk(g, g.arm[0], l0, r, rls, 1);
        } else if (g.form == 1) {   // X^{N/2} * v: v[x] -> x + N/2, v[x + N/2] -> -(x)
            mc_walk(g, g.arm[0], l0, r + g.n / 2, rls, 1);
            mc_walk(g, g.arm[0], l1, r, rls, 2);
        } else {
            mc_walk(g, g.arm[0], l0, r, rls, 1);
            mc_walk(g, g.arm[0], l1, r + g.n / 2, rls, 1);
            mc_walk(g, g.arm[1], l0, r + g.n / 2, rls, 3);
            mc_walk(g, g.arm[1], l1, r, rls, 4);
        }
    }
}

// k_cnv_by_const on a batch (convolution.rs:147-203, wrapping i64): grid (ceil(n/256), min_size, batch * cols), every column of every
// ciphertext into res_big [ct][limb < big][col][n] - the composed cross-base path (and the cross-check of k_mul_const_nz)
struct CnvConstBatchArgs {
    long long* res;
    const long long* a;
    const long long* b;       // b_size device constants
    long long res_bs, a_bs;
    int cols, res_size, a_size, b_size, offset, n;
};
__global__ void __launch_bounds__(256) k_cnv_by_const_batched(CnvConstBatchArgs g) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= g.n) return;
    const int kk = blockIdx.y, c = (int)(blockIdx.z % g.cols);
    const long long bt = blockIdx.z / g.cols;
    const int k = kk + g.offset;
    unsigned long long acc = 0;
    if (k < g.a_size + g.b_size) {
        const int j_min = k >= g.a_size - 1 ? k - (g.a_size - 1) : 0;
        const int j_max = min(k + 1, g.b_size);
        for (int j = j_min; j < j_max; ++j)
            acc += (unsigned long long)g.a[bt * g.a_bs + (long long)g.n * ((long long)(k - j) * g.cols + c) + x] * (unsigned long long)g.b[j];
    }
    g.res[bt * g.res_bs + (long long)g.n * ((long long)kk * g.cols + c) + x] = (long long)acc;
}

// =====================================================================================================================================
// k_mid_cnv_pt<AS, BS>: the middle of GLWE x plaintext on the row-major pipeline layout (m = m1 x 128), in the pattern of k_mid_cnv3
// (device_cnv.hpp).  Tile = one frequency row q1 of one ciphertext: the plaintext's BS rows and the rank + 1 columns' AS rows are loaded and
// row-transformed ONCE; each thread keeps the plaintext's BS values of its point in registers and convolves them with every column
// (k_mid_cnv's sums, same order); the min_size result rows of a column are inverse-row-transformed into T2[col][ct][kk][m] for the
// normalizing tail.  Columns run from the last to the first: a column's results take the place of its own operand rows and of the
// already consumed rows behind them.  The plaintext's T' has its own batch stride: 0 when one plaintext serves the whole batch, so its
// pass 1 runs once per call.
// =====================================================================================================================================
constexpr int kMidPtRS = 144;   // row stride of the tile, as k_mid_cnv (z[k1][o] at k1 * 9 + o)
struct MidCnvPtArgs {
    const cplx *a_main, *a_last;   // [ct][limb < AS - 1][col][m], [ct][col][m]
    const cplx *b_main, *b_last;   // [pt][limb < BS - 1][m], [pt][m]
    long long b_main_bs, b_last_bs;   // points between plaintexts (0: shared)
    cplx* T2;                      // [col][ct][kk < min_size][m]
    int cols, min_size, offset, m1, batch;
    const cplx* wL2;
    const cplx* tw12t;
};
__host__ __device__ constexpr int mid_pt_rows(int as, int bs, int cols, int min_size) { return bs + cols * as + (min_size > as ? min_size - as : 0); }

template <int AS, int BS>
__global__ void __launch_bounds__(256) k_mid_cnv_pt(MidCnvPtArgs g) {
    constexpr int M2 = 128, RS = kMidPtRS;
    extern __shared__ cplx lds[];
    const int tid = threadIdx.x, row = tid >> 3, o = tid & 7;
    const int q1 = blockIdx.x % g.m1, bt = blockIdx.x / g.m1;
    const long long m = (long long)g.m1 * M2;
    const int rin = BS + g.cols * AS;
    cplx* wl = lds + mid_pt_rows(AS, BS, g.cols, g.min_size) * RS;
    cplx* twrow = wl + M2;
    if (tid < M2) { wl[tid] = g.wL2[tid]; twrow[tid] = g.tw12t[(long long)q1 * M2 + tid]; }
    __syncthreads();
    // ---- forward row DFT of the plaintext rows and of every column's rows, 32 rows per sweep (k_mid_cnv's row transform) ----
    for (int r0 = 0; r0 < rin; r0 += 32) {
        const int r = r0 + row;
        if (r < rin) {
            const cplx* src;
            if (r < BS) src = r < BS - 1 ? g.b_main + (long long)bt * g.b_main_bs + (long long)r * m : g.b_last + (long long)bt * g.b_last_bs;
            else {
                const int c = (r - BS) / AS, l = (r - BS) % AS;
                src = l < AS - 1 ? g.a_main + (((long long)bt * (AS - 1) + l) * g.cols + c) * m : g.a_last + ((long long)bt * g.cols + c) * m;
            }
            src += (long long)q1 * M2 + o;
            cplx x[16];
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) x[n1] = ld_stream(src + 8 * n1);
            cplx* rowbuf = lds + r * RS;
            Bfly<16, false>::run(x);
#pragma unroll
            for (int k1 = 0; k1 < 16; ++k1) {
                cplx v = x[k1];
                if (k1 > 0) v = cmul(v, wl[o * k1]);
                rowbuf[k1 * 9 + o] = v;
            }
            row_sync();
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int oo = 0; oo < 8; ++oo) x[8 * h + oo] = rowbuf[(o + 8 * h) * 9 + oo];
            Bfly<8, false>::run(x);
            Bfly<8, false>::run(x + 8);
            row_sync();
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2) rowbuf[o + 8 * h + 16 * k2] = x[8 * h + k2];
        }
    }
    __syncthreads();
    const int pt = tid & 127, par = tid >> 7;
    cplx bv[BS];   // the plaintext at this point, for every column
#pragma unroll
    for (int j = 0; j < BS; ++j) bv[j] = lds[j * RS + pt];
    for (int c = g.cols - 1; c >= 0; --c) {
        cplx* base = lds + (BS + c * AS) * RS;
        cplx accs[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int kk = par + 2 * u;
            cplx acc = make_double2(0.0, 0.0);
            if (kk < g.min_size) {
                const int k = kk + g.offset;
#pragma unroll
                for (int j = 0; j < BS; ++j) {   // j ascending over [max(0, k - AS + 1), min(k + 1, BS)): k_mid_cnv's order
                    const int i = k - j;
                    if (i >= 0 && i < AS) {
                        const cplx av = base[i * RS + pt], b = bv[j];
                        acc.x = __builtin_fma(av.x, b.x, acc.x);
                        acc.x = __builtin_fma(-av.y, b.y, acc.x);
                        acc.y = __builtin_fma(av.x, b.y, acc.y);
                        acc.y = __builtin_fma(av.y, b.x, acc.y);
                    }
                }
            }
            accs[u] = acc;
        }
        __syncthreads();   // (every read of this column's rows, and the previous column's inverse transform, are done)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int kk = par + 2 * u;
            if (kk < g.min_size) base[kk * RS + pt] = accs[u];
        }
        __syncthreads();
        // ---- inverse row DFT of the result rows, x conj tw12 -> T2' ----
        for (int r0 = 0; r0 < g.min_size; r0 += 32) {
            const int r = r0 + row;
            if (r < g.min_size) {
                cplx* rowbuf = base + r * RS;
                cplx u[16];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k2 = 0; k2 < 8; ++k2) u[8 * h + k2] = rowbuf[o + 8 * h + 16 * k2];
                Bfly<8, true>::run(u);
                Bfly<8, true>::run(u + 8);
                row_sync();
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int oo = 0; oo < 8; ++oo) {
                        cplx v = u[8 * h + oo];
                        const int k1 = o + 8 * h;
                        if (k1 > 0 && oo > 0) v = cmulc(v, wl[oo * k1]);
                        rowbuf[k1 * 9 + oo] = v;
                    }
                row_sync();
#pragma unroll
                for (int k1 = 0; k1 < 16; ++k1) u[k1] = rowbuf[k1 * 9 + o];
                Bfly<16, true>::run(u);
                cplx* dst = g.T2 + (((long long)c * g.batch + bt) * g.min_size + r) * m + (long long)q1 * M2 + o;
#pragma unroll
                for (int n1 = 0; n1 < 16; ++n1) st_stream(dst + 8 * n1, cmulc(u[n1], twrow[o + 8 * n1]));
            }
        }
    }
}

}  // namespace pz
