// device_small.hpp — two-kernel GLWE product pipeline for N = 1024 / 2048 / 4096 (m = M1 x 128, M1 = 4 / 8 / 16), where a whole
// polynomial (<= 32 KiB of spectrum) fits in LDS.  The three-kernel pipeline moves 1.5 MiB per ciphertext at BASELINE configs[1] (N = 4096, 4 limbs: limbs in,
// T', T' again, T2', T2' again, limbs out); here the spectra cross HBM once:
//   k_small_fwd : i64 limbs -> full forward transform in LDS (column pass in registers, row pass as in the middle kernel) -> S
//   k_small_inv : one workgroup per (ciphertext, output column): pointwise product with the row-sliced key in registers (no LDS:
//                 the product needs no exchange), two output limbs at a time -> inverse row pass + inverse column pass in LDS ->
//                 round, (+ key-switch body), carry chain with the carries in registers -> balanced digits
// = 1.0 MiB per ciphertext (+ the second column's re-read of S, served by the XCD's L2: both columns of a ciphertext are placed on
// one XCD).  Same tables, same stage formulas as k_fwd_pass1 / k_mid128 / k_inv_tail, regrouped; dsize = 1, one base2k, <= 4 key limbs.
//   S  : S[poly][q1][q2]     (the tile layout of the middle kernel after its forward row pass)
//   Pp : P'[q1][r][c][q2]    (the row-sliced key of the three-kernel pipeline)
// Variants of k_small_inv (template flags): NOPROD - the spectra are given (blind rotation: the block step produced them), FWD - the
// forward transform of the new digits follows in the same workgroup (the next block's input), AU - the glwe_automorphism family
// (phi as an index / sign map in the carry-chain stage; optionally the trace's one-bit shift on the way out).
#pragma once
#include "device_fft.hpp"

namespace pz {

constexpr int kSmallM2 = 128, kSmallRS = 16 * 9;   // row stride as in k_mid128 (z[k1][o] at k1*9 + o)
constexpr int kSmallIdftRS = kSmallRS + 1;
// k_small_inv<.., NOPROD> (blind rotation's tail): the spectra arrive in the standard order and consecutive lanes drop them at M1 consecutive ROWS
// of the tile - with a row stride of 144 points (= 0 mod 64 banks) an M1-way bank conflict on every write (round 5 counters: 4.6 conflict cycles per
// LDS instruction, profiles/r05_br_pmc/n2048_pmc.txt).  Row stride = 144 + d with (row * d + column) mod 16 distinct over the 16 lanes of a
// 128-bit access: d = 4 (M1 = 4: 4 rows x 4 columns), 2 (8 rows x 2 columns), 1 (16 rows).  The in-row layout (k1 * 9 + o) is untouched.
constexpr int small_inv_rs(int m1, bool noprod) { return noprod ? kSmallRS + (m1 == 16 ? 1 : (m1 == 8 ? 2 : 4)) : kSmallRS; }
#ifndef PZ_SMALL_STAMP
#define PZ_SMALL_STAMP 0   // diagnostic build: per-phase s_memtime totals of k_small_inv, printed by three waves of three workgroups
#endif

#ifndef PZ_SMALL_PROBE
#define PZ_SMALL_PROBE 1   // (A/B: -DPZ_SMALL_PROBE=0 compiles the run-time rounding-margin probe out of the small-ring kernels)
#endif
// the 2 M1 coefficients thread t of a polynomial owns in the forward column pass (i = j1 128 + t and m + i), as wrapping i64 differences.
// SRC 1: t - f; 2: X^rot f - f.  Digits of D span one bit more than a normalized source (more on un-normalized input): they stay 64-bit
// integers up to the conversion to f64, like every input of this kernel.
template <int M1, int SRC>
__device__ __forceinline__ void small_diff_load(const SmallDiff& d, int p, int t, long long (&re)[M1], long long (&im)[M1]) {
    constexpr int M2 = 128;
    constexpr unsigned m = (unsigned)M1 * M2, n = 2 * m;
    const int limb = (p / d.fmap.ni) % d.fmap.nj;
    const bool hf = limb < d.f_size, ht = SRC == 1 && limb < d.t_size;
    const long long* fa = d.f + map_off(d.fmap, p);
    unsigned long long fr[M1], fi[M1], tr[M1], ti[M1];
#pragma unroll
    for (int j1 = 0; j1 < M1; ++j1) { fr[j1] = fi[j1] = tr[j1] = ti[j1] = 0ull; }
    if (hf) {
#pragma unroll
        for (int j1 = 0; j1 < M1; ++j1) {
            fr[j1] = (unsigned long long)fa[j1 * M2 + t];
            fi[j1] = (unsigned long long)fa[m + j1 * M2 + t];
        }
        if constexpr (SRC == 2) {
#pragma unroll
            for (int j1 = 0; j1 < M1; ++j1) {
                const unsigned s0 = ((unsigned)(j1 * M2 + t) - d.rot) & (2 * n - 1), s1 = (m + (unsigned)(j1 * M2 + t) - d.rot) & (2 * n - 1);
                const unsigned long long v0 = (unsigned long long)fa[s0 & (n - 1)], v1 = (unsigned long long)fa[s1 & (n - 1)];
                tr[j1] = s0 >= n ? 0ull - v0 : v0;
                ti[j1] = s1 >= n ? 0ull - v1 : v1;
            }
        }
    }
    if constexpr (SRC == 1) {
        if (ht) {
            const long long* ta = d.t + map_off(d.tmap, p);
#pragma unroll
            for (int j1 = 0; j1 < M1; ++j1) {
                tr[j1] = (unsigned long long)ld_stream(ta + j1 * M2 + t);
                ti[j1] = (unsigned long long)ld_stream(ta + m + j1 * M2 + t);
            }
        }
    }
#pragma unroll
    for (int j1 = 0; j1 < M1; ++j1) { re[j1] = (long long)(tr[j1] - fr[j1]); im[j1] = (long long)(ti[j1] - fi[j1]); }
}

// Rotated source of a key switch (pz_lwe_from_glwe_many_batched): the 2 M1 coefficients thread t owns of X^rot a, read from `a`
// through the monomial's index and sign map (coefficient i = a[(i - rot) mod 2n], negated where that index is >= n), as SRC = 2 above reads t = X^rot f
template <int M1>
__device__ __forceinline__ void small_rot_load(const long long* a, unsigned rot, int t, long long (&re)[M1], long long (&im)[M1]) {
    constexpr int M2 = 128;
    constexpr unsigned m = (unsigned)M1 * M2, n = 2 * m;
#pragma unroll
    for (int j1 = 0; j1 < M1; ++j1) {
        const unsigned s0 = ((unsigned)(j1 * M2 + t) - rot) & (2 * n - 1), s1 = (m + (unsigned)(j1 * M2 + t) - rot) & (2 * n - 1);
        const unsigned long long v0 = (unsigned long long)a[s0 & (n - 1)], v1 = (unsigned long long)a[s1 & (n - 1)];
        re[j1] = (long long)(s0 >= n ? 0ull - v0 : v0);
        im[j1] = (long long)(s1 >= n ? 0ull - v1 : v1);
    }
}

struct SmallFwdArgs {
    const long long* src;
    PolyMap smap;
    cplx* S;
    int npolys;
    const cplx* tw1;     // [16] twist of the column pass
    const cplx* tw12t;   // [q1][j2]
    const cplx* wL2;     // exp(2 pi i t / 128)
    int natural;         // 1: spectrum written in the standard device order [q1 + M1 q2] (pointwise consumers holding standard keys: the
                         // blind rotation's block step) instead of S[q1][q2]; the 8 M1 threads of a store still cover 8 M1 consecutive points
    // per-op vec_znx_dft_apply / svp_apply_dft in ONE kernel (round 3; natural order only): polynomial p goes to S + map_off(dmap, p) / 2
    // instead of S + p m, multiplied pointwise by mul (an SvpPPol, standard order) when given
    int use_dmap;
    PolyMap dmap;
    const cplx* mul;
    SmallDiff diff;      // SRC != 0: the two sources of the difference (src / smap are not read)
};

// 256 threads = 2 polynomials x 128 threads; LDS 2 x M1 rows x 144 points + wL2.  SRC: 0 the limbs of `src`, 1 / 2 the CMUX forms (SmallDiff)
// GATHER (the BDD evaluator's level launches, SRC = 1): polynomial p belongs to ciphertext p / npi of the launch, whose two sources are tab[p / npi].t / .f
// (each addressed as ciphertext 0 of its own pointer); the spectra stay dense by launch index.
template <int M1, int SRC, bool GATHER>
__device__ __forceinline__ void small_fwd_body(const SmallFwdArgs& g, const SmallGather* __restrict__ tab) {
    static_assert(!GATHER || SRC == 1, "gathered form: the two-source CMUX");
    constexpr int M2 = kSmallM2, RS = kSmallRS;
    constexpr long long m = (long long)M1 * kSmallM2;
    extern __shared__ cplx lds[];
    const int tid = threadIdx.x, pl = tid >> 7, t = tid & 127;
    cplx* wl = lds + 2 * M1 * RS;
    if (tid < M2) wl[tid] = g.wL2[tid];
    const int p = blockIdx.x * 2 + pl;
    const bool active = p < g.npolys;
    cplx* buf = lds + pl * M1 * RS;
    // ---- column pass: thread t owns column j2 = t, M1 points over j1 (k_fwd_pass1 with one radix-M1 butterfly)
    {
        long long re[M1], im[M1];
        if constexpr (SRC == 0) {
            const long long* a = g.src + map_off(g.smap, active ? p : g.npolys - 1);
#pragma unroll
            for (int j1 = 0; j1 < M1; ++j1) {
                re[j1] = ld_stream(a + j1 * M2 + t);
                im[j1] = ld_stream(a + m + j1 * M2 + t);
            }
        } else if constexpr (GATHER) {
            const int npi = g.diff.fmap.nj * g.diff.fmap.ni, pp = active ? p : g.npolys - 1;
            const SmallGather e = tab[pp / npi];
            SmallDiff d = g.diff;
            d.t = e.t; d.f = e.f;
            small_diff_load<M1, SRC>(d, pp % npi, t, re, im);
        } else {
            small_diff_load<M1, SRC>(g.diff, active ? p : g.npolys - 1, t, re, im);
        }
        cplx v[M1];
#pragma unroll
        for (int j1 = 0; j1 < M1; ++j1) v[j1] = cmul(make_double2((double)re[j1], (double)im[j1]), g.tw1[j1]);
        Bfly<M1, false>::run(v);
#pragma unroll
        for (int q1 = 0; q1 < M1; ++q1) buf[q1 * RS + t] = cmul(v[q1], g.tw12t[q1 * M2 + t]);
    }
    __syncthreads();
    // ---- row pass: 8 lanes per row, exactly the forward pass of k_mid128 (8 * M1 of the polynomial's 128 threads)
    const int row = t >> 3, o = t & 7;
    if (row < M1) {
        cplx* rowbuf = buf + row * RS;
        cplx x[16];
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) x[n1] = rowbuf[o + 8 * n1];
        row_sync();
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
        if (active) {
            cplx* dst = g.S + (g.use_dmap ? map_off(g.dmap, p) / 2 : (long long)p * m) + (g.natural ? row + M1 * o : row * M2 + o);
            const int qs = g.natural ? M1 : 1;
            if (g.mul) {   // (natural order) x ppol[q], q = row + M1 (o + 8h + 16 k2)
                const cplx* mp = g.mul + row + M1 * o;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k2 = 0; k2 < 8; ++k2) x[8 * h + k2] = cmul(x[8 * h + k2], mp[(8 * h + 16 * k2) * M1]);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2) dst[(8 * h + 16 * k2) * qs] = x[8 * h + k2];   // S[q1][q2 = o + 8h + 16 k2]: re-read twice, kept cacheable
        }
    }
}
template <int M1, int SRC = 0>
__global__ void __launch_bounds__(256, 2) k_small_fwd(SmallFwdArgs g) { small_fwd_body<M1, SRC, false>(g, nullptr); }
template <int M1>
__global__ void __launch_bounds__(256, 2) k_small_fwd_gather(SmallFwdArgs g, const SmallGather* __restrict__ tab) { small_fwd_body<M1, 1, true>(g, tab); }

// standard device VmpPMat  P[p][q1 + M1*q2]  ->  P'[q1][p][q2]  for the ring degrees without a pipeline plan (one thread per point)
template <int M1>
__global__ void __launch_bounds__(256) k_small_permute(const cplx* __restrict__ P, cplx* __restrict__ Pp, int npolys) {
    constexpr int M2 = kSmallM2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // over [q1][p][q2]
    const long long total = (long long)M1 * npolys * M2;
    if (idx >= total) return;
    const int q2 = (int)(idx % M2);
    const long long t = idx / M2;
    const int p = (int)(t % npolys), q1 = (int)(t / npolys);
    Pp[idx] = P[(long long)p * (M1 * M2) + q1 + M1 * q2];
}

// Per-op vec_znx_idft_apply in one kernel for N = 1024 / 2048 / 4096 (round 3): spectrum in the standard device order -> inverse row pass
// (k_mid128's) x conj tw12 -> inverse column pass, x tw1inv (1/m folded in), round half away, saturating i64 -> VecZnxBig.  The per-op
// path otherwise runs k_inv_pass2 + k_inv_pass1 with the spectrum's worth of T between them in HBM (32 B per coefficient instead of 16).
struct SmallIdftArgs {
    const cplx* S;       // spectra, polynomial p at S + map_off(smap, p) / 2 (standard order [q1 + M1 q2])
    PolyMap smap;
    long long* res;      // i64 coefficients, polynomial p at res + map_off(dmap, p)
    PolyMap dmap;
    int npolys;
    const cplx* tw12t;
    const cplx* wL2;
    const cplx* tw1inv;
    unsigned long long* margin;   // rounding-margin probe (margin_note, device_fft.hpp); null = off
};
// 256 threads = 2 polynomials x 128 threads; LDS 2 x M1 rows x 144 points + wL2
template <int M1>
__global__ void __launch_bounds__(256, 2) k_small_idft(SmallIdftArgs g) {
    // row stride 145 points (= 4 dwords mod 64 banks): the transposing drop below writes M1 consecutive rows at one column from
    // consecutive lanes - with the tile's usual 144 (= 0 mod 64) that is an M1-way bank conflict (N = 4096: 0.79 vs 0.46 ms per GiB)
    constexpr int M2 = kSmallM2, RS = kSmallIdftRS;
    constexpr long long m = (long long)M1 * kSmallM2;
    extern __shared__ cplx lds[];
    const int tid = threadIdx.x, pl = tid >> 7, t = tid & 127;
    cplx* wl = lds + 2 * M1 * RS;
    cplx* tw1i = wl + M2;   // untwist factors as LDS broadcasts (k_small_inv)
    if (tid < M2) wl[tid] = g.wL2[tid];
    else if (tid < M2 + M1) tw1i[tid - M2] = g.tw1inv[tid - M2];
    const int p = blockIdx.x * 2 + pl;
    const bool active = p < g.npolys;
    const cplx* src = g.S + map_off(g.smap, active ? p : g.npolys - 1) / 2;
    cplx* buf = lds + pl * M1 * RS;
    // consecutive threads read consecutive points q = q1 + M1 q2 and drop them at (q1, q2) of the tile; all M1 loads first (left to
    // itself the compiler waited for each one before its LDS store: 61 of the 63 loads of the N = 4096 kernel sat behind vmcnt(0))
    {
        cplx in[M1];
#pragma unroll
        for (int i = 0; i < M1; ++i) in[i] = src[t + 128 * i];
        // q = t + 128 i: q % M1 = t % M1, q / M1 = t / M1 + (128 / M1) i
        cplx* drop = buf + (t % M1) * RS + t / M1;
#pragma unroll
        for (int i = 0; i < M1; ++i) drop[(128 / M1) * i] = in[i];
    }
    __syncthreads();
    // inverse row pass: 8 lanes per row (8 M1 of the polynomial's 128 threads)
    const int row = t >> 3, o = t & 7;
    if (row < M1) {
        cplx* rowbuf = buf + row * RS;
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
                if (oo > 0) v = cmulc(v, wl[oo * k1]);   // (k1 = 0 reads W^0 = 1: exact)
                rowbuf[k1 * 9 + oo] = v;
            }
        row_sync();
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) u[k1] = rowbuf[k1 * 9 + o];
        Bfly<16, true>::run(u);
        row_sync();
        const cplx* tw = g.tw12t + row * M2 + o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // two batches of 8 loads (k_small_inv)
            cplx t8[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t8[i] = tw[8 * (8 * h + i)];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) rowbuf[o + 8 * (8 * h + i)] = cmulc(u[8 * h + i], t8[i]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    // inverse column pass: thread t owns column j2 = t
    {
        cplx v[M1];
#pragma unroll
        for (int q1 = 0; q1 < M1; ++q1) v[q1] = buf[q1 * RS + t];
        Bfly<M1, true>::run(v);
        double big = 0.0;   // a SUM, so that a NaN or an infinity selects the saturating conversion (k_small_inv)
#pragma unroll
        for (int j1 = 0; j1 < M1; ++j1) big += fabs(v[j1].x) + fabs(v[j1].y);
        big *= 1.0 / (double)m;
        if (PZ_SMALL_PROBE && g.margin && active) {
            double worst = 0.0;
#pragma unroll
            for (int j1 = 0; j1 < M1; ++j1) {
                const cplx val = cmul(v[j1], tw1i[j1]);
                worst = fmax(worst, fmax(margin_dist(val.x), margin_dist(val.y)));
            }
            margin_note(g.margin, worst);
        }
        if (active) {
            long long* dst = g.res + map_off(g.dmap, p) + t;
            if (big < 2251799813685247.0) {
#pragma unroll
                for (int j1 = 0; j1 < M1; ++j1) {
                    const cplx val = cmul(v[j1], tw1i[j1]);
                    dst[j1 * M2] = fast_i64_from_integral(round_half_away(val.x));
                    dst[m + j1 * M2] = fast_i64_from_integral(round_half_away(val.y));
                }
            } else {
#pragma unroll
                for (int j1 = 0; j1 < M1; ++j1) {
                    const cplx val = cmul(v[j1], tw1i[j1]);
                    dst[j1 * M2] = sat_i64_from_integral(round_half_away(val.x));
                    dst[m + j1 * M2] = sat_i64_from_integral(round_half_away(val.y));
                }
            }
        }
    }
}

struct SmallInvArgs {
    const cplx* S;
    const cplx* Pp;
    long long* res;
    const long long* small;      // key-switch body operand (added to column body_col), may be null
    long long res_bs, small_bs;
    int batch, npi, nrows, ncols, cols_out, ksz;
    int res_cols, res_size, small_cols, small_size, base2k, body_col;
    const cplx* tw12t;
    const cplx* wL2;
    const cplx* tw1inv;          // [16] untwist with 1/m folded in
    int post_rsh;                // AU: the digits leave through vec_znx_rsh_assign by one bit (k_inv_tail<.., RSH>, device_fft.hpp); base2k <= 29
    unsigned au_p;               // AU: Galois element mod 2n (coefficient i goes to i * au_p mod 2n, negated beyond n)
    unsigned au_pinv;            // AU: its inverse mod 2n (set by launch_small_inv)
    int au_mode;                 // AU: 0 phi(normalize(big)), 1 normalize(phi(big) + a), 2 normalize(phi(big) - a), 3 normalize(a - phi(big));
                                 //     a = column `col` of `small` (the key-switch input itself), big includes the body (body_col)
    cplx* S_out;                 // FWD: spectra of the first fwd_limbs limbs of the NEW res column, standard order, [b][limb * cols_out + col]
    const cplx* tw1;             // FWD: twist of the forward column pass
    int fwd_limbs;               // FWD: <= min(KS, res_size)
    unsigned long long* margin;  // rounding-margin probe (margin_note, device_fft.hpp); null = off
    int acc32;                   // NOPROD (blind rotation's tail): bit 0 `small` holds 32-bit digits, bit 1 `res` takes 32-bit digits (bits 2 / 3: 16-bit digits) - same
                                 // element strides, half the bytes: between the blocks of a rotation the accumulator only ever holds normalized
                                 // digits (base2k <= 31), and this kernel moves them at HBM rate (api_br.hip)
    // DUAL (conditional swap, pz_glwe_cswap_batched): a second result from the same big value, res2 = normalize(small2 - big) on every column
    // (vec_znx_big_sub_small_a: limbs of big beyond small2_size enter negated); both containers have res_cols columns
    long long* res2;
    const long long* small2;
    long long res2_bs, small2_bs;
    int res2_size, small2_size;
};

// 64 M1 threads (1024 at N = 4096: 16 waves, the product phase is latency-bound with fewer); LDS holds the KS output polynomials of one
// (ciphertext, column): KS x M1 rows x 144 points + wL2 — 149.5 KiB at N = 4096, KS = 4 (one workgroup per CU), 75.7 KiB at N = 2048 (two),
// 38.9 KiB at N = 1024 (four).  Variants that kept two workgroups per CU — two limbs in LDS at a time, the other accumulators in registers, or one
// product pass per limb pair — either spilled (128 accumulator registers at 256 threads) or re-read S from HBM (0.26 - 0.36 ms per 1024
// ciphertexts against 0.35 ms for the whole three-kernel pipeline).  Also tried: a persistent workgroup in two roles of 512 threads (role A:
// the next item's product in registers, role B: this item's transforms in the tile, hand-over between barriers) — at the 128-VGPR cap of a
// 1024-thread workgroup role A's 64 accumulator registers leave no room for prefetch slots (spills, 0.93 ms at 4 limbs; 0.25 vs 0.17 ms
// at 3).  And (end of round 2): a persistent 512-thread workgroup (four product positions per thread, 256 registers) with the next item's
// product spread in eight row steps between the stages of the current item's transform - bit-exact, slower: 2.17 vs 3.05 M/s at 4 limbs,
// 3.8 vs 4.07 at 3, key switch 3.5 vs 5.2 (the transform stages are latency-bound and take about twice as long with 8 waves instead of
// 16, which costs more than the hidden loads; 116 - 276 bytes of scratch at 3 - 4 limbs).  And (round 3): the same kernel as TWO 512-thread
// workgroups per CU, each with two limbs in the tile at a time (75 KiB), four product positions per thread, the limb groups through the tile from the
// last limb up with the carries and the waiting accumulators in registers - bit-exact, two workgroups resident, and 20 - 40 % slower (3 limbs 1.55 ->
// 1.88 ms per 10 launches, key switch 1.25 -> 1.64, 4 limbs 2.31 -> 3.27; profiles/r03_small_inv_stamps.txt): 8 waves keep half as many key / spectrum
// requests in flight per workgroup at the 128-register cap, and each transform stage runs on 4 waves.  KS = key limbs (g.ksz).  NOPROD: the spectra of the (ciphertext, column) are given, in the standard device order [q1 + M1 q2]:
// S[b][l * cols_out + col] (npi = ksz * cols_out), no key (the blind rotation's block step produced them).  FWD (blind rotation: the
// result is the accumulator the next block transforms): the digits go back into the tile as doubles and the forward transform of
// k_small_fwd runs on them before the workgroup ends - the next block's k_small_fwd launch and its read of the accumulator are saved.
// AU (glwe_automorphism family, automorphism/glwe_ct.rs:51-275): a thread owns OUTPUT positions, takes the big value's coefficient
// i = position * p^-1 mod 2n from the tile (LDS gather), negates it where phi = X -> X^p wraps, adds / subtracts the operand at its
// position, runs the carry chain and stores the digits - coalesced (rounds 1 - 2 owned the SOURCE coefficient and scattered 8-byte
// stores; round 3: glwe_trace at N = 4096 +24 %).  The key-switch body is added at the source positions by the column pass (coalesced
// loads).  In place (res == a): those loads happen before the barrier in front of the carry phase, i.e. before any thread stores; the
// operand at a thread's own positions is loaded before its first store.
// DUAL (Cswap::cswap, eval.rs:417-461): ONE product and ONE inverse transform, two carry chains - the coefficient's big value x enters the first
// as x + small (stored to res) and the second as small2 - x (stored to res2).  In place on both (res == small, res2 == small2): a thread loads
// both operands at exactly the positions it later stores, before the barrier in front of the carry phase; no other thread touches them.
// The kernel's text is device_small_inv_body.hpp, compiled twice: k_small_inv, and k_small_inv_gather (the BDD evaluator's level launches: per-ciphertext
// operand, result and key from a device table).
#define PZ_SMALL_INV_GATHER 0
#include "device_small_inv_body.hpp"
#undef PZ_SMALL_INV_GATHER
#define PZ_SMALL_INV_GATHER 1
#include "device_small_inv_body.hpp"
#undef PZ_SMALL_INV_GATHER


}  // namespace pz
