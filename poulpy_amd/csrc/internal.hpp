// internal.hpp — interfaces between the translation units of libpoulpy_hip.so.
//
//   launch_fft.hip   the four passes of the two-pass negacyclic FFT (device_fft.hpp)
//   launch_tail.hip  fused inverse column pass + carry chain (k_inv_tail)
//   launch_mid.hip   fused row pass + VMP + inverse row pass (device_mid.hpp), key re-slicing
//   mid_forms.hpp    which k_mid128 / k_mid128r instantiation a shape gets, and the list of them (plain C++, no HIP; launch_mid.hip walks it)
//   launch_small.hip small-ring pipelines for N = 1024 / 2048 / 4096: whole polynomials in LDS (device_small.hpp, device_small_one.hpp)
//   launch_bdd.hip   the BDD evaluator's gather table and the gathered forms of the small-ring CMUX kernels
//   bdd_schedule.cpp the BDD circuit compiler (plain C++, no HIP)
//   pack_levels.cpp  the level map of FheUint::pack (plain C++, no HIP)
//   word_ops.cpp     the stage plan of the FheUint byte operations (plain C++, no HIP)
//   launch_ops.hip   elementwise / permutation / normalize / VMP kernels (device_ops.hpp)
//   launch_br.hip    blind-rotation kernels (device_br.hpp + the block step of device_br_ops.hpp)
//   tail_plan.hpp    which launches of k_inv_tail a call becomes: columns, role, form, refusals (plain C++, no HIP; launch_tail.hip runs the plan)
//   tail_forms.hpp / br_forms.hpp   the launch of one form of the fused tail; the forms of the blind rotation (one-kernel forms; block-step forms in plain C++)
//   launch_cnv.hip   bivariate convolution kernels (device_cnv.hpp)
//   launch_plain.hip GLWE x constant / plaintext kernels (device_plain.hpp), weighted sums by constants (device_lincomb.hpp)
//   api.hip          C ABI: module, memory, key pinning / mirrors
//   api_glwe.hip     C ABI: the batched GLWE product (glwe_op), its host-container entry path, the hoisted rotations
//   api_ggsw.hip     C ABI: GGSW and automorphism-key composites (loops of glwe_op over matrix entries)
//   api_gates.hip    C ABI: CMUX, blind rotation by encrypted bits, conditional swap, blind retrieval
//   api_bdd.hip      C ABI: BDD circuit object and executor
//   api_trace.hip    C ABI: glwe_trace, glwe_pack
//   api_fhe_uint.hip C ABI: FheUint pack / execute and the byte operations
//   api_hal.hip      C ABI: the per-op HalImpl methods (VecZnxDft, SVP, VMP, VecZnxBig, i64 VecZnx family)
//   api_br.hip       C ABI: blind rotation, circuit bootstrapping (composites on glwe_op; HIP-graph replay)
//   api_cnv.hip      C ABI: convolution family, GLWE tensoring, batched i64 family
//   api_lincomb.hip  C ABI: weighted sums of GLWE batches by constants
//   api_sum.hip      C ABI and launcher: normalized signed sums of GLWE batches, one pass (device_sum.hpp)
//   api_lwe.hip      C ABI: LWE glue of the gate bootstrap (+ its index kernels)
//   api_dist.hip     C ABI: RCCL key broadcast (dlopen)
//   api_common.hpp / api_glwe.hpp / glwe_call.hpp   what those share (staging and argument checks; graph cache; GlweCall, glwe_op / glwe_trace / ...)
//
// Every kernel is instantiated in exactly one translation unit (the one that launches it), so the units compile
// independently and in parallel; only plain functions cross unit boundaries.
#pragma once
#include "module.hpp"

namespace pz {

// ---- shared small helpers -----------------------------------------------------------------------------------------
template <typename K>
inline int set_lds(K kernel, size_t bytes) {
    if (bytes > 48 * 1024)
        PZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PZ_OK;
}
// one launch of `kernel` with `lds` bytes of dynamic shared memory: a dispatch arm names its instantiation once
template <typename K, typename... A>
inline int launch_k(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    PZ_TRY(set_lds(kernel, lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return PZ_OK;
}
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// what a buffer of normalized digits holds per coefficient (the blind rotation keeps its accumulator narrow between two blocks); each kernel's own bit
// mask is made from these in one place: tail_args (launch_tail.hip) and launch_small_inv
enum class Digits { I64, I32, I16 };

struct DV {          // a batched VecZnx-like container on the device
    void* p;
    long long bs;    // scalars between consecutive batch objects
    int cols, size;
};
inline long long limb_stride(const pz_module* M, const DV& v) { return (long long)v.cols * (long long)M->n; }
inline void* poly_ptr(const pz_module* M, const DV& v, int col, int limb) {
    return (char*)v.p + 8 * ((long long)M->n * ((long long)limb * v.cols + col));
}

// ---- launch_fft.hip -----------------------------------------------------------------------------------------------
// src_digits = I32 (row-major, 128-point-row plans): `src` holds 32-bit digits at the same element offsets
int launch_fwd_pass1(pz_module* M, int npolys, const long long* src, PolyMap smap, cplx* T, bool rowmajor = false, long long mask = -1,
                     Digits src_digits = Digits::I64);
// the row-major form on 16-bit digits in the fused tail's tile order (TailD16; smap addresses limbs of n int16)
int launch_fwd_pass1_t16(pz_module* M, int npolys, const short* src, PolyMap smap, cplx* T);
// the row-major form on i64 coefficients that also leaves them as 16-bit values in the tile order, polynomial p at w16 + p n, and raises the module's
// wide flag (module.hpp: wide16) for a value beyond 16 bits
int launch_fwd_pass1_w16(pz_module* M, int npolys, const long long* src, PolyMap smap, cplx* T, short* w16);
bool tail_d16_only_supported(const pz_module* M);   // the tensoring tails that leave 16-bit digits only + the operand form that reads them
int launch_fwd_pass2(pz_module* M, int npolys, const cplx* T, double* dst, PolyMap dmap, const cplx* mul);
int launch_inv_pass2(pz_module* M, int npolys, const double* src, PolyMap smap, cplx* T);
int launch_inv_pass1(pz_module* M, int npolys, const cplx* T, long long* dst, PolyMap dmap);

// ---- launch_tail.hip ----------------------------------------------------------------------------------------------
bool tail_supported(const pz_module* M);
// One launch of the fused tail (k_inv_tail, device_fft.hpp): the big value held in T - nlimbs x ncols polynomials per ciphertext, still
// one inverse column pass away from coefficients - leaves as normalized base2k digits in `res`.  Every field has a name at the call
// site (round 3 passed these as 28 positional arguments, 8 of them bool); the defaults are the plain external-product tail.
struct TailCall {
    // ---- the value and where its digits go ----
    int batch = 0;
    const cplx* T = nullptr;          // T[j2][q1] (output of inverse pass 2) or, rowmajor, T2'[q1][j2] (output of the middle kernel)
    bool rowmajor = false;
    int nlimbs = 0, ncols = 0;        // limbs / columns of the VecZnxBig being consumed
    long long* res = nullptr;
    long long res_bs = 0;             // i64 elements between consecutive ciphertexts of res
    int res_cols = 0, res_size = 0;
    int base2k = 0;
    // ---- operand added in front of the carry chain (vec_znx_big_add_small_assign, keyswitching/glwe.rs:237) ----
    const long long* small = nullptr; // null: none (external product)
    long long small_bs = 0;
    int small_cols = 1, small_size = 0;
    bool small_all = false;           // false: column 0 of `small` lands on body_col only; true: column c of `small` on column c
    bool small_neg = false;           // the operand is subtracted (sub forms of the automorphism family)
    int body_col = 0;                 // 0 for a key switch, `col` for ggsw_expand_row
    // ---- body-column operand prepared elsewhere (spectral automorphism forms: phi(body) +- a0 in the workspace) ----
    const long long* body_src = nullptr;
    long long body_bs = 0, body_ls = 0;   // batch / limb strides of body_src
    bool body_only = false;               // only the body column has an operand (plain glwe_automorphism)
    // the pre-pass left the body-column operand as 16-bit values in the tail's tile order, body16[ciphertext][limb][n] with body16_limbs limbs per
    // ciphertext, and raised *body16_wide if a value did not fit; launch_inv_tail then runs that column twice - the 16-bit-operand form (returns at
    // once if the flag is up) and the operand variant on body_src, which a conditional second pre-pass filled (returns at once if the flag is down)
    const short* body16 = nullptr;
    int body16_limbs = 0;
    const unsigned* body16_wide = nullptr;
    // add / sub forms at rank 1: the other column's operand +-a[1] as 16-bit values too (pass 1 of the key switch left them: launch_fwd_pass1_w16),
    // other16[ciphertext][limb][n] with small_size limbs per ciphertext; same flag, same pair of launches on that column
    const short* other16 = nullptr;
    // ---- signs of X -> X^p (automorphism/glwe_ct.rs:96-275; TailArgs in device_fft.hpp) ----
    unsigned auto_mul = 0;            // != 0: the value enters the chain as s(n) (big + small), s(n) = -1 iff (n auto_mul) mod 2N >= N
    bool auto_neg = false;            // flips every s(n)
    bool post_neg = false;            // put s(n) back on the digits (plain form: phi acts on the normalized value)
    bool big_neg = false;             // the value enters the chain as small - big on every column (vec_znx_big_sub_small_a: limbs of big beyond the operand
                                      // enter negated) - the second result of a conditional swap.  Needs small_all; on its own, not with auto_mul /
                                      // post_neg / the gathered or prepared operands (launch_tail.hip expresses it through the kernel's sign and operand forms)
    bool keyauto = false;             // key switch by a permuted key (wave_keyauto_tail): every column's chain between the signs of auto_mul, body operand as it is
    unsigned gather_mul = 0;          // != 0: the operand is -+phi^-1(small), gathered inside the tail (older, non-spectral scheme)
    bool gather_neg = false;
    // ---- blind rotation's accumulator between two blocks: 32-bit digits at the same element strides, or 16-bit digits in the tail's tile order ----
    Digits small_digits = Digits::I64, res_digits = Digits::I64;
    // non-null (with small_all): the operand is a GLWETensor held as 16-bit digits in the tail's tile order, small16[column][ciphertext][limb][n],
    // small16_cs int16 elements between columns (`small` only has to be non-null then)
    const short* small16 = nullptr;
    long long small16_cs = 0;
    // ---- glwe_trace: the digits leave through a one-bit vec_znx_rsh_assign ----
    bool post_rsh = false;
};
int launch_inv_tail(pz_module* M, const TailCall& c);
bool tail_rsh_supported(const pz_module* M);
bool tail_narrow_supported(const pz_module* M);   // 32- / 16-bit accumulator digits (TailCall::small_digits / res_digits; launch_fwd_pass1's I32 source covers the same plans)
// One launch of a convolution middle kernel (k_mid_cnv, k_mid_cnv3: launch_cnv.hip; k_mid_cnv_pt: launch_plain.hip); a wave fills it once.
struct MidCnvCall {
    // ---- T' of the operand limbs as pass 1 left them: all limbs but the last, and the last one (masked) ----
    const cplx *a_main = nullptr, *a_last = nullptr, *b_main = nullptr, *b_last = nullptr;
    cplx* T2 = nullptr;
    // ---- columns per operand, limbs of a / b, and the product limbs [offset, offset + min_size) that are kept ----
    int cols = 0, a_size = 0, b_size = 0, min_size = 0, offset = 0;
    // ---- k_mid_cnv: the term, columns (col_i, col_j) of both operands; col_j = -1: the diagonal term ----
    int col_i = 0, col_j = -1;
    // ---- k_mid_cnv_pt: one plaintext for every ciphertext ----
    bool b_shared = false;
};
bool mid_cnv_supported(const pz_module* M, int a_size, int b_size, int min_size);
int launch_mid_cnv(pz_module* M, int batch, const MidCnvCall& c);
// k_mid_cnv3: the three terms of a rank-1 tensoring in one launch; T2 = [term][pair][limb < min_size][m] (launch_cnv.hip)
bool mid_cnv3_supported(const pz_module* M, int cols, int a_size, int b_size, int min_size);
int launch_mid_cnv3(pz_module* M, int batch, const MidCnvCall& c);
struct NzCombine;
// 16-bit side copies of the diagonal terms' digits (round 6; base2k <= 16): [pair][res limb][n] int16 in the tail's own tile order.  A diagonal
// launch (NZ1) mirrors every digit it stores into `w`; the pairwise launch (mode 5) reads `ra` / `rb` instead of the low dwords of the two
// i64 tensor columns (8 B fetched per coefficient and column for a 12-bit digit: 4.3 of the pairwise launch's 8.8 GB, profiles/r04_tensor_traffic.json)
// only: the digits leave ONLY as those copies, the i64 column is not written (the fused multiply + relinearize, api_cnv.hip: the pairwise launch
// then writes its own values pair - d_i - d_j into `w` too, base2k <= 14)
struct TailD16 { short* w = nullptr; const short* ra = nullptr; const short* rb = nullptr; bool only = false; };
// The inverse column pass on the row-major T with vec_znx_normalize's same-base steps in its stores (launch_tail.hip)
struct NzTailCall {
    const cplx* T = nullptr;
    int nlimbs = 0;                   // limbs of T that are transformed; the other a_size - nlimbs are zero
    // ---- where the digits go: column res_col of `res`, shifted by res_offset bits ----
    long long* res = nullptr;
    long long res_bs = 0;
    int res_cols = 0, res_size = 0, res_col = 0;
    int base2k = 0;
    long long res_offset = 0;
    int a_size = 0;
    const NzCombine* cb = nullptr;    // how they reach res_col and up to two more columns; null: plain stores
    const TailD16* d16 = nullptr;     // 16-bit side copies
};
int launch_inv_tail_nz(pz_module* M, int batch, const NzTailCall& c);

// ---- launch_mid.hip -----------------------------------------------------------------------------------------------
// scratch rows behind T2: one 64-row x 128-point tile per persistent workgroup of k_mid128 (<= 256 of them: 32 MiB), which also covers
// the 512 x 256 points k_mid<CT> shares
constexpr size_t kMidDummyBytes = (size_t)256 * 64 * 128 * sizeof(cplx) + (1 << 20);
bool mid_supported(const pz_module* M, int npi, int npo);
int launch_permute_pmat(pz_module* M, const double* P, cplx* Pp, int npolys);
// the row-sliced copy of phi_g(key), g odd: spectrum index q' of the copy reads index (mul q' + add) mod m of the key, conjugated if conj
// (m2 = 128 plans; key_perm in api_ggsw.hip derives the map from g)
struct KeyPerm { unsigned mul = 1, add = 0; bool conj = false; };
int launch_permute_pmat_gal(pz_module* M, const double* P, cplx* Pp, int npolys, const KeyPerm& kp);
// mul != 0: spectrum permutation of X -> X^p folded into the middle kernel (m2 = 128 plans only; see MidArgs and spectral_perm in api_glwe.hip);
// conj: the spectrum of phi(a) is the conjugate of the permuted one (p = 3 mod 4)
struct SpectralPerm { bool on = false; unsigned mul = 0, add = 0; bool conj = false; };
// digit-selected product (dsize > 1, m2 = 128 plans): term t = input polynomial in[t] x key row row[t], columns shifted by coff[t],
// reaching the first cb[t] output polynomials
struct MidDigits {
    int n = 0;
    unsigned char in[32], row[32], coff[32], cb[32];
};
// CGGI block step (m2 = 128 plans): Pp = the row-sliced copy of the blk GGSWs of one LWE block (blk * nrows key rows per frequency
// row), nrows = npi; the products are weighted by the monomial factors DFT(X^a_i - 1) of each ciphertext (MidArgs, BR)
struct MidBr {
    const long long* lwe;   // [batch][lwe_bs] mod-switched LWEs
    long long lwe_bs;
    int i0, blk;            // first coefficient of the block, block size (<= 16)
};
struct MidCall {
    // ---- T' in, T2' out, the row-sliced key; scratch rows (kMidDummyBytes) ----
    const cplx* T = nullptr;
    cplx* T2 = nullptr;
    const cplx* Pp = nullptr;
    cplx* dummy = nullptr;
    int npi = 0, npo = 0;             // polynomials per ciphertext in / out
    int nrows = 0, ncols = 0;         // the key matrix
    // ---- the product form: plain, or one of ----
    SpectralPerm perm;
    const MidDigits* digits = nullptr;
    const MidBr* br = nullptr;
};
int launch_mid(pz_module* M, int batch, const MidCall& c);

// ---- launch_small.hip ---------------------------------------------------------------------------------------------
// two-kernel pipeline for N = 1024 / 2048 / 4096 (device_small.hpp): full forward transform -> S[poly][q1][q2]; product with the row-sliced key +
// full inverse transform + carry chain per (ciphertext, output column).  dsize 1, one base2k, <= 4 key limbs.
bool small_supported(const pz_module* M, int npi, int key_limbs);
// standard device VmpPMat -> P'[q1][p][q2] with m = M1 x 128 (ring degrees whose plan is not M1 x 128: no launch_permute_pmat there)
int launch_small_permute(pz_module* M, const double* P, cplx* Pp, int npolys);
int launch_small_fwd(pz_module* M, int npolys, const long long* src, PolyMap smap, cplx* S, bool natural_order = false,
                     const PolyMap* dmap = nullptr, const cplx* mul = nullptr);
// the CMUX forms of the forward stage: polynomial p = diff.t - diff.f (diff.t null: X^rot f - f), in the launch order of diff.fmap
int launch_small_fwd_diff(pz_module* M, int npolys, const SmallDiff& diff, cplx* S);
bool small_transform_supported(const pz_module* M);   // N = 1024 / 2048 / 4096: per-op transforms in one kernel (launch_small.hip)
int launch_small_idft(pz_module* M, int npolys, const double* a, PolyMap smap, long long* res, PolyMap dmap);
// the groups both small-ring product launchers share; glwe_small_ring fills them once per wave
struct SmallKey {                     // the re-sliced key and the product's shape
    const cplx* Pp = nullptr;
    int npi = 0, nrows = 0, ncols = 0, cols_out = 0, ksz = 0;
};
struct SmallRes {                     // where the normalized digits go
    long long* p = nullptr;
    long long bs = 0;                 // i64 elements between consecutive ciphertexts
    int cols = 0, size = 0, base2k = 0;
};
struct SmallOperand {                 // added in front of the carry chain; p = null: none (external product)
    const long long* p = nullptr;
    long long bs = 0;
    int cols = 0, size = 0;
    int body_col = 0;                 // < 0: column c of the operand lands on column c
};
struct SmallInvCall {
    const cplx* S = nullptr;          // the spectra k_small_fwd left (product-free form: the big value's own spectrum)
    SmallKey key;
    SmallRes res;
    SmallOperand small;
    // ---- product-free form (blind rotation: the block step made the product), optionally with the forward transform of the first fwd_limbs
    //      limbs of the new accumulator chained behind the carry chain, into fwd_S ----
    bool noprod = false;
    cplx* fwd_S = nullptr;
    int fwd_limbs = 0;
    // ---- automorphism family: X -> X^au_p, au_mode as AutoSpec::mode ----
    bool au = false;
    unsigned au_p = 0;
    int au_mode = 0;
    // ---- glwe_trace: the digits leave through a one-bit shift ----
    bool post_rsh = false;
    // ---- blind rotation's accumulator between two blocks (product-free form) ----
    Digits small_digits = Digits::I64, res_digits = Digits::I64;
    // ---- conditional swap (pz_glwe_cswap_batched): res2.p != null - a second result from the same big value, res2 = normalize(small2 - big) on
    //      every column beside res = normalize(big + small); plain product form only, both containers with the columns of res ----
    SmallRes res2;
    SmallOperand small2;
};
int launch_small_inv(pz_module* M, int batch, const SmallInvCall& c);
// ONE kernel per call for N = 1024 / 2048 (device_small_one.hpp): forward transforms, product, inverse transforms and carry chains of a ciphertext in
// one workgroup; rank 1 (2 output columns), <= 8 input polynomials, <= 4 key limbs, key columns = ksz * 2
bool small_one_supported(const pz_module* M, int npi, int nrows, int ncols, int cols_out, int ksz, int batch);
struct SmallOneCall {
    const long long* src = nullptr;   // the input limbs, addressed by smap
    PolyMap smap{1, 1, 0, 0, 0, 0};
    SmallKey key;
    SmallRes res;
    SmallOperand small;
    const SmallDiff* diff = nullptr;  // CMUX: the input polynomials are differences of two sources (src / smap are not read)
    SmallRes res2;                    // conditional swap: res2.p != null - res2 = normalize(small2 - big) beside res (SmallInvCall)
    SmallOperand small2;
    // rotated-source key switch: ciphertext b = X^rot of ciphertext `word` of src / small, (word, rot) = rot_tab[b] (device); no diff, no res2
    const RotSrc* rot_tab = nullptr;
};
int launch_small_one(pz_module* M, int batch, const SmallOneCall& c);

int ensure_small_tables(pz_module* M);   // the m = M1 x 128 tables of the small-ring kernels, built on first use

// ---- launch_bdd.hip -----------------------------------------------------------------------------------------------
// The BDD evaluator's kernels (pz_bdd_circuit_execute_batched): the per-call gather table, and the gathered forms of the small-ring
// CMUX kernels - one launch per level, ciphertext c of the launch addressed through tab[c] (SmallGather, device_fft.hpp).
struct BddGate;
struct BddTableCall {
    const BddGate* gates = nullptr;          // device: the circuit's compact level tables (immutable)
    const uint32_t* level_start = nullptr;   // device: levels + 1 offsets
    int levels = 0;
    uint32_t total = 0;                      // gates of all levels
    int batch = 0, nbits = 0;
    long long* state = nullptr;              // slot-major [slots][batch]
    long long* out = nullptr;                // slot-major [n_out][batch]
    long long ct = 0;                        // i64 elements of one ciphertext
    const cplx* const* keys = nullptr;       // device: [batch][nbits] row-sliced keys (entries the circuit never selects are not read)
    SmallGather* tab = nullptr;              // out: level l at tab + level_start[l] * batch, input-major, the level's gates (sorted by selector) inside
};
int launch_bdd_table(pz_module* M, const BddTableCall& c);
// the constant one of the initial state in a zeroed slot: digits d0 / d1 at limbs 0 / 1 of coefficient 0, column 0 (limb_stride elements apart)
int launch_bdd_one(pz_module* M, long long* slot, long long ct, int batch, long long limb_stride, long long d0, long long d1, int used);
struct SmallGatherShape { int cols = 0, size = 0, ksz = 0, dnum = 0, base2k = 0; };   // t, f and res: `size` limbs of `cols` columns
bool small_one_gather_supported(const pz_module* M, const SmallGatherShape& s);
int launch_small_one_gather(pz_module* M, int batch, const SmallGatherShape& s, const SmallGather* tab);
int launch_small_fwd_gather(pz_module* M, int batch, const SmallGatherShape& s, const SmallGather* tab, cplx* S);
int launch_small_inv_gather(pz_module* M, int batch, const SmallGatherShape& s, const SmallGather* tab, const cplx* S);

// ---- launch_ops.hip -----------------------------------------------------------------------------------------------
int launch_ew(pz_module* M, int op, void* res, long long res_bs, long long res_ls, const void* a, long long a_bs,
              long long a_ls, const void* b, long long b_bs, long long b_ls, int nlimbs, int batch);
// acc += terms[0] + ... + terms[nterms - 1] on GLWETensors held as 16-bit digits, all of one layout: `cols` columns col_stride int16 apart,
// the first col_elems of each in use (both multiples of 8, the pointers 16-byte aligned); 1 <= nterms <= 4 (k_t16_sum)
int launch_t16_sum(pz_module* M, short* acc, const short* const* terms, int nterms, int cols, long long col_elems, long long col_stride);
// zero-fill as a kernel node (not hipMemsetAsync: see launch_ops.hip) - for everything that can run under graph capture
int launch_zero_bytes(pz_module* M, void* ptr, size_t bytes);
// dst = +-src(X^p-gather with multiplier mul) [+ add]; see k_automorphism
// `flags`: the first three reach the kernel as AutoArgs::flags (device_ops.hpp), the other two choose the launch
enum AutoFlags : int {
    AUTO_PLAIN = 0,        // the gather alone, no signs
    AUTO_SIGN = 1,         // apply the sign X -> X^p gives each coefficient
    AUTO_NEGATE = 2,       // negate every output
    AUTO_ADD_FIRST = 4,    // `add` only for polynomials whose innermost PolyMap index is 0
    AUTO_SUB16 = 16,       // 16-bit output (dst16) only: `add` is subtracted
    AUTO_IF_WIDE = 32,     // the i64 fallback of the 16-bit body pre-pass: runs only if the module's wide flag is up
};
int launch_automorphism(pz_module* M, int npolys, const long long* src, PolyMap sm, long long* dst, PolyMap dm, unsigned mul,
                        int flags, const long long* add = nullptr, PolyMap am = PolyMap{1, 1, 0, 0, 0, 0}, short* dst16 = nullptr);
// the 16-bit tile-order pre-pass for `nrot` Galois elements from one read of the source (k_automorphism_t16_many): copy r, made with the
// gather multiplier muls[r] and phi's signs, lands at dst16 + r * stride + map_off(dm); raises the module's wide flag like launch_automorphism
int launch_automorphism_t16_many(pz_module* M, int npolys, const long long* src, PolyMap sm, short* dst16, PolyMap dm, long long stride,
                                 const unsigned* muls, int nrot);
// per-ciphertext shift: polynomial i turns by shift[(i / polys_per_batch) * shift_bs + shift_idx] (mode: see k_rotate)
int launch_rotate(pz_module* M, int npolys, const long long* src, PolyMap sm, long long* dst, PolyMap dm, int mode,
                  int polys_per_batch, const long long* shift, long long shift_bs, long long shift_idx, long long shift_const);
// dst = X^k src on every polynomial
inline int launch_rotate(pz_module* M, int npolys, const long long* src, PolyMap sm, long long* dst, PolyMap dm, long long k) {
    return launch_rotate(M, npolys, src, sm, dst, dm, 0, npolys, nullptr, 0, 0, k);
}
int launch_rsh(pz_module* M, int batch, long long* data, long long bs, int cols, int size, int col0, int ncols, int base2k, int k);
// One level of FheUint::pack (pz_fhe_uint_pack_batched) on the dense buffer bits[slot][batch]: pair k merges slot lo[k] (a, the
// survivor) and slot hi[k] (b).  pre: hi[k] <- rsh1(X^-t a + b), diff[k][batch] <- normalize(rsh1(X^-t a - b)); post: slot lo[k] of `dst` <-
// X^t normalize(hi[k] - diff[k]).  diff overlaps neither bits nor dst; dst = bits or a buffer apart from both.
struct PackLevelCall {
    long long* bits = nullptr;
    long long* diff = nullptr;
    long long* dst = nullptr;
    int cols = 0, size = 0, base2k = 0, batch = 0, pairs = 0;
    unsigned t = 0;
    const unsigned char *lo = nullptr, *hi = nullptr;
};
int launch_pack_level(pz_module* M, bool post, const PackLevelCall& c);
// The element-wise kernels of the FheUint byte operations (pz_fhe_uint_get_batched / _zero_byte_ / _splice_ / _sext_): `batch`
// ciphertexts of cols columns and size limbs behind every pointer.
//   launch_word_pre        out[it][batch] <- X^-exp[it] src[sel[it]], it < items <= 128; shift: followed by the one-bit vec_znx_rsh_assign in base2k.
//                          out overlaps no source
//   launch_word_post       res <- base + X^r (tp - tm), wrapping; tp / tm may be null; res == base allowed, res overlaps neither tp nor tm
//   launch_word_replicate  out <- sum_{m < 8} X^(m n / 8) s; out overlaps s nowhere
struct WordPreCall {
    const long long* src[4] = {nullptr, nullptr, nullptr, nullptr};
    long long* out = nullptr;
    int cols = 0, size = 0, base2k = 0, batch = 0, items = 0;
    bool shift = false;
    const unsigned* exp = nullptr;
    const unsigned char* sel = nullptr;
};
int launch_word_pre(pz_module* M, const WordPreCall& c);
int launch_word_post(pz_module* M, long long* res, const long long* base, const long long* tp, const long long* tm, unsigned r, int cols, int size,
                     int batch);
int launch_word_replicate(pz_module* M, long long* out, const long long* s, int cols, int size, int batch);
// vmp_apply_dft_to_dft  [vmp.rs:144-264, zero-tail semantics for limb_offset > 0]
int dev_vmp(pz_module* M, int batch, DV res, DV a, const double* pmat, int rows, int cols_in, int cols_out, int size, int limb_offset);
// vec_znx_(big_)normalize on one column  [normalize.rs:18-401]
// cb (same base2k only): how the digits reach res_col (mode) and up to two more columns of `res` that take them too - 1 = v, 2 = -v,
// 3 += v, 4 -= v (wrapping), 0 none; nullptr: plain stores
struct NzCombine { int mode; int col2[2]; int mode2[2]; };
int dev_normalize(pz_module* M, int batch, DV res, int res_base2k, long long res_offset, int res_col, DV a, int a_base2k, int a_col,
                  const NzCombine* cb = nullptr);

// ---- launch_br.hip ------------------------------------------------------------------------------------------------
// whole rotation in one kernel (device_br.hpp) when the shape fits: *launched says whether it did
int br_try_fused(pz_module* M, int64_t* res, const int64_t* lwe_2n, const int64_t* lut, const double* brk,
                 const pz_blind_rotation_params* p, size_t batch, bool* launched);
// zero + block_size x (vmp, svp, add, sub) of one LWE block in one kernel; *launched = false: shape not covered
int br_block_step(pz_module* M, const double* acc_dft, long long a_bs, double* acc_add, long long o_bs, const double* brk,
                  size_t pmat_doubles, int row_max, int ncols, int B, int i0, int blk, const int64_t* lwe_2n, long long lwe_bs,
                  bool* launched);
int launch_xai_acc(pz_module* M, double* acc_add, long long acc_bs, const double* v, long long v_bs, int polys, int B,
                   const int64_t* lwe_2n, long long lwe_bs, int idx);
int launch_xai_ext(pz_module* M, double* acc_add, const double* v, int polys, int log_ext, int B, const int64_t* lwe_2n, long long lwe_bs,
                   int idx);
int launch_br_ext_init(pz_module* M, int64_t* acc, const int64_t* lut, const int64_t* lwe_2n, long long lwe_bs, int log_ext, int cols,
                       int rsz, int lut_size, int B);

// ---- launch_cnv.hip -----------------------------------------------------------------------------------------------
// bivariate convolution in the DFT domain (reference/fft64/convolution.rs:210-345): res limb kk of column res_col =
//   sum_j A[kk + offset - j] * B[j],  A = a[col_i] (+ a[col_j] when pairwise), B = b[b_i] (+ b[b_j]); limbs >= min_size untouched here.
// a / b: device CnvPVec layout [col][limb][m points], batch strides in doubles; res: VecZnxDft layout.
int launch_cnv_apply(pz_module* M, int batch, double* res, long long res_bs, int res_cols, int res_col, int min_size, int offset,
                     const double* a, long long a_bs, int a_size, int a_i, int a_j, const double* b, long long b_bs, int b_size, int b_i,
                     int b_j);
// convolution.rs:147-203: i64, wrapping; bconst: b_size device constants
int launch_cnv_by_const(pz_module* M, long long* res, int res_cols, int res_col, int min_size, int offset, const long long* a, int a_cols,
                        int a_size, int a_col, const long long* bconst, int b_size);

// ---- launch_plain.hip ---------------------------------------------------------------------------------------------
// GLWE x constant (k_mul_const_nz, device_plain.hpp): one arm = the host constant b (b_size digits), res_big's limb count and cnv_offset_hi
struct MulConstArmSpec { const int64_t* b; int b_size, big_size, hi; };
// GLWE x plaintext middle kernel (k_mid_cnv_pt<AS, BS>, device_plain.hpp): a = the operand columns' T' as k_mid_cnv reads them, b = the
// plaintext's T' [pt][limb < b_size - 1][m] / [pt][m] with b_bs points between plaintexts (0: shared); T2 = [col][ct][kk < min_size][m]
bool mid_cnv_pt_supported(const pz_module* M, int cols, int a_size, int b_size, int min_size);
int launch_mid_cnv_pt(pz_module* M, int batch, const MidCnvCall& c);
// k_cnv_by_const on every column of `batch` ciphertexts: res_big [ct][limb < res_size][col][n] (limbs >= min_size untouched)
int launch_cnv_by_const_batched(pz_module* M, int batch, long long* res, long long res_bs, int res_size, int min_size, int offset, const long long* a,
                                long long a_bs, int cols, int a_size, const long long* bconst, int b_size);
// same base2k, b_size <= 32, a_size <= 64
bool mul_const_nz_supported(const pz_module* M, int a_size, int b_size);
// form 0: arm0; 1: X^{N/2} arm0; 2: arm0 + X^{N/2} arm1 - every column of `batch` ciphertexts (a: a_size limbs, res: res_size limbs, cols columns)
int launch_mul_const_nz(pz_module* M, int batch, long long* res, long long res_bs, const long long* a, long long a_bs, int cols, int a_size,
                        int res_size, int base2k, long long res_offset, int form, const MulConstArmSpec* arms);
// k_lincomb_const (device_lincomb.hpp): res = [res] +- sum_t (constant_t x a_t), every column of `batch` ciphertexts in one pass.  One term:
// the operand (a_bs 0: shared by the batch), the constant re + i im (host digits, either or both null) with the product's cnv_offset, and
// how the product joins the accumulator (0: acc +- tmp; 1: acc +- lsh(tmp, k); 2: lsh(acc, k) +- tmp)
struct LinTermSpec {
    const long long* a;
    long long a_bs;
    int a_size;
    size_t cnv_offset;
    const int64_t *re, *im;
    int b_size;
    int join, neg;
    size_t k;
};
constexpr int kLincombMaxTerms = 64;
constexpr size_t kLincombMaxLds = (size_t)160 * 1024;
// dynamic LDS of a launch: (a_max + res_size, + res_size again where a join shifts) x (2 if paired) x 128 threads x 8 B
size_t lincomb_lds_bytes(int a_max, int res_size, bool pair, bool has_tmp);
// plans the terms into the module's page-locked staging and copies them to its device table, on the stream, outside any graph
int lincomb_stage(pz_module* M, const LinTermSpec* terms, int nterms, int res_size, int base2k);
int launch_lincomb(pz_module* M, int batch, long long* res, long long res_bs, int cols, int res_size, int base2k, int nterms, int init_res,
                   int normalize, bool pair, int a_max, bool has_tmp);

}  // namespace pz
