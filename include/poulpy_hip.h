/*
 * poulpy_hip.h — C ABI of libpoulpy_hip.so, the MI355X (gfx950) FFT64 backend
 * for poulpy-hal.
 *
 * Every entry point below is what a `poulpy-hip-mi355x` Rust crate binds with
 * `extern "C"` to implement `unsafe trait HalImpl<FFT64Hip>`
 * (poulpy-hal/src/oep/hal_impl.rs:25) for the FFT64 hot path; the reference
 * method each function replaces is cited as hal_impl.rs:<line> (all paths
 * relative to /root/reference).  INTEGRATION.md shows the Rust side.
 *
 * Conventions
 *  - Plain pointers + sizes only.  A VecZnx / VecZnxDft / VecZnxBig is passed as
 *    (ptr, cols, size): limb j of column i starts at scalar offset
 *    n*(j*cols + i) (poulpy-hal/src/layouts/znx_base.rs:52-82); n comes from the
 *    module.  `size` is the *current* size (VecZnx::size(), after set_size).
 *  - Pointers may be host memory (pageable, or pinned from pz_alloc_bytes) or
 *    device memory (pz_device_alloc): the library detects which
 *    (hipPointerGetAttributes).  Host buffers are staged through the module's
 *    device workspace (H2D, kernels, D2H) and the call returns only when the
 *    results are visible in the caller's buffer — "logically synchronous"
 *    (poulpy-hal/docs/backend_safety_contract.md:16-19).  Device buffers are
 *    processed in place on the module stream; the call returns after enqueue
 *    and pz_module_sync() (or any host-pointer call) drains the stream.  The
 *    module stream is NOT ordered with any other stream (it is non-blocking with
 *    respect to the null stream too): a device buffer written by the caller's own
 *    kernels or copies on another stream must be complete (event or stream sync)
 *    before it is passed in, and must stay alive until pz_module_sync().
 *  - The bytes of VecZnxDft / SvpPPol / VmpPMat (ScalarPrep = f64) are
 *    backend-private ("device order"): same byte sizes as the
 *    reference (n*cols*size*8, module.rs:51-65) but NOT the reference's
 *    [re | im] bit-reversed layout; callers must treat them as opaque, which is
 *    what poulpy-core does.
 *  - Return value: 0 on success, negative pz_status on failure.  Nothing throws
 *    across the ABI; pz_last_error() gives a thread-local message.  The Rust
 *    shim panics on non-zero, matching the reference's assert!/panic! behaviour.
 *  - All *_batched entry points take DEVICE pointers only and treat `batch`
 *    independent objects laid out back to back (object b at ptr + b*object_len).
 *    Exception: the four GLWE-level calls pz_glwe_external_product_batched, pz_glwe_keyswitch_batched,
 *    pz_glwe_automorphism_batched and pz_glwe_tensor_relinearize_batched also accept HOST containers for res / a (staged, the
 *    call is then logically synchronous; when both are PINNED and batch >= 2 the first three run upload, kernels and download
 *    of successive slices on three streams at once) and a HOST-resident prepared key: poulpy-hal's buffers are host-addressable by contract
 *    (Backend::OwnedBuf: DataMut), so this is what the Rust shim's CoreImpl overrides pass.  A host key is mirrored on the
 *    device on first use and re-used afterwards; the mirror is validated on every call by a sampled fingerprint of the host
 *    bytes and dropped by pz_vmp_prepare / pz_vmp_zero on that buffer and by pz_free_bytes of its block.  A caller that modifies a prepared matrix in place by
 *    other means (e.g. deserializes into it) must call pz_module_forget_host_key before the next use.
 */
#ifndef POULPY_HIP_H
#define POULPY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pz_module pz_module;

/* the ABI revision this header describes (pz_abi_version() of a matching library returns it) */
#define PZ_ABI_VERSION 4u

typedef enum {
    PZ_OK = 0,
    PZ_ERR_INVALID = -1,     /* shape / argument violation (reference: assert!/debug_assert!) */
    PZ_ERR_UNSUPPORTED = -2, /* e.g. n < 32 */
    PZ_ERR_HIP = -3,         /* HIP runtime failure (no device, OOM, launch error) */
    PZ_ERR_ALIAS = -4,       /* overlapping arguments that the op cannot honour */
    PZ_ERR_RCCL = -5
} pz_status;

const char* pz_last_error(void);
/* library/ABI version, bumped on any signature change.  PZ_ABI_VERSION is the version this header describes: clients compare it
 * with pz_abi_version() of the library they loaded before the first call (poulpy_hip.hpp's Module, hal.py and the Rust handle do) */
uint32_t pz_abi_version(void);

/* ---- module (Backend + HalImpl::new) ------------------------------------ */
/* HalImpl::new, hal_impl.rs:320 ; FFT64RefHandle, poulpy-cpu-ref/src/fft64/module.rs:34-69 */
int pz_module_new(uint64_t n, pz_module** out);
int pz_module_new_on_device(uint64_t n, int device, pz_module** out);
/* Backend::destroy, poulpy-hal/src/layouts/module.rs:74-82,260-266 */
void pz_module_free(pz_module* m);
uint64_t pz_module_n(const pz_module* m);
int pz_module_device(const pz_module* m);
/* drains the module stream (needed only after device-pointer calls) */
/* A sibling of `m` for another host thread.  Calls on ONE module are serialised by its lock (one HIP stream, one workspace); poulpy
 * callers share `&Module` across scoped threads (poulpy-bin-fhe bdd_arithmetic/eval.rs:210-221), so the shim gives every other thread a
 * sibling: it shares m's immutable device tables (reference-counted: free in any order) and owns its stream, workspaces, staging arena,
 * pinned-key list, key mirrors, graph cache and lock — calls on different siblings overlap on the device (copies of one with kernels of
 * another).  Knobs (fusion, chunk, graphs) are copied at clone time. */
int pz_module_clone(pz_module* m, pz_module** out);
int pz_module_sync(pz_module* m);
/* raw hipStream_t of the module, for callers that want to order their own work */
void* pz_module_stream(pz_module* m);

/* Backend::alloc_bytes, module.rs:38-43 — pinned host memory, 64 B aligned (lib.rs:146) */
void* pz_alloc_bytes(size_t len);
/* also drops, in every live module, the device mirror of a host-resident prepared key that lies inside the block (see "host
 * containers" below) — a prepared key's `Drop` needs no other hook */
void pz_free_bytes(void* p);
/* device-resident buffers for the batched path */
int pz_device_alloc(pz_module* m, size_t len, void** out);
int pz_device_free(pz_module* m, void* p);
int pz_memcpy_h2d(pz_module* m, void* dst_dev, const void* src_host, size_t len);
int pz_memcpy_d2h(pz_module* m, void* dst_host, const void* src_dev, size_t len);
int pz_memset_d(pz_module* m, void* dst_dev, int value, size_t len);

/* Backend::bytes_of_*, module.rs:51-65 */
size_t pz_bytes_of_vec_znx(uint64_t n, size_t cols, size_t size);
size_t pz_bytes_of_vec_znx_dft(uint64_t n, size_t cols, size_t size);
size_t pz_bytes_of_vec_znx_big(uint64_t n, size_t cols, size_t size);
size_t pz_bytes_of_svp_ppol(uint64_t n, size_t cols);
size_t pz_bytes_of_vmp_pmat(uint64_t n, size_t rows, size_t cols_in, size_t cols_out, size_t size);

/* ---- VecZnxDft ----------------------------------------------------------- */
/* hal_impl.rs:529 vec_znx_dft_apply */
int pz_vec_znx_dft_apply(pz_module* m, size_t step, size_t offset,
                         double* res, size_t res_cols, size_t res_size, size_t res_col,
                         const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:534 */
size_t pz_vec_znx_idft_apply_tmp_bytes(const pz_module* m);
/* hal_impl.rs:536 vec_znx_idft_apply */
int pz_vec_znx_idft_apply(pz_module* m,
                          int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                          const double* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:541 vec_znx_idft_apply_tmpa (a may be clobbered) */
int pz_vec_znx_idft_apply_tmpa(pz_module* m,
                               int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                               double* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:546 vec_znx_idft_apply_consume: all cols x limbs in place, buffer re-typed to VecZnxBig */
int pz_vec_znx_idft_apply_consume(pz_module* m, void* data, size_t cols, size_t size);
/* hal_impl.rs:553 */
int pz_vec_znx_dft_add_into(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                            const double* a, size_t a_cols, size_t a_size, size_t a_col,
                            const double* b, size_t b_cols, size_t b_size, size_t b_col);
/* hal_impl.rs:559 */
int pz_vec_znx_dft_add_scaled_assign(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                                     const double* a, size_t a_cols, size_t a_size, size_t a_col, int64_t a_scale);
/* hal_impl.rs:564 */
int pz_vec_znx_dft_add_assign(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                              const double* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:569 */
int pz_vec_znx_dft_sub(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                       const double* a, size_t a_cols, size_t a_size, size_t a_col,
                       const double* b, size_t b_cols, size_t b_size, size_t b_col);
/* hal_impl.rs:575 */
int pz_vec_znx_dft_sub_assign(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                              const double* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:580 */
int pz_vec_znx_dft_sub_negate_assign(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                                     const double* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:585 */
int pz_vec_znx_dft_copy(pz_module* m, size_t step, size_t offset,
                        double* res, size_t res_cols, size_t res_size, size_t res_col,
                        const double* a, size_t a_cols, size_t a_size, size_t a_col);
/* hal_impl.rs:590 */
int pz_vec_znx_dft_zero(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col);

/* ---- SVP ------------------------------------------------------------------ */
/* hal_impl.rs:595 svp_prepare (ScalarZnx(n, a_cols) -> SvpPPol(n, res_cols)) */
int pz_svp_prepare(pz_module* m, double* res, size_t res_cols, size_t res_col,
                   const int64_t* a, size_t a_cols, size_t a_col);
/* hal_impl.rs:600 svp_apply_dft */
int pz_svp_apply_dft(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                     const double* ppol, size_t a_cols, size_t a_col,
                     const int64_t* b, size_t b_cols, size_t b_size, size_t b_col);
/* hal_impl.rs:606 svp_apply_dft_to_dft */
int pz_svp_apply_dft_to_dft(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                            const double* ppol, size_t a_cols, size_t a_col,
                            const double* b, size_t b_cols, size_t b_size, size_t b_col);
/* hal_impl.rs:612 svp_apply_dft_to_dft_assign */
int pz_svp_apply_dft_to_dft_assign(pz_module* m, double* res, size_t res_cols, size_t res_size, size_t res_col,
                                   const double* ppol, size_t a_cols, size_t a_col);

/* ---- VMP ------------------------------------------------------------------ */
/* hal_impl.rs:618 ; the reference's scratch sizes are returned unchanged so that
 * poulpy-core sizes its host arena identically — the device path
 * does not use caller scratch. */
size_t pz_vmp_prepare_tmp_bytes(const pz_module* m, size_t rows, size_t cols_in, size_t cols_out, size_t size);
/* hal_impl.rs:620 vmp_prepare (MatZnx -> VmpPMat, device order) */
int pz_vmp_prepare(pz_module* m, double* pmat, const int64_t* mat,
                   size_t rows, size_t cols_in, size_t cols_out, size_t size);
/* hal_impl.rs:626 */
size_t pz_vmp_apply_dft_tmp_bytes(const pz_module* m, size_t res_size, size_t a_size,
                                  size_t b_rows, size_t b_cols_in, size_t b_cols_out, size_t b_size);
/* hal_impl.rs:636 vmp_apply_dft */
int pz_vmp_apply_dft(pz_module* m, double* res, size_t res_cols, size_t res_size,
                     const int64_t* a, size_t a_cols, size_t a_size,
                     const double* pmat, size_t rows, size_t cols_in, size_t cols_out, size_t size);
/* hal_impl.rs:643 */
size_t pz_vmp_apply_dft_to_dft_tmp_bytes(const pz_module* m, size_t res_size, size_t a_size,
                                         size_t b_rows, size_t b_cols_in, size_t b_cols_out, size_t b_size);
/* hal_impl.rs:653 vmp_apply_dft_to_dft.  DEVIATION for limb_offset > 0: cpu-ref's FFT64 core clamps the key columns it reads to
 * res_size and leaves the last limb_offset limbs of res unwritten (stale scratch, vmp.rs:217-263); this backend follows the NTT120
 * sibling's semantics instead (reference/ntt120/vmp.rs:190,281-287): res[c] = sum_r a[r] * P[r][c + off] for every c with a key
 * column, zero beyond — every limb of res is written.  Byte parity with FFT64Ref is therefore claimed for
 * limb_offset = 0 (dsize = 1: every BASELINE config) only; limb_offset > 0 (the dsize > 1 callers) is validated against the exact
 * bivariate product. */
int pz_vmp_apply_dft_to_dft(pz_module* m, double* res, size_t res_cols, size_t res_size,
                            const double* a, size_t a_cols, size_t a_size,
                            const double* pmat, size_t rows, size_t cols_in, size_t cols_out, size_t size,
                            size_t limb_offset);
/* hal_impl.rs:665 vmp_zero */
int pz_vmp_zero(pz_module* m, double* pmat, size_t rows, size_t cols_in, size_t cols_out, size_t size);

/* ---- VecZnxBig ------------------------------------------------------------- */
/* hal_impl.rs:428 */
size_t pz_vec_znx_big_normalize_tmp_bytes(const pz_module* m);
/* hal_impl.rs:431 vec_znx_big_normalize (same- and cross-base2k, any res_offset) */
int pz_vec_znx_big_normalize(pz_module* m,
                             int64_t* res, size_t res_cols, size_t res_size, size_t res_base2k, int64_t res_offset, size_t res_col,
                             const int64_t* a, size_t a_cols, size_t a_size, size_t a_base2k, size_t a_col);
/* hal_impl.rs:362 vec_znx_big_add_small_assign */
int pz_vec_znx_big_add_small_assign(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                    const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);

/* hal_impl.rs:225 vec_znx_rotate, :230 _assign_tmp_bytes, :232 _assign (reference/znx/rotate.rs:3-27: res = X^k * a in Z[X]/(X^n+1),
 * any k; limbs of res beyond a.size zeroed).  Used by glwe_rotate_assign between the rows of a circuit bootstrapping. */
size_t pz_vec_znx_rotate_assign_tmp_bytes(const pz_module* m);
int pz_vec_znx_rotate(pz_module* m, int64_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                      const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_rotate_assign(pz_module* m, int64_t k, int64_t* res, size_t cols, size_t size, size_t col);
/* hal_impl.rs:217 vec_znx_rsh_assign (reference/vec_znx/shift.rs:186-243): res >>= k bits in place, normalizing; used by
 * glwe_rsh / glwe_trace.  k <= base2k * size. */
size_t pz_vec_znx_rsh_tmp_bytes(const pz_module* m);
int pz_vec_znx_rsh_assign(pz_module* m, size_t base2k, size_t k, int64_t* res, size_t cols, size_t size, size_t col);

/* ---- i64 VecZnx limb-wise family (hal_impl.rs:34 zero, :41 normalize, :55 normalize_assign, :59 add_into,
 * :65 add_assign, :90 sub, :96 sub_assign, :101 sub_negate_assign, :126 negate, :131 negate_assign, :289 copy): the i64
 * operations poulpy-core runs between the hot-path calls (glwe_add / sub / copy / normalize ...), so that ciphertexts can
 * stay on the device.  Limb-range rules of reference/vec_znx/{add,sub,negate,copy}.rs (common limbs combined, the longer
 * operand copied / negated, the rest of res zeroed), wrapping i64 arithmetic.  Host or device pointers. ------------------- */
int pz_vec_znx_add_into(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                        const int64_t* a, size_t a_cols, size_t a_size, size_t a_col,
                        const int64_t* b, size_t b_cols, size_t b_size, size_t b_col);
int pz_vec_znx_sub(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                   const int64_t* a, size_t a_cols, size_t a_size, size_t a_col,
                   const int64_t* b, size_t b_cols, size_t b_size, size_t b_col);
int pz_vec_znx_add_assign(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                          const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_sub_assign(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                          const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_sub_negate_assign(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                 const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_negate(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                      const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_negate_assign(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col);
int pz_vec_znx_copy(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                    const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_zero(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_col);
/* vec_znx_normalize: the function vec_znx_big_normalize forwards to when ScalarBig = i64; _assign: in place, same base
 * (reference/vec_znx/normalize.rs:18-48, :403-425) */
size_t pz_vec_znx_normalize_tmp_bytes(const pz_module* m);
int pz_vec_znx_normalize(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t res_base2k, int64_t res_offset,
                         size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_base2k, size_t a_col);
int pz_vec_znx_normalize_assign(pz_module* m, size_t base2k, int64_t* res, size_t cols, size_t size, size_t col);
/* vec_znx_lsh (hal_impl.rs:165), vec_znx_rsh (:137), vec_znx_lsh_assign (:221), tmp bytes (:163): bit shifts of the torus value
 * by k bits with renormalization (reference/vec_znx/shift.rs:68-135, :245-342, :16-66); at equal bases these are the limb
 * walks of vec_znx_normalize with res_offset = +k / -k.  (vec_znx_rsh_assign: below.) */
size_t pz_vec_znx_lsh_tmp_bytes(const pz_module* m);
int pz_vec_znx_lsh(pz_module* m, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                   const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_rsh(pz_module* m, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                   const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_lsh_assign(pz_module* m, size_t base2k, size_t k, int64_t* res, size_t cols, size_t size, size_t col);

/* ---- X -> X^p on i64 containers (the glwe_automorphism callers) ---------------------- *
 * hal_impl.rs:236 vec_znx_automorphism, :241 _assign_tmp_bytes, :243 _assign; :517 vec_znx_big_automorphism, :522, :524.
 * reference/znx/automorphism.rs:1-17: res[(i*p) mod 2n] = a[i], negated when the index wraps past n; limbs of res beyond
 * a.size are zeroed (vec_znx/automorphism.rs:32-34).  p may be negative; it must be odd (an even p is not a ring
 * automorphism: PZ_ERR_INVALID).  The non-assign forms reject res == a.                                           */
size_t pz_vec_znx_automorphism_assign_tmp_bytes(const pz_module* m);
int pz_vec_znx_automorphism(pz_module* m, int64_t p, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                            const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_automorphism_assign(pz_module* m, int64_t p, int64_t* res, size_t cols, size_t size, size_t col);
size_t pz_vec_znx_big_automorphism_assign_tmp_bytes(const pz_module* m);
int pz_vec_znx_big_automorphism(pz_module* m, int64_t p, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_big_automorphism_assign(pz_module* m, int64_t p, int64_t* res, size_t cols, size_t size, size_t col);

/* ---- batched, device-resident path (the measured one) ---------------------- *
 * Coarser boundary: unsafe trait CoreImpl<BE>, poulpy-core/src/oep/core_impl.rs:34
 *   glwe_external_product :120  (poulpy-core/src/external_product/glwe.rs:99-141,197-271)
 *   glwe_keyswitch        :42   (poulpy-core/src/keyswitching/glwe.rs:53-109,207-239,298-380)
 * applied to `batch` independent GLWE ciphertexts that share one prepared key.
 * All pointers are device pointers; ciphertext b of `a` starts at
 * a + b*n*(rank+1)*a_size, of `res` at res + b*n*(rank+1)*res_size.            */
typedef struct {
    uint64_t rank;        /* GLWE rank; cols = rank + 1 */
    uint64_t dnum;        /* rows of the prepared GGSW / GGLWE */
    uint64_t dsize;       /* digit size (1 on every BASELINE config) */
    uint64_t key_size;    /* limbs of the prepared key */
    uint64_t key_base2k;
    uint64_t a_size;
    uint64_t a_base2k;
    uint64_t res_size;
    uint64_t res_base2k;
    uint64_t rank_out;    /* keyswitch only: output rank (key cols_out = rank_out+1, cols_in = rank) */
} pz_glwe_op_params;

int pz_glwe_external_product_batched(pz_module* m, int64_t* res, const int64_t* a, const double* ggsw_pmat,
                                     const pz_glwe_op_params* p, size_t batch);
int pz_glwe_keyswitch_batched(pz_module* m, int64_t* res, const int64_t* a, const double* key_pmat,
                              const pz_glwe_op_params* p, size_t batch);
/* CoreImpl glwe_automorphism family (poulpy-core/src/automorphism/glwe_ct.rs) on `batch` ciphertexts sharing one
 * prepared automorphism key (a GGLWE rank -> rank; `gal` = key.p(), odd):
 *   PZ_AUTO             res = phi(keyswitch(a))                      glwe_ct.rs:51-72
 *   PZ_AUTO_ADD         res = normalize(phi(big) + a)                :96-140
 *   PZ_AUTO_SUB         res = normalize(phi(big) - a)                :185-229
 *   PZ_AUTO_SUB_NEGATE  res = normalize(a - phi(big))                :231-275
 * with big = the key-switch value before normalization (keyswitching/glwe.rs:207-239) and phi = X -> X^gal.
 * The *_assign forms of the reference are the same calls with res == a (same layout), which is allowed: every
 * ciphertext is fully consumed before its result is written.                                                    */
enum { PZ_AUTO = 0, PZ_AUTO_ADD = 1, PZ_AUTO_SUB = 2, PZ_AUTO_SUB_NEGATE = 3 };
int pz_glwe_automorphism_batched(pz_module* m, int64_t* res, const int64_t* a, const double* key_pmat,
                                 const pz_glwe_op_params* p, int64_t gal, int mode, size_t batch);
/* res[r][b] = glwe_automorphism(a[b], key_pmats[r], gals[r])  (PZ_AUTO, glwe_ct.rs:51-72) for r < nrot, b < batch.
 * gals / key_pmats: HOST arrays of nrot entries (as for pz_glwe_trace_batched); every key_pmats[r], a and res are device pointers.
 * Rotation-major result: ciphertext b of rotation r at res + (r*batch + b) * n*(rank+1)*res_size, so each rotation is a
 * contiguous batch for the next call.  res must not overlap a.  Bit-identical to nrot calls of pz_glwe_automorphism_batched.
 * Where the three-kernel pipeline serves the shape, the forward column pass and the read of the body column - the work that does
 * not depend on the Galois element - run once per wave for all rotations ("hoisted rotations"); every other shape, and nrot == 1, takes one
 * pz_glwe_automorphism_batched per rotation.  nrot == 0, an even Galois element, a null key or an overlap: PZ_ERR_INVALID, nothing
 * is launched.  The workspace query covers nrot row-sliced key copies (keys pinned with pz_module_pin_key use their cached ones). */
int pz_glwe_automorphism_many_batched(pz_module* m, int64_t* res, const int64_t* a, size_t nrot, const int64_t* gals,
                                      const double* const* key_pmats, const pz_glwe_op_params* p, size_t batch);
size_t pz_glwe_automorphism_many_workspace_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t nrot, size_t batch);
/* CoreImpl glwe_trace_assign (poulpy-core/src/glwe_trace.rs:129-176) on `batch` ciphertexts:
 * for s < nsteps:  res = rsh(res, 1 bit);  res = glwe_automorphism_add_assign(res, key_s)   (:164-174).
 * The caller resolves the steps skip..log_n into Galois elements (i = 0: -1, else galois_element(2^(i-1)),
 * poulpy-hal/src/layouts/module.rs:214-226) and the matching prepared automorphism keys: gals[s], key_pmats[s] are HOST
 * arrays; each key_pmats[s] and res are device pointers.  res and keys of one base2k: p describes one step (a_size = res_size,
 * equal base2k).  res in another base than the keys (:153-163, the case test_suite/trace.rs runs): (res_size, res_base2k) is res,
 * (a_size, a_base2k = key_base2k) its layout re-expressed in the keys' base, a_size = ceil(res.max_k / key_base2k); res is
 * normalized into a temporary of that layout, traced there and normalized back. */
int pz_glwe_trace_batched(pz_module* m, int64_t* res, size_t nsteps, const int64_t* gals, const double* const* key_pmats,
                          const pz_glwe_op_params* p, size_t batch);
/* GLWEPacking::glwe_pack (poulpy-core/src/glwe_packing.rs:122-176, pack_internal :15-87) on `batch` independent packing
 * problems that share the occupancy pattern; ciphertexts, keys and result share base2k and size (p: a_size = res_size).
 *   indices / cts   HOST arrays of nslots entries: cts[s] -> the `batch` contiguous device GLWEs of index indices[s] (the
 *                   reference's HashMap<usize, &mut GLWE>); they are CLOBBERED, as the reference's entries are
 *   gals / key_pmats HOST arrays of log2(n) entries: Galois element and prepared automorphism key of trace step i
 *                   (i = 0: -1, else galois_element(2^(i-1)); glwe_pack_galois_elements :100-102)
 *   res             batch contiguous GLWEs: the packed result after the final partial trace (:175)
 *   tmp             device scratch of pz_glwe_pack_tmp_bytes */
size_t pz_glwe_pack_tmp_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t batch);
int pz_glwe_pack_batched(pz_module* m, int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts,
                         size_t log_gap_out, const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p,
                         void* tmp, size_t tmp_bytes, size_t batch);
/* the same with the automorphism keys in their own base (the case test_suite/glwe_packing.rs:40-42 runs: ciphertexts and result in
 * base2k - 1, keys in base2k): p->a = p->res = the ciphertexts' layout, p->key_base2k the keys'; trace_size = limbs of the closing
 * trace's temporary in the keys' base, ceil(max(a.max_k, res.max_k) / key_base2k) (glwe_trace.rs:107-112) */
size_t pz_glwe_pack_bases_tmp_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t trace_size, size_t batch);
int pz_glwe_pack_bases_batched(pz_module* m, int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts,
                               size_t log_gap_out, const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p,
                               size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch);
/* CMUX, the gate of poulpy-bin-fhe's bdd_arithmetic (poulpy-bin-fhe/src/bdd_arithmetic/eval.rs:524-626), on `batch` ciphertexts sharing
 * one prepared GGSW:   res = normalize((t - f) (x) GGSW(bit) + f)   - res = t when bit = 1, f when bit = 0.
 *   D[l]  = t[l] - f[l] on the p->a_size limbs of the difference container, missing limbs of either side zero, NOT normalized
 *           (glwe_sub / glwe_sub_assign, poulpy-core/src/api/operations.rs:330-394)
 *   big   = glwe_external_product_internal(D, ggsw)   (external_product/glwe.rs:197-271; key_size limbs, any dsize >= 1)
 *   big  += f on every column, min(key_size, f_size) limbs (vec_znx_big_add_small_assign), IN FRONT of the carry chain - which is why the
 *           gate is not pz_glwe_external_product_batched followed by an addition
 *   res   = vec_znx_big_normalize(big) on every column
 * The three forms of the reference are this call with different aliasing:
 *   cmux            (eval.rs:550-572)  t, f, res distinct                      p->a_size = res_size (the difference is written into res)
 *   cmux_assign     (:606-625)         res == t, f = a                         p->a_size = res_size
 *   cmux_assign_neg (:575-603)         res == f, t = a                         p->a_size = ceil(max(res.k, a.k) / base2k)
 * p: rank, the GGSW (dnum, dsize, key_size, key_base2k), a_size = limbs of D, res_size; t, f, res and the GGSW share ONE base2k
 * (external_product/glwe.rs:213): anything else is PZ_ERR_INVALID, nothing launched.  t_size / f_size: limbs of t and of f.
 * res == t and res == f (equal layouts) are allowed: every ciphertext is consumed before its result is written.  Any other overlap of
 * res with t or f: PZ_ERR_ALIAS.
 * Rotated source: t == NULL means t = X^{t_rot} f (negacyclic, t_rot taken mod 2N and read in this form only; t_size == f_size) - glwe_rotate followed by cmux_assign,
 * one step of glwe_blind_rotation_assign (bdd_arithmetic/blind_rotation.rs:225-232); res must not overlap f then (PZ_ERR_ALIAS).
 * t, f, res: device pointers; the prepared GGSW resolves as for every GLWE call (pinned, host with a device mirror, device).
 * N = 1024 / 2048 / 4096 on the small-ring kernels form the difference inside the forward stage (D never reaches memory); every other
 * shape writes D to the module's second workspace first (POULPY_DBG_CMUX_FUSED=0 sends every shape that way). */
int pz_glwe_cmux_batched(pz_module* m, int64_t* res, const int64_t* t, size_t t_size, int64_t t_rot, const int64_t* f, size_t f_size,
                         const double* ggsw_pmat, const pz_glwe_op_params* p, size_t batch);
/* what the call reserves in the module's grow-only workspace: the external product's figure with a_size = limbs of D.  NOT counted: on the
 * materialised route (N >= 8192, N < 1024, dsize > 1, N = 4096 with the small path off, POULPY_DBG_CMUX_FUSED=0) D itself goes to the module's
 * second grow-only workspace, batch * N * (rank + 1) * a_size * 8 bytes - for the WHOLE batch, not per wave of ciphertexts */
size_t pz_glwe_cmux_workspace_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t batch);
/* GLWEBlindRotation::glwe_blind_rotation / _assign (poulpy-bin-fhe/src/bdd_arithmetic/blind_rotation.rs:196-264) on `batch` ciphertexts:
 *   res = a X^{+-((k >> bit_rsh) mod 2^bit_mask) << bit_lsh}   by nbits = bit_mask CMUX steps; step i is the rotated-source CMUX by
 * +-2^(i + bit_lsh) (sign != 0: +) with the GGSW of bit i + bit_rsh.  The steps ping-pong between res and tmp (:218-236); in place an odd
 * step count ends with a copy into res (:238-241); out of place with one layout for a and res, step 0 reads a itself and the last step lands
 * in res.  Bit-identical to nbits calls of pz_glwe_cmux_batched.
 *   bits   HOST array of nbits device pointers to prepared GGSWs: bits[i] = the GGSW of bit i + bit_rsh (the caller resolves get_bit, as it
 *          resolves the keys of pz_glwe_trace_batched)
 *   p      rank, the GGSWs' layout, a_size = limbs of a, res_size; one base2k.  Every step works on the layout of res
 *   tmp    device scratch of pz_glwe_blind_rotation_tmp_bytes (one batch in the layout of res)
 * res == a (equal layouts) is glwe_blind_rotation_assign; nbits == 0 copies a.  ggsw_blind_rotation / _assign (:45-106) is the same call
 * on the dnum (rank + 1) GLWE entries of `count` contiguous GGSWs (MatZnx layout: the entries are contiguous): batch = count dnum (rank + 1).
 * A call repeated with the same arguments is replayed as one HIP graph (pz_module_set_graphs). */
size_t pz_glwe_blind_rotation_tmp_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t batch);
int pz_glwe_blind_rotation_batched(pz_module* m, int64_t* res, const int64_t* a, size_t nbits, const double* const* bits, int sign,
                                   size_t bit_lsh, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch);
/* Conditional swap, the other gate of bdd_arithmetic: Cswap::cswap (poulpy-bin-fhe/src/bdd_arithmetic/eval.rs:417-461, the equal-base
 * branch) on `batch` pairs sharing one prepared GGSW; IN PLACE on a and b - (a, b) stays when bit = 0 and becomes (b, a) when bit = 1:
 *   D     = b - a  on p->a_size limbs (glwe_sub, missing limbs zero, NOT normalized)
 *   big   = glwe_external_product_internal(D, ggsw)                (key_size limbs)
 *   a'[j] = vec_znx_big_normalize(big[j] + a[j])    (vec_znx_big_add_small_into: min(key_size, a_size) limbs of a)
 *   b'[j] = vec_znx_big_normalize(b[j] - big[j])    (vec_znx_big_sub_small_a: limbs of big beyond b_size enter negated)
 * for every column j; a' has a_size limbs, b' has b_size limbs.  ONE external product, both results from its one big value - which is why
 * the gate is not two calls of pz_glwe_cmux_batched (two products of +-D, other digits).
 * p: rank, the GGSW (dnum, any dsize >= 1, key_size, key_base2k), a_size = limbs of D = max(a_size, b_size) (tmp_c, eval.rs:437-442),
 * res_size = a_size.  a, b and the GGSW share ONE base2k (eval.rs:427, external_product/glwe.rs:213): anything else is PZ_ERR_INVALID,
 * nothing launched - the reference's other branch, res_base2k != s_base2k (:462-511), is not provided.
 * a, b: device pointers to `batch` packed ciphertexts each; ANY overlap of the two ranges, a == b included, is PZ_ERR_ALIAS and nothing
 * is launched.  The prepared GGSW resolves as for every GLWE call (pinned, host with a device mirror, device).
 * N = 1024 / 2048 / 4096 on the small-ring kernels form D inside the forward stage and run both carry chains behind one inverse
 * transform; every other shape writes D to the module's second workspace and leaves the two results from the one big value of its
 * pipeline (POULPY_DBG_CMUX_FUSED=0 sends every shape that way). */
int    pz_glwe_cswap_batched(pz_module* m, int64_t* a, size_t a_size, int64_t* b, size_t b_size,
                             const double* ggsw_pmat, const pz_glwe_op_params* p, size_t batch);
/* what the call reserves in the module's grow-only workspace: the external product's figure with a_size = limbs of D.  NOT counted: on the
 * materialised route D itself goes to the module's second grow-only workspace, batch * N * (rank + 1) * a_size * 8 bytes */
size_t pz_glwe_cswap_workspace_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t batch);

/* GLWEBlindRetrieval::glwe_blind_retrieval_statefull (reverse == 0, blind_retrieval.rs:214-236) / _rev (reverse != 0, :243-265)
 * on `batch` independent vectors of nslots ciphertexts of one layout: afterwards slot 0 holds the element at the encrypted index
 * (bits >> bit_rsh) mod 2^nbits; the reverse call undoes the permutation.
 *   slots  dense slot-major device buffer [nslots][batch]: slot s of every vector at slots + s * batch * n * (rank + 1) * size;
 *          p->a_size == p->res_size = size, one base2k
 *   bits   HOST array of nbits device pointers to prepared GGSWs: bits[i] = the GGSW of bit bit_rsh + i (the caller resolves get_bit,
 *          as for pz_glwe_blind_rotation_batched); a null entry is PZ_ERR_INVALID
 * Level i uses t = 2^(nbits - 1 - i) and bits[nbits - 1 - i]; the reference's loop `for j in 0..t { if j + t < len { cswap(res[j],
 * res[j + t]) } }` is ONE pz_glwe_cswap_batched on cnt * batch contiguous pairs, cnt = t < nslots ? min(t, nslots - t) : 0, a = slot 0,
 * b = slot t (disjoint: cnt <= t); a level with cnt == 0 launches nothing.  Forward: levels 0 .. nbits - 1; reverse: the same levels in
 * the opposite order.  nslots == 0 or nbits == 0: PZ_OK, nothing launched.  Bit-identical to the per-level pz_glwe_cswap_batched calls.
 * A call repeated with the same arguments is replayed as one HIP graph (pz_module_set_graphs).
 * Not provided: GLWEBlindRetriever (blind_retrieval.rs:31-179) - glwe_copy + cmux_assign_neg, i.e. pz_glwe_cmux_batched as it is. */
int    pz_glwe_blind_retrieval_batched(pz_module* m, int64_t* slots, size_t nslots, size_t nbits, const double* const* bits,
                                       int reverse, const pz_glwe_op_params* p, size_t batch);
/* the swap's figure at the largest level */
size_t pz_glwe_blind_retrieval_workspace_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t nslots, size_t nbits, size_t batch);

/* ---- BDD circuits: ExecuteBDDCircuit (poulpy-bin-fhe/src/bdd_arithmetic/eval.rs:104-305) --------------------------------------
 * A circuit is one node list per output bit, in chunks of state_size nodes, one chunk per level (eval_level, :241-305).  The state is two banks
 * of state_size GLWEs in the layout of the result, all zero but slot 1 of the 2 state_size, which is encode_coeff_i64(base2k, col 0, k = 2,
 * idx 0, 1): the value 2^-2 at coefficient 0.  Per level, node j of the chunk:
 *   PZ_BDD_CMUX(sel, hi, lo)   next[j] = cmux(prev[hi], prev[lo], GGSW(sel)) - pz_glwe_cmux_batched out of place, t = prev[hi], f = prev[lo]
 *   PZ_BDD_COPY                next[j] = prev[j]
 *   PZ_BDD_NONE                next[j] stays what it was
 * then the banks are swapped.  The last chunk is [cmux, none, ...]: its gate writes the output bit.  An output with state_size 0 has no nodes
 * and is zero. */
typedef enum { PZ_BDD_NONE = 0, PZ_BDD_COPY = 1, PZ_BDD_CMUX = 2 } pz_bdd_kind;
/* (declared WITH its tag, unlike the parameter structs of this header: poulpy_amd/abi.py lists untagged structs in abi.STRUCTS, whose exact contents -
 * the six parameter structs - tests/test_abi_and_host.py pins; the node is typed from this declaration all the same, into abi.TAGGED_STRUCTS) */
typedef struct pz_bdd_node { uint32_t kind, sel, hi, lo; } pz_bdd_node;
typedef struct pz_bdd_circuit pz_bdd_circuit;
/* Host only (no module, no device).  nodes[o] / node_count[o] / state_size[o]: the node list of output bit o, o < output_size; input_size:
 * the number of input bits (every selector is below it).  Validates - node_count a positive multiple of state_size, hi and lo below
 * state_size, sel below input_size, the last chunk [cmux, none, ...], no nodes on a state_size-0 output - and returns NULL on a violation,
 * pz_last_error naming the output bit and the node.  Compiles the schedule the device runs:
 *   levels   level l holds level l of every output that is that deep (start-aligned); all its gates are ONE launch, so no gate of a level
 *            writes a slot a gate of the same level reads or writes
 *   slots    every live value has a physical slot, at most 2 state_size per output, plus two shared by all: slot 0 = zero, slot 1 = one.
 *            A COPY moves nothing: the value keeps its slot and its readers are pointed at it (moved_copies == 0)
 *   order    the gates of a level sorted by selector; the root gates write the output itself
 * The handle is immutable and may be used by any number of modules and threads; freeing it before a module that has run it is safe (a module
 * keeps its own device copy of the tables). */
pz_bdd_circuit* pz_bdd_circuit_new(const pz_bdd_node* const* nodes, const size_t* node_count, const size_t* state_size, size_t output_size,
                                   size_t input_size);
void   pz_bdd_circuit_free(pz_bdd_circuit* c);
size_t pz_bdd_circuit_input_size(const pz_bdd_circuit* c);
size_t pz_bdd_circuit_output_size(const pz_bdd_circuit* c);
size_t pz_bdd_circuit_max_state_size(const pz_bdd_circuit* c);
size_t pz_bdd_circuit_levels(const pz_bdd_circuit* c);         /* launches of the gathered route */
size_t pz_bdd_circuit_gates(const pz_bdd_circuit* c);          /* = the CMUX nodes of the circuit */
size_t pz_bdd_circuit_moved_copies(const pz_bdd_circuit* c);   /* COPY nodes that cost a ciphertext copy: 0 */
size_t pz_bdd_circuit_slots(const pz_bdd_circuit* c);          /* the two shared slots + every output's */
/* the slots of output bit o: [*first, *first + *count), count <= 2 state_size; returns 0, or -1 for an o out of range */
int    pz_bdd_circuit_output_slots(const pz_bdd_circuit* c, size_t o, size_t* first, size_t* count);
/* the gates of level `level` as 4 words each - t slot, f slot, res (a slot, or 0x80000000 | output bit), selector - the first `cap` of them into
 * gates4 (may be NULL with cap 0); returns the number of gates of the level */
size_t pz_bdd_circuit_level_gates(const pz_bdd_circuit* c, size_t level, uint32_t* gates4, size_t cap);
/* ExecuteBDDCircuit::execute_bdd_circuit on `batch` independent inputs; bit-identical to the node-by-node walk through pz_glwe_cmux_batched.
 *   out    dense slot-major device buffer [n_out][batch] of GLWEs of p->res_size limbs, n_out >= output_size; output bit o of input b at
 *          out + (o * batch + b) * n * (rank + 1) * res_size.  Slots of state_size-0 outputs and slots beyond output_size are zeroed (:225-237).
 *          out overlaps neither tmp nor a key: PZ_ERR_ALIAS
 *   bits   HOST array [batch][nbits], nbits >= input_size: bits[b * nbits + i] = the prepared GGSW of input bit i of input b, resolved as for
 *          every GLWE call (pinned, host with a device mirror, device); the same pointer may occur many times; an entry the circuit never
 *          selects may be NULL, a selected NULL entry is PZ_ERR_INVALID.  Host-resident entries cost what they cost every GLWE call - each distinct one
 *          is fingerprinted on EVERY call to validate its mirror (a sampled hash: its first and last 4 KiB and about 8 000 words strided over
 *          the rest, read on the host) - and a module holds at most 64 mirrors (48 GiB):
 *          more distinct host-resident selected GGSWs than that in one call is PZ_ERR_UNSUPPORTED, nothing launched; keys of an adder belong on the device
 *   p      rank, the GGSWs (dnum, any dsize >= 1, key_size, key_base2k), a_size == res_size (take_glwe_slice(.., res): one layout), ONE
 *          base2k for state, result and GGSWs; anything else PZ_ERR_INVALID with nothing launched
 *   tmp    device scratch of pz_bdd_circuit_execute_tmp_bytes:
 *            align256(slots * batch * ct)                      the state pool, ct = n * (rank + 1) * res_size * 8
 *          + align256(gates * batch * 32)                      the per-call gather table
 *          + align256(batch * nbits * 8)                       the per-call key pointers, nbits = input_size in the query (a call with a
 *                                                              larger nbits needs batch * (nbits - input_size) * 8 more)
 *          + batch * selected * align256(key bytes)            row-sliced copies of the selected keys that are not pinned (worst case: all
 *                                                              distinct, none pinned); key bytes = n * 8 * dnum * (rank + 1)^2 * key_size
 *          a short tmp is refused before anything is launched
 * Routes: N = 1024 / 2048 / 4096 on the small-ring kernels (dsize 1, fusion on) run every level as ONE launch of the gathered CMUX kernels
 * ("bdd: gathered small-one" / "bdd: gathered small two-kernel"); every other shape - and every shape under POULPY_DBG_BDD_GATHER=0 - runs the
 * same schedule by one CMUX per (gate, input) on the existing kernels ("bdd: per-gate (...)").  The module's grow-only workspace is reserved
 * as the CMUX does it.  A call repeated with the same arguments is replayed as one HIP graph (pz_module_set_graphs); the keys are not part of
 * the graph on the gathered route - a new bits array behind the same arguments is picked up.
 * batch == 0 or output_size == 0: PZ_OK; only the zeroing of out happens, if any. */
size_t pz_bdd_circuit_execute_tmp_bytes(const pz_module* m, const pz_bdd_circuit* c, const pz_glwe_op_params* p, size_t batch);
int    pz_bdd_circuit_execute_batched(pz_module* m, const pz_bdd_circuit* c, int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                                      const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch);
/* CoreImpl ggsw_external_product (poulpy-core/src/external_product/ggsw.rs:54-58): res[row][col] = a[row][col] (x) ggsw
 * for the a_dnum * (rank+1) GLWE entries of the GGSW `a` (MatZnx layout: entries are contiguous), device pointers. */
int pz_ggsw_external_product(pz_module* m, int64_t* res, const int64_t* a, size_t a_dnum, const double* ggsw_pmat,
                             const pz_glwe_op_params* p);
/* CoreImpl ggsw_expand_row (poulpy-core/src/conversion/gglwe_to_ggsw.rs:116-268; the second half of ggsw_from_gglwe
 * :32-61 and of circuit bootstrapping) on `count` contiguous GGSWs (MatZnx layout, rows = dnum, cols_in = cols_out =
 * rank+1, size = p->res_size), in place: entry (row, col), col >= 1, becomes the key switch of the mask of entry (row, 0)
 * by tsk_pmat[col-1] (= tsk.at(col-1), a prepared GGLWE rank -> rank) with the body of entry (row, 0) added to column
 * `col`; entries (row, 0) are not written.  tsk_pmat is a HOST array of rank device pointers; p describes the key switch
 * (a_size = res_size, a_base2k = res_base2k = the GGSW's; rank_out = rank). */
int pz_ggsw_expand_row_batched(pz_module* m, int64_t* ggsw, size_t dnum, const double* const* tsk_pmat,
                               const pz_glwe_op_params* p, size_t count);
/* CoreImpl ggsw_from_gglwe (poulpy-core/src/conversion/gglwe_to_ggsw.rs:32-61) on `count` contiguous device GGLWEs `a`
 * (MatZnx layout, rows = dnum, cols_in = a_cols_in, cols_out = rank+1, size = p->res_size: same size and base as the
 * GGSW) -> `count` contiguous GGSWs: entries (row, 0) are copied from a.at(row, 0), then pz_ggsw_expand_row_batched. */
int pz_ggsw_from_gglwe_batched(pz_module* m, int64_t* ggsw, const int64_t* a, size_t a_cols_in, size_t dnum,
                               const double* const* tsk_pmat, const pz_glwe_op_params* p, size_t count);
/* CoreImpl glwe_automorphism_key_automorphism / _assign (poulpy-core/src/automorphism/gglwe_atk.rs:42-155) on `count` contiguous
 * device GGLWEs `a` (automorphism keys of Galois element a_gal; MatZnx layout, rows = a_dnum, cols_in = rank, cols_out = rank+1,
 * size = p->a_size) sharing one prepared automorphism key (device or host-resident): every entry (row < res_dnum, col) of `res`
 * (rows = res_dnum <= a_dnum, size = p->res_size) becomes phi_g(glwe_keyswitch(phi_p(a.at(row, col)), key)), p = a_gal (odd),
 * g = p^-1 mod 2N (:77-107).  p->rank_out = p->rank, p->res_base2k = p->a_base2k (asserted by the reference).  res == a with equal
 * layouts is the _assign form.  The Galois element of the result is a_gal * key_gal mod 2N (res.set_p, :110): the applying key's own
 * element takes no part in the arithmetic, the bindings return the product. */
int pz_glwe_automorphism_key_automorphism_batched(pz_module* m, int64_t* res, size_t res_dnum, const int64_t* a, size_t a_dnum,
                                                  int64_t a_gal, const double* key_pmat, const pz_glwe_op_params* p, size_t count);
/* CoreImpl ggsw_keyswitch / _assign (poulpy-core/src/keyswitching/ggsw.rs:37-85) on `count` contiguous device GGSWs (MatZnx layout,
 * rows = dnum, cols_in = cols_out = rank+1): entries (row, 0) go through glwe_keyswitch (:52-54, :80-82; kp describes that key
 * switch, a's GLWE layout -> res's), then pz_ggsw_expand_row_batched on res (tsk_pmat, tp: its arguments).  res == a with equal
 * layouts is the _assign form. */
int pz_ggsw_keyswitch_batched(pz_module* m, int64_t* res, const int64_t* a, size_t dnum, const double* key_pmat,
                              const double* const* tsk_pmat, const pz_glwe_op_params* kp, const pz_glwe_op_params* tp, size_t count);
/* CoreImpl ggsw_automorphism / _assign (poulpy-core/src/automorphism/ggsw_ct.rs:32-82): the same with glwe_automorphism (PZ_AUTO,
 * gal = key.p(); :54-56, :77-79) on the entries (row, 0), row < res_dnum <= a_dnum. */
int pz_ggsw_automorphism_batched(pz_module* m, int64_t* res, size_t res_dnum, const int64_t* a, size_t a_dnum, const double* key_pmat,
                                 int64_t gal, const double* const* tsk_pmat, const pz_glwe_op_params* kp, const pz_glwe_op_params* tp,
                                 size_t count);
/* ---- convolution family (BASELINE configs[4], CKKS tensoring) ----------------------------- *
 * Bivariate convolution over Z[X, Y]/(X^N + 1), Y = 2^-base2k (poulpy-hal/src/api/convolution.rs; reference
 * poulpy-cpu-ref/src/reference/fft64/convolution.rs).  CnvPVecL / CnvPVecR (ScalarPrep = f64) are opaque prepared operands of
 * n * cols * size scalars (module.rs:66-73), passed as (ptr, cols, size); in this backend polynomial (col, limb) is its spectrum
 * in device order at (col*size + limb)*n.  Host or device pointers, like every per-op entry point.
 * cnv_apply_dft: res limb k (k < min(res_size, a_size + b_size - 1)) = sum_j a[k + offset - j] * b[j], offset = min(cnv_offset,
 * a_size + b_size - 1); the other limbs of column res_col are zeroed.  NOTE: the reference's FFT64 implementation stores the
 * product at the raw start of `res` (convolution.rs:232, :251), i.e. it is only meaningful for a one-column res with
 * res_col = 0, which is what every caller passes; this backend writes column res_col of a res with any number of columns. */
/* hal_impl.rs:670 */
size_t pz_cnv_prepare_left_tmp_bytes(const pz_module* m, size_t res_size, size_t a_size);
/* hal_impl.rs:672 cnv_prepare_left: DFT of every limb of every column; `mask` is ANDed into the coefficients of the last active
 * limb min(res_size, a_size) - 1 (convolution.rs:56-61); limbs beyond it are zero */
int pz_cnv_prepare_left(pz_module* m, double* res, size_t res_cols, size_t res_size,
                        const int64_t* a, size_t a_cols, size_t a_size, int64_t mask);
/* hal_impl.rs:677, :679 */
size_t pz_cnv_prepare_right_tmp_bytes(const pz_module* m, size_t res_size, size_t a_size);
int pz_cnv_prepare_right(pz_module* m, double* res, size_t res_cols, size_t res_size,
                         const int64_t* a, size_t a_cols, size_t a_size, int64_t mask);
/* hal_impl.rs:684, :686 */
size_t pz_cnv_apply_dft_tmp_bytes(const pz_module* m, size_t cnv_offset, size_t res_size, size_t a_size, size_t b_size);
size_t pz_cnv_by_const_apply_tmp_bytes(const pz_module* m, size_t cnv_offset, size_t res_size, size_t a_size, size_t b_size);
/* hal_impl.rs:695 cnv_by_const_apply: i64 domain, res (VecZnxBig) limb k = sum_j a[k + offset - j] * b[j] (wrapping), b = b_len constants */
int pz_cnv_by_const_apply(pz_module* m, size_t cnv_offset, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                          const int64_t* a, size_t a_cols, size_t a_size, size_t a_col, const int64_t* b, size_t b_len);
/* hal_impl.rs:709 cnv_apply_dft */
int pz_cnv_apply_dft(pz_module* m, size_t cnv_offset, double* res, size_t res_cols, size_t res_size, size_t res_col,
                     const double* a, size_t a_cols, size_t a_size, size_t a_col,
                     const double* b, size_t b_cols, size_t b_size, size_t b_col);
/* hal_impl.rs:724, :733 cnv_pairwise_apply_dft: (a[i] + a[j]) * (b[i] + b[j]); i == j: a[i] * b[i] */
size_t pz_cnv_pairwise_apply_dft_tmp_bytes(const pz_module* m, size_t cnv_offset, size_t res_size, size_t a_size, size_t b_size);
int pz_cnv_pairwise_apply_dft(pz_module* m, size_t cnv_offset, double* res, size_t res_cols, size_t res_size, size_t res_col,
                              const double* a, size_t a_cols, size_t a_size, const double* b, size_t b_cols, size_t b_size,
                              size_t col_i, size_t col_j);
/* hal_impl.rs:748, :750 cnv_prepare_self: left and right prepared from the same `a` (both (cols, size)) */
size_t pz_cnv_prepare_self_tmp_bytes(const pz_module* m, size_t res_size, size_t a_size);
int pz_cnv_prepare_self(pz_module* m, double* left, double* right, size_t cols, size_t size,
                        const int64_t* a, size_t a_cols, size_t a_size, int64_t mask);

/* GLWE tensoring on `batch` device-resident ciphertext pairs (poulpy-core/src/operations/glwe.rs): PZ_TENSOR_APPLY glwe_tensor_apply
 * :700-807, PZ_TENSOR_APPLY_ADD_ASSIGN glwe_tensor_apply_add_assign :809-913, PZ_TENSOR_SQUARE glwe_tensor_square_apply :609-698
 * (b is ignored).  a / b: batch GLWEs (rank+1 columns, a_size / b_size limbs, one base2k); res: batch GLWETensors =
 * VecZnx((rank+1)(rank+2)/2, res_size), the pair (i, j >= i) in column i*(rank+1) - i*(i+1)/2 + j.  a_effective_k / b_effective_k:
 * the callers' precision in bits (div_ceil(base2k) must equal the size; the bits below it in the bottom limb are masked). */
typedef struct {
    uint64_t rank;
    uint64_t a_size, b_size, ab_base2k;
    uint64_t a_effective_k, b_effective_k;
    uint64_t res_size, res_base2k;
    uint64_t cnv_offset;
} pz_glwe_tensor_params;
enum { PZ_TENSOR_APPLY = 0, PZ_TENSOR_APPLY_ADD_ASSIGN = 1, PZ_TENSOR_SQUARE = 2 };
size_t pz_glwe_tensor_apply_workspace_bytes(const pz_module* m, const pz_glwe_tensor_params* p, int mode, size_t batch);
int pz_glwe_tensor_apply_batched(pz_module* m, int64_t* res, const int64_t* a, const int64_t* b, const pz_glwe_tensor_params* p, int mode,
                                 size_t batch);
/* glwe_tensor_relinearize (operations/glwe.rs:541-607) on `batch` GLWETensors `a` (VecZnx((rank+1)(rank+2)/2, p->a_size)) sharing one
 * prepared tensor key tsk_pmat (GGLWE rank*(rank+1)/2 -> rank: rows = p->dnum, cols_in = rank*(rank+1)/2, cols_out = rank+1,
 * size = p->key_size): the pair columns are key-switched, the first rank+1 columns are added to the big value, res = batch GLWEs
 * (rank+1, p->res_size).  Runs on the fused three-kernel pipeline for dsize = 1 and equal base2k (the configs[4] case). */
int pz_glwe_tensor_relinearize_batched(pz_module* m, int64_t* res, const int64_t* a, const double* tsk_pmat, const pz_glwe_op_params* p,
                                       size_t batch);
/* glwe_tensor_apply (mode PZ_TENSOR_APPLY) or glwe_tensor_square_apply (PZ_TENSOR_SQUARE, b ignored) followed by glwe_tensor_relinearize
 * with the GLWETensor in scratch - poulpy-ckks's ciphertext multiplication / square (poulpy-ckks/src/leveled/default/mul.rs:49-85,
 * :131-170: `tmp` taken from the scratch space, filled by the tensoring, consumed by the relinearization).  tp describes the tensoring
 * (tp->res_size / res_base2k: the tensor), rp the relinearization (rp->a_size = tp->res_size, rp->a_base2k = tp->res_base2k).  Same
 * digits as the two calls above on an i64 tensor; where every digit of the tensor fits 16 bits (one base2k <= 14 throughout, pipeline
 * plans) the tensor only exists as 16-bit copies in the workspace: 2 B per coefficient written and read instead of 8.  Device pointers. */
int pz_glwe_tensor_mul_relinearize_batched(pz_module* m, int64_t* res, const int64_t* a, const int64_t* b, const double* tsk_pmat,
                                           const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, int mode, size_t batch);
/* The same product on operands that sit in larger containers, in place, or joined to res: what poulpy-ckks's ckks_mul_assign /
 * ckks_square_assign (leveled/default/mul.rs:86-200), ckks_mul_add_ct_into / ckks_mul_sub_ct_into and ckks_mul_many
 * (leveled/delegates/composite.rs:239-254, :103-165) need beyond ckks_mul_into (the mapping is poulpy_amd/ckks.py and DESIGN.md 4.6f).
 * tp, rp, mode, tsk_pmat: as above.
 *   Operands.  a_stride / b_stride: limbs per ciphertext of the CONTAINERS of a / b (0: tp->a_size / tp->b_size; never below them).
 *     Ciphertext i of a starts at a + i n cols a_stride and its first tp->a_size limbs are the operand (limbs are outermost inside a
 *     ciphertext, so the limbs a rescale leaves in use are a prefix); b alike; PZ_TENSOR_SQUARE ignores b and b_stride.  The digits are
 *     those of pz_glwe_tensor_mul_relinearize_batched on compacted copies (the reference reallocates there: ckks_compact_limbs,
 *     layouts/ciphertext.rs:216-232; glwe_tensor_apply asserts size == effective_k.div_ceil(base2k), operations/glwe.rs:722-723).
 *   accumulate = 0: res = the product; join, k, sign and normalize are ignored.  res may BE a and / or b: the same pointer, and that
 *     operand's stride equal to rp->res_size (dst = dst a, dst = dst^2).  Only the first pass of a wave reads the operands and every store
 *     to res comes behind it, so at equal strides a wave overwrites exactly what it has read and nothing is staged; at unequal strides a
 *     wave would overwrite ciphertexts that later waves still read, which is refused.  Any other overlap of res with an operand:
 *     PZ_ERR_ALIAS.
 *   accumulate = 1: wave by wave (pz_module_set_chunk) the product - a normalized GLWE of rp->res_size limbs - goes to a segment of the
 *     module's workspace, never to caller memory, and is joined to res while it is hot, with sign = +1 / -1:
 *       PZ_JOIN_PLAIN     res +- product (k must be 0)          PZ_JOIN_LSH_TERM  res +- lsh(product, k)
 *       PZ_JOIN_LSH_ACC   lsh(res, k), then +- product
 *     (ckks_add_assign_unsafe / ckks_sub_assign_unsafe, leveled/default/add.rs:122-146, sub.rs alike).  normalize = 1: the join is
 *     pz_glwe_sum_batched's two-term chain - term 0 res in place, term 1 the product - so glwe_normalize_assign follows (ckks_add_assign /
 *     ckks_sub_assign); normalize = 0: the same two terms through pz_glwe_combine_batched's kernel, un-normalized.  The limits of those
 *     calls hold (a PZ_JOIN_LSH_ACC by a limb or more shifts res in place: 32 limbs at the most).  res must not overlap a or b:
 *     PZ_ERR_ALIAS.  No caller-owned scratch batch: the workspace holds one wave's product.
 * PZ_ERR_INVALID: a stride below the operand's size, accumulate / normalize not 0 or 1, an unknown join, k != 0 on a plain join, a shift
 * out of range, sign not +1 / -1, and whatever pz_glwe_tensor_mul_relinearize_batched refuses.  Nothing is launched on a refusal.
 * Device pointers, 16-byte aligned.  Kernel nodes only: a call repeated with the same arguments is replayed as one HIP graph
 * (pz_module_set_graphs); the buffers' contents may change between calls.  _workspace_bytes: what the call needs of the module's two
 * workspaces for `batch` ciphertexts at the module's chunk setting.
 * (The seven values that describe operands and join are plain arguments, not a struct: the parameter blocks of this header are a fixed list.) */
size_t pz_glwe_tensor_mul_relinearize_acc_workspace_bytes(const pz_module* m, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp,
                                                          int accumulate, int mode, size_t batch);
int pz_glwe_tensor_mul_relinearize_acc_batched(pz_module* m, int64_t* res, const int64_t* a, const int64_t* b, const double* tsk_pmat,
                                               const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, size_t a_stride, size_t b_stride,
                                               int accumulate, int join, size_t k, int sign, int normalize, int mode, size_t batch);
/* The sum of npairs products in ONE GLWETensor, relinearized once - the fast branch of poulpy-ckks's ckks_dot_product_ct
 * (leveled/delegates/composite.rs:671-699).  For every ciphertext index t of the batch: tensor = glwe_tensor_apply(a[0][t], b[0][t]), then
 * glwe_tensor_apply_add_assign(a[i][t], b[i][t]) for i = 1 .. npairs - 1 (operations/glwe.rs:700-917), all with the one tp, then
 * glwe_tensor_relinearize into res[t] (tp, rp, tsk_pmat as for pz_glwe_tensor_mul_relinearize_batched).  The digits are those of npairs calls of
 * pz_glwe_tensor_apply_batched (PZ_TENSOR_APPLY, then PZ_TENSOR_APPLY_ADD_ASSIGN) on one i64 tensor followed by
 * pz_glwe_tensor_relinearize_batched.  The accumulated tensor of a wave (pz_module_set_chunk) lives in the module's workspace and never
 * reaches caller memory; npairs = 1 is pz_glwe_tensor_mul_relinearize_batched.
 *   Operands.  a, b: HOST arrays of npairs device pointers; the same pointer may appear in several pairs.  a_stride / b_stride: host
 *     arrays, per pair the limbs per ciphertext of the CONTAINERS (NULL, or an entry 0: tp->a_size / tp->b_size; never below them):
 *     ciphertext t of pair i starts at a[i] + t n cols a_stride[i] and its first tp->a_size limbs are the operand, b alike.
 *   Aliasing.  res must not overlap any of the 2 npairs operand ranges: PZ_ERR_ALIAS.
 *   The accumulated tensor.  Everywhere: an i64 tensor, the two calls above as they are.  Where the one-call product keeps its tensor as
 *     16-bit digits (one base2k <= 14 throughout, pipeline plans) AND every accumulated value provably fits an int16 - a pairwise column
 *     holds pair - d_i - d_j, three digits, so npairs 3 2^(base2k-1) <= 2^15 - 1: 5 pairs at base2k 12, 2 at 13 - pair 0 goes straight into
 *     the accumulated 16-bit tensor, the others into term tensors that one streaming kernel adds to it, four per launch.
 * PZ_ERR_INVALID: npairs = 0 or above 64, a stride below the operand's size, and whatever pz_glwe_tensor_mul_relinearize_batched refuses.
 * Nothing is launched on a refusal.  Device pointers, 16-byte aligned.  Kernel nodes only: a call repeated with the same arguments (every
 * pointer and stride of every pair) is replayed as one HIP graph; the buffers' contents may change between calls.  _workspace_bytes: what
 * the call needs of the module's two workspaces for `batch` ciphertexts at the module's chunk setting.
 * (Plain arguments, not a struct: the parameter blocks of this header are a fixed list.) */
size_t pz_glwe_tensor_dot_relinearize_workspace_bytes(const pz_module* m, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp,
                                                      size_t npairs, size_t batch);
int pz_glwe_tensor_dot_relinearize_batched(pz_module* m, int64_t* res, const int64_t* const* a, const int64_t* const* b, size_t npairs,
                                           const size_t* a_stride, const size_t* b_stride, const double* tsk_pmat,
                                           const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, size_t batch);

/* GLWE x plaintext polynomial on `batch` device-resident ciphertexts (poulpy-core/src/operations/glwe.rs): PZ_MUL_PLAIN glwe_mul_plain
 * :184-248, PZ_MUL_PLAIN_ASSIGN glwe_mul_plain_assign :250-303.  The tensor params are reused: a / res = batch GLWEs
 * VecZnx(rank+1, a_size | res_size), pt = VecZnx(1, b_size) with b_effective_k (bottom limbs of both operands masked), one base2k
 * ab_base2k for the operands; each column is normalized to res_base2k with cnv_offset_lo.  pt_shared != 0: one plaintext for the whole
 * batch, else one per ciphertext.  PZ_MUL_PLAIN_ASSIGN: res is the operand (a NULL or == res; a_size = res_size, res_base2k =
 * ab_base2k, a_effective_k = the operand's).  Device pointers; res aliases neither pt nor (PZ_MUL_PLAIN) a. */
enum { PZ_MUL_PLAIN = 0, PZ_MUL_PLAIN_ASSIGN = 1 };
size_t pz_glwe_mul_plain_workspace_bytes(const pz_module* m, const pz_glwe_tensor_params* p, int mode, int pt_shared, size_t batch);
int pz_glwe_mul_plain_batched(pz_module* m, int64_t* res, const int64_t* a, const int64_t* pt, int pt_shared, const pz_glwe_tensor_params* p,
                              int mode, size_t batch);
/* GLWE x constant, one constant for the whole batch: PZ_MUL_CONST glwe_mul_const (operations/glwe.rs:66-96), PZ_MUL_CONST_ASSIGN
 * glwe_mul_const_assign (:98-133: res_big has res_size limbs; a NULL or == res, a_size = res_size, a_base2k = res_base2k).  re / im:
 * HOST arrays of b_size digits, either may be NULL.  re alone: the poulpy-core call itself; with im, or with neither, poulpy-ckks's
 * complex constant (leveled/default/mul.rs:342-415): re product, im product normalized then times X^{N/2}, the two added without
 * renormalization; neither: res = 0.  Device pointers for res / a. */
typedef struct {
    uint64_t rank;
    uint64_t a_size, a_base2k;
    uint64_t res_size, res_base2k;
    uint64_t cnv_offset;
} pz_glwe_mul_const_params;
enum { PZ_MUL_CONST = 0, PZ_MUL_CONST_ASSIGN = 1 };
int pz_glwe_mul_const_batched(pz_module* m, int64_t* res, const int64_t* a, const int64_t* re, const int64_t* im, size_t b_size,
                              const pz_glwe_mul_const_params* p, int mode, size_t batch);

/* GLWE linear combination on `batch` device-resident ciphertexts, one pass over HBM (the CKKS linear operations of poulpy-ckks
 * leveled/default/{add,sub,neg,pow2,rescale}.rs; the mapping is poulpy_amd/ckks.py and DESIGN.md 4.6c).  res = batch GLWEs
 * VecZnx(res_cols, res_size), overwritten with the terms applied in order to a zero container, column by column:
 *   PZ_TERM_RAW  res += sign * a (limbs as stored, 0 past a_size: vec_znx_add_into / sub / add_assign / negate); k must be 0
 *   PZ_TERM_LSH  vec_znx_lsh_add_into (sign +1) / vec_znx_lsh_sub (-1) of a by k bits (poulpy-cpu-ref vec_znx/shift.rs:68-180)
 *   PZ_TERM_RSH  vec_znx_rsh_add_into / vec_znx_rsh_sub of a by k bits (shift.rs:245-...): adds the shifted digits and renormalizes
 *                the limbs of res above them with the shift's carry, so it depends on the terms before it
 * then, with normalize = 1, vec_znx_normalize_assign(base2k) on every column (glwe_normalize_assign).  operands[t] is term t's
 * operand: batch GLWEs VecZnx(res_cols, a_size) back to back, or one when shared = 1; col0_only = 1: a has ONE column and the term applies to column
 * 0 only (a plaintext).  base2k of a term: 0 or res's (one base2k per call, operations/glwe.rs:1150).  A term may be res itself (same
 * pointer, a_size = res_size, not col0_only / shared): the in-place forms; an in-place LSH then holds at most 32 limbs.  Any other
 * overlap with res: PZ_ERR_ALIAS.  1 to 4 terms.  Device pointers, 16-byte aligned.  No workspace; kernel nodes only. */
enum { PZ_TERM_RAW = 0, PZ_TERM_LSH = 1, PZ_TERM_RSH = 2 };
typedef struct {
    size_t a_size;
    size_t k;
    size_t base2k;
    int kind;
    int sign;
    int col0_only;
    int shared;
} pz_glwe_term;
int pz_glwe_combine_batched(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                            const pz_glwe_term* terms, size_t nterms, int normalize, size_t batch);

/* Weighted sum of `batch` device-resident ciphertexts by constants, one pass over HBM: poulpy-ckks's ckks_mul_add_pt_const_* /
 * ckks_mul_sub_pt_const_* / ckks_dot_product_pt_const_znx (leveled/delegates/composite.rs:290-330, :423-463, :760-784; the mapping is
 * poulpy_amd/ckks.py and DESIGN.md 4.6d).  res = batch GLWEs VecZnx(rank+1, res_size) at base2k.  init = PZ_LINCOMB_INIT_RES: the
 * accumulator starts as res (mul_add / mul_sub); PZ_LINCOMB_INIT_NONE: term 0's product overwrites it and its join is ignored (the dot
 * product).  Term t, in order: the product of operands[t] (batch GLWEs VecZnx(rank+1, a_size[t]) back to back, or one when shared[t]) by
 * the constant re[t] + i im[t] (HOST arrays of b_size[t] digits, either or both NULL) with cnv_offset[t], exactly as
 * pz_glwe_mul_const_batched (PZ_MUL_CONST) writes it into a res_size-limb container; then, with sign[t] = +1 / -1 (ckks_add_assign_unsafe
 * / ckks_sub_assign_unsafe, leveled/default/add.rs:122-146):
 *   PZ_JOIN_PLAIN     acc +- product (k[t] must be 0)
 *   PZ_JOIN_LSH_TERM  acc +- lsh(product, k[t])                  (glwe_lsh_add / glwe_lsh_sub)
 *   PZ_JOIN_LSH_ACC   lsh(acc, k[t]), then +- product            (glwe_lsh_assign on the running sum)
 * then, with normalize = 1, glwe_normalize_assign; every limb of res is stored once.  Every array has nterms entries.
 * PZ_ERR_INVALID: sizes, shifts or digit counts out of range, nterms = 0 or nterms > 2^(63 - base2k) (ensure_accumulation_fits).
 * PZ_ERR_ALIAS: an operand that overlaps res, unless init = PZ_LINCOMB_INIT_RES and it IS res (same pointer, a_size = res_size, not
 * shared).  PZ_ERR_UNSUPPORTED: more than 64 terms, a_size > 64 or b_size > 32, or
 *   (max_t a_size[t] + s res_size) x (2 if any im[t] is given, else 1) x 128 x 8 bytes > 160 KiB (the workgroup's LDS), with s = 2 if any
 *   join but a dot product's first is not PZ_JOIN_PLAIN, else 1.
 * Nothing is launched on a refusal.  Device pointers for res / operands.  No workspace; inside a graph, kernel nodes only: the constants
 * travel through a module-owned table written in front of the graph, so a repeated call picks up new constants behind the same arguments. */
enum { PZ_LINCOMB_INIT_NONE = 0, PZ_LINCOMB_INIT_RES = 1 };
enum { PZ_JOIN_PLAIN = 0, PZ_JOIN_LSH_TERM = 1, PZ_JOIN_LSH_ACC = 2 };
int pz_glwe_lincomb_const_batched(pz_module* m, int64_t* res, size_t rank, size_t res_size, size_t base2k, const int64_t* const* operands,
                                  const int* shared, const size_t* a_size, const size_t* cnv_offset, const int64_t* const* re,
                                  const int64_t* const* im, const size_t* b_size, const int* join, const size_t* k, const int* sign, size_t nterms,
                                  int init, int normalize, size_t batch);

/* Normalized signed sum of up to 64 device-resident ciphertext batches, one pass over HBM: poulpy-ckks's ckks_add_many
 * (leveled/delegates/composite.rs:63-93) and the join of its dot products (accumulate_unnormalized, :478-506; the mapping is
 * poulpy_amd/ckks.py and DESIGN.md 4.6e).  res = batch GLWEs VecZnx(res_cols, res_size) at base2k, overwritten with the digits of this
 * chain on a zero container acc of res_size limbs.  Term t, in order, with a = operands[t] (batch GLWEs VecZnx(res_cols, a_size[t]) back
 * to back, or one when shared[t]) and sign[t] = +1 / -1:
 *   PZ_JOIN_PLAIN     acc +- a: limbs as stored, 0 past a_size, the first res_size limbs of a longer operand (vec_znx_add_assign /
 *                     sub_assign); k[t] must be 0
 *   PZ_JOIN_LSH_TERM  glwe_lsh_add / glwe_lsh_sub of a by k[t] bits (term 0 of an add_many: glwe_lsh into the zero container)
 *   PZ_JOIN_LSH_ACC   glwe_lsh_assign(acc, k[t]) on the un-normalized running sum, then acc +- a
 * then glwe_normalize_assign, always (the un-normalized forms keep pz_glwe_combine_batched).  Bit-identical to that chain on every input
 * on which none of its steps overflows i64.  Every array has nterms entries.
 * PZ_ERR_INVALID: nterms = 0 or nterms > 2^(63 - base2k) (ensure_accumulation_fits, composite.rs:43-51), sizes or shifts out of range,
 * k != 0 on a plain join.  PZ_ERR_UNSUPPORTED: more than 64 terms.  PZ_ERR_ALIAS: an operand that overlaps res, unless it is term 0 and
 * IS res (same pointer, a_size = res_size, not shared: the partial sum a chunked dot product continues from).  Where a shift - term 0's
 * own or a later PZ_JOIN_LSH_ACC - moves that in-place term by a limb or more, its limbs are staged in the thread's LDS slice, 32 limbs at
 * the most; a longer one is refused with PZ_ERR_ALIAS (pz_glwe_combine_batched has the same limit for an in-place shift: sum into another
 * container instead).
 * Nothing is launched on a refusal.  Device pointers, 16-byte aligned.  No workspace; one launch, a kernel node: the term plans travel in
 * the kernel's arguments. */
int pz_glwe_sum_batched(pz_module* m, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                        const int* shared, const size_t* a_size, const int* join, const size_t* k, const int* sign, size_t nterms, size_t batch);

/* BlindRotationExecute<CGGI>::blind_rotation_execute (poulpy-bin-fhe/src/blind_rotation/algorithms/cggi/algorithm.rs:76-118)
 * on `batch` LWE ciphertexts that share the lookup table and the prepared blind-rotation key:
 *   block_size > 1 : execute_block_binary  (:265-368)       block_size == 1 : execute_standard (:370-440)
 * (extension_factor > 1, execute_block_binary_extended :121-273: pz_blind_rotation_execute_extended_batched below).
 *   res     batch x GLWE(rank+1, res_size), overwritten
 *   lwe_2n  batch x (n_lwe+1) i64: the output of mod_switch_2n (algorithms/mod.rs:136-171, host i64 code that stays in the
 *           caller): [b, a_1 .. a_n_lwe]
 *   lut     VecZnx(1, lut_size), shared                      brk  n_lwe prepared GGSWs (pz_vmp_prepare; rows = dnum,
 *           cols_in = cols_out = rank+1, size = brk_size), contiguous, shared
 * The prepared monomials x_pow_a of BlindRotationKeyPrepared (key_prepared.rs:66-74) are not an argument: in this
 * backend's spectrum order DFT(X^a) is a row of roots of unity and is generated from a 2n-entry table.
 * All pointers are device pointers. */
typedef struct {
    uint64_t rank;
    uint64_t n_lwe;
    uint64_t block_size;
    uint64_t dnum;      /* rows of each GGSW of the key */
    uint64_t brk_size;  /* limbs of the key */
    uint64_t base2k;    /* of res, lut and key (the reference asserts they agree) */
    uint64_t res_size;
    uint64_t lut_size;
} pz_blind_rotation_params;
int pz_blind_rotation_execute_batched(pz_module* m, int64_t* res, const int64_t* lwe_2n, const int64_t* lut, const double* brk,
                                      const pz_blind_rotation_params* p, size_t batch);
size_t pz_blind_rotation_workspace_bytes(const pz_module* m, const pz_blind_rotation_params* p, size_t batch);

/* ---- LWE glue of the gate bootstrap (BASELINE configs[3]: mod switch -> blind rotation -> sample extract / LWE key switch) on
 * device-resident batches.  An LWE is the reference's container VecZnx(n = n_lwe + 1, one column, `size` limbs): limb i =
 * [b, a_0 .. a_{n_lwe-1}] at i * (n_lwe + 1); a batch is `batch` of them back to back.  Device pointers only.
 *
 * mod_switch_2n (poulpy-bin-fhe/src/blind_rotation/algorithms/mod.rs:136-176): res = batch vectors of n_lwe + 1 values, the input
 * of pz_blind_rotation_execute_batched; n2 = 2 * extension_factor * n_glwe; negate != 0 = LookUpTableRotationDirection::Left.
 * Restated literally: base2k > log2n rounds limb 0, otherwise the following limbs are appended (un-negated, as in the reference). */
int pz_lwe_mod_switch_2n_batched(pz_module* m, int64_t* res, const int64_t* lwe, size_t n_lwe, size_t lwe_size, size_t base2k, size_t n2,
                                 int negate, size_t batch);
/* LWESampleExtract::lwe_sample_extract (poulpy-core/src/api/conversion.rs:15-40): coefficient 0 of column 0 and the first
 * res_n_lwe coefficients of column 1 of each GLWE (a_cols columns, a_size limbs); limbs beyond min(res_size, a_size) are zero */
int pz_lwe_sample_extract_batched(pz_module* m, int64_t* res, size_t res_n_lwe, size_t res_size, const int64_t* a, size_t a_cols,
                                  size_t a_size, size_t batch);
/* LWEKeySwitch::lwe_keyswitch (poulpy-core/src/keyswitching/lwe.rs:49-94): embed -> glwe_keyswitch -> sample extract.
 * p: rank = rank_out = 1; a_size / a_base2k = the input LWE's, res_size / res_base2k = the output LWE's; ksk_pmat: the prepared
 * GGLWE (rows = p->dnum, cols_in = 1, cols_out = 2, size = p->key_size), device or host-resident like any prepared key */
int pz_lwe_keyswitch_batched(pz_module* m, int64_t* res, size_t res_n_lwe, const int64_t* a, size_t a_n_lwe, const double* ksk_pmat,
                             const pz_glwe_op_params* p, size_t batch);
/* GLWEFromLWE::glwe_from_lwe (poulpy-core/src/conversion/lwe_to_glwe.rs:46-121): the LWE is embedded into a rank-1 GLWE in the
 * KEY's base with p->a_size = ceil(lwe_size * lwe_base2k / key_base2k) limbs (cross-base: vec_znx_normalize per column, :82-116),
 * then key-switched rank 1 -> p->rank_out.  res = batch GLWEs (rank_out + 1, p->res_size). */
int pz_glwe_from_lwe_batched(pz_module* m, int64_t* res, const int64_t* lwe, size_t n_lwe, size_t lwe_size, size_t lwe_base2k,
                             const double* ksk_pmat, const pz_glwe_op_params* p, size_t batch);
/* LWEFromGLWE::lwe_from_glwe (poulpy-core/src/conversion/glwe_to_lwe.rs:42-90): multiply by X^-a_idx (a_idx != 0), key switch
 * p->rank -> 1 into a GLWE with the LWE's base and size, sample extract.  a = batch GLWEs (p->rank + 1, p->a_size). */
int pz_lwe_from_glwe_batched(pz_module* m, int64_t* res, size_t res_n_lwe, const int64_t* a, size_t a_idx, const double* ksk_pmat,
                             const pz_glwe_op_params* p, size_t batch);
/* lwe_from_glwe of every one of `batch` GLWEs at every one of `nidx` coefficient indices (the bits of FheUint words):
 * one launch chain over all nidx * batch ciphertexts.  Where the one-kernel small-ring key switch serves the shape with every object in
 * the key's base (N = 1024) X^-idx[j] is applied where that kernel reads its source, from a per-ciphertext device table, and
 * the rotated copies are never written; elsewhere ONE table-driven rotation launch writes them.  Then one batched key switch, one
 * fused tail.  Index-major result: LWE (j, b) at res + (j*batch + b) * (res_n_lwe+1) * p->res_size.  Bit-identical to nidx calls of
 * pz_lwe_from_glwe_batched; idx[j] == 0 is no special case.
 *   idx      HOST array of nidx coefficient indices, each < n
 *   res      may be NULL when lwe_2n is given (the LWE limbs are then never written)
 *   lwe_2n   optional: the nidx * batch vectors [b, a_1 .. a_n_lwe] of mod_switch_2n(n2, negate) of the results, in the order of
 *            res, written by the kernel that extracts the sample (base2k = p->res_base2k; n2 / negate as for
 *            pz_lwe_mod_switch_2n_batched); NULL: no mod switch
 *   tmp      device scratch of pz_lwe_from_glwe_many_tmp_bytes */
size_t pz_lwe_from_glwe_many_tmp_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t nidx, size_t batch);
int pz_lwe_from_glwe_many_batched(pz_module* m, int64_t* res, size_t res_n_lwe, const int64_t* a, size_t nidx, const size_t* idx /*HOST*/,
                                  const double* ksk_pmat, const pz_glwe_op_params* p, int64_t* lwe_2n, size_t n2, int negate, void* tmp,
                                  size_t tmp_bytes, size_t batch);
/* ggsw_prepare (poulpy-core GGSWPrepare: vmp_prepare of the GGSW's MatZnx) on `count` contiguous GGSWs, device to device: MatZnx layout
 * in (rows = dnum, cols_in = cols_out = rank+1, `size` limbs), VmpPMat layout out.  The transform of pz_vmp_prepare on one grid over
 * all count * dnum * (rank+1)^2 * size polynomials (one launch pair, or one per workspace chunk): equal as bytes to pz_vmp_prepare on
 * each matrix.  No host-key bookkeeping: both pointers are device pointers, and pmat must not overlap ggsw (PZ_ERR_ALIAS). */
int pz_ggsw_prepare_batched(pz_module* m, double* pmat, const int64_t* ggsw, size_t count, size_t dnum, size_t rank, size_t size);
/* execute_block_binary_extended (algorithm.rs:121-273): extension_factor > 1 (a power of two), block_size > 1.  lwe_2n is the
 * output of mod_switch_2n(2 * n * extension_factor); lut = the extension_factor polynomials lut.data[j], each
 * VecZnx(1, lut_size), contiguous; tmp = device scratch of pz_blind_rotation_extended_tmp_bytes; batch * extension_factor
 * <= 65535 per call.  The reference's skipped updates (:217, :233, :244) are reproduced. */
size_t pz_blind_rotation_extended_tmp_bytes(const pz_module* m, const pz_blind_rotation_params* p, size_t extension_factor, size_t batch);
int pz_blind_rotation_execute_extended_batched(pz_module* m, int64_t* res, const int64_t* lwe_2n, const int64_t* lut, const double* brk,
                                               const pz_blind_rotation_params* p, size_t extension_factor, void* tmp, size_t tmp_bytes,
                                               size_t batch);
/* CircuitBootstrappingExecute::circuit_bootstrapping_execute_to_constant (poulpy-bin-fhe/src/circuit_bootstrapping/
 * circuit.rs:177-195, core :219-370 with to_exponent = false) on `batch` LWE ciphertexts -> `batch` contiguous GGSWs
 * (MatZnx layout, rows = res_dnum, cols_in = cols_out = rank+1, size = res_size), for the case the reference's own
 * benchmark runs (poulpy-bench bench_suite/schemes/circuit_bootstrapping.rs: one base2k for the blind-rotation key, the
 * automorphism keys, the tensor keys and the result) and the one its tests run (a base2k per object: the fields at the end of
 * the params).  execute_to_exponent (:197-216) with
 * log_gap_in == log_gap_out is the same call with the step list of the partial trace (post_process :418-420: steps
 * log_n - log_gap_in + 1 .. log_n) and the table / mod-switch direction the shim builds for that mode (:276-301);
 * pz_circuit_bootstrapping_execute_to_exponent_batched below does that mapping and the repacking branch (:392-417).
 *   lwe_2n, lut, brk   as for pz_blind_rotation_execute_batched (the shim builds the table with the reference's host code
 *                      lookup_table.rs and passes gap = 2*lut.drift/extension_factor, circuit.rs:333)
 *   gals / atk_pmats   HOST arrays, one per trace step skip..log_n (as for pz_glwe_trace_batched; skip = 0 in constant mode): prepared automorphism keys
 *                      (rank -> rank, rows = atk_dnum, size = atk_size)
 *   tsk_pmats          HOST array of rank prepared tensor keys tsk.at(c) (rows = tsk_dnum, size = tsk_size)
 *   tmp                device scratch of pz_circuit_bootstrapping_tmp_bytes (the reference's `scratch`, circuit.rs:149-175) */
typedef struct {
    pz_blind_rotation_params br; /* res_size = limbs of the GLWE the rotation produces (brk layout = atk layout) */
    uint64_t atk_dnum, atk_size;
    uint64_t tsk_dnum, tsk_size;
    uint64_t res_dnum, res_size; /* the output GGSW */
    uint64_t gap;
    uint64_t extension_factor;   /* 0 or 1: execute_block_binary / execute_standard; > 1: the extended rotation (lut = that many
                                    polynomials, lwe_2n switched to 2*n*extension_factor, gap as circuit.rs:333 computes it) */
    /* One base2k per object, as the reference's own tests run it (circuit_bootstrapping/tests/circuit_bootstrapping.rs:49-53: result 15,
     * blind-rotation key 13, automorphism keys 11, tensor keys 12); br.base2k is the blind-rotation key's.  0 = br.base2k. */
    uint64_t atk_base2k, tsk_base2k, res_base2k;
    uint64_t atk_glwe_size;      /* limbs of the rotated GLWE re-expressed in the automorphism keys' base (circuit.rs:311-331:
                                    ceil(brk.max_k / atk_base2k)); 0 = br.res_size */
    uint64_t trace_size;         /* limbs of glwe_trace's temporary (glwe_trace.rs:107-112: ceil(max(brk.max_k, res.max_k) / atk_base2k));
                                    0 = max(atk_glwe_size, res_size), which is that value when the bases are equal */
} pz_circuit_bootstrapping_params;
size_t pz_circuit_bootstrapping_tmp_bytes(const pz_module* m, const pz_circuit_bootstrapping_params* p, size_t batch);
int pz_circuit_bootstrapping_execute_to_constant_batched(pz_module* m, int64_t* ggsw, const int64_t* lwe_2n, const int64_t* lut,
                                                         const double* brk, size_t nsteps, const int64_t* gals,
                                                         const double* const* atk_pmats, const double* const* tsk_pmats,
                                                         const pz_circuit_bootstrapping_params* p, void* tmp, size_t tmp_bytes,
                                                         size_t batch);
/* circuit_bootstrapping_execute_to_exponent (circuit.rs:197-216, post_process :373-421), same conventions; gals / atk_pmats
 * cover ALL log2(n) trace steps; log_gap_in = bits(gap * next_pow2(res_dnum) - 1) (circuit.rs:342) comes from the shim.
 * log_gap_in == log_gap_out: the partial trace (:418-420); otherwise the repacking branch (:392-417: 2^log_domain shifted
 * copies + glwe_pack), which needs res_size <= br.res_size and the larger scratch of *_to_exponent_tmp_bytes. */
size_t pz_circuit_bootstrapping_to_exponent_tmp_bytes(const pz_module* m, const pz_circuit_bootstrapping_params* p, size_t log_domain,
                                                      size_t batch);
int pz_circuit_bootstrapping_execute_to_exponent_batched(pz_module* m, int64_t* ggsw, const int64_t* lwe_2n, const int64_t* lut,
                                                         const double* brk, const int64_t* gals, const double* const* atk_pmats,
                                                         const double* const* tsk_pmats, const pz_circuit_bootstrapping_params* p,
                                                         size_t log_gap_in, size_t log_gap_out, size_t log_domain, void* tmp,
                                                         size_t tmp_bytes, size_t batch);
/* FheUintPrepared::prepare (poulpy-bin-fhe/src/bdd_arithmetic/ciphertexts/fhe_uint_prepared.rs:399-460, fhe_uint_prepare_custom) on
 * `batch` FheUint words: each word is one GLWE (rank+1 columns, ks_glwe.a_size limbs, or ks_lwe.a_size without ks_glwe) carrying bit i
 * at coefficient bit_index(i) << log_gap, bit_index(i) = ((i & 7) << log2(word_bits / 8)) | (i >> 3), log_gap = log2(n / word_bits)
 * (bdd_arithmetic/mod.rs:97-99, fhe_uint.rs:384).  Per bit i in [bit_start, bit_start + bit_count), in the reference's order:
 *   get_bit_lwe (fhe_uint.rs:369-399): [glwe_keyswitch by ks_glwe] -> X^-coefficient -> glwe_keyswitch by ks_lwe -> sample extract
 *   mod_switch_2n(2 n, negated: constant mode keeps the table's default direction, Left) -> circuit bootstrapping to constant
 *   (log_domain = 1, extension_factor = 1) -> ggsw_prepare
 * The reference runs the ks_glwe key switch once per BIT on the same word; it is deterministic, so this call runs it ONCE PER WORD and
 * takes every bit from that one result - the outputs are the same bits.  Bits outside the range are zeroed (ggsw_zero, :453-459).
 *   words         batch GLWEs
 *   ks_glwe_pmat  may be NULL; else the rank -> ks_glwe.rank_out key switch of fhe_uint.rs:385-394 (ks_glwe.res_* = the intermediate:
 *                 the LWE key's base, k = min(ks_lwe.max_k, word.max_k)); then ks_lwe.rank = ks_glwe.rank_out and ks_lwe.a_* = ks_glwe.res_*
 *   ks_lwe_pmat   the rank -> 1 key switch of lwe_from_glwe; ks_lwe.res_size / res_base2k = lwe_size / lwe_base2k
 *   lut .. tsk_pmats   exactly as pz_circuit_bootstrapping_execute_to_constant_batched takes them
 *   res_pmat      word-major [batch][word_bits] prepared GGSWs (rows = cbt.res_dnum, cols = cbt.br.rank+1, size = cbt.res_size)
 *   ggsw_out      optional, same order: the unprepared i64 GGSWs       lwe_out   optional: [batch][bit_count] LWEs (n_lwe+1, lwe_size)
 *   tmp           device scratch; pz_fhe_uint_prepare_tmp_bytes(m, p, batch, 0) holds every bit of every word at once,
 *                 (m, p, batch, chunk_bits) the call's fixed part + `chunk_bits` (word, bit) pairs per pass: the call splits
 *                 batch * bit_count into the passes that fit tmp (each at most 65535, the blind rotation's limit).
 * Plain stream launches.  Refused with PZ_ERR_INVALID before anything is launched: a null params / key / table pointer, word_bits
 * not one of the five, n no multiple of it, a bit range that leaves the word, an LWE or key-switch shape that is empty or does not
 * chain (ks_glwe -> ks_lwe -> LWE), limbs that do not reach 2n in mod_switch_2n, a tmp below one pair per pass.  The remaining shape
 * checks of the circuit bootstrapping (its bases, atk_glwe_size, trace_size) and of the key switches are made by those stages
 * themselves: such a call also returns PZ_ERR_INVALID, but the zero fills and the stages in front of the refusing one have run. */
struct pz_fhe_uint_prepare_params {
    pz_circuit_bootstrapping_params cbt;
    pz_glwe_op_params ks_glwe, ks_lwe;
    uint64_t n_lwe, lwe_size, lwe_base2k;
    uint64_t word_bits;           /* 8 / 16 / 32 / 64 / 128; n is a multiple of it */
    uint64_t bit_start, bit_count;
};
typedef struct pz_fhe_uint_prepare_params pz_fhe_uint_prepare_params;
size_t pz_fhe_uint_prepare_tmp_bytes(const pz_module* m, const pz_fhe_uint_prepare_params* p, size_t batch, size_t chunk_bits);
int pz_fhe_uint_prepare_batched(pz_module* m, double* res_pmat, int64_t* ggsw_out, int64_t* lwe_out, const int64_t* words,
                                const double* ks_glwe_pmat, const double* ks_lwe_pmat, const int64_t* lut, const double* brk, size_t nsteps,
                                const int64_t* gals, const double* const* atk_pmats, const double* const* tsk_pmats,
                                const pz_fhe_uint_prepare_params* p, void* tmp, size_t tmp_bytes, size_t batch);
/* FheUint::pack (bdd_arithmetic/ciphertexts/fhe_uint.rs:239-255) on `batch` words: the word_bits single-bit GLWEs of every word become one
 * GLWE with bit i at coefficient bit_index(i) << log_gap, log_gap = log2(n / word_bits).  Bit-identical, on every limb, to
 * pz_glwe_pack_batched (trace_size == 0) / pz_glwe_pack_bases_batched (trace_size >= 1) called with indices[s] = bit_index(s) << log_gap,
 * cts[s] = bits + s * batch * ct, log_gap_out = log_gap.  Every index of the word is occupied, so only the both-present branch of
 * pack_internal (glwe_packing.rs:42-69) runs, and the merges of one level are independent and share one key: each of the log2(word_bits)
 * levels is ONE batch of pairs * batch ciphertexts - a pre-kernel (a X^-t -+ b, halved; the half-difference normalized), one automorphism
 * call, a post-kernel (normalize(a' - automorphism), turned by X^t into the survivor's slot) - and the closing glwe_trace of log_gap steps.
 *   bits        dense slot-major device buffer [word_bits][batch] of GLWEs of p->res_size limbs: slot s = bit s of every word (the evaluator's
 *               `out`).  CLOBBERED: its contents after the call are unspecified
 *   res         the batch packed words
 *   gals / key_pmats   HOST arrays, the log2(n) trace steps and their prepared automorphism keys, as for pz_glwe_pack_batched; every one of
 *               them is used (the first log2(word_bits) by the merges, the others by the trace): a null key or an even element is PZ_ERR_INVALID
 *   p           as for pz_glwe_pack_batched: a_size == res_size, a_base2k == res_base2k, dsize == 1, rank_out == rank
 *   trace_size  0: ciphertexts and keys share one base2k (another key_base2k is PZ_ERR_INVALID); else the keys have their own base and
 *               trace_size is what it is for pz_glwe_pack_bases_batched
 *   word_bits   8 / 16 / 32 / 64 / 128 with n % word_bits == 0; n == word_bits: log_gap = 0, no closing trace
 *   tmp         device scratch of pz_fhe_uint_pack_tmp_bytes: align256(word_bits / 2 * batch * ct) for the half-differences of a level
 *               + align256(batch * n * (rank + 1) * trace_size * 8) for the trace in the keys' base (never below what the general pack takes)
 * res, bits, tmp and the keys are pairwise disjoint: PZ_ERR_ALIAS otherwise.  A refused call launches nothing; batch == 0 is PZ_OK and
 * launches nothing.  Routes: "fhe_uint_pack: by levels (...)" by default; POULPY_DBG_PACK_LEVELS=0 (read per call) sends the call through
 * the general pack, one merge at a time ("fhe_uint_pack: per pair (...)").  On the level route a call repeated with the same arguments is
 * replayed as one HIP graph of kernel nodes (pz_module_set_graphs). */
size_t pz_fhe_uint_pack_tmp_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t word_bits, size_t trace_size, size_t batch);
int    pz_fhe_uint_pack_batched(pz_module* m, int64_t* res, int64_t* bits, size_t word_bits, const int64_t* gals,
                                const double* const* key_pmats, const pz_glwe_op_params* p, size_t trace_size,
                                void* tmp, size_t tmp_bytes, size_t batch);
/* Host only (no module, no device): the merges of level `level` < log2(word_bits) of pz_fhe_uint_pack_batched as 3 words each - the slot of
 * the survivor a, the slot of b, t (the level turns a by X^-t and the survivor back by X^t) - in the order of the survivor's index, the first
 * `cap` of them into pairs3 (may be NULL with cap 0); returns the number of pairs of the level, 0 for a shape or level out of range. */
size_t pz_fhe_uint_pack_level_pairs(size_t n, size_t word_bits, size_t level, uint32_t* pairs3, size_t cap);
/* execute_bdd_circuit_2w_to_1w / _1w_to_1w (bdd_arithmetic/bdd_2w_to_1w.rs:103-136, bdd_1w_to_1w.rs:46-70): the evaluator into a slot buffer
 * [word_bits][batch] carved from tmp, then pz_fhe_uint_pack_batched into res - bit-identical to pz_bdd_circuit_execute_batched (out = that
 * buffer, n_out = word_bits) followed by pz_fhe_uint_pack_batched, under one module lock.
 *   c, bits, nbits, gate_p    exactly the arguments of pz_bdd_circuit_execute_batched (the rows of the one or two prepared words concatenated);
 *                             output_size <= word_bits, slots beyond output_size and zero outputs are zero ciphertexts
 *   gals, atk_pmats, pack_p, trace_size   exactly the arguments of pz_fhe_uint_pack_batched; pack_p->res_size == gate_p->res_size and
 *                             pack_p->res_base2k == gate_p->res_base2k, anything else PZ_ERR_INVALID with nothing launched
 *   tmp    [align256(word_bits * batch * ct) slot buffer][max(evaluator tmp, pack tmp)] (bdd_2w_to_1w.rs:70-74); the query returns the sum
 * The two halves replay as their own HIP graphs, one behind the other (the evaluator's rule holds: on its gathered route a new bits
 * array behind the same arguments is picked up). */
size_t pz_fhe_uint_execute_tmp_bytes(const pz_module* m, const pz_bdd_circuit* c, const pz_glwe_op_params* gate_p,
                                     const pz_glwe_op_params* pack_p, size_t word_bits, size_t trace_size, size_t batch);
int    pz_fhe_uint_execute_batched(pz_module* m, const pz_bdd_circuit* c, int64_t* res, size_t word_bits,
                                   const double* const* bits, size_t nbits, const pz_glwe_op_params* gate_p,
                                   const int64_t* gals, const double* const* atk_pmats, const pz_glwe_op_params* pack_p,
                                   size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch);
/* The byte operations of FheUint (bdd_arithmetic/ciphertexts/fhe_uint.rs:259-524) on `batch` words: get_bit_glwe / get_byte, zero_byte,
 * splice_u8 / splice_u16, sext - the operations that move bytes between words without a bootstrap.  With g = log2(n / word_bits),
 * c(i) = bit_index(i) << g (pz_fhe_uint_bit_coefficient), ts = 3 and tr_s = glwe_trace_assign from step s:
 *   get         res[i][b] = tr_0(X^-c(idx[i]) words[b]) (PZ_WORD_BIT) or tr_ts(X^-c(8 idx[i]) words[b]) (PZ_WORD_BYTE); index-major [nidx][batch],
 *               nidx <= 128, normalized (the trace ends in a normalizing tail).  All bits of a word: the inverse of pz_fhe_uint_pack_batched
 *   zero_byte   res = a - X^r tr_ts(X^-r a), r = c(8 byte)
 *   splice      width 8: res = a with byte dst replaced by byte src of b = a + X^rd (tr_ts(X^-rs b) - tr_ts(X^-rd a)); width 16: bytes
 *               2 dst, 2 dst + 1 from 2 src, 2 src + 1 (dst, src < word_bits / 16), the second splice on the first one's result
 *   sext        in place: the bytes above `byte` become copies of its sign (byte = the last one: PZ_OK, nothing launched)
 * The last three return the reference's limbs, UN-normalized: its rotations, adds and subs are wrapping i64 operations that neither
 * normalize nor carry, and regrouping them around the traces changes no bit.  The traces are not regrouped: each sees exactly the word the
 * reference traces.  The traces an operation needs fall into stages; those of a stage are independent and share their keys, so a stage is one
 * pre-kernel (the rotations into a dense array [item][batch]; with the words in the keys' base also the trace's first one-bit shift), ONE
 * trace call on items * batch ciphertexts, and one closing kernel: 1 stage for a get, zero_byte and splice_u8 (the reference: nidx, 1, 2
 * traces), 2 for splice_u16 (4), 1 + k for sext, k = bytes above `byte` (1 + 2k).
 *   words, a, b, res   `batch` contiguous GLWEs of one layout (p->res_size limbs in base p->res_base2k)
 *   gals / key_pmats   HOST arrays, all log2(n) trace steps and their prepared automorphism keys, as for pz_fhe_uint_pack_batched (the call
 *               takes skip .. log2(n) itself): a null key or an even element is PZ_ERR_INVALID
 *   p           exactly what pz_glwe_trace_batched takes, its form for keys in another base than the words included
 *   tmp         device scratch of pz_fhe_uint_word_op_tmp_bytes (max_items: nidx of a get, anything up to 128 otherwise): six ciphertext
 *               arrays [batch]; a shorter one is PZ_ERR_INVALID
 * res == a and res == b (whole) and a == b are allowed (every source of a stage is consumed by its pre-kernel before the closing kernel
 * writes); a get's res, and any other overlap among res, a, b, tmp and the keys, is PZ_ERR_ALIAS.  word_bits outside 8 / 16 / 32 / 64 / 128,
 * n % word_bits != 0, an index out of range, a width other than 8 or 16: PZ_ERR_INVALID.  A refused call launches nothing; batch == 0 and
 * nidx == 0 are PZ_OK and launch nothing.  Routes: "fhe_uint_word: by stages (...)" by default, replayed as one HIP graph of kernel nodes
 * when repeated with the same arguments; POULPY_DBG_WORD_STAGES=0 (read per call) takes the reference's literal order - one rotation, one
 * trace, one add or sub at a time, plain launches ("fhe_uint_word: literal (...)"), byte for byte the same result. */
enum { PZ_WORD_BIT = 0, PZ_WORD_BYTE = 1 };
size_t pz_fhe_uint_word_op_tmp_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t word_bits, size_t max_items, size_t batch);
int    pz_fhe_uint_get_batched(pz_module* m, int64_t* res, const int64_t* words, size_t word_bits, int unit, size_t nidx, const uint32_t* idx,
                               const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes,
                               size_t batch);
int    pz_fhe_uint_zero_byte_batched(pz_module* m, int64_t* res, const int64_t* a, size_t word_bits, size_t byte, const int64_t* gals,
                                     const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch);
int    pz_fhe_uint_splice_batched(pz_module* m, int64_t* res, const int64_t* a, const int64_t* b, size_t word_bits, size_t width, size_t dst,
                                  size_t src, const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp,
                                  size_t tmp_bytes, size_t batch);
int    pz_fhe_uint_sext_batched(pz_module* m, int64_t* word, size_t word_bits, size_t byte, const int64_t* gals, const double* const* key_pmats,
                                const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch);
/* Host only (no module, no device).  pz_fhe_uint_bit_coefficient: bit_index(bit) << log_gap, (size_t)-1 for a shape or bit out of range.
 * pz_fhe_uint_word_plan: the stages of one operation as plain words - per stage  skip, nitems, nitems x (source, exponent, slot), closing
 * step, its first operand, the slot added, the slot subtracted, r  (sources: 0 a, 1 b, 2 the running word, 3 sext's replicated sign;
 * closing steps: 0 none, 1 res = operand + X^r (T[added] - T[subtracted]), 2 sext's eight-term sum from slot 0 into slot 1; 0xFFFFFFFF: no
 * slot) - the first `cap` of them into words (may be NULL with cap 0); returns their number.  args: the indices of a get, {byte}, or
 * {dst, src}.  *status (may be NULL): PZ_OK, or PZ_ERR_INVALID for what the calls above refuse (0 is returned then; an empty plan is valid). */
enum { PZ_WORD_OP_GET_BIT = 0, PZ_WORD_OP_GET_BYTE = 1, PZ_WORD_OP_ZERO_BYTE = 2, PZ_WORD_OP_SPLICE_U8 = 3, PZ_WORD_OP_SPLICE_U16 = 4,
       PZ_WORD_OP_SEXT = 5 };
size_t pz_fhe_uint_bit_coefficient(size_t n, size_t word_bits, size_t bit);
size_t pz_fhe_uint_word_plan(size_t n, size_t word_bits, uint32_t op, const uint32_t* args, size_t nargs, uint32_t* words, size_t cap,
                             int* status);
/* device workspace the GLWE-level calls reserve for `batch` ciphertexts, for the pipeline the call will actually take (fused
 * three-kernel or five-kernel) incl. the growth slack of the module's grow-only arena; keyswitch: 0 external product, 1 key switch,
 * 2 automorphism family, 3 tensor relinearization */
size_t pz_glwe_op_workspace_bytes(const pz_module* m, const pz_glwe_op_params* p, size_t batch, int keyswitch);
/* Optional: declare a prepared key (device pointer from pz_vmp_prepare) immutable until unpinned.  The batched calls
 * above then reuse a row-sliced copy built once here instead of rebuilding it per call (+~3 % at the metric shape,
 * costs one extra copy of the key in HBM).  Modifying a pinned key without unpinning it first is a caller error. */
int pz_module_pin_key(pz_module* m, const double* pmat, size_t rows, size_t cols_in, size_t cols_out, size_t size);
int pz_module_unpin_key(pz_module* m, const double* pmat);
/* drops the device mirror of a host-resident prepared key (see "Conventions" above); unknown pointers are ignored */
int pz_module_forget_host_key(pz_module* m, const double* host_pmat);
/* number of host-resident prepared keys currently mirrored on the device (diagnostic) */
size_t pz_module_host_key_mirrors(pz_module* m);
/* Tuning knob: number of ciphertexts pushed through the three-kernel pipeline per
 * wave so that intermediates stay in the 256 MiB Infinity Cache (0 = auto). */
int pz_module_set_chunk(pz_module* m, size_t cts_per_chunk);
/* Kernel-fusion knobs of the batched GLWE ops (both on by default; the unfused path is the per-op one,
 * kept selectable so that tests can compare the two bit for bit). */
int pz_module_set_fusion(pz_module* m, int fuse_tail, int fuse_mid);
/* N = 4096 only: plain external products / key switches with <= 4 key limbs run a two-kernel pipeline (whole polynomials in LDS,
 * the spectra cross HBM once) instead of the three-kernel one; on by default, selectable so that tests can compare the two. */
int pz_module_set_small_path(pz_module* m, int enable);
/* The launch-bound composite calls (pz_blind_rotation_execute_batched, pz_glwe_trace_batched,
 * pz_circuit_bootstrapping_execute_to_constant_batched: hundreds of short kernels per call) are captured into a HIP graph
 * the second time they are issued with the same arguments and replayed as one graph launch afterwards (on by default;
 * the buffers' CONTENTS may change between calls, their addresses and shapes are the key).  pz_module_graph_launches
 * counts the calls served by a graph. */
int pz_module_set_graphs(pz_module* m, int enable);
uint64_t pz_module_graph_launches(const pz_module* m);
/* Diagnostic only: run a subset of the fused pipeline's stages (bit 0 pass 1, bit 1 middle, bit 2 tail); outputs are
 * meaningless unless mask == 7.  Used by tools/dbg to measure stage overlap. */
int pz_module_set_debug_stages(pz_module* m, int mask);

/* batched primitives (device pointers; object b at ptr + b*len(object)) */
int pz_vec_znx_dft_apply_batched(pz_module* m, size_t batch, size_t step, size_t offset,
                                 double* res, size_t res_cols, size_t res_size, size_t res_col,
                                 const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_idft_apply_consume_batched(pz_module* m, size_t batch, void* data, size_t cols, size_t size);
int pz_vmp_apply_dft_to_dft_batched(pz_module* m, size_t batch, double* res, size_t res_cols, size_t res_size,
                                    const double* a, size_t a_cols, size_t a_size,
                                    const double* pmat, size_t rows, size_t cols_in, size_t cols_out, size_t size,
                                    size_t limb_offset);
int pz_vec_znx_big_normalize_batched(pz_module* m, size_t batch,
                                     int64_t* res, size_t res_cols, size_t res_size, size_t res_base2k, int64_t res_offset, size_t res_col,
                                     const int64_t* a, size_t a_cols, size_t a_size, size_t a_base2k, size_t a_col);

/* ---- batched i64 VecZnx family: the limb-wise ops poulpy-core runs between the hot-path calls, on `batch`
 * device-resident containers back to back (object b at ptr + b*n*cols*size) — one launch per limb range instead of one call per
 * ciphertext.  Same semantics as the per-container functions above (hal_impl.rs:59-131, :225, :289, :41, :137, :165). ----------- */
int pz_vec_znx_add_into_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                const int64_t* a, size_t a_cols, size_t a_size, size_t a_col,
                                const int64_t* b, size_t b_cols, size_t b_size, size_t b_col);
int pz_vec_znx_sub_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                           const int64_t* a, size_t a_cols, size_t a_size, size_t a_col,
                           const int64_t* b, size_t b_cols, size_t b_size, size_t b_col);
int pz_vec_znx_add_assign_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                  const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_sub_assign_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                  const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_sub_negate_assign_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                         const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_negate_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                              const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_copy_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                            const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_zero_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col);
int pz_vec_znx_rotate_batched(pz_module* m, size_t batch, int64_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                              const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_normalize_batched(pz_module* m, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_base2k,
                                 int64_t res_offset, size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_base2k,
                                 size_t a_col);
int pz_vec_znx_lsh_batched(pz_module* m, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                           size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_rsh_batched(pz_module* m, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                           size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
/* the accumulating shifts (poulpy-cpu-ref vec_znx/shift.rs): lsh_add_into = vec_znx_lsh::<false> :68-135, lsh_sub :137-180,
 * rsh_add_into = vec_znx_rsh::<false> :245-342, rsh_sub :344-...; limbs the reference leaves alone stay as they are.  One launch of
 * pz_glwe_combine_batched's kernel (RAW(res) + shifted a).  a may be res (same column: the in-place walk; another column: plain read). */
int pz_vec_znx_lsh_add_into_batched(pz_module* m, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                                    size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_lsh_sub_batched(pz_module* m, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                               size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_rsh_add_into_batched(pz_module* m, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                                    size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);
int pz_vec_znx_rsh_sub_batched(pz_module* m, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                               size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col);

/* ---- multi-GPU ---------------------------------------------------------------------------------- *
 * One process per GPU; independent ciphertexts are block-sharded over the ranks by the caller and never exchanged.  The only
 * collective of the path is the broadcast of a prepared evaluation key from the rank that prepared it: RCCL (ncclBroadcast)
 * over xGMI, on the module stream.  RCCL is loaded on first use.  Bootstrap like NCCL: rank 0 obtains an id, every rank
 * receives it out of band (MPI, a file, torch.distributed ...) and calls pz_comm_init_rank. */
size_t pz_comm_unique_id_bytes(void);                 /* 128 */
int pz_comm_available(void);                          /* PZ_OK when RCCL can be loaded in this process (dlopen + symbols); no id drawn, no socket opened */
int pz_comm_unique_id(void* out_id);                  /* ncclGetUniqueId */
int pz_comm_init_rank(pz_module* m, int world_size, int rank, const void* unique_id);
int pz_comm_destroy(pz_module* m);
int pz_comm_rank(const pz_module* m);                 /* -1 without a communicator */
int pz_comm_world_size(const pz_module* m);
/* in-place broadcast of `bytes` bytes of device memory from `root` (64 MiB buckets); asynchronous on the module stream */
int pz_bcast_key(pz_module* m, void* dev_buf, size_t bytes, int root);

/* ---- instrumentation ------------------------------------------------------- */
/* Times `reps` back-to-back launches of the last pipeline's dominant kernel with HIP
 * events on the module stream; bench.py uses pz_event_* to bracket launches. */
int pz_event_create(void** ev);
int pz_event_destroy(void* ev);
int pz_event_record(pz_module* m, void* ev);
int pz_event_elapsed_ms(void* ev0, void* ev1, float* ms); /* synchronises on ev1 */
/* Per-kernel-class timing with HIP events on the module stream (what bench.py's "roofline"
 * object is computed from).  Classes: */
enum {
    PZ_K_FWD_PASS1 = 0, /* i64 -> T      (column pass of the forward transform)        */
    PZ_K_FWD_PASS2 = 1, /* T -> spectrum  (row pass)                                    */
    PZ_K_VMP = 2,       /* vector-matrix product in the DFT domain                      */
    PZ_K_INV_PASS2 = 3, /* spectrum -> T                                                */
    PZ_K_INV_PASS1 = 4, /* T -> i64, round(x/m)                                         */
    PZ_K_NORMALIZE = 5, /* base-2^k carry chain                                         */
    PZ_K_ELEMENTWISE = 6,
    PZ_K_FUSED_MID = 7, /* fused row pass + VMP + inverse row pass                      */
    PZ_K_FUSED_TAIL = 8, /* fused inverse column pass + normalize                       */
    PZ_KCLASS_COUNT = 9
};
int pz_module_set_kernel_timing(pz_module* m, int enable); /* enabling resets the counters */
/* synchronises the stream and returns accumulated launches / milliseconds of one class */
int pz_module_get_kernel_stats(pz_module* m, int kclass, uint64_t* launches, double* total_ms);
const char* pz_kernel_class_name(int kclass);

/* Rounding-margin probe.  While enabled, EVERY kernel that rounds an inverse-FFT value to an integer (the fused tail in all its
 * forms, the per-op inverse pass, the small-ring inverse, the one-kernel blind rotation) records the largest |x - round(x)| it
 * saw; pz_module_get_margin returns that maximum since the probe was last enabled.  0.5 is the point where a rounding flips,
 * the tests assert < 0.05 on every path.  The probed instantiations are separate (slower) kernels: measure with the probe off. */
int pz_module_set_margin_probe(pz_module* m, int enable);
int pz_module_get_margin(pz_module* m, double* max_frac);

/* Which kernel instantiations the hot dispatch sites (middle kernel, fused tail, blind-rotation kernels) have chosen since the last reset, as one
 * "; "-separated string: measurement tools print it next to their numbers. */
int pz_module_dispatch_notes(pz_module* m, char* buf, size_t len, int reset);

/* Debug: workspace guards.  With POULPY_DBG_CANARY=1 in the environment every segment the library carves out of its workspaces is
 * followed by a 256-byte guard that is verified when the API call returns (the process aborts with a message on an overrun; HIP
 * graphs are not used in this mode).  pz_debug_workspace_overrun carves two segments of `bytes` and writes `overrun` bytes past the
 * end of the first one: the self-test of that mechanism (returns PZ_OK when the mode is off: nothing is checked then). */
int pz_debug_workspace_overrun(pz_module* m, size_t bytes, size_t overrun);
/* Bytes of the module's grow-only device workspace as allocated now (0 before the first call that needs one): what the
 * *_workspace_bytes queries bound.  Read it between calls. */
size_t pz_module_workspace_bytes(const pz_module* m);

#ifdef __cplusplus
}
#endif
#endif
