"""ctypes binding of libpoulpy_hip.so + a ``Module`` with poulpy-hal's method names.

Method names / argument order follow the api traits of the reference
(poulpy-hal/src/api/{vec_znx_dft,svp_ppol,vmp_pmat,vec_znx_big}.rs), minus the
``scratch`` argument (the device path keeps its own workspace; the `*_tmp_bytes`
functions still return the reference's sizes).  A non-zero status from the C ABI raises
``PoulpyHipError`` — the Rust shim panics in the same places.

This module NEVER falls back to a CPU implementation: without the shared library or
without a HIP device every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from ctypes import c_double, c_int64, c_uint64, c_void_p

import numpy as np

from . import abi
from .layouts import CnvPVecL, CnvPVecR, MatZnx, ScalarZnx, SvpPPol, VecZnx, VecZnxBig, VecZnxDft, VmpPMat

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpoulpy_hip.so")


class PoulpyHipError(RuntimeError):
    pass


# the parameter structs of include/poulpy_hip.h, under the names tests/, tools/ and bench.py import
GlweOpParams = abi.pz_glwe_op_params
BlindRotationParams = abi.pz_blind_rotation_params
CircuitBootstrappingParams = abi.pz_circuit_bootstrapping_params
FheUintPrepareParams = abi.pz_fhe_uint_prepare_params
GlweTensorParams = abi.pz_glwe_tensor_params
GlweMulConstParams = abi.pz_glwe_mul_const_params
GlweTerm = abi.pz_glwe_term   # one term of pz_glwe_combine_batched

_lib = None
PZ_ABI_VERSION = 4   # pz_abi_version() of include/poulpy_hip.h this mirror was written against


def load_library(path: str | None = None) -> C.CDLL:
    """Load libpoulpy_hip.so (built by ``__graft_entry__.build()``) with every prototype of the header; raises if missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("POULPY_HIP_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise PoulpyHipError(
            f"{p} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (restype, argtypes) in abi.PROTOTYPES.items():
        if hasattr(lib, name):   # a stale build may lack an entry point: the version check names the cause
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    if lib.pz_abi_version() != PZ_ABI_VERSION:   # struct layouts and entry points of this mirror belong to ONE generation of the header
        raise PoulpyHipError(f"{p} has ABI version {lib.pz_abi_version()}, poulpy_amd/hal.py mirrors version {PZ_ABI_VERSION} "
                             "(a stale or variant build: rebuild with __graft_entry__.build())")
    if path is None:
        _lib = lib
    return lib


def _p(arr: np.ndarray):
    return arr.ctypes.data_as(c_void_p)


def _ptrs(ptrs):
    """host array of device pointers (c_void_p or int addresses)"""
    return (c_void_p * len(ptrs))(*[p.value if isinstance(p, c_void_p) else int(p) for p in ptrs])


class DeviceBuffer:
    """A raw HBM allocation owned by a Module (pz_device_alloc)."""

    def __init__(self, module: "Module", nbytes: int):
        self.module, self.nbytes = module, int(nbytes)
        out = c_void_p()
        module._ck(module.lib.pz_device_alloc(module.handle, self.nbytes, C.byref(out)))
        self.ptr = out

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.module._ck(self.module.lib.pz_memcpy_h2d(self.module.handle, self.ptr, _p(arr), arr.nbytes))
        return self

    def download(self, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        src = c_void_p(self.ptr.value + offset_bytes)
        self.module._ck(self.module.lib.pz_memcpy_d2h(self.module.handle, _p(out), src, out.nbytes))
        return out

    def at(self, offset_bytes: int) -> c_void_p:
        return c_void_p(self.ptr.value + int(offset_bytes))

    def free(self):
        if self.ptr is not None and self.ptr.value:
            self.module.lib.pz_device_free(self.module.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Module:
    """``Module<FFT64Hip>`` — poulpy-hal/src/layouts/module.rs:97-189."""

    def __init__(self, n: int, device: int | None = None, lib: C.CDLL | None = None):
        self.lib = lib or load_library()
        h = c_void_p()
        if device is None:
            st = self.lib.pz_module_new(n, C.byref(h))
        else:
            st = self.lib.pz_module_new_on_device(n, device, C.byref(h))
        self.handle = h
        self._n = int(n)
        if st != 0:
            self.handle = None
            raise PoulpyHipError(f"pz_module_new({n}) failed [{st}]: {self.lib.pz_last_error().decode()}")

    # -- plumbing -------------------------------------------------------------
    def _ck(self, st: int):
        if st != 0:
            raise PoulpyHipError(f"[{st}] {self.lib.pz_last_error().decode()}")

    def n(self) -> int:
        return self._n

    def sync(self):
        self._ck(self.lib.pz_module_sync(self.handle))

    def clone(self) -> "Module":
        """A sibling for another host thread (pz_module_clone): shares the device tables, owns its stream / workspaces / lock."""
        sib = object.__new__(Module)
        sib.lib, sib._n = self.lib, self._n
        h = c_void_p()
        st = self.lib.pz_module_clone(self.handle, C.byref(h))
        sib.handle = h if st == 0 else None
        if st != 0:
            raise PoulpyHipError(f"pz_module_clone failed [{st}]: {self.lib.pz_last_error().decode()}")
        return sib

    def close(self):
        if self.handle is not None:
            self.lib.pz_module_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def set_chunk(self, cts: int):
        self._ck(self.lib.pz_module_set_chunk(self.handle, cts))

    def set_fusion(self, fuse_tail: bool = True, fuse_mid: bool = True):
        self._ck(self.lib.pz_module_set_fusion(self.handle, int(fuse_tail), int(fuse_mid)))

    def set_small_path(self, enable: bool = True):
        """N = 4096: the two-kernel pipeline (device_small.hpp) on / off (on by default)."""
        self._ck(self.lib.pz_module_set_small_path(self.handle, 1 if enable else 0))

    def set_margin_probe(self, enable: bool):
        self._ck(self.lib.pz_module_set_margin_probe(self.handle, 1 if enable else 0))

    def get_margin(self) -> float:
        out = c_double()
        self._ck(self.lib.pz_module_get_margin(self.handle, C.byref(out)))
        return out.value

    def rounding_margin_of(self, run) -> float:
        """max |x - round(x)| over every value the inverse transforms of `run()` round (0.5 = a wrong limb): one more execution of `run`
        with the probing instantiations of the rounding kernels in the same dispatch (pz_module_set_margin_probe)."""
        self.sync()
        self.set_margin_probe(True)
        try:
            run()
            self.sync()
            return self.get_margin()
        finally:
            self.set_margin_probe(False)

    # the PZ_K_* classes (header order = value order = the `kclass` of pz_module_get_kernel_stats), "fwd_pass1" ... "fused_tail"
    KERNEL_CLASSES = tuple(k[len("PZ_K_"):].lower() for k in abi.CONSTANTS if k.startswith("PZ_K_"))

    def dispatch_notes(self, reset: bool = False) -> str:
        """Kernel instantiations chosen by the hot dispatch sites since the last reset (include/poulpy_hip.h)."""
        buf = C.create_string_buffer(16384)
        self._ck(self.lib.pz_module_dispatch_notes(self.handle, buf, 16384, 1 if reset else 0))
        return buf.value.decode()

    def set_kernel_timing(self, enable: bool):
        self._ck(self.lib.pz_module_set_kernel_timing(self.handle, 1 if enable else 0))

    def kernel_stats(self) -> dict:
        """{class name: (launches, total_ms)} measured with HIP events on the module stream."""
        out = {}
        for k, name in enumerate(self.KERNEL_CLASSES):
            cnt, ms = c_uint64(), c_double()
            self._ck(self.lib.pz_module_get_kernel_stats(self.handle, k, C.byref(cnt), C.byref(ms)))
            out[name] = (cnt.value, ms.value)
        return out

    # -- allocation (api/*Alloc traits) -----------------------------------------
    def vec_znx_dft_alloc(self, cols, size) -> VecZnxDft:
        return VecZnxDft(self._n, cols, size)

    def vec_znx_big_alloc(self, cols, size) -> VecZnxBig:
        return VecZnxBig(self._n, cols, size)

    def svp_ppol_alloc(self, cols) -> SvpPPol:
        return SvpPPol(self._n, cols)

    def vmp_pmat_alloc(self, rows, cols_in, cols_out, size) -> VmpPMat:
        return VmpPMat(self._n, rows, cols_in, cols_out, size)

    def bytes_of_vec_znx_dft(self, cols, size) -> int:
        return self.lib.pz_bytes_of_vec_znx_dft(self._n, cols, size)

    def bytes_of_vmp_pmat(self, rows, cols_in, cols_out, size) -> int:
        return self.lib.pz_bytes_of_vmp_pmat(self._n, rows, cols_in, cols_out, size)

    # -- VecZnxDft (api/vec_znx_dft.rs) -------------------------------------------
    def vec_znx_dft_apply(self, step, offset, res: VecZnxDft, res_col, a: VecZnx, a_col):
        self._ck(self.lib.pz_vec_znx_dft_apply(self.handle, step, offset, _p(res.data), res.cols, res.size, res_col,
                                               _p(a.data), a.cols, a.size, a_col))

    def vec_znx_idft_apply_tmp_bytes(self) -> int:
        return self.lib.pz_vec_znx_idft_apply_tmp_bytes(self.handle)

    def vec_znx_idft_apply(self, res: VecZnxBig, res_col, a: VecZnxDft, a_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_idft_apply(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_idft_apply_tmpa(self, res: VecZnxBig, res_col, a: VecZnxDft, a_col):
        self._ck(self.lib.pz_vec_znx_idft_apply_tmpa(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_idft_apply_consume(self, a: VecZnxDft) -> VecZnxBig:
        self._ck(self.lib.pz_vec_znx_idft_apply_consume(self.handle, _p(a.data), a.cols, a.size))
        return a.into_big()

    def _dft3(self, fn, res, res_col, a, a_col, b, b_col):
        self._ck(fn(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col, _p(b.data), b.cols, b.size, b_col))

    def _dft2(self, fn, res, res_col, a, a_col, *extra):
        self._ck(fn(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col, *extra))

    def vec_znx_dft_add_into(self, res, res_col, a, a_col, b, b_col):
        self._dft3(self.lib.pz_vec_znx_dft_add_into, res, res_col, a, a_col, b, b_col)

    def vec_znx_dft_sub(self, res, res_col, a, a_col, b, b_col):
        self._dft3(self.lib.pz_vec_znx_dft_sub, res, res_col, a, a_col, b, b_col)

    def vec_znx_dft_add_assign(self, res, res_col, a, a_col):
        self._dft2(self.lib.pz_vec_znx_dft_add_assign, res, res_col, a, a_col)

    def vec_znx_dft_add_scaled_assign(self, res, res_col, a, a_col, a_scale):
        self._dft2(self.lib.pz_vec_znx_dft_add_scaled_assign, res, res_col, a, a_col, a_scale)

    def vec_znx_dft_sub_assign(self, res, res_col, a, a_col):
        self._dft2(self.lib.pz_vec_znx_dft_sub_assign, res, res_col, a, a_col)

    def vec_znx_dft_sub_negate_assign(self, res, res_col, a, a_col):
        self._dft2(self.lib.pz_vec_znx_dft_sub_negate_assign, res, res_col, a, a_col)

    def vec_znx_dft_copy(self, step, offset, res, res_col, a, a_col):
        self._ck(self.lib.pz_vec_znx_dft_copy(self.handle, step, offset, _p(res.data), res.cols, res.size, res_col,
                                              _p(a.data), a.cols, a.size, a_col))

    def vec_znx_dft_zero(self, res, res_col):
        self._ck(self.lib.pz_vec_znx_dft_zero(self.handle, _p(res.data), res.cols, res.size, res_col))

    # -- SVP (api/svp_ppol.rs) -------------------------------------------------------
    def svp_prepare(self, res: SvpPPol, res_col, a: ScalarZnx, a_col):
        self._ck(self.lib.pz_svp_prepare(self.handle, _p(res.data), res.cols, res_col, _p(a.data), a.cols, a_col))

    def svp_apply_dft(self, res: VecZnxDft, res_col, a: SvpPPol, a_col, b: VecZnx, b_col):
        self._ck(self.lib.pz_svp_apply_dft(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data),
                                           a.cols, a_col, _p(b.data), b.cols, b.size, b_col))

    def svp_apply_dft_to_dft(self, res: VecZnxDft, res_col, a: SvpPPol, a_col, b: VecZnxDft, b_col):
        self._ck(self.lib.pz_svp_apply_dft_to_dft(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data),
                                                  a.cols, a_col, _p(b.data), b.cols, b.size, b_col))

    def svp_apply_dft_to_dft_assign(self, res: VecZnxDft, res_col, a: SvpPPol, a_col):
        self._ck(self.lib.pz_svp_apply_dft_to_dft_assign(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a_col))

    # -- VMP (api/vmp_pmat.rs) -------------------------------------------------------
    def vmp_prepare_tmp_bytes(self, rows, cols_in, cols_out, size) -> int:
        return self.lib.pz_vmp_prepare_tmp_bytes(self.handle, rows, cols_in, cols_out, size)

    def vmp_prepare(self, res: VmpPMat, a: MatZnx, scratch=None):
        assert (res.rows, res.cols_in, res.cols_out, res.size) == (a.rows, a.cols_in, a.cols_out, a.size)
        self._ck(self.lib.pz_vmp_prepare(self.handle, _p(res.data), _p(a.data), a.rows, a.cols_in, a.cols_out, a.size))

    def vmp_apply_dft_tmp_bytes(self, res_size, a_size, b_rows, b_cols_in, b_cols_out, b_size) -> int:
        return self.lib.pz_vmp_apply_dft_tmp_bytes(self.handle, res_size, a_size, b_rows, b_cols_in, b_cols_out, b_size)

    def vmp_apply_dft(self, res: VecZnxDft, a: VecZnx, b: VmpPMat, scratch=None):
        self._ck(self.lib.pz_vmp_apply_dft(self.handle, _p(res.data), res.cols, res.size, _p(a.data), a.cols, a.size,
                                           _p(b.data), b.rows, b.cols_in, b.cols_out, b.size))

    def vmp_apply_dft_to_dft_tmp_bytes(self, res_size, a_size, b_rows, b_cols_in, b_cols_out, b_size) -> int:
        return self.lib.pz_vmp_apply_dft_to_dft_tmp_bytes(self.handle, res_size, a_size, b_rows, b_cols_in, b_cols_out, b_size)

    def vmp_apply_dft_to_dft(self, res: VecZnxDft, a: VecZnxDft, b: VmpPMat, limb_offset=0, scratch=None):
        self._ck(self.lib.pz_vmp_apply_dft_to_dft(self.handle, _p(res.data), res.cols, res.size, _p(a.data),
                                                  a.cols, a.size, _p(b.data), b.rows, b.cols_in, b.cols_out, b.size,
                                                  limb_offset))

    def vmp_zero(self, res: VmpPMat):
        self._ck(self.lib.pz_vmp_zero(self.handle, _p(res.data), res.rows, res.cols_in, res.cols_out, res.size))

    # -- VecZnxBig (api/vec_znx_big.rs) ------------------------------------------------
    def vec_znx_big_normalize_tmp_bytes(self) -> int:
        return self.lib.pz_vec_znx_big_normalize_tmp_bytes(self.handle)

    def vec_znx_big_normalize(self, res: VecZnx, res_base2k, res_offset, res_col, a: VecZnxBig, a_base2k, a_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_big_normalize(self.handle, _p(res.data), res.cols, res.size, res_base2k, res_offset,
                                                   res_col, _p(a.data), a.cols, a.size, a_base2k, a_col))

    def vec_znx_big_add_small_assign(self, res: VecZnxBig, res_col, a: VecZnx, a_col):
        self._ck(self.lib.pz_vec_znx_big_add_small_assign(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    # -- i64 VecZnx limb-wise family (hal_impl.rs:34-131, :289) ---------------------------------------
    def _znx3(self, fn, res, res_col, a, a_col, b, b_col):
        self._ck(fn(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col, _p(b.data), b.cols, b.size, b_col))

    def _znx2(self, fn, res, res_col, a, a_col):
        self._ck(fn(self.handle, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_add_into(self, res: VecZnx, res_col, a: VecZnx, a_col, b: VecZnx, b_col):
        self._znx3(self.lib.pz_vec_znx_add_into, res, res_col, a, a_col, b, b_col)

    def vec_znx_sub(self, res: VecZnx, res_col, a: VecZnx, a_col, b: VecZnx, b_col):
        self._znx3(self.lib.pz_vec_znx_sub, res, res_col, a, a_col, b, b_col)

    def vec_znx_add_assign(self, res: VecZnx, res_col, a: VecZnx, a_col):
        self._znx2(self.lib.pz_vec_znx_add_assign, res, res_col, a, a_col)

    def vec_znx_sub_assign(self, res: VecZnx, res_col, a: VecZnx, a_col):
        self._znx2(self.lib.pz_vec_znx_sub_assign, res, res_col, a, a_col)

    def vec_znx_sub_negate_assign(self, res: VecZnx, res_col, a: VecZnx, a_col):
        self._znx2(self.lib.pz_vec_znx_sub_negate_assign, res, res_col, a, a_col)

    def vec_znx_negate(self, res: VecZnx, res_col, a: VecZnx, a_col):
        self._znx2(self.lib.pz_vec_znx_negate, res, res_col, a, a_col)

    def vec_znx_copy(self, res: VecZnx, res_col, a: VecZnx, a_col):
        self._znx2(self.lib.pz_vec_znx_copy, res, res_col, a, a_col)

    def vec_znx_negate_assign(self, res: VecZnx, res_col):
        self._ck(self.lib.pz_vec_znx_negate_assign(self.handle, _p(res.data), res.cols, res.size, res_col))

    def vec_znx_zero(self, res: VecZnx, res_col):
        self._ck(self.lib.pz_vec_znx_zero(self.handle, _p(res.data), res.cols, res.size, res_col))

    def vec_znx_normalize_tmp_bytes(self) -> int:
        return self.lib.pz_vec_znx_normalize_tmp_bytes(self.handle)

    def vec_znx_normalize(self, res: VecZnx, res_base2k, res_offset, res_col, a: VecZnx, a_base2k, a_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_normalize(self.handle, _p(res.data), res.cols, res.size, res_base2k, res_offset,
                                               res_col, _p(a.data), a.cols, a.size, a_base2k, a_col))

    def vec_znx_normalize_assign(self, base2k, res: VecZnx, res_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_normalize_assign(self.handle, base2k, _p(res.data), res.cols, res.size, res_col))

    def vec_znx_lsh(self, base2k, k, res: VecZnx, res_col, a: VecZnx, a_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_lsh(self.handle, base2k, k, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_rsh(self, base2k, k, res: VecZnx, res_col, a: VecZnx, a_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_rsh(self.handle, base2k, k, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_lsh_assign(self, base2k, k, res: VecZnx, res_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_lsh_assign(self.handle, base2k, k, _p(res.data), res.cols, res.size, res_col))

    # -- X -> X^p on i64 containers (hal_impl.rs:236-243, :517-524) ----------------------------
    def vec_znx_automorphism(self, p: int, res: VecZnx, res_col, a: VecZnx, a_col):
        self._ck(self.lib.pz_vec_znx_automorphism(self.handle, p, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_automorphism_assign(self, p: int, res: VecZnx, res_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_automorphism_assign(self.handle, p, _p(res.data), res.cols, res.size, res_col))

    def vec_znx_automorphism_assign_tmp_bytes(self) -> int:
        return self.lib.pz_vec_znx_automorphism_assign_tmp_bytes(self.handle)

    def vec_znx_big_automorphism(self, p: int, res: VecZnxBig, res_col, a: VecZnxBig, a_col):
        self._ck(self.lib.pz_vec_znx_big_automorphism(self.handle, p, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_big_automorphism_assign(self, p: int, res: VecZnxBig, res_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_big_automorphism_assign(self.handle, p, _p(res.data), res.cols, res.size, res_col))

    def vec_znx_big_automorphism_assign_tmp_bytes(self) -> int:
        return self.lib.pz_vec_znx_big_automorphism_assign_tmp_bytes(self.handle)

    def vec_znx_rotate(self, k: int, res: VecZnx, res_col, a: VecZnx, a_col):
        """hal_impl.rs:225: res = X^k * a."""
        self._ck(self.lib.pz_vec_znx_rotate(self.handle, k, _p(res.data), res.cols, res.size, res_col, _p(a.data), a.cols, a.size, a_col))

    def vec_znx_rotate_assign(self, k: int, res: VecZnx, res_col, scratch=None):
        self._ck(self.lib.pz_vec_znx_rotate_assign(self.handle, k, _p(res.data), res.cols, res.size, res_col))

    def vec_znx_rsh_assign(self, base2k: int, k: int, res: VecZnx, res_col, scratch=None):
        """hal_impl.rs:217 (reference/vec_znx/shift.rs:186-243)."""
        self._ck(self.lib.pz_vec_znx_rsh_assign(self.handle, base2k, k, _p(res.data), res.cols, res.size, res_col))

    def glwe_trace_batched(self, res: c_void_p, gals, key_ptrs, params: GlweOpParams, batch: int):
        """poulpy-core glwe_trace.rs:129-176 on device-resident ciphertexts: gals[s] / key_ptrs[s] (device pointers) per step."""
        ns = len(gals)
        g = (c_int64 * ns)(*[int(x) for x in gals])
        ptrs = _ptrs(key_ptrs)
        self._ck(self.lib.pz_glwe_trace_batched(self.handle, res, ns, g, ptrs, C.byref(params), batch))

    # -- batched device-resident GLWE ops (CoreImpl overrides) ---------------------------
    AUTO_MODES = {"automorphism": abi.PZ_AUTO, "add": abi.PZ_AUTO_ADD, "sub": abi.PZ_AUTO_SUB, "sub_negate": abi.PZ_AUTO_SUB_NEGATE}

    def glwe_automorphism_batched(self, res: c_void_p, a: c_void_p, key_pmat: c_void_p, params: GlweOpParams, gal: int, mode, batch: int):
        """poulpy-core automorphism/glwe_ct.rs:51-275; mode: "automorphism" | "add" | "sub" | "sub_negate"."""
        mode = self.AUTO_MODES[mode] if isinstance(mode, str) else int(mode)
        self._ck(self.lib.pz_glwe_automorphism_batched(self.handle, res, a, key_pmat, C.byref(params), gal, mode, batch))

    def glwe_automorphism_many_batched(self, res: c_void_p, a: c_void_p, gals, key_ptrs, params: GlweOpParams, batch: int):
        """One batch rotated by many Galois elements (glwe_automorphism, glwe_ct.rs:51-72, per element): gals[r] / key_ptrs[r] (device
        pointers) per rotation; rotation r of ciphertext b is ciphertext r * batch + b of res.  res must not overlap a."""
        nr = len(gals)
        g = (c_int64 * max(nr, 1))(*[int(x) for x in gals])
        ptrs = _ptrs(key_ptrs) if len(key_ptrs) else (c_void_p * 1)()
        self._ck(self.lib.pz_glwe_automorphism_many_batched(self.handle, res, a, nr, g, ptrs, C.byref(params), batch))

    def glwe_automorphism_many_workspace_bytes(self, params: GlweOpParams, nrot: int, batch: int) -> int:
        return self.lib.pz_glwe_automorphism_many_workspace_bytes(self.handle, C.byref(params), nrot, batch)

    def glwe_cmux_batched(self, res: c_void_p, t, f: c_void_p, ggsw_pmat: c_void_p, params: GlweOpParams, batch: int, *,
                          t_size: int, f_size: int, t_rot: int = 0):
        """poulpy-bin-fhe bdd_arithmetic/eval.rs:524-626: res = normalize((t - f) (x) GGSW + f); params.a_size = limbs of the difference.
        res may be t (cmux_assign) or f (cmux_assign_neg).  t = None: t = X^t_rot f, the step of glwe_blind_rotation_assign."""
        self._ck(self.lib.pz_glwe_cmux_batched(self.handle, res, t, t_size, t_rot, f, f_size, ggsw_pmat, C.byref(params), batch))

    def glwe_cmux_workspace_bytes(self, params: GlweOpParams, batch: int) -> int:
        return self.lib.pz_glwe_cmux_workspace_bytes(self.handle, C.byref(params), batch)

    def glwe_blind_rotation_tmp_bytes(self, params: GlweOpParams, batch: int) -> int:
        return self.lib.pz_glwe_blind_rotation_tmp_bytes(self.handle, C.byref(params), batch)

    def glwe_blind_rotation_batched(self, res: c_void_p, a: c_void_p, bit_ptrs, sign: bool, bit_lsh: int, params: GlweOpParams, tmp: c_void_p,
                                    tmp_bytes: int, batch: int):
        """bdd_arithmetic/blind_rotation.rs:196-264: res = a X^{+-(bits) << bit_lsh} by len(bit_ptrs) CMUX steps; bit_ptrs[i]: the device
        pointer of the prepared GGSW of bit i + bit_rsh.  res may be a.  The GLWE entries of GGSWs are a batch like any other (:45-106)."""
        nb = len(bit_ptrs)
        ptrs = _ptrs(bit_ptrs) if nb else (c_void_p * 1)()
        self._ck(self.lib.pz_glwe_blind_rotation_batched(self.handle, res, a, nb, ptrs, 1 if sign else 0, bit_lsh, C.byref(params), tmp, tmp_bytes,
                                                         batch))

    def glwe_cswap_batched(self, a: c_void_p, b: c_void_p, ggsw_pmat: c_void_p, params: GlweOpParams, batch: int, *, a_size: int, b_size: int):
        """poulpy-bin-fhe bdd_arithmetic/eval.rs:417-461 (one base2k), in place: (a, b) stays under a GGSW of 0 and becomes (b, a) under 1 - one
        external product of b - a, both results from its one big value.  params.a_size = max(a_size, b_size), params.res_size = a_size."""
        self._ck(self.lib.pz_glwe_cswap_batched(self.handle, a, a_size, b, b_size, ggsw_pmat, C.byref(params), batch))

    def glwe_cswap_workspace_bytes(self, params: GlweOpParams, batch: int) -> int:
        return self.lib.pz_glwe_cswap_workspace_bytes(self.handle, C.byref(params), batch)

    def glwe_blind_retrieval_batched(self, slots: c_void_p, nslots: int, bit_ptrs, reverse: bool, params: GlweOpParams, batch: int):
        """bdd_arithmetic/blind_retrieval.rs:195-266 on `batch` vectors of nslots ciphertexts, slot-major [nslots][batch]: slot 0 ends up holding the
        element at the encrypted index (reverse: the network undone); bit_ptrs[i]: the device pointer of the prepared GGSW of bit i + bit_rsh."""
        nb = len(bit_ptrs)
        ptrs = _ptrs(bit_ptrs) if nb else (c_void_p * 1)()
        self._ck(self.lib.pz_glwe_blind_retrieval_batched(self.handle, slots, nslots, nb, ptrs, 1 if reverse else 0, C.byref(params), batch))

    def glwe_blind_retrieval_workspace_bytes(self, params: GlweOpParams, nslots: int, nbits: int, batch: int) -> int:
        return self.lib.pz_glwe_blind_retrieval_workspace_bytes(self.handle, C.byref(params), nslots, nbits, batch)

    # -- BDD circuits (poulpy-bin-fhe bdd_arithmetic/eval.rs:104-305) -------------------------------------------------------
    def bdd_circuit_new(self, circuit) -> c_void_p:
        """pz_bdd_circuit_new: validate and compile `circuit` (poulpy_amd.bdd.Circuit, or anything with input_size and outputs = [(nodes,
        state_size)], a node being (kind, sel, hi, lo)); host only - see bdd_circuit_new below.  Free with bdd_circuit_free."""
        return bdd_circuit_new(circuit, self.lib)

    def bdd_circuit_free(self, handle: c_void_p):
        self.lib.pz_bdd_circuit_free(handle)

    def bdd_circuit_execute_tmp_bytes(self, handle: c_void_p, params: GlweOpParams, batch: int) -> int:
        return self.lib.pz_bdd_circuit_execute_tmp_bytes(self.handle, handle, C.byref(params), batch)

    def bdd_circuit_execute_batched(self, handle: c_void_p, out: c_void_p, n_out: int, bits, params: GlweOpParams, tmp: c_void_p, tmp_bytes: int,
                                    batch: int):
        """ExecuteBDDCircuit on `batch` inputs: out = dense slot-major [n_out][batch]; bits[b][i] = the prepared GGSW of input bit i of input b
        (a pointer, or None where the circuit never selects the bit); every row has the same length nbits >= input_size."""
        nbits = len(bits[0]) if batch else 0
        assert all(len(row) == nbits for row in bits) and len(bits) == batch
        flat = [0 if p is None else (p.value if isinstance(p, c_void_p) else int(p)) or 0 for row in bits for p in row]
        arr = (c_void_p * max(len(flat), 1))(*flat)
        self._ck(self.lib.pz_bdd_circuit_execute_batched(self.handle, handle, out, n_out, arr, nbits, C.byref(params), tmp, tmp_bytes, batch))

    def ggsw_external_product(self, res: c_void_p, a: c_void_p, a_dnum: int, ggsw_pmat: c_void_p, params: GlweOpParams):
        """poulpy-core external_product/ggsw.rs:54-58 on a device-resident GGSW (MatZnx layout)."""
        self._ck(self.lib.pz_ggsw_external_product(self.handle, res, a, a_dnum, ggsw_pmat, C.byref(params)))

    def ggsw_from_gglwe_batched(self, ggsw: c_void_p, a: c_void_p, a_cols_in: int, dnum: int, tsk_pmats, params: GlweOpParams, count: int = 1):
        """conversion/gglwe_to_ggsw.rs:32-61 on `count` contiguous device GGLWEs -> GGSWs."""
        arr = _ptrs(tsk_pmats)
        self._ck(self.lib.pz_ggsw_from_gglwe_batched(self.handle, ggsw, a, a_cols_in, dnum, arr, C.byref(params), count))

    def ggsw_expand_row_batched(self, ggsw: c_void_p, dnum: int, tsk_pmats, params: GlweOpParams, count: int = 1):
        """conversion/gglwe_to_ggsw.rs:116-268 on `count` contiguous device GGSWs, in place; tsk_pmats: rank device pointers."""
        arr = _ptrs(tsk_pmats)
        self._ck(self.lib.pz_ggsw_expand_row_batched(self.handle, ggsw, dnum, arr, C.byref(params), count))

    def glwe_automorphism_key_automorphism_batched(self, res: c_void_p, res_dnum: int, a: c_void_p, a_dnum: int, a_gal: int, key_pmat: c_void_p,
                                                   key_gal: int, params: GlweOpParams, count: int = 1) -> int:
        """automorphism/gglwe_atk.rs:42-155 on `count` contiguous device GGLWEs of Galois element a_gal (res == a: the _assign form); returns
        the Galois element of the result, a_gal * key_gal mod 2N (res.set_p, :110)."""
        self._ck(self.lib.pz_glwe_automorphism_key_automorphism_batched(self.handle, res, res_dnum, a, a_dnum, a_gal, key_pmat, C.byref(params), count))
        return (int(a_gal) * int(key_gal)) % (2 * self.n())

    def ggsw_keyswitch_batched(self, res: c_void_p, a: c_void_p, dnum: int, key_pmat: c_void_p, tsk_pmats, ks_params: GlweOpParams,
                               tsk_params: GlweOpParams, count: int = 1):
        """keyswitching/ggsw.rs:37-85 on `count` contiguous device GGSWs: glwe_keyswitch on the entries (row, 0), then ggsw_expand_row."""
        arr = _ptrs(tsk_pmats)
        self._ck(self.lib.pz_ggsw_keyswitch_batched(self.handle, res, a, dnum, key_pmat, arr, C.byref(ks_params), C.byref(tsk_params), count))

    def ggsw_automorphism_batched(self, res: c_void_p, res_dnum: int, a: c_void_p, a_dnum: int, key_pmat: c_void_p, gal: int, tsk_pmats,
                                  ks_params: GlweOpParams, tsk_params: GlweOpParams, count: int = 1):
        """automorphism/ggsw_ct.rs:32-82 on `count` contiguous device GGSWs: glwe_automorphism on the entries (row, 0), then ggsw_expand_row."""
        arr = _ptrs(tsk_pmats)
        self._ck(self.lib.pz_ggsw_automorphism_batched(self.handle, res, res_dnum, a, a_dnum, key_pmat, gal, arr, C.byref(ks_params),
                                                       C.byref(tsk_params), count))

    def glwe_external_product_batched(self, res: c_void_p, a: c_void_p, ggsw_pmat: c_void_p, params: GlweOpParams, batch: int):
        self._ck(self.lib.pz_glwe_external_product_batched(self.handle, res, a, ggsw_pmat, C.byref(params), batch))

    def glwe_keyswitch_batched(self, res: c_void_p, a: c_void_p, key_pmat: c_void_p, params: GlweOpParams, batch: int):
        self._ck(self.lib.pz_glwe_keyswitch_batched(self.handle, res, a, key_pmat, C.byref(params), batch))

    def blind_rotation_execute_batched(self, res: c_void_p, lwe_2n: c_void_p, lut: c_void_p, brk: c_void_p, params: BlindRotationParams,
                                       batch: int):
        """poulpy-bin-fhe blind_rotation/algorithms/cggi/algorithm.rs:76-118,265-440 on a batch of mod-switched LWE ciphertexts."""
        self._ck(self.lib.pz_blind_rotation_execute_batched(self.handle, res, lwe_2n, lut, brk, C.byref(params), batch))

    def glwe_pack_tmp_bytes(self, params: GlweOpParams, batch: int) -> int:
        return self.lib.pz_glwe_pack_tmp_bytes(self.handle, C.byref(params), batch)

    def glwe_pack_batched(self, res: c_void_p, indices, ct_ptrs, log_gap_out: int, gals, key_ptrs, params: GlweOpParams, tmp: c_void_p,
                          tmp_bytes: int, batch: int):
        """poulpy-core glwe_packing.rs:122-176 on `batch` problems: ct_ptrs[s] -> batch contiguous device GLWEs of index indices[s]."""
        ns = len(indices)
        idx = (c_uint64 * ns)(*[int(i) for i in indices])
        cp = _ptrs(ct_ptrs)
        ng = len(gals)
        g = (c_int64 * ng)(*[int(x) for x in gals])
        kp = _ptrs(key_ptrs)
        self._ck(self.lib.pz_glwe_pack_batched(self.handle, res, ns, idx, cp, log_gap_out, g, kp, C.byref(params), tmp, tmp_bytes, batch))

    def glwe_pack_bases_tmp_bytes(self, params: GlweOpParams, trace_size: int, batch: int) -> int:
        return self.lib.pz_glwe_pack_bases_tmp_bytes(self.handle, C.byref(params), trace_size, batch)

    def glwe_pack_bases_batched(self, res: c_void_p, indices, ct_ptrs, log_gap_out: int, gals, key_ptrs, params: GlweOpParams,
                                trace_size: int, tmp: c_void_p, tmp_bytes: int, batch: int):
        """glwe_pack with the automorphism keys in their own base (poulpy-core test_suite/glwe_packing.rs:40-42)."""
        ns = len(indices)
        idx = (c_uint64 * ns)(*[int(i) for i in indices])
        cp = _ptrs(ct_ptrs)
        ng = len(gals)
        g = (c_int64 * ng)(*[int(x) for x in gals])
        kp = _ptrs(key_ptrs)
        self._ck(self.lib.pz_glwe_pack_bases_batched(self.handle, res, ns, idx, cp, log_gap_out, g, kp, C.byref(params),
                                                     trace_size, tmp, tmp_bytes, batch))

    # -- FheUint words: the evaluator's bits to one word (bdd_arithmetic/ciphertexts/fhe_uint.rs:239-255, bdd_2w_to_1w.rs:103-136) ----------
    def fhe_uint_pack_tmp_bytes(self, params: GlweOpParams, word_bits: int, batch: int, trace_size: int = 0) -> int:
        return self.lib.pz_fhe_uint_pack_tmp_bytes(self.handle, C.byref(params), word_bits, trace_size, batch)

    def fhe_uint_pack_batched(self, res: c_void_p, bits: c_void_p, word_bits: int, gals, key_ptrs, params: GlweOpParams, tmp: c_void_p,
                              tmp_bytes: int, batch: int, trace_size: int = 0):
        """FheUint::pack on `batch` words, level by level: bits = dense slot-major [word_bits][batch] (CLOBBERED), res = the batch words;
        gals / key_ptrs: the log2(n) trace steps and their prepared automorphism keys (None: a null key); trace_size >= 1: the keys have
        their own base2k."""
        g = (c_int64 * max(len(gals), 1))(*[int(x) for x in gals])
        kp = _ptrs([0 if k is None else k for k in key_ptrs]) if len(key_ptrs) else (c_void_p * 1)()
        self._ck(self.lib.pz_fhe_uint_pack_batched(self.handle, res, bits, word_bits, g, kp, C.byref(params), trace_size, tmp, tmp_bytes, batch))

    def fhe_uint_pack_level_pairs(self, word_bits: int, level: int, n: int = None) -> list:
        """Host only: the merges of one level of fhe_uint_pack_batched as (slot of the survivor, slot merged into it, t); [] beyond the last."""
        return fhe_uint_pack_level_pairs(self.n() if n is None else n, word_bits, level, self.lib)

    def fhe_uint_execute_tmp_bytes(self, handle: c_void_p, gate_params: GlweOpParams, pack_params: GlweOpParams, word_bits: int, batch: int,
                                   trace_size: int = 0) -> int:
        return self.lib.pz_fhe_uint_execute_tmp_bytes(self.handle, handle, C.byref(gate_params), C.byref(pack_params), word_bits, trace_size, batch)

    def fhe_uint_execute_batched(self, handle: c_void_p, res: c_void_p, word_bits: int, bits, gate_params: GlweOpParams, gals, key_ptrs,
                                 pack_params: GlweOpParams, tmp: c_void_p, tmp_bytes: int, batch: int, trace_size: int = 0):
        """execute_bdd_circuit_2w_to_1w / _1w_to_1w on `batch` inputs: bits[b][i] as for bdd_circuit_execute_batched, the packed words in res."""
        nbits = len(bits[0]) if batch else 0
        assert all(len(row) == nbits for row in bits) and len(bits) == batch
        flat = [0 if p is None else (p.value if isinstance(p, c_void_p) else int(p)) or 0 for row in bits for p in row]
        arr = (c_void_p * max(len(flat), 1))(*flat)
        g = (c_int64 * max(len(gals), 1))(*[int(x) for x in gals])
        kp = _ptrs([0 if k is None else k for k in key_ptrs]) if len(key_ptrs) else (c_void_p * 1)()
        self._ck(self.lib.pz_fhe_uint_execute_batched(self.handle, handle, res, word_bits, arr, nbits, C.byref(gate_params), g, kp,
                                                      C.byref(pack_params), trace_size, tmp, tmp_bytes, batch))

    # -- FheUint byte operations (bdd_arithmetic/ciphertexts/fhe_uint.rs:259-524) ---------------------------------------------
    def fhe_uint_word_op_tmp_bytes(self, params: GlweOpParams, word_bits: int, batch: int, max_items: int = 1) -> int:
        return self.lib.pz_fhe_uint_word_op_tmp_bytes(self.handle, C.byref(params), word_bits, max_items, batch)

    def _word_keys(self, gals, key_ptrs):
        g = (c_int64 * max(len(gals), 1))(*[int(x) for x in gals])
        kp = _ptrs([0 if k is None else k for k in key_ptrs]) if len(key_ptrs) else (c_void_p * 1)()
        return g, kp

    def fhe_uint_get_batched(self, res: c_void_p, words: c_void_p, word_bits: int, unit: int, idx, gals, key_ptrs, params: GlweOpParams,
                             tmp: c_void_p, tmp_bytes: int, batch: int):
        """get_bit_glwe (unit = abi.PZ_WORD_BIT) / get_byte (PZ_WORD_BYTE) of every word at every index of idx: res = index-major
        [len(idx)][batch], normalized; gals / key_ptrs: all log2(n) trace steps."""
        g, kp = self._word_keys(gals, key_ptrs)
        ix = (C.c_uint32 * max(len(idx), 1))(*[int(i) for i in idx])
        self._ck(self.lib.pz_fhe_uint_get_batched(self.handle, res, words, word_bits, unit, len(idx), ix, g, kp, C.byref(params), tmp, tmp_bytes, batch))

    def fhe_uint_zero_byte_batched(self, res: c_void_p, a: c_void_p, word_bits: int, byte: int, gals, key_ptrs, params: GlweOpParams,
                                   tmp: c_void_p, tmp_bytes: int, batch: int):
        """zero_byte: res = a with byte `byte` zeroed (res == a allowed); un-normalized, as the reference's."""
        g, kp = self._word_keys(gals, key_ptrs)
        self._ck(self.lib.pz_fhe_uint_zero_byte_batched(self.handle, res, a, word_bits, byte, g, kp, C.byref(params), tmp, tmp_bytes, batch))

    def fhe_uint_splice_batched(self, res: c_void_p, a: c_void_p, b: c_void_p, word_bits: int, width: int, dst: int, src: int, gals, key_ptrs,
                                params: GlweOpParams, tmp: c_void_p, tmp_bytes: int, batch: int):
        """splice_u8 (width 8) / splice_u16 (width 16): res = a with byte / half-word dst replaced by byte / half-word src of b (res == a,
        res == b, a == b allowed); un-normalized, as the reference's."""
        g, kp = self._word_keys(gals, key_ptrs)
        self._ck(self.lib.pz_fhe_uint_splice_batched(self.handle, res, a, b, word_bits, width, dst, src, g, kp, C.byref(params), tmp, tmp_bytes, batch))

    def fhe_uint_sext_batched(self, word: c_void_p, word_bits: int, byte: int, gals, key_ptrs, params: GlweOpParams, tmp: c_void_p,
                              tmp_bytes: int, batch: int):
        """sext, in place: the bytes above `byte` become copies of its sign bit."""
        g, kp = self._word_keys(gals, key_ptrs)
        self._ck(self.lib.pz_fhe_uint_sext_batched(self.handle, word, word_bits, byte, g, kp, C.byref(params), tmp, tmp_bytes, batch))

    def set_graphs(self, enable: bool):
        """HIP-graph replay of the launch-bound composite calls (blind rotation, trace, circuit bootstrapping); on by default."""
        self._ck(self.lib.pz_module_set_graphs(self.handle, 1 if enable else 0))

    def graph_launches(self) -> int:
        return int(self.lib.pz_module_graph_launches(self.handle))

    def circuit_bootstrapping_tmp_bytes(self, params: CircuitBootstrappingParams, batch: int) -> int:
        return self.lib.pz_circuit_bootstrapping_tmp_bytes(self.handle, C.byref(params), batch)

    def circuit_bootstrapping_execute_to_constant_batched(self, ggsw: c_void_p, lwe_2n: c_void_p, lut: c_void_p, brk: c_void_p, gals,
                                                          atk_ptrs, tsk_ptrs, params: CircuitBootstrappingParams, tmp: c_void_p,
                                                          tmp_bytes: int, batch: int):
        """poulpy-bin-fhe circuit_bootstrapping/circuit.rs:177-195 (core :219-370, constant mode, one base2k) on a batch of LWEs."""
        ns = len(gals)
        g = (c_int64 * ns)(*[int(x) for x in gals])
        ap = _ptrs(atk_ptrs)
        tp = _ptrs(tsk_ptrs)
        self._ck(self.lib.pz_circuit_bootstrapping_execute_to_constant_batched(self.handle, ggsw, lwe_2n, lut, brk, ns, g, ap, tp,
                                                                               C.byref(params), tmp, tmp_bytes, batch))

    def circuit_bootstrapping_to_exponent_tmp_bytes(self, params: CircuitBootstrappingParams, log_domain: int, batch: int) -> int:
        return self.lib.pz_circuit_bootstrapping_to_exponent_tmp_bytes(self.handle, C.byref(params), log_domain, batch)

    def circuit_bootstrapping_execute_to_exponent_batched(self, ggsw: c_void_p, lwe_2n: c_void_p, lut: c_void_p, brk: c_void_p, gals,
                                                          atk_ptrs, tsk_ptrs, params: CircuitBootstrappingParams, log_gap_in: int,
                                                          log_gap_out: int, log_domain: int, tmp: c_void_p, tmp_bytes: int, batch: int):
        """circuit.rs:197-216 + post_process :373-421 (one base2k); gals / atk_ptrs: all log2(n) trace steps."""
        ns = len(gals)
        g = (c_int64 * ns)(*[int(x) for x in gals])
        ap = _ptrs(atk_ptrs)
        tp = _ptrs(tsk_ptrs)
        self._ck(self.lib.pz_circuit_bootstrapping_execute_to_exponent_batched(
            self.handle, ggsw, lwe_2n, lut, brk, g, ap, tp, C.byref(params), log_gap_in, log_gap_out, log_domain, tmp,
            tmp_bytes, batch))

    def blind_rotation_extended_tmp_bytes(self, params: BlindRotationParams, ext: int, batch: int) -> int:
        return self.lib.pz_blind_rotation_extended_tmp_bytes(self.handle, C.byref(params), ext, batch)

    def blind_rotation_execute_extended_batched(self, res: c_void_p, lwe_2n: c_void_p, lut: c_void_p, brk: c_void_p,
                                                params: BlindRotationParams, ext: int, tmp: c_void_p, tmp_bytes: int, batch: int):
        """algorithm.rs:121-273 (extension_factor > 1): lut = ext contiguous VecZnx(1, lut_size), lwe_2n switched to 2*n*ext."""
        self._ck(self.lib.pz_blind_rotation_execute_extended_batched(self.handle, res, lwe_2n, lut, brk, C.byref(params), ext, tmp, tmp_bytes, batch))

    def blind_rotation_workspace_bytes(self, params: BlindRotationParams, batch: int) -> int:
        return self.lib.pz_blind_rotation_workspace_bytes(self.handle, C.byref(params), batch)

    # -- batched primitives on device pointers (object b at ptr + b * len(object)) ----------------
    def vec_znx_dft_apply_batched(self, batch, step, offset, res: c_void_p, res_cols, res_size, res_col, a: c_void_p, a_cols, a_size, a_col):
        self._ck(self.lib.pz_vec_znx_dft_apply_batched(self.handle, batch, step, offset, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col))

    def vec_znx_idft_apply_consume_batched(self, batch, data: c_void_p, cols, size):
        self._ck(self.lib.pz_vec_znx_idft_apply_consume_batched(self.handle, batch, data, cols, size))

    def vmp_apply_dft_to_dft_batched(self, batch, res: c_void_p, res_cols, res_size, a: c_void_p, a_cols, a_size, pmat: c_void_p, rows, cols_in,
                                     cols_out, size, limb_offset=0):
        self._ck(self.lib.pz_vmp_apply_dft_to_dft_batched(self.handle, batch, res, res_cols, res_size, a, a_cols, a_size,
                                                          pmat, rows, cols_in, cols_out, size, limb_offset))

    def vec_znx_big_normalize_batched(self, batch, res: c_void_p, res_cols, res_size, res_base2k, res_offset, res_col, a: c_void_p, a_cols,
                                      a_size, a_base2k, a_col):
        self._ck(self.lib.pz_vec_znx_big_normalize_batched(self.handle, batch, res, res_cols, res_size, res_base2k,
                                                           res_offset, res_col, a, a_cols, a_size, a_base2k, a_col))

    # -- convolution family (api/convolution.rs; hal_impl.rs:670-754) --------------------------------------
    def cnv_pvec_left_alloc(self, cols, size) -> CnvPVecL:
        return CnvPVecL(self._n, cols, size)

    def cnv_pvec_right_alloc(self, cols, size) -> CnvPVecR:
        return CnvPVecR(self._n, cols, size)

    def cnv_prepare_left_tmp_bytes(self, res_size, a_size) -> int:
        return self.lib.pz_cnv_prepare_left_tmp_bytes(self.handle, res_size, a_size)

    def cnv_prepare_right_tmp_bytes(self, res_size, a_size) -> int:
        return self.lib.pz_cnv_prepare_right_tmp_bytes(self.handle, res_size, a_size)

    def cnv_prepare_self_tmp_bytes(self, res_size, a_size) -> int:
        return self.lib.pz_cnv_prepare_self_tmp_bytes(self.handle, res_size, a_size)

    def cnv_apply_dft_tmp_bytes(self, cnv_offset, res_size, a_size, b_size) -> int:
        return self.lib.pz_cnv_apply_dft_tmp_bytes(self.handle, cnv_offset, res_size, a_size, b_size)

    def cnv_pairwise_apply_dft_tmp_bytes(self, cnv_offset, res_size, a_size, b_size) -> int:
        return self.lib.pz_cnv_pairwise_apply_dft_tmp_bytes(self.handle, cnv_offset, res_size, a_size, b_size)

    def cnv_by_const_apply_tmp_bytes(self, cnv_offset, res_size, a_size, b_size) -> int:
        return self.lib.pz_cnv_by_const_apply_tmp_bytes(self.handle, cnv_offset, res_size, a_size, b_size)

    def cnv_prepare_left(self, res: CnvPVecL, a: VecZnx, mask: int = -1, scratch=None):
        self._ck(self.lib.pz_cnv_prepare_left(self.handle, _p(res.data), res.cols, res.size, _p(a.data), a.cols, a.size, mask))

    def cnv_prepare_right(self, res: CnvPVecR, a: VecZnx, mask: int = -1, scratch=None):
        self._ck(self.lib.pz_cnv_prepare_right(self.handle, _p(res.data), res.cols, res.size, _p(a.data), a.cols, a.size, mask))

    def cnv_prepare_self(self, left: CnvPVecL, right: CnvPVecR, a: VecZnx, mask: int = -1, scratch=None):
        assert (left.cols, left.size) == (right.cols, right.size)
        self._ck(self.lib.pz_cnv_prepare_self(self.handle, _p(left.data), _p(right.data), left.cols, left.size, _p(a.data), a.cols, a.size, mask))

    def cnv_apply_dft(self, cnv_offset, res: VecZnxDft, res_col, a: CnvPVecL, a_col, b: CnvPVecR, b_col, scratch=None):
        self._ck(self.lib.pz_cnv_apply_dft(self.handle, cnv_offset, _p(res.data), res.cols, res.size, res_col, _p(a.data),
                                           a.cols, a.size, a_col, _p(b.data), b.cols, b.size, b_col))

    def cnv_pairwise_apply_dft(self, cnv_offset, res: VecZnxDft, res_col, a: CnvPVecL, b: CnvPVecR, i, j, scratch=None):
        self._ck(self.lib.pz_cnv_pairwise_apply_dft(self.handle, cnv_offset, _p(res.data), res.cols, res.size, res_col, _p(a.data),
                                                    a.cols, a.size, _p(b.data), b.cols, b.size, i, j))

    def cnv_by_const_apply(self, cnv_offset, res: VecZnxBig, res_col, a: VecZnx, a_col, b, scratch=None):
        b = np.ascontiguousarray(b, dtype=np.int64)
        self._ck(self.lib.pz_cnv_by_const_apply(self.handle, cnv_offset, _p(res.data), res.cols, res.size, res_col, _p(a.data),
                                                a.cols, a.size, a_col, _p(b), b.size))

    TENSOR_MODES = {"apply": abi.PZ_TENSOR_APPLY, "add_assign": abi.PZ_TENSOR_APPLY_ADD_ASSIGN, "square": abi.PZ_TENSOR_SQUARE}

    def glwe_tensor_apply_workspace_bytes(self, params: GlweTensorParams, mode, batch: int) -> int:
        mode = self.TENSOR_MODES[mode] if isinstance(mode, str) else int(mode)
        return self.lib.pz_glwe_tensor_apply_workspace_bytes(self.handle, C.byref(params), mode, batch)

    def glwe_tensor_apply_batched(self, res: c_void_p, a: c_void_p, b, params: GlweTensorParams, mode, batch: int):
        """poulpy-core operations/glwe.rs:609-913 on device-resident ciphertexts; mode: "apply" | "add_assign" | "square"."""
        mode = self.TENSOR_MODES[mode] if isinstance(mode, str) else int(mode)
        self._ck(self.lib.pz_glwe_tensor_apply_batched(self.handle, res, a, b if b is not None else a, C.byref(params), mode, batch))

    def glwe_tensor_relinearize_batched(self, res: c_void_p, a: c_void_p, tsk_pmat: c_void_p, params: GlweOpParams, batch: int):
        """poulpy-core operations/glwe.rs:541-607 on device-resident GLWETensors sharing one prepared tensor key."""
        self._ck(self.lib.pz_glwe_tensor_relinearize_batched(self.handle, res, a, tsk_pmat, C.byref(params), batch))

    def glwe_tensor_mul_relinearize_batched(self, res: c_void_p, a: c_void_p, b, tsk_pmat: c_void_p, tparams: GlweTensorParams, rparams: GlweOpParams,
                                            mode, batch: int):
        """glwe_tensor_apply / _square_apply + glwe_tensor_relinearize with the tensor in scratch (poulpy-ckks leveled/default/mul.rs:49-85, :131-170);
        mode: "apply" | "square"."""
        mode = self.TENSOR_MODES[mode] if isinstance(mode, str) else int(mode)
        self._ck(self.lib.pz_glwe_tensor_mul_relinearize_batched(self.handle, res, a, b if b is not None else a, tsk_pmat, C.byref(tparams),
                                                                 C.byref(rparams), mode, batch))

    def glwe_tensor_mul_relinearize_acc_batched(self, res: c_void_p, a: c_void_p, b, tsk_pmat: c_void_p, tparams: GlweTensorParams,
                                                rparams: GlweOpParams, mode, batch: int, a_stride: int = 0, b_stride: int = 0, accumulate=False,
                                                join="plain", k: int = 0, sign: int = 1, normalize=True):
        """The one-call product on operands in containers of a_stride / b_stride limbs (0: the operand's size), in place (res is a and / or
        b at equal strides), or - accumulate - joined to res wave by wave with the product kept in the module's workspace: join "plain" |
        "lsh_term" | "lsh_acc", k, sign +1 / -1, normalize (include/poulpy_hip.h).  mode: "apply" | "square"."""
        mode = self.TENSOR_MODES[mode] if isinstance(mode, str) else int(mode)
        join = self.JOIN_KINDS[join] if isinstance(join, str) else int(join)
        self._ck(self.lib.pz_glwe_tensor_mul_relinearize_acc_batched(self.handle, res, a, b if b is not None else a, tsk_pmat, C.byref(tparams),
                                                                     C.byref(rparams), a_stride, b_stride, int(bool(accumulate)), join, k, sign,
                                                                     int(bool(normalize)), mode, batch))

    def glwe_tensor_mul_relinearize_acc_workspace_bytes(self, tparams: GlweTensorParams, rparams: GlweOpParams, accumulate, mode, batch: int) -> int:
        mode = self.TENSOR_MODES[mode] if isinstance(mode, str) else int(mode)
        return self.lib.pz_glwe_tensor_mul_relinearize_acc_workspace_bytes(self.handle, C.byref(tparams), C.byref(rparams), int(bool(accumulate)),
                                                                           mode, batch)

    @staticmethod
    def _dot_lists(a_ptrs, b_ptrs, a_strides, b_strides):
        n = len(a_ptrs)
        if len(b_ptrs) != n or any(s is not None and len(s) != n for s in (a_strides, b_strides)):
            raise ValueError("glwe_tensor_dot_relinearize: one b pointer and one stride per a pointer")
        m = max(n, 1)
        pa, pb = (c_void_p * m)(), (c_void_p * m)()
        for i in range(n):
            pa[i] = a_ptrs[i].value if isinstance(a_ptrs[i], c_void_p) else a_ptrs[i]
            pb[i] = b_ptrs[i].value if isinstance(b_ptrs[i], c_void_p) else b_ptrs[i]
        sa = None if a_strides is None else (C.c_size_t * m)(*[int(s) for s in a_strides])
        sb = None if b_strides is None else (C.c_size_t * m)(*[int(s) for s in b_strides])
        return n, pa, pb, sa, sb

    def glwe_tensor_dot_relinearize_batched(self, res: c_void_p, a_ptrs, b_ptrs, tsk_pmat: c_void_p, tparams: GlweTensorParams,
                                            rparams: GlweOpParams, batch: int, a_strides=None, b_strides=None):
        """sum_i a_ptrs[i] (x) b_ptrs[i] in ONE accumulated GLWETensor (glwe_tensor_apply, then glwe_tensor_apply_add_assign), relinearized
        once: the fast branch of poulpy-ckks's ckks_dot_product_ct (include/poulpy_hip.h).  a_ptrs / b_ptrs: device pointers,
        one per pair; a_strides / b_strides: limbs of the containers per pair (None: the operands' sizes)."""
        n, pa, pb, sa, sb = self._dot_lists(a_ptrs, b_ptrs, a_strides, b_strides)
        self._ck(self.lib.pz_glwe_tensor_dot_relinearize_batched(self.handle, res, pa, pb, n, sa, sb, tsk_pmat, C.byref(tparams), C.byref(rparams), batch))

    def glwe_tensor_dot_relinearize_workspace_bytes(self, tparams: GlweTensorParams, rparams: GlweOpParams, npairs: int, batch: int) -> int:
        return self.lib.pz_glwe_tensor_dot_relinearize_workspace_bytes(self.handle, C.byref(tparams), C.byref(rparams), npairs, batch)

    MUL_PLAIN_MODES = {"into": abi.PZ_MUL_PLAIN, "assign": abi.PZ_MUL_PLAIN_ASSIGN}   # = PZ_MUL_CONST / PZ_MUL_CONST_ASSIGN

    def glwe_mul_plain_workspace_bytes(self, params: GlweTensorParams, mode, pt_shared: bool, batch: int) -> int:
        mode = self.MUL_PLAIN_MODES[mode] if isinstance(mode, str) else int(mode)
        return self.lib.pz_glwe_mul_plain_workspace_bytes(self.handle, C.byref(params), mode, int(bool(pt_shared)), batch)

    def glwe_mul_plain_batched(self, res: c_void_p, a, pt: c_void_p, pt_shared: bool, params: GlweTensorParams, mode, batch: int):
        """poulpy-core operations/glwe.rs:184-303 (glwe_mul_plain / _assign) on device-resident GLWEs; params: b_size / b_effective_k describe
        the plaintext VecZnx(1, b_size); pt_shared: one plaintext for the batch; mode: "into" | "assign" (a None: res is the operand)."""
        mode = self.MUL_PLAIN_MODES[mode] if isinstance(mode, str) else int(mode)
        self._ck(self.lib.pz_glwe_mul_plain_batched(self.handle, res, a, pt, int(bool(pt_shared)), C.byref(params), mode, batch))

    def glwe_mul_const_batched(self, res: c_void_p, a, re, im, params: GlweMulConstParams, mode, batch: int, b_size: int | None = None):
        """poulpy-core operations/glwe.rs:66-133 (glwe_mul_const / _assign; `re` alone) and poulpy-ckks leveled/default/mul.rs:342-415 (the
        complex constant: `im`, or neither); re / im: host digit arrays or None; mode: "into" | "assign" (a None: res is the operand)."""
        mode = self.MUL_PLAIN_MODES[mode] if isinstance(mode, str) else int(mode)
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (re, im)]
        sizes = {x.size for x in arrs if x is not None}
        assert len(sizes) <= 1, "re and im carry the same number of digits"
        if b_size is None:
            b_size = sizes.pop() if sizes else 0
        ptrs = [None if x is None else _p(x) for x in arrs]
        self._ck(self.lib.pz_glwe_mul_const_batched(self.handle, res, a, ptrs[0], ptrs[1], b_size, C.byref(params), mode, batch))

    TERM_KINDS = {"raw": abi.PZ_TERM_RAW, "lsh": abi.PZ_TERM_LSH, "rsh": abi.PZ_TERM_RSH}

    def glwe_combine_batched(self, res: c_void_p, res_cols: int, res_size: int, base2k: int, terms, normalize: bool, batch: int):
        """res = the terms applied in order to a zero GLWE batch, then optionally glwe_normalize_assign (include/poulpy_hip.h,
        DESIGN.md 4.6c).  terms: dicts with keys a (device pointer), a_size, kind ("raw" | "lsh" | "rsh"), and optional
        k, sign (+1 / -1), col0_only, shared, base2k (0 = res's)."""
        arr = (GlweTerm * max(len(terms), 1))()
        ops = (c_void_p * max(len(terms), 1))()
        for i, t in enumerate(terms):
            kind = self.TERM_KINDS[t["kind"]] if isinstance(t["kind"], str) else int(t["kind"])
            a = t["a"]
            ops[i] = a.value if isinstance(a, c_void_p) else a
            arr[i] = GlweTerm(int(t["a_size"]), int(t.get("k", 0)), int(t.get("base2k", 0)), kind, int(t.get("sign", 1)),
                              int(bool(t.get("col0_only", False))), int(bool(t.get("shared", False))))
        self._ck(self.lib.pz_glwe_combine_batched(self.handle, res, res_cols, res_size, base2k, ops, arr, len(terms), int(bool(normalize)), batch))

    JOIN_KINDS = {"plain": abi.PZ_JOIN_PLAIN, "lsh_term": abi.PZ_JOIN_LSH_TERM, "lsh_acc": abi.PZ_JOIN_LSH_ACC}

    def glwe_lincomb_const_batched(self, res: c_void_p, rank: int, res_size: int, base2k: int, terms, init_res: bool, normalize: bool, batch: int):
        """res = [res] +- sum_t constant_t x a_t in one pass (include/poulpy_hip.h): poulpy-ckks's mul_add / mul_sub /
        dot product by constants.  terms: dicts with keys a (device pointer), a_size, cnv_offset, re / im (host digit arrays or None) and
        optional shared, join ("plain" | "lsh_term" | "lsh_acc"), k, sign (+1 / -1).  init_res: the accumulator starts as res."""
        nt = max(len(terms), 1)
        ops, rp, ip = (c_void_p * nt)(), (c_void_p * nt)(), (c_void_p * nt)()
        shared, join, sign = (C.c_int * nt)(), (C.c_int * nt)(), (C.c_int * nt)()
        a_size, cnv, b_size, k = (C.c_size_t * nt)(), (C.c_size_t * nt)(), (C.c_size_t * nt)(), (C.c_size_t * nt)()
        keep = []
        for i, t in enumerate(terms):
            a = t["a"]
            ops[i] = a.value if isinstance(a, c_void_p) else a
            arrs = [None if t.get(x) is None else np.ascontiguousarray(t[x], dtype=np.int64) for x in ("re", "im")]
            sizes = {x.size for x in arrs if x is not None}
            assert len(sizes) <= 1, "re and im carry the same number of digits"
            keep.append(arrs)
            rp[i], ip[i] = [None if x is None else x.ctypes.data for x in arrs]
            b_size[i] = int(t["b_size"]) if "b_size" in t else (sizes.pop() if sizes else 0)
            shared[i], a_size[i], cnv[i] = int(bool(t.get("shared", False))), int(t["a_size"]), int(t["cnv_offset"])
            j = t.get("join", "plain")
            join[i] = self.JOIN_KINDS[j] if isinstance(j, str) else int(j)
            k[i], sign[i] = int(t.get("k", 0)), int(t.get("sign", 1))
        init = abi.PZ_LINCOMB_INIT_RES if init_res else abi.PZ_LINCOMB_INIT_NONE
        self._ck(self.lib.pz_glwe_lincomb_const_batched(self.handle, res, rank, res_size, base2k, ops, shared, a_size, cnv, rp, ip, b_size, join, k,
                                                        sign, len(terms), init, int(bool(normalize)), batch))

    def glwe_sum_batched(self, res: c_void_p, res_cols: int, res_size: int, base2k: int, terms, batch: int):
        """res = glwe_normalize_assign of the terms joined in order to a zero GLWE batch, in one pass, up to 64 terms (include/poulpy_hip.h,
        DESIGN.md 4.6e): poulpy-ckks's add_many and the join of its dot products.  terms: dicts with keys a (device pointer), a_size and
        optional shared, join ("plain" | "lsh_term" | "lsh_acc"), k, sign (+1 / -1).  Term 0 may be res itself."""
        nt = max(len(terms), 1)
        ops = (c_void_p * nt)()
        shared, join, sign = (C.c_int * nt)(), (C.c_int * nt)(), (C.c_int * nt)()
        a_size, k = (C.c_size_t * nt)(), (C.c_size_t * nt)()
        for i, t in enumerate(terms):
            a = t["a"]
            ops[i] = a.value if isinstance(a, c_void_p) else a
            shared[i], a_size[i] = int(bool(t.get("shared", False))), int(t["a_size"])
            j = t.get("join", "plain")
            join[i] = self.JOIN_KINDS[j] if isinstance(j, str) else int(j)
            k[i], sign[i] = int(t.get("k", 0)), int(t.get("sign", 1))
        self._ck(self.lib.pz_glwe_sum_batched(self.handle, res, res_cols, res_size, base2k, ops, shared, a_size, join, k, sign, len(terms), batch))

    def _shift_acc(self, name, batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col):
        self._ck(getattr(self.lib, name)(self.handle, batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col))

    def vec_znx_copy_batched(self, batch, res: c_void_p, res_cols, res_size, res_col, a: c_void_p, a_cols, a_size, a_col):
        """vec_znx_copy (poulpy-cpu-ref vec_znx/copy.rs) on every object of the batch: the common limbs copied, the rest of res zeroed."""
        self._ck(self.lib.pz_vec_znx_copy_batched(self.handle, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col))

    def vec_znx_lsh_add_into_batched(self, batch, base2k, k, res: c_void_p, res_cols, res_size, res_col, a: c_void_p, a_cols, a_size, a_col):
        """vec_znx_lsh::<false> (poulpy-cpu-ref vec_znx/shift.rs:68-135) on every object of the batch."""
        self._shift_acc("pz_vec_znx_lsh_add_into_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col)

    def vec_znx_lsh_sub_batched(self, batch, base2k, k, res: c_void_p, res_cols, res_size, res_col, a: c_void_p, a_cols, a_size, a_col):
        """vec_znx_lsh_sub (shift.rs:137-180) on every object of the batch."""
        self._shift_acc("pz_vec_znx_lsh_sub_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col)

    def vec_znx_rsh_add_into_batched(self, batch, base2k, k, res: c_void_p, res_cols, res_size, res_col, a: c_void_p, a_cols, a_size, a_col):
        """vec_znx_rsh::<false> (shift.rs:245-342) on every object of the batch."""
        self._shift_acc("pz_vec_znx_rsh_add_into_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col)

    def vec_znx_rsh_sub_batched(self, batch, base2k, k, res: c_void_p, res_cols, res_size, res_col, a: c_void_p, a_cols, a_size, a_col):
        """vec_znx_rsh_sub (shift.rs:344-...) on every object of the batch."""
        self._shift_acc("pz_vec_znx_rsh_sub_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col)

    # -- LWE glue of the gate bootstrap (device-resident batches; an LWE = VecZnx(n_lwe + 1, 1, size)) -------------
    def lwe_mod_switch_2n_batched(self, res: c_void_p, lwe: c_void_p, n_lwe: int, lwe_size: int, base2k: int, n2: int, negate: bool, batch: int):
        """poulpy-bin-fhe blind_rotation/algorithms/mod.rs:136-176."""
        self._ck(self.lib.pz_lwe_mod_switch_2n_batched(self.handle, res, lwe, n_lwe, lwe_size, base2k, n2, 1 if negate else 0, batch))

    def lwe_sample_extract_batched(self, res: c_void_p, res_n_lwe: int, res_size: int, a: c_void_p, a_cols: int, a_size: int, batch: int):
        """poulpy-core api/conversion.rs:15-40."""
        self._ck(self.lib.pz_lwe_sample_extract_batched(self.handle, res, res_n_lwe, res_size, a, a_cols, a_size, batch))

    def lwe_keyswitch_batched(self, res: c_void_p, res_n_lwe: int, a: c_void_p, a_n_lwe: int, ksk_pmat: c_void_p, params: GlweOpParams, batch: int):
        """poulpy-core keyswitching/lwe.rs:49-94."""
        self._ck(self.lib.pz_lwe_keyswitch_batched(self.handle, res, res_n_lwe, a, a_n_lwe, ksk_pmat, C.byref(params), batch))

    def glwe_from_lwe_batched(self, res: c_void_p, lwe: c_void_p, n_lwe: int, lwe_size: int, lwe_base2k: int, ksk_pmat: c_void_p,
                              params: GlweOpParams, batch: int):
        """poulpy-core conversion/lwe_to_glwe.rs:46-121."""
        self._ck(self.lib.pz_glwe_from_lwe_batched(self.handle, res, lwe, n_lwe, lwe_size, lwe_base2k, ksk_pmat, C.byref(params), batch))

    def lwe_from_glwe_batched(self, res: c_void_p, res_n_lwe: int, a: c_void_p, a_idx: int, ksk_pmat: c_void_p, params: GlweOpParams, batch: int):
        """poulpy-core conversion/glwe_to_lwe.rs:42-90."""
        self._ck(self.lib.pz_lwe_from_glwe_batched(self.handle, res, res_n_lwe, a, a_idx, ksk_pmat, C.byref(params), batch))

    def lwe_from_glwe_many_tmp_bytes(self, params: GlweOpParams, nidx: int, batch: int) -> int:
        return self.lib.pz_lwe_from_glwe_many_tmp_bytes(self.handle, C.byref(params), nidx, batch)

    def lwe_from_glwe_many_batched(self, res: c_void_p, res_n_lwe: int, a: c_void_p, idx, ksk_pmat: c_void_p, params: GlweOpParams, tmp: c_void_p,
                                   tmp_bytes: int, batch: int, lwe_2n: c_void_p = None, n2: int = 0, negate: bool = False):
        """lwe_from_glwe (glwe_to_lwe.rs:42-90) of every one of `batch` GLWEs at every coefficient of `idx`: index-major LWEs in `res`
        (None: not written) and, with `lwe_2n`, their mod_switch_2n(n2, negate) vectors from the same kernel."""
        arr = (C.c_size_t * max(len(idx), 1))(*[int(i) for i in idx])
        self._ck(self.lib.pz_lwe_from_glwe_many_batched(self.handle, res, res_n_lwe, a, len(idx), arr, ksk_pmat, C.byref(params), lwe_2n, n2,
                                                        1 if negate else 0, tmp, tmp_bytes, batch))

    def ggsw_prepare_batched(self, pmat: c_void_p, ggsw: c_void_p, count: int, dnum: int, rank: int, size: int):
        """ggsw_prepare on `count` contiguous device GGSWs (MatZnx layout) -> VmpPMat layout, equal as bytes to vmp_prepare per matrix."""
        self._ck(self.lib.pz_ggsw_prepare_batched(self.handle, pmat, ggsw, count, dnum, rank, size))

    def fhe_uint_prepare_tmp_bytes(self, params: FheUintPrepareParams, batch: int, chunk_bits: int = 0) -> int:
        return self.lib.pz_fhe_uint_prepare_tmp_bytes(self.handle, C.byref(params), batch, chunk_bits)

    def fhe_uint_prepare_batched(self, res_pmat: c_void_p, words: c_void_p, ks_glwe_pmat, ks_lwe_pmat: c_void_p, lut: c_void_p, brk: c_void_p, gals,
                                 atk_ptrs, tsk_ptrs, params: FheUintPrepareParams, tmp: c_void_p, tmp_bytes: int, batch: int,
                                 ggsw_out: c_void_p = None, lwe_out: c_void_p = None):
        """FheUintPrepared::prepare (bdd_arithmetic/ciphertexts/fhe_uint_prepared.rs:399-460) on `batch` words -> word-major
        [batch][word_bits] prepared GGSWs; ks_glwe_pmat may be None."""
        ns = len(gals)
        g = (c_int64 * max(ns, 1))(*[int(x) for x in gals])
        ap = _ptrs(atk_ptrs)
        tp = _ptrs(tsk_ptrs)
        self._ck(self.lib.pz_fhe_uint_prepare_batched(self.handle, res_pmat, ggsw_out, lwe_out, words, ks_glwe_pmat, ks_lwe_pmat, lut, brk, ns, g,
                                                      ap, tp, C.byref(params), tmp, tmp_bytes, batch))

    # -- multi-GPU: RCCL broadcast of prepared keys on the module stream ---------------------
    def comm_available(self):
        """Raises unless RCCL can be loaded in this process (pz_comm_available: dlopen + symbols; draws no id, opens no socket)."""
        self._ck(self.lib.pz_comm_available())

    def comm_unique_id(self) -> bytes:
        """ncclGetUniqueId (call on ONE rank, ship the bytes to the others out of band)."""
        n = self.lib.pz_comm_unique_id_bytes()
        buf = C.create_string_buffer(n)
        self._ck(self.lib.pz_comm_unique_id(buf))
        return buf.raw

    def comm_init_rank(self, world_size: int, rank: int, unique_id: bytes):
        self._ck(self.lib.pz_comm_init_rank(self.handle, world_size, rank, unique_id))

    def comm_destroy(self):
        self._ck(self.lib.pz_comm_destroy(self.handle))

    def bcast_key(self, dev_ptr: c_void_p, nbytes: int, root: int = 0):
        """In-place ncclBroadcast of a device buffer (a prepared key) from `root`, asynchronous on the module stream."""
        self._ck(self.lib.pz_bcast_key(self.handle, dev_ptr, nbytes, root))

    def pin_key(self, pmat: c_void_p, rows: int, cols_in: int, cols_out: int, size: int):
        """Declare a prepared device key immutable: the fused pipeline keeps its row-sliced copy instead of rebuilding it per call."""
        self._ck(self.lib.pz_module_pin_key(self.handle, pmat, rows, cols_in, cols_out, size))

    def unpin_key(self, pmat: c_void_p):
        self._ck(self.lib.pz_module_unpin_key(self.handle, pmat))

    def workspace_bytes(self) -> int:
        """bytes of the module's grow-only device workspace as allocated now (pz_module_workspace_bytes)"""
        return self.lib.pz_module_workspace_bytes(self.handle)

    def glwe_op_workspace_bytes(self, params: GlweOpParams, batch: int, keyswitch: bool) -> int:
        return self.lib.pz_glwe_op_workspace_bytes(self.handle, C.byref(params), batch, int(keyswitch))

    # events on the module stream
    def event_create(self) -> c_void_p:
        ev = c_void_p()
        self._ck(self.lib.pz_event_create(C.byref(ev)))
        return ev

    def event_record(self, ev):
        self._ck(self.lib.pz_event_record(self.handle, ev))

    def event_elapsed_ms(self, e0, e1) -> float:
        ms = C.c_float()
        self._ck(self.lib.pz_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value


BddNode = abi.pz_bdd_node


def bdd_circuit_new(circuit, lib: C.CDLL | None = None) -> c_void_p:
    """pz_bdd_circuit_new on a circuit in the evaluator's node format: host only (no module, no device).  Raises PoulpyHipError with the
    library's message - it names the output bit and the node - when the circuit is not well formed."""
    lib = lib or load_library()
    outs = list(circuit.outputs)
    arrays = [(BddNode * max(len(nodes), 1))(*[BddNode(*nd) for nd in nodes]) for nodes, _ in outs]
    ptrs = (c_void_p * max(len(outs), 1))(*[C.addressof(a) for a in arrays])
    counts = (C.c_size_t * max(len(outs), 1))(*[len(nodes) for nodes, _ in outs])
    states = (C.c_size_t * max(len(outs), 1))(*[int(s) for _, s in outs])
    handle = lib.pz_bdd_circuit_new(ptrs, counts, states, len(outs), int(circuit.input_size))
    if not handle:
        raise PoulpyHipError(f"[{abi.PZ_ERR_INVALID}] {lib.pz_last_error().decode()}")
    return c_void_p(handle)


def bdd_circuit_free(handle: c_void_p, lib: C.CDLL | None = None):
    (lib or load_library()).pz_bdd_circuit_free(handle)


def fhe_uint_pack_level_pairs(n: int, word_bits: int, level: int, lib: C.CDLL | None = None) -> list:
    """pz_fhe_uint_pack_level_pairs: host only (no module, no device) - the (lo slot, hi slot, t) triples of one merge level of
    pz_fhe_uint_pack_batched, [] for a shape or level out of range."""
    lib = lib or load_library()
    cnt = int(lib.pz_fhe_uint_pack_level_pairs(n, word_bits, level, None, 0))
    buf = (C.c_uint32 * max(3 * cnt, 1))()
    lib.pz_fhe_uint_pack_level_pairs(n, word_bits, level, buf, cnt)
    return [(int(buf[3 * k]), int(buf[3 * k + 1]), int(buf[3 * k + 2])) for k in range(cnt)]


def fhe_uint_bit_coefficient(n: int, word_bits: int, bit: int, lib: C.CDLL | None = None) -> int:
    """pz_fhe_uint_bit_coefficient: host only - the coefficient bit_index(bit) << log_gap of a bit of a word; ValueError out of range."""
    v = int((lib or load_library()).pz_fhe_uint_bit_coefficient(n, word_bits, bit))
    if v >= n:
        raise ValueError("fhe_uint_bit_coefficient: n %d, word_bits %d, bit %d out of range" % (n, word_bits, bit))
    return v


def fhe_uint_word_plan(n: int, word_bits: int, op: int, args, lib: C.CDLL | None = None) -> list:
    """pz_fhe_uint_word_plan: host only - the stages of one FheUint byte operation (op: abi.PZ_WORD_OP_*; args: the indices of a get, [byte]
    or [dst, src]) as dicts {skip, items: [(source, exponent, slot)], close, base, plus, minus, r}; ValueError for what the calls refuse."""
    lib = lib or load_library()
    a = (C.c_uint32 * max(len(args), 1))(*[int(x) for x in args])
    st = C.c_int(0)
    cnt = int(lib.pz_fhe_uint_word_plan(n, word_bits, op, a, len(args), None, 0, C.byref(st)))
    if st.value != 0:
        raise ValueError(lib.pz_last_error().decode())
    buf = (C.c_uint32 * max(cnt, 1))()
    lib.pz_fhe_uint_word_plan(n, word_bits, op, a, len(args), buf, cnt, C.byref(st))
    w, stages, i = [int(x) for x in buf[:cnt]], [], 0
    while i < cnt:
        skip, nitems = w[i], w[i + 1]
        items = [tuple(w[i + 2 + 3 * k:i + 5 + 3 * k]) for k in range(nitems)]
        i += 2 + 3 * nitems
        none = lambda v: None if v == 0xFFFFFFFF else v   # noqa: E731
        stages.append(dict(skip=skip, items=items, close=w[i], base=w[i + 1], plus=none(w[i + 2]), minus=none(w[i + 3]), r=w[i + 4]))
        i += 5
    return stages
