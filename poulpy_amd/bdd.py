"""Helpers on top of the gate entry points (pz_glwe_cmux_batched, pz_glwe_cswap_batched) for poulpy-bin-fhe's bdd_arithmetic."""
from __future__ import annotations

from ctypes import c_void_p


def _addr(p) -> int:
    return p.value if isinstance(p, c_void_p) else int(p)


def glwe_blind_selection(mod, buf, bit_ptrs, params, batch: int) -> c_void_p:
    """GLWEBlindSelection::glwe_blind_selection (bdd_arithmetic/blind_selection.rs:41-104) on `batch` independent maps.

    buf: device pointer to a dense slot-major buffer [2^bit_mask slots][batch] of GLWE ciphertexts (one layout: params.a_size ==
    params.res_size limbs), slot s holding entry s of every map; an absent entry is a zero ciphertext (:75-76, :82-83).  bit_ptrs[i]: the
    prepared GGSW of bit bit_rsh + i (device pointers), bit_mask = len(bit_ptrs).  The buffer is CLOBBERED, as the reference's entries are.

    Level i (bit bit_rsh + bit_mask - 1 - i, :62) pairs entry j with entry j + t, t = 2^(bit_mask - 1 - i), by cmux_assign(lo = a[j + t],
    hi = a[j]) (:70): with the live entries kept in the LAST 2t slots that is ONE call - f = the first t of them, res = t = the last t, on
    t * batch ciphertexts - and the survivors are the last t slots.  Returns the device pointer of the result: the last slot."""
    assert params.a_size == params.res_size
    bit_mask = len(bit_ptrs)
    slots = 1 << bit_mask
    size = int(params.res_size)
    slot_bytes = batch * mod.n() * (int(params.rank) + 1) * size * 8
    base = _addr(buf)
    for i in range(bit_mask):
        t = 1 << (bit_mask - 1 - i)
        lo = c_void_p(base + (slots - t) * slot_bytes)
        hi = c_void_p(base + (slots - 2 * t) * slot_bytes)
        mod.glwe_cmux_batched(lo, lo, hi, bit_ptrs[bit_mask - 1 - i], params, t * batch, t_size=size, f_size=size)
    return c_void_p(base + (slots - 1) * slot_bytes)


def glwe_blind_retrieval(mod, buf, nslots: int, bit_ptrs, params, batch: int, reverse: bool = False) -> c_void_p:
    """GLWEBlindRetrieval::glwe_blind_retrieval_statefull / _rev (bdd_arithmetic/blind_retrieval.rs:195-266) on `batch` independent vectors.

    buf: device pointer to a dense slot-major buffer [nslots][batch] of GLWE ciphertexts (one layout: params.a_size == params.res_size limbs),
    slot s holding element s of every vector.  bit_ptrs[i]: the prepared GGSW of bit bit_rsh + i (device pointers), bit_mask = len(bit_ptrs).
    The buffer is permuted IN PLACE, as the reference's Vec is: afterwards slot 0 holds the element at the encrypted index; reverse=True applies
    the same network backwards and restores the order.

    Level i (bit bit_rsh + bit_mask - 1 - i, :222-223) pairs element j with element j + t, t = 2^(bit_mask - 1 - i), for every j < t with
    j + t < nslots (:224-230): one conditional swap on min(t, nslots - t) * batch contiguous pairs.  All levels are ONE call of
    pz_glwe_blind_retrieval_batched.  Returns the device pointer of slot 0."""
    assert params.a_size == params.res_size
    mod.glwe_blind_retrieval_batched(buf, nslots, bit_ptrs, reverse, params, batch)
    return c_void_p(_addr(buf))
