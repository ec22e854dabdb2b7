"""Cases for the encrypt / multiply / decrypt tests of the tensor family (tests/ only): poulpy-core's test_glwe_tensoring,
test_glwe_tensor_apply_add_assign and test_glwe_tensor_square (poulpy-core/src/test_suite/glwe_tensor.rs:24-431) as case builders, their
negative controls, and the oracle runner and noise check that tests/test_tensor_semantics.py (oracle) and
tests/test_gpu_tensor_semantics.py (device) share.  The builders call neither the oracle nor the device: secrets, tensor keys and
ciphertexts come from tests/fhe_sk.py, and each case carries the exact product every output must decrypt to and its bound.

What a tensor means (operations/glwe.rs:699-818, tests/test_oracle_cnv.py::test_p17_*): the tensor's phase is the product of the two
phases as REAL polynomials, times 2^cnv_offset, mod 1.  A phase is m 2^-bits + e + I with I the integer polynomial the torus drops
(a_0 + sum a_i s_i wraps; var I = rank N / 24 + 1 / 12 for uniform masks and a ternary secret of density 1/2), so the product is
m m' 2^(cnv_offset - 2 bits) + (I e' + I' e) 2^cnv_offset + integers + smaller terms: the message sits at 2^(cnv_offset - 2 bits) and the
noise at about N sqrt(rank / 12) sigma 2^(cnv_offset - k).  The reference takes bits = scale = 2 in_base2k and cnv_offset = scale + res_offset
and bounds the noise by -(k - scale - res_offset - log2 N - (rank - 1) / sqrt 2) = -(k - cnv_offset - log2 N - ...) with a margin of 0.5
(glwe_tensor.rs:186-199), before and after the relinearization: the statement above to within 0.6 bit at every N.  Every case here uses
that bound, with k the coarser of the two inputs' encryption precisions.  The square form has e' = e and I' = I, so its two cross terms
coincide instead of adding in variance: half a bit more, which `square` cases add (the reference only checks square == apply(a, a),
which run_oracle asserts too).  At the route shapes the message precision `bits` is chosen so that the product lies above that noise
(at base2k 12 with 3 limbs and N = 8192, scale = 24 would leave nothing to decrypt); a wrong result is uniform on the torus, deviation
2^-1.79, and `margin` records how far below that (or below the product's own size, if smaller) the bound lies.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from poulpy_amd.layouts import VecZnx
from tests import fhe_sk as fs
from tests.core_cases import prepare
from tests.helpers import seeded

N = 256
BASE2K = 17     # poulpy-cpu-ref/src/tests.rs:154-158
WANT_BASE2K = 16
MODES = ("apply", "add_assign", "square")


def _message(n, rng):
    """glwe_tensor.rs:119-122: (next & 7) - 4."""
    return rng.integers(0, 8, n, dtype=np.int64) - 4


def reference_bound(n, rank, k, cnv_offset):
    """glwe_tensor.rs:186-188 with scale + res_offset = cnv_offset, and the 0.5 the assertion allows."""
    return -((k - cnv_offset - math.log2(n)) - (rank - 1) / math.sqrt(2.0)) + 0.5


def tensor_case(n, rank, in_base2k, a_size, b_size, res_size, res_base2k, cnv_offset, batch, seed, mode="apply", bits=None, a_bits_off=0,
                k_enc=None, key=None, relin=None, t_size=None, one_call=False, want_offset=0, order=None, limb_shift=0,
                reverse_pairs=False, drop_cross_factor=False, undecryptable=()):
    """glwe_tensor.rs:24-202 (apply), :204-272 (add_assign), :274-431 (square) on `batch` message pairs of their own.

    key = (key_base2k, k_tsk, dnum, dsize): the tensor key; relin = (size, base2k) of the relinearized GLWE.
    one_call: the tensor is a temporary of t_size limbs at in_base2k and only the relinearized GLWE comes out (poulpy-ckks
    leveled/default/mul.rs:49-85).  add_assign starts from a fresh encryption of a third message, read as a tensor with zero pair
    columns.  Controls: want_offset (want read at cnv_offset + want_offset), order / limb_shift (the tensor key), reverse_pairs (the
    checker's pair secrets), drop_cross_factor (square of m + m' expected as m^2 + m m' + m'^2).  undecryptable names the stages whose
    result the reference itself leaves unreadable (see ROUTES); they are compared with the oracle and must miss the bound."""
    rng = seeded(seed)
    square = mode == "square"
    bits = 2 * in_base2k if bits is None else bits        # glwe_tensor.rs:117
    cols, pairs = rank + 1, rank * (rank + 1) // 2
    tcols = cols + pairs
    a_k = a_size * in_base2k - a_bits_off                 # the effective k the call is given (a.max_k() in the reference)
    b_k = a_k if square else b_size * in_base2k
    # where the encryption puts its noise: at the effective k unless given.  Below a masked bottom limb it is given: the mask truncates
    # every column of a by up to 2^a_bits_off units of 2^-(a_size in_base2k), a phase error of deviation 2^(a_bits_off - 1.8) sqrt(1 + rank N / 2)
    # of those units, which a ciphertext whose own noise stands there or higher (as the effective k promises) does not feel
    ka_enc, kb_enc = (a_k, b_k) if k_enc is None else k_enc if isinstance(k_enc, tuple) else (k_enc, k_enc)
    kb_enc = ka_enc if square else kb_enc
    assert fs.limbs_for(ka_enc, in_base2k) == a_size and (square or fs.limbs_for(kb_enc, in_base2k) == b_size)
    if one_call:
        res_size, res_base2k = t_size, in_base2k
    k_res = res_size * res_base2k
    out_bits = 2 * bits - cnv_offset
    assert 0 < out_bits <= k_res
    assert bits <= cnv_offset       # I m' 2^(cnv_offset - bits) must be an integer polynomial (the reference: cnv_offset >= scale)
    sk = fs.ternary_secret(n, rank, rng)
    tsk = key_base2k = dsize = None
    if key is not None:
        key_base2k, k_tsk, dnum, dsize = key
        tsk = fs.tensor_key(sk, key_base2k, k_tsk, dnum, dsize, rng, order=order, limb_shift=limb_shift)
    a_all, b_all, acc_all, wants, prods, mcs = [], [], [], [], [], []
    for _ in range(batch):
        ma, mb = _message(n, rng), _message(n, rng)
        if drop_cross_factor:
            assert square
            m, m2 = ma, mb
            ma = m + m2
            assert np.array_equal(fs.mul_msg(ma, ma), fs.mul_msg(m, m) + 2 * fs.mul_msg(m, m2) + fs.mul_msg(m2, m2))
            prod = fs.mul_msg(m, m) + fs.mul_msg(m, m2) + fs.mul_msg(m2, m2)
        else:
            prod = fs.mul_msg(ma, ma if square else mb)
        a_all.append(fs.glwe_encrypt(sk, fs.encode(ma, in_base2k, bits, a_size), in_base2k, ka_enc, rng))
        if not square:
            b_all.append(fs.glwe_encrypt(sk, fs.encode(mb, in_base2k, bits, b_size), in_base2k, kb_enc, rng))
        if mode == "add_assign":
            mc = _message(n, rng)
            mcs.append(mc)
            acc = np.zeros((res_size, tcols, n), dtype=np.int64)
            acc[:, :cols] = fs.glwe_encrypt(sk, fs.encode(mc, res_base2k, out_bits, res_size), res_base2k, k_res, rng)
            acc_all.append(acc)
            prod = prod + mc
        prods.append(prod)
        wants.append(fs.torus_from_int(prod, out_bits - want_offset, WANT_BASE2K))
    bnd = reference_bound(n, rank, min(ka_enc, kb_enc), cnv_offset) + (0.5 if square else 0.0)
    if mode == "add_assign":   # the accumulator's fresh noise on top, in variance
        bnd = 0.5 * math.log2(4.0 ** bnd + (fs.SIGMA * 2.0 ** -k_res) ** 2)
    # a wrong result: the product's own size (N terms of second moment 5.5^2 at 2^-out_bits), at most the uniform torus element's
    wrong = min(0.5 * math.log2(n * 5.5 * 5.5) - out_bits, -0.5 * math.log2(12.0))
    return SimpleNamespace(n=n, rank=rank, mode=mode, in_base2k=in_base2k, a=np.stack(a_all), b=None if square else np.stack(b_all),
                           acc=np.stack(acc_all) if acc_all else None, a_k=a_k, b_k=b_k, cnv_offset=cnv_offset, res_size=res_size,
                           res_base2k=res_base2k, key=tsk, key_base2k=key_base2k, dsize=dsize, relin=relin, one_call=one_call, sk=sk,
                           want=wants, prod=prods, mc=mcs, bits=bits, bound=bnd, margin=wrong - bnd, reverse_pairs=reverse_pairs, undecryptable=tuple(undecryptable),
                           broken=(("tensor",) if reverse_pairs else ("relin",) if (order is not None or limb_shift) else ("tensor", "relin")))


def at_offset(c, cnv_offset):
    """The same secret, key and inputs at another cnv_offset (the reference encrypts once and loops res_offset, glwe_tensor.rs:159):
    only what the offset enters changes (the accumulator of add_assign too: it encrypts at the product's precision)."""
    assert c.bits <= cnv_offset < 2 * c.bits
    d = SimpleNamespace(**vars(c))
    d.cnv_offset = cnv_offset
    if c.mode == "add_assign":
        rng = seeded(cnv_offset)
        d.acc = np.zeros_like(c.acc)
        for t, mc in enumerate(c.mc):
            d.acc[t, :, :c.rank + 1] = fs.glwe_encrypt(c.sk, fs.encode(mc, c.res_base2k, 2 * c.bits - cnv_offset, c.res_size), c.res_base2k,
                                                       c.res_size * c.res_base2k, rng)
    d.want = [fs.torus_from_int(p, 2 * c.bits - cnv_offset, WANT_BASE2K) for p in c.prod]
    d.bound = c.bound + (cnv_offset - c.cnv_offset)
    d.margin = None
    return d


# ---- the reference's loops and the controls (N = 256, base2k 17) ----
def _reference_shape(base2k):
    in_b, out_b, k = base2k - 1, base2k - 2, 8 * base2k + 1       # glwe_tensor.rs:41-46
    k_tsk = k + base2k
    key = (base2k, k_tsk, -(-k // base2k), 1)
    return in_b, out_b, k, fs.limbs_for(k, in_b), fs.limbs_for(k, out_b), key


def reference_cases(kind, batch, ranks=(1, 2, 3), offsets=None, base2k=BASE2K, n=N):
    """The loops of test_glwe_tensoring (kind "apply"), _square and _apply_add_assign: rank 1..3, res_offset in 0..scale (or `offsets`),
    as (label, case).  The add_assign form runs at the reference's k = 4 base2k + 1 too (:213), on encrypted inputs: there the reference
    only compares limbs (which run_oracle does), and at that k the bound passes -1.79 from res_offset 26 on, so the decryption says
    something at the lower offsets only; the k = 8 base2k + 1 shape carries the statement at every offset."""
    in_b, out_b, k, size_in, size_out, key = _reference_shape(base2k)
    scale = 2 * in_b
    k4 = 4 * base2k + 1
    shapes = [(k, size_in, size_out, key)] + ([(k4, fs.limbs_for(k4, in_b), fs.limbs_for(k4, out_b), None)] if kind == "add_assign" else [])
    for rank in ranks:
        for (kk, si, so, ky) in shapes:
            base = None
            for off in (range(scale) if offsets is None else offsets):
                if base is None:
                    base = tensor_case(n, rank, in_b, si, si, so, out_b, scale + off, batch, 1000 * rank + si, mode=kind, k_enc=kk, key=ky,
                                       relin=(so, out_b) if ky else None)
                yield ((kind, rank, off, si), at_offset(base, scale + off))


DEVICE_OFFSETS = (0, 1, BASE2K - 2, BASE2K - 1, 2 * (BASE2K - 1) - 1)     # {0, 1, in_base2k - 1, in_base2k, scale - 1}


def control_cases(batch, base2k=BASE2K, n=N):
    """Negative controls 1-5, each through the procedure of its operation, as (label, case)."""
    in_b, out_b, k, size_in, size_out, key = _reference_shape(base2k)
    cnv = 2 * in_b + 3
    common = dict(k_enc=k, key=key, relin=(size_out, out_b))
    yield ("rank-2 tensor key, pair columns s0 s1 and s1^2 exchanged", tensor_case(n, 2, in_b, size_in, size_in, size_out, out_b, cnv, batch, 601,
                                                                                   order=(0, 2, 1), **common))
    yield ("tensor-key messages one limb off", tensor_case(n, 1, in_b, size_in, size_in, size_out, out_b, cnv, batch, 602, limb_shift=1, **common))
    yield ("cnv_offset read one bit off", tensor_case(n, 1, in_b, size_in, size_in, size_out, out_b, cnv, batch, 603, want_offset=1, **common))
    yield ("rank-2 tensor decrypted with the pair secrets reversed", tensor_case(n, 2, in_b, size_in, size_in, size_out, out_b, cnv, batch, 604,
                                                                                 reverse_pairs=True, **common))
    yield ("square of m + m' without the factor 2 on m m'", tensor_case(n, 1, in_b, size_in, size_in, size_out, out_b, cnv, batch, 605, mode="square",
                                                                         drop_cross_factor=True, **common))


# ---- running and checking ----
def _vec(x):
    return VecZnx(x.shape[2], x.shape[1], x.shape[0], np.ascontiguousarray(x))


def run_oracle(ref, c):
    """-> {"tensor": (batch, res_size, tcols, n)} and / or {"relin": (batch, size, rank + 1, n)}.  The square form is also run as
    apply(a, a) and must agree bit for bit, before and after the relinearization (glwe_tensor.rs:404, :420)."""
    n, cols = c.n, c.rank + 1
    tcols = cols * (cols + 1) // 2
    batch = len(c.a)
    pm = prepare(ref, c.key) if c.key is not None else None
    tensor = np.zeros((batch, c.res_size, tcols, n), dtype=np.int64) if c.acc is None else c.acc.copy()
    relin = np.empty((batch, c.relin[0], cols, n), dtype=np.int64) if c.relin else None
    for t in range(batch):
        a = _vec(c.a[t])
        r = _vec(tensor[t])
        if c.mode == "square":
            ref.glwe_tensor_square_apply(c.cnv_offset, r, c.res_base2k, a, c.a_k, c.in_base2k)
            r2 = VecZnx(n, tcols, c.res_size)
            ref.glwe_tensor_apply(c.cnv_offset, r2, c.res_base2k, a, c.a_k, a, c.a_k, c.in_base2k)
            assert np.array_equal(r.data, r2.data), "square != apply(a, a)"
        else:
            ref.glwe_tensor_apply(c.cnv_offset, r, c.res_base2k, a, c.a_k, _vec(c.b[t]), c.b_k, c.in_base2k, add_assign=(c.mode == "add_assign"))
            if c.mode == "add_assign":      # glwe_tensor.rs:269-270: acc + product, limb for limb
                r2 = VecZnx(n, tcols, c.res_size)
                ref.glwe_tensor_apply(c.cnv_offset, r2, c.res_base2k, a, c.a_k, _vec(c.b[t]), c.b_k, c.in_base2k)
                assert np.array_equal(r.data, c.acc[t] + r2.data), "add_assign != acc + apply"
        tensor[t] = r.data
        if relin is not None:
            g = VecZnx(n, cols, c.relin[0])
            ref.glwe_tensor_relinearize(g, c.relin[1], r, c.res_base2k, pm, c.dsize, c.key_base2k)
            relin[t] = g.data
    out = {} if c.one_call else {"tensor": tensor}
    if relin is not None:
        out["relin"] = relin
    return out


def noises(c, out):
    have = {}
    for stage, res in out.items():
        if stage == "tensor":
            ph = [fs.glwe_tensor_phase(x, c.sk, c.res_base2k, reverse_pairs=c.reverse_pairs) for x in res]
            b2k = c.res_base2k
        else:
            ph = [fs.glwe_phase(x, c.sk) for x in res]
            b2k = c.relin[1]
        e = [fs.torus_diff(p, b2k, w, WANT_BASE2K) for p, w in zip(ph, c.want)]
        have[stage] = [math.log2(s) if s > 0 else -math.inf for s in (float(np.std(x)) for x in e)]
    return have


def check(label, c, out, fail=False):
    """Every output of every stage against its own product: the worst noise within the bound; for a control, the best noise of each
    stage it breaks beyond the bound, and the stages it leaves alone still within it."""
    have = noises(c, out)
    for stage, h in have.items():
        wrong = f" (a wrong result: {c.bound + c.margin:.2f})" if c.margin is not None else ""
        print(f"[noise] {label} {stage}: noise_have {max(h):.2f} (min {min(h):.2f}) noise_want {c.bound:.2f}{wrong}")
        if (fail and stage in c.broken) or stage in c.undecryptable:
            assert min(h) > c.bound, (label, stage, h, c.bound, "a negative control met the bound")
        else:
            assert max(h) <= c.bound, (label, stage, h, c.bound)
    if fail:
        assert any(stage in c.broken for stage in have), (label, "the control checked nothing")
    return have


# ---- the device's routes (shapes after tests/test_gpu_cnv.py), each with a message precision its noise leaves readable ----
# name -> (tensor_case keywords, knobs of the device run).  "kind": "apply" = pz_glwe_tensor_apply_batched alone, "two_calls" = that and
# pz_glwe_tensor_relinearize_batched, "one_call" = pz_glwe_tensor_mul_relinearize_batched.  host: the oracle half also runs in the host suite.
NOTE_T16 = "16-bit tensor in tile order"


def _route(kind, host=True, chunk=0, fuse=(True, True), pin=False, mid_cnv=None, t16=None, **case):
    return case, SimpleNamespace(kind=kind, host=host, chunk=chunk, fuse=fuse, pin=pin, mid_cnv=mid_cnv, t16=t16)


ROUTES = {}
for _rank in (1, 2):
    for _mode in MODES:
        # fused row pass k_mid_cnv: N = 8192, one base2k 12, ragged (4, 3, 5), a_effective_k 3 bits short, cnv_offset below base2k
        ROUTES[f"n8192-row-pass-rank{_rank}-{_mode}"] = _route("apply", chunk=2, mid_cnv=True, n=8192, rank=_rank, in_base2k=12, a_size=4, b_size=3,
                                                             res_size=5, res_base2k=12, cnv_offset=5, bits=5, a_bits_off=3, k_enc=(40, 36), mode=_mode,
                                                             seed=8100 + 10 * _rank + len(_mode))
    # the same ring with two bases: the per-op composition; cnv_offset above base2k
    ROUTES[f"n8192-two-bases-rank{_rank}"] = _route("apply", chunk=2, mid_cnv=False, n=8192, rank=_rank, in_base2k=12, a_size=4, b_size=4, res_size=4,
                                                   res_base2k=15, cnv_offset=13, bits=10, a_bits_off=3, k_enc=(40, 48), seed=8200 + _rank)
    for _fuse in ((True, True), (False, False)):
        _f = "fused" if _fuse[0] else "unfused"
        # relinearization at N = 4096: dsize 2 at base2k 13; every base different; res_base2k == key_base2k != a_base2k.  In that last
        # case operations/glwe.rs:595-598 adds the tensor's GLWE columns, limbs at a_base2k, to the accumulator at key_base2k limb by limb
        # (the branch asks res_base2k == key_base2k where it means a_base2k == key_base2k; the reference's own tests never reach it: 15 / 16 / 17).
        # The oracle and the device follow the reference bit for bit, so the tensor decrypts and the relinearized GLWE does not: the
        # case asserts both, and says so when the reference changes
        ROUTES[f"n4096-relin-dsize2-rank{_rank}-{_f}"] = _route("two_calls", host=_fuse[0], chunk=3, fuse=_fuse, n=4096, rank=_rank, in_base2k=13, a_size=4, b_size=4,
                                                                res_size=4, res_base2k=13, cnv_offset=16, bits=11, key=(13, 65, 2, 2), relin=(4, 13),
                                                                seed=4100 + _rank)
        ROUTES[f"n4096-relin-three-bases-rank{_rank}-{_f}"] = _route("two_calls", host=_fuse[0], chunk=3, fuse=_fuse, n=4096, rank=_rank, in_base2k=15, a_size=3, b_size=3,
                                                                     res_size=3, res_base2k=15, cnv_offset=17, bits=12, key=(12, 60, 4, 1), relin=(4, 13),
                                                                     seed=4300 + _rank)
        ROUTES[f"n4096-relin-key-base-rank{_rank}-{_f}"] = _route("two_calls", host=_fuse[0], chunk=3, fuse=_fuse, n=4096, rank=_rank, in_base2k=16, a_size=3, b_size=3,
                                                                  res_size=3, res_base2k=16, cnv_offset=18, bits=12, key=(12, 60, 4, 1), relin=(4, 12),
                                                                  undecryptable=("relin",), seed=4200 + _rank)
    for _mode in ("apply", "square"):
        # one call: the tensor as 16-bit digits at base2k 12 and 14 (the gate's last side), as i64 at base2k 15
        ROUTES[f"n8192-one-call-b12-rank{_rank}-{_mode}"] = _route("one_call", chunk=2, t16=True, n=8192, rank=_rank, in_base2k=12, a_size=4, b_size=3,
                                                                   t_size=5, res_size=None, res_base2k=None, one_call=True, cnv_offset=5, bits=5,
                                                                   a_bits_off=3, k_enc=(40, 36), key=(12, 60, 5, 1), relin=(4, 12), mode=_mode, seed=8300 + _rank)
    ROUTES[f"n8192-one-call-b14-rank{_rank}"] = _route("one_call", chunk=2, t16=True, n=8192, rank=_rank, in_base2k=14, a_size=3, b_size=3, t_size=4,
                                                      res_size=None, res_base2k=None, one_call=True, cnv_offset=14, bits=10, key=(14, 56, 4, 1),
                                                      relin=(4, 14), mode=("apply", "square")[_rank - 1], seed=8400 + _rank)
    ROUTES[f"n8192-one-call-b15-rank{_rank}"] = _route("one_call", chunk=2, t16=False, n=8192, rank=_rank, in_base2k=15, a_size=3, b_size=3, t_size=4,
                                                      res_size=None, res_base2k=None, one_call=True, cnv_offset=14, bits=10, key=(15, 60, 4, 1),
                                                      relin=(4, 15), mode=("square", "apply")[_rank - 1], seed=8500 + _rank)
for _mode, _pin in (("apply", False), ("square", True)):
    # BASELINE configs[4] as one call: N = 2^16, 16 limbs, base2k 12, rank 1, cnv_offset = 16 12 - 20; the reference's bound leaves 4 bits
    # there (k - cnv_offset - log2 N), so the message stands at 2^-6 and a wrong result shows as the uniform torus element's 2^-1.79
    ROUTES[f"n65536-config5-{_mode}"] = _route("one_call", host=False, pin=_pin, t16=True, n=65536, rank=1, in_base2k=12, a_size=16, b_size=16, t_size=16,
                                              res_size=None, res_base2k=None, one_call=True, cnv_offset=16 * 12 - 20, bits=89, key=(12, 192, 16, 1),
                                              relin=(16, 12), mode=_mode, seed=6500 + _pin)

# controls 1 and 3 once more at the N = 8192 one-call multiply
LARGE_CONTROLS = {
    "n8192 one call: rank-2 tensor key, pair columns exchanged": dict(ROUTES["n8192-one-call-b12-rank2-apply"][0], order=(0, 2, 1), seed=8601),
    "n8192 one call: cnv_offset read one bit off": dict(ROUTES["n8192-one-call-b12-rank1-apply"][0], want_offset=1, seed=8603),
}


def route_case(name, batch):
    kw, knobs = ROUTES[name]
    return tensor_case(batch=batch, **kw), knobs


# ---- plaintext and constant products (glwe_tensor.rs:433-682; poulpy-ckks leveled/default/mul.rs:342-415 for the complex constant) ----
# The same statement: the result's phase is phase(a) B 2^cnv_offset with B the plaintext's (the constant's) torus value taken as a real
# number.  phase(a) = x + e + I, so B 2^cnv_offset has to be an integer polynomial for I to drop out: the reference's two-limb plaintext
# at cnv_offset = scale + res_offset, its one-digit constant in limb 0 at cnv_offset >= base2k, and here a plaintext of precision
# b_bits <= cnv_offset.  want = x B 2^cnv_offset on exact integers; the bound is the tensor's (glwe_tensor.rs:552, :677).
def _noise_int(ct, base2k, sk, want):
    """log2 of the deviation of phase(ct) - want mod 1; want = (exact integers, bits)."""
    x, bits = want
    ka = base2k * ct.shape[0]
    kk = max(ka, bits)
    d = (fs.to_int(fs.glwe_phase(ct, sk), base2k) << (kk - ka)) - (x << (kk - bits))
    q = 1 << kk
    d = (d + q // 2) % q - q // 2
    sd = float(np.std(np.ldexp(np.array([float(v) for v in d], dtype=np.float64), -kk)))
    return math.log2(sd) if sd > 0 else -math.inf


def _small_or_uniform(n, size, base2k, bits, rng):
    """(limbs, exact integers, bits of precision): the reference's full-width uniform limbs (bits None), or (next & 7) - 4 at 2^-bits."""
    if bits is None:
        pt = fs.uniform_digits((size, n), base2k, rng)
        return pt, fs.to_int(pt, base2k), size * base2k
    m = _message(n, rng)
    return fs.encode(m, base2k, bits, size), m.astype(object), bits


def mul_plain_case(n, rank, a_size, b_size, res_size, ab, rb, cnv_offset, batch, seed, mode="into", shared=False, a_bits=None, b_bits=None,
                   a_bits_off=0, k_enc=None, times_x=False):
    """glwe_tensor.rs:433-557: a GLWE of x times a plaintext b, one per ciphertext or one shared by the batch; into a result at rb or in
    place (one base, res = a).  a_bits / b_bits None: the reference's full-width uniform limbs (N <= 4096: the exact product is the
    schoolbook one); else small messages at those precisions.  times_x (a control): want from X b."""
    rng = seeded(seed)
    cols = rank + 1
    assign = mode == "assign"
    if assign:
        a_size, rb = res_size, ab
    a_k, b_k = a_size * ab - a_bits_off, b_size * ab
    k_enc = a_k if k_enc is None else k_enc
    assert fs.limbs_for(k_enc, ab) == a_size
    sk = fs.ternary_secret(n, rank, rng)
    pts, pt_vals = [], []
    for _ in range(1 if shared else batch):
        limbs, val, bb = _small_or_uniform(n, b_size, ab, b_bits, rng)
        assert bb <= cnv_offset, "B 2^cnv_offset must be an integer polynomial"
        pts.append(limbs[:, None, :])
        pt_vals.append(fs.rotate(val, 1) if times_x else val)
    a_all, wants = [], []
    for t in range(batch):
        limbs, val, ba = _small_or_uniform(n, a_size, ab, a_bits, rng)
        a_all.append(fs.glwe_encrypt(sk, limbs, ab, k_enc, rng))
        b_val = pt_vals[0 if shared else t]
        prod = fs.mul_exact(val, b_val.astype(np.int64)) if n <= fs.SCHOOLBOOK_MAX_N else fs.mul_msg(val.astype(np.int64), b_val.astype(np.int64)).astype(object)
        out_bits = ba + bb - cnv_offset
        assert out_bits > 0
        wants.append((prod, out_bits))
    return SimpleNamespace(op="plain", n=n, rank=rank, mode=mode, shared=shared, a=np.stack(a_all), pt=np.stack(pts), a_k=a_k, b_k=b_k, ab=ab, rb=rb,
                           res_size=res_size, cnv_offset=cnv_offset, sk=sk, want=wants, bound=reference_bound(n, rank, k_enc, cnv_offset))


def mul_const_case(n, rank, a_size, res_size, ab, rb, cnv_offset, batch, seed, mode="into", arms="re", limb=0, digit_shift=0, a_bits=None,
                   wide=False, flip_im=False):
    """glwe_tensor.rs:559-682 and mul.rs:342-415: a GLWE of x times a constant of 3 limbs at ab with one non-zero limb (`limb`), a small
    digit times 2^digit_shift, or (wide) the reference's full 17-bit digit: c = digit 2^-((limb + 1) ab).  arms: re, im or both;
    want = re x + im X^(N/2) x.  flip_im (a control): the imaginary arm's sign flipped in want."""
    rng = seeded(seed)
    assign = mode == "assign"
    if assign:
        a_size, ab = res_size, rb
    c_bits = (limb + 1) * ab
    assert c_bits - digit_shift <= cnv_offset, "c 2^cnv_offset must be an integer"
    k = a_size * ab
    sk = fs.ternary_secret(n, rank, rng)

    def digit():
        if wide:        # glwe_tensor.rs:627-631: a sign-extended 17-bit value
            return int(rng.integers(-(1 << 16), 1 << 16))
        return int(rng.choice([-7, -5, -3, 3, 5, 7])) << digit_shift

    re = im = None
    d_re = d_im = 0
    if arms in ("re", "both"):
        re = np.zeros(3, dtype=np.int64)
        re[limb] = d_re = digit()
    if arms in ("im", "both"):
        im = np.zeros(3, dtype=np.int64)
        im[limb] = d_im = digit()
    a_all, wants = [], []
    for _ in range(batch):
        limbs, val, ba = _small_or_uniform(n, a_size, ab, a_bits, rng)
        a_all.append(fs.glwe_encrypt(sk, limbs, ab, k, rng))
        x = val * d_re + fs.rotate(val, n // 2) * (-d_im if flip_im else d_im)
        out_bits = ba + c_bits - cnv_offset
        assert out_bits > 0
        wants.append((x, out_bits))
    return SimpleNamespace(op="const", n=n, rank=rank, mode=mode, a=np.stack(a_all), re=re, im=im, ab=ab, rb=rb, res_size=res_size,
                           cnv_offset=cnv_offset, sk=sk, want=wants, bound=reference_bound(n, rank, k, cnv_offset))


def plain_reference_cases(kind, batch, ranks=(1, 2, 3), offsets=None, base2k=BASE2K, n=N):
    """test_glwe_mul_plain (in base2k - 1, out base2k - 2, k = 8 base2k + 1, a two-limb plaintext: :443-447, :473) and test_glwe_mul_const
    (one base, a 3-limb constant with a 17-bit digit in limb 0: :573-577, :626-632), rank 1..3, res_offset in 0..scale."""
    k = 8 * base2k + 1
    for rank in ranks:
        if kind == "plain":
            in_b, out_b = base2k - 1, base2k - 2
            scale = 2 * in_b
            for off in (range(scale) if offsets is None else offsets):
                yield ((kind, rank, off), mul_plain_case(n, rank, fs.limbs_for(k, in_b), 2, fs.limbs_for(k, out_b), in_b, out_b, scale + off, batch,
                                                         1200 + rank, k_enc=k))
        else:
            scale = 2 * base2k
            size = fs.limbs_for(k, base2k)
            for off in (range(scale) if offsets is None else offsets):
                yield ((kind, rank, off), mul_const_case(n, rank, size, size, base2k, base2k, scale + off, batch, 1300 + rank, wide=True))


def plain_control_cases(batch, base2k=BASE2K, n=N):
    """Negative controls 6 and 7."""
    k = 8 * base2k + 1
    size = fs.limbs_for(k, base2k)
    yield ("mul_const: the imaginary arm's sign flipped", mul_const_case(n, 1, size, size, base2k, base2k, 2 * base2k + 3, batch, 606, arms="both",
                                                                        wide=True, flip_im=True))
    in_b, out_b = base2k - 1, base2k - 2
    yield ("mul_plain: want from X b", mul_plain_case(n, 1, fs.limbs_for(k, in_b), 2, fs.limbs_for(k, out_b), in_b, out_b, 2 * in_b + 3, batch, 607,
                                                      k_enc=k, times_x=True))


# one shape per dispatch route of tests/test_gpu_mul_plain.py PLAIN_GRID / CONST_GRID (those with cnv_offset 0 cannot decrypt: B is not an integer)
PLAIN_ROUTES = {
    "plain-n256-into-per-ct": (mul_plain_case, dict(n=256, rank=1, a_size=4, b_size=3, res_size=5, ab=12, rb=12, cnv_offset=24, a_bits=9, b_bits=22,
                                                    a_bits_off=3, k_enc=40, seed=2561), True),
    "plain-n256-assign-shared-b1": (mul_plain_case, dict(n=256, rank=2, a_size=4, b_size=1, res_size=4, ab=13, rb=13, cnv_offset=5, a_bits=7, b_bits=5,
                                                         mode="assign", shared=True, seed=2562), True),
    "plain-n256-two-bases": (mul_plain_case, dict(n=256, rank=1, a_size=4, b_size=4, res_size=6, ab=12, rb=15, cnv_offset=30, a_bits=9, b_bits=28,
                                                  seed=2563), True),
    "plain-n4096-per-op": (mul_plain_case, dict(n=4096, rank=1, a_size=8, b_size=3, res_size=8, ab=12, rb=12, cnv_offset=31, a_bits=9, b_bits=29,
                                                shared=True, seed=40961), True),
    "plain-n4096-two-bases": (mul_plain_case, dict(n=4096, rank=1, a_size=6, b_size=3, res_size=6, ab=12, rb=14, cnv_offset=29, a_bits=9, b_bits=27,
                                                   seed=40962), True),
    "plain-n8192-mid-cnv-into": (mul_plain_case, dict(n=8192, rank=1, a_size=8, b_size=3, res_size=8, ab=12, rb=12, cnv_offset=31, a_bits=9, b_bits=29,
                                                      seed=81921), True),
    "plain-n8192-mid-cnv-assign-shared": (mul_plain_case, dict(n=8192, rank=2, a_size=16, b_size=1, res_size=16, ab=12, rb=12, cnv_offset=25, a_bits=20,
                                                               b_bits=12, mode="assign", shared=True, seed=81922), True),
    "plain-n8192-5-2": (mul_plain_case, dict(n=8192, rank=1, a_size=5, b_size=2, res_size=5, ab=12, rb=12, cnv_offset=20, a_bits=9, b_bits=18,
                                             seed=81923), True),
    # N = 2^16, 16 limbs, a 3-limb plaintext shared by the batch, cnv_offset = b.max_k (mul.rs:480-496)
    "plain-n65536-shared": (mul_plain_case, dict(n=65536, rank=1, a_size=16, b_size=3, res_size=16, ab=12, rb=12, cnv_offset=36, a_bits=20, b_bits=30,
                                                 shared=True, seed=655361), False),
    "const-n256-re-into": (mul_const_case, dict(n=256, rank=1, a_size=4, res_size=4, ab=12, rb=12, cnv_offset=24, limb=1, a_bits=9, arms="re",
                                                seed=2571), True),
    "const-n256-im-assign": (mul_const_case, dict(n=256, rank=2, a_size=5, res_size=5, ab=13, rb=13, cnv_offset=7, limb=0, digit_shift=6, a_bits=9,
                                                  arms="im", mode="assign", seed=2572), True),
    "const-n1024-two-bases-both": (mul_const_case, dict(n=1024, rank=1, a_size=5, res_size=4, ab=12, rb=16, cnv_offset=40, limb=2, a_bits=12, arms="both",
                                                        seed=10241), True),
    "const-n4096-both-into": (mul_const_case, dict(n=4096, rank=1, a_size=8, res_size=8, ab=12, rb=12, cnv_offset=31, limb=1, a_bits=12, arms="both",
                                                   seed=40971), True),
    "const-n4096-both-assign": (mul_const_case, dict(n=4096, rank=2, a_size=6, res_size=6, ab=12, rb=12, cnv_offset=31, limb=1, a_bits=12, arms="both",
                                                     mode="assign", seed=40972), True),
    "const-n65536-both": (mul_const_case, dict(n=65536, rank=1, a_size=16, res_size=16, ab=12, rb=12, cnv_offset=36, limb=2, a_bits=20, arms="both",
                                               seed=655371), False),
}


def plain_route_case(name, batch):
    builder, kw, _ = PLAIN_ROUTES[name]
    return builder(batch=batch, **kw)


def run_plain_oracle(ref, c):
    from tests import plain_oracle as po
    n, cols = c.n, c.rank + 1
    out = np.empty((len(c.a), c.res_size, cols, n), dtype=np.int64)
    for t, ct in enumerate(c.a):
        a = _vec(ct.copy())
        r = a if c.mode == "assign" else VecZnx(n, cols, c.res_size)
        if c.op == "plain":
            pt = _vec(c.pt[0 if c.shared else t].copy())
            if c.mode == "assign":
                po.glwe_mul_plain_assign(ref, c.cnv_offset, r, c.a_k, pt, c.b_k, c.ab)
            else:
                po.glwe_mul_plain(ref, c.cnv_offset, r, c.rb, a, c.a_k, pt, c.b_k, c.ab)
        elif c.mode == "assign":
            po.ckks_mul_pt_const_assign(ref, c.cnv_offset, r, c.rb, c.re, c.im)
        else:
            po.ckks_mul_pt_const_into(ref, c.cnv_offset, r, c.rb, a, c.ab, c.re, c.im)
        out[t] = r.data
    return out


def check_plain(label, c, out, fail=False):
    have = [_noise_int(out[t], c.rb, c.sk, c.want[t]) for t in range(len(out))]
    print(f"[noise] {label}: noise_have {max(have):.2f} (min {min(have):.2f}) noise_want {c.bound:.2f}")
    if fail:
        assert min(have) > c.bound, (label, have, c.bound, "a negative control met the bound")
    else:
        assert max(have) <= c.bound, (label, have, c.bound)
    return have
