"""Cases for the encrypt / trace / decrypt and encrypt / pack / decrypt tests (tests/ only): poulpy-core's test_glwe_trace_assign
(poulpy-core/src/test_suite/trace.rs) and test_glwe_packing (test_suite/glwe_packing.rs) as case builders, their negative controls, and
the oracle runners and noise checks that tests/test_trace_semantics.py (oracle) and tests/test_gpu_trace_semantics.py (device) share.
The builders call neither the oracle nor the device: there is one real automorphism key per Galois element (tests/fhe_sk.py), and
`want` comes from applying the definition step by step to the plaintext on exact integers, one more bit of precision per step and no
rounding; no knowledge of which coefficients survive goes in.

A trace step is a one-bit shift of the ciphertext and x <- x + phi_g(x) (glwe_trace.rs:164-174), so the phase becomes
(x + I) / 2 + phi_g((x + I) / 2) with I the integer polynomial the torus drops: the halving is only defined mod 1/2
(glwe_packing.rs:34-38).  Over the full trace, and over its last steps alone (the Galois elements 1 + N / 2^j fix or negate every
monomial they do not move to one a later step negates), every such I / 2 ends up doubled or cancelled and the result equals the
definition mod 1.  A trace through the FIRST steps only (-1, 5, 25, ...: the shapes of tests/test_gpu_parity.py::test_glwe_trace_shifted_stores)
leaves multiples of 2^-steps behind, so those cases compare 2^steps (have - want) mod 1 (`shift`): the top `steps` bits of a uniform
plaintext go unchecked, every other bit is checked, and the bound moves up by `steps` bits.
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


def trace_gals(n):
    """glwe_trace.rs:34-44: -1, then 5^(2^(i-1))."""
    log_n = n.bit_length() - 1
    return [-1] + [pow(5, 1 << i, 2 * n) for i in range(log_n - 1)]


def trace_noise_want(n, rank, key_base2k, k, k_key):
    """trace.rs:133-147, log2 of the deviation."""
    v = fs.var_noise_gglwe_product(n, key_base2k, 0.5, 0.5, 1.0 / 12.0, fs.SIGMA * fs.SIGMA, 0.0, rank, k, k_key)
    v += fs.SIGMA * fs.SIGMA * 4.0 ** -k
    v += n / 12.0 * 0.5 * rank * 4.0 ** -k
    return 0.5 * math.log2(v)


def _keys(sk, gals, key_base2k, k_key, dnum, rng, for_g=False):
    n = sk.shape[1]
    return [fs.automorphism_key(sk, g, key_base2k, k_key, dnum, 1, rng, encrypt_for=(g % (2 * n)) if for_g else None) for g in gals]


def _step(x, g):
    """x + phi_g(x) on exact integers: the caller reads the result at one more bit of precision."""
    return x + fs.automorphism(x, g)


def trace_case(n, rank, size, base2k, key_base2k, gals, batch, seed, k=None, k_key=None, dnum=None, upper_only=False, swap_keys=None,
               for_g=False, drop_halving=False):
    """trace.rs:36-154: a uniform plaintext at base2k, k bits (default size base2k), one automorphism key per element of `gals` at
    key_base2k (k_key bits, default k + key_base2k as :43, dnum = ceil(k / key_base2k) as :46); res in another base than the keys takes
    glwe_trace.rs:153-163.  Controls: swap_keys = (i, j) exchanges the keys of two steps, for_g makes every key for g instead of g^-1,
    drop_halving reads want with one halving less."""
    rng = seeded(seed)
    k = size * base2k if k is None else k
    assert fs.limbs_for(k, base2k) == size
    k_key = k + key_base2k if k_key is None else k_key
    dnum = fs.limbs_for(k, key_base2k) if dnum is None else dnum
    sk = fs.ternary_secret(n, rank, rng)
    keys = _keys(sk, gals, key_base2k, k_key, dnum, rng, for_g=for_g)
    if swap_keys is not None:
        i, j = swap_keys
        keys[i], keys[j] = keys[j], keys[i]
    full = trace_gals(n)
    clean = [g % (2 * n) for g in gals] == [g % (2 * n) for g in full[len(full) - len(gals):]]
    cts, wants = [], []
    for _ in range(batch):
        pt = fs.uniform_digits((size, n), base2k, rng)
        cts.append(fs.glwe_encrypt(sk, pt, base2k, k, rng))
        x = fs.to_int(pt, base2k)
        for g in gals:
            x = _step(x, g)
        if len(gals) == len(full):      # trace.rs:124: the full trace keeps coefficient 0 and nothing else
            assert x[0] == fs.to_int(pt, base2k)[0] << len(gals) and not np.any(x[1:])
        wants.append((x, size * base2k + len(gals) - int(drop_halving)))
    return SimpleNamespace(op="trace", n=n, rank=rank, base2k=base2k, key_base2k=key_base2k, gals=list(gals), keys=keys, a=np.stack(cts),
                           sk=sk, want=wants, shift=0 if clean else len(gals), noise_want=trace_noise_want(n, rank, key_base2k, k, k_key),
                           upper_only=upper_only, conv_size=fs.limbs_for(k, key_base2k))


# ---- packing ----
def _pack_plain(pts, n, log_gap_out):
    """glwe_packing.rs:145-170 with pack_internal (:29-83) on exact integer plaintexts {index: (n,) object array}: every step reads
    its result at one more bit.  -> the packed plaintext, log_n bits finer than the inputs."""
    log_n = n.bit_length() - 1
    gals = trace_gals(n)
    a = dict(pts)
    for i in range(log_n - log_gap_out):
        t = 1 << (log_n - 1 - i)
        g = gals[i]
        for j in range(t):
            lo, hi = a.pop(j, None), a.pop(j + t, None)
            if lo is not None and hi is not None:       # a + b X^t + phi(a - b X^t), as :45-68 computes it
                r = fs.rotate(lo, -t)
                lo = fs.rotate((r + hi) - fs.automorphism(r - hi, g), t)
            elif lo is not None:                        # a + phi(a)
                lo = _step(lo, g)
            elif hi is not None:                        # b X^t - phi(b X^t)
                r = fs.rotate(hi, t)
                lo = r - fs.automorphism(r, g)
            if lo is not None:
                a[j] = lo
    x = a[0]
    for g in gals[log_n - log_gap_out:]:
        x = _step(x, g)
    return x


def pack_case(n, rank, size, ct_base2k, key_base2k, indices, log_gap_out, batch, seed, k_ct=None, bound=None, want_gap=None, swap=None):
    """glwe_packing.rs:39-148: the message i -> i (+ 17 per batch member) at precision 2 base2k + 1 (base2k = the keys' base, :44), rotated
    so that the ciphertext of index j carries coefficient j in its coefficient 0 (:110-132); keys of k_ct + key_base2k bits, dnum =
    ceil(k_ct / key_base2k) (:47-49).  Controls: want_gap computes want with another log_gap_out, swap = (i, j) hands the device the
    ciphertexts of two indices exchanged.

    The bound.  The reference's own assertion says nothing (log2 of the deviation <= k_ct - out_base2k, a positive number: :148).  A
    pack step is a shift and an automorphism-add like a trace step, so the bound is the trace's noise_want (trace.rs:133-147) at the
    same key parameters, + 1, the upper side only.  The oracle meets it at every one-base shape below; at the reference's two-base rank-3
    shape it does not (each of the three mask columns is converted between the bases at every step), so there `bound` is the oracle's
    worst noise_have over 8 seeds (9100..9107, 3 ciphertexts each) + 1 bit:
      N = 64, rank 3, ciphertexts base2k 16, keys 17, k_ct 69: noise_have -62.97 -63.06 -63.00 -63.01 -62.83 -62.87 -63.21 -63.08
        (formula: -64.14 + 1) -> bound -61.83
      N = 64, rank 3, ciphertexts base2k 12, keys 13, k_ct 53: noise_have -47.01 -46.96 -46.94 -46.89 -46.85 -46.85 -46.91 -46.82
        (formula: -48.14 + 1) -> bound -45.82
    A broken convention gives noise at the message's scale (2^-2 base2k - 1 + log2 N), ten bits and more above either."""
    rng = seeded(seed)
    log_n = n.bit_length() - 1
    k_ct = size * ct_base2k if k_ct is None else k_ct
    assert fs.limbs_for(k_ct, ct_base2k) == size
    pt_k = 2 * key_base2k + 1
    assert pt_k <= k_ct
    k_key = k_ct + key_base2k
    dnum = fs.limbs_for(k_ct, key_base2k)
    sk = fs.ternary_secret(n, rank, rng)
    keys = _keys(sk, trace_gals(n), key_base2k, k_key, dnum, rng)
    cts = {j: [] for j in indices}
    wants = []
    for b in range(batch):
        data = np.arange(n, dtype=np.int64) + 17 * b
        pt = fs.encode(data, ct_base2k, pt_k, size)
        pts = {}
        for j in indices:
            pj = fs.rotate(pt, -j)
            cts[j].append(fs.glwe_encrypt(sk, pj, ct_base2k, k_ct, rng))
            pts[j] = fs.to_int(pj, ct_base2k)
        x = _pack_plain(pts, n, log_gap_out)
        unit = 1 << (size * ct_base2k - pt_k + log_n)
        for j in indices:       # glwe_packing.rs:138-146: coefficient j carries j
            assert x[j] == int(data[j]) * unit, (j, x[j])
        if want_gap is not None:
            x = _pack_plain(pts, n, want_gap)
        wants.append((x, size * ct_base2k + log_n))
    a = {j: np.stack(v) for j, v in cts.items()}
    if swap is not None:
        i, j = swap
        a[i], a[j] = a[j], a[i]
    nw = trace_noise_want(n, rank, key_base2k, k_ct, k_key)
    return SimpleNamespace(op="pack", n=n, rank=rank, base2k=ct_base2k, key_base2k=key_base2k, gals=trace_gals(n), keys=keys, a=a,
                           indices=list(indices), log_gap_out=log_gap_out, sk=sk, want=wants, shift=0, noise_want=nw if bound is None else bound - 1.0,
                           upper_only=True, conv_size=fs.limbs_for(k_ct, key_base2k), size=size)


# ---- the reference's loops and the controls (N = 256, base2k 17) ----
def reference_cases(kind, batch, base2k=BASE2K, n=N):
    if kind == "trace":         # trace.rs:36-46: result at base2k, keys at base2k - 1, k = 4 base2k + 1, rank 1..2, the full trace
        k = 4 * base2k + 1
        for rank in (1, 2):
            yield ((kind, rank), trace_case(n, rank, fs.limbs_for(k, base2k), base2k, base2k - 1, trace_gals(n), batch, 700 + rank, k=k))
    else:                       # glwe_packing.rs:40-49 at N = 64 as tests/test_gpu_parity.py: ciphertexts base2k - 1, keys base2k, rank 3, every 5th
        k = 4 * base2k + 1
        yield ((kind, 3), pack_case(64, 3, fs.limbs_for(k, base2k - 1), base2k - 1, base2k, list(range(0, 64, 5)), 0, batch, 710, k_ct=k,
                                    bound=-61.83))


def control_cases(batch, base2k=BASE2K, n=N):
    """Negative controls 8-12 as (label, case)."""
    k = 4 * base2k + 1
    size = fs.limbs_for(k, base2k)
    gals = trace_gals(n)
    yield ("trace: keys of two steps exchanged", trace_case(n, 1, size, base2k, base2k - 1, gals, batch, 801, k=k, swap_keys=(2, 5)))
    yield ("trace: keys for g instead of g^-1", trace_case(n, 1, size, base2k, base2k - 1, gals, batch, 802, k=k, for_g=True))
    yield ("trace: want lacks one halving", trace_case(n, 1, size, base2k, base2k - 1, gals, batch, 803, k=k, drop_halving=True))
    yield ("pack: log_gap_out off by one in want", pack_case(64, 1, 3, 13, 13, list(range(0, 64, 4)), 2, batch, 804, want_gap=3))
    yield ("pack: two ciphertexts' indices exchanged", pack_case(64, 1, 3, 13, 13, [0, 5, 17, 32, 33, 63], 0, batch, 805, swap=(5, 32)))


# ---- running and checking ----
def _gal(g, n):
    return g if g < 0 else g % (2 * n)


def run_oracle(ref, c):
    n, cols = c.n, c.rank + 1
    pms = [prepare(ref, key) for key in c.keys]
    gals = [_gal(g, n) for g in c.gals]
    if c.op == "trace":
        out = np.empty_like(c.a)
        for b, ct in enumerate(c.a):
            v = VecZnx(n, cols, ct.shape[0], np.ascontiguousarray(ct).copy())
            if c.base2k == c.key_base2k:
                ref.glwe_trace_assign(v, c.base2k, gals, pms)
            else:
                ref.glwe_trace_assign_bases(v, c.base2k, c.conv_size, c.key_base2k, gals, pms)
            out[b] = v.data
        return out
    batch = len(c.want)
    out = np.empty((batch, c.size, cols, n), dtype=np.int64)
    for b in range(batch):
        cts = {j: VecZnx(n, cols, c.size, np.ascontiguousarray(c.a[j][b]).copy()) for j in c.indices}
        res = VecZnx(n, cols, c.size)
        if c.base2k == c.key_base2k:
            ref.glwe_pack(res, c.base2k, cts, c.log_gap_out, gals, pms)
        else:
            ref.glwe_pack_bases(res, c.base2k, c.key_base2k, c.conv_size, cts, c.log_gap_out, gals, pms)
        out[b] = res.data
    return out


def noise_log2(ct, base2k, sk, want, shift=0):
    """log2 of the deviation of 2^shift (phase(ct) - want) mod 1; want = (exact integers, bits)."""
    x, bits = want
    ka = base2k * ct.shape[0]
    kk = max(ka, bits)
    d = (fs.to_int(fs.glwe_phase(ct, sk), base2k) << (kk - ka)) - (x << (kk - bits))
    q = 1 << kk
    d = ((d << shift) + q // 2) % q - q // 2
    sd = float(np.std(np.ldexp(np.array([float(v) for v in d], dtype=np.float64), -kk)))
    return math.log2(sd) if sd > 0 else -math.inf


def check(label, c, out, fail=False):
    """trace.rs:149-153: |noise_have - noise_want| < 1 (the upper side only where the case says so), every output against its own
    plaintext; a control's best noise lies beyond the upper side."""
    have = [noise_log2(out[b], c.base2k, c.sk, c.want[b], c.shift) for b in range(len(out))]
    want = c.noise_want + c.shift
    print(f"[noise] {label}: noise_have {max(have):.2f} (min {min(have):.2f}) noise_want {want:.2f} +- 1" + (" (upper side)" if c.upper_only else ""))
    if fail:
        assert min(have) > want + 1.0, (label, have, want, "a negative control met the bound")
    else:
        assert max(have) < want + 1.0, (label, have, want)
        assert c.upper_only or min(have) > want - 1.0, (label, have, want)
    return have


# ---- the device's routes (shapes after tests/test_gpu_parity.py::test_glwe_trace_batched, _shifted_stores, _pack_batched) ----
# name -> (builder, keywords, knobs of the device run); host: the oracle half also runs in the host suite
def _route(builder, host=True, fuse=(True, True), **kw):
    return builder, kw, SimpleNamespace(host=host, fuse=fuse)


ROUTES = {
    # the five-kernel path: N = 512, the full 9-step trace
    "trace-n512-full": _route(trace_case, n=512, rank=1, size=3, base2k=13, key_base2k=13, gals=trace_gals(512), seed=512),
    # N = 4096 (k_small_inv<.., AU>): -1 first with 4 limbs, and two steps with more key limbs than the ciphertext's
    "trace-n4096-first4": _route(trace_case, n=4096, rank=1, size=4, base2k=12, key_base2k=12, gals=[-1, 5, 25, 625], k_key=48, seed=4096),
    "trace-n4096-5-25": _route(trace_case, n=4096, rank=1, size=3, base2k=12, key_base2k=12, gals=[5, 25], seed=4097),
    # N = 8192, the fused pipeline and the per-op composition; rank 2 at base2k 14
    "trace-n8192-fused": _route(trace_case, n=8192, rank=1, size=4, base2k=12, key_base2k=12, gals=[-1, 5, 25], k_key=48, seed=8192),
    "trace-n8192-unfused": _route(trace_case, host=False, fuse=(False, False), n=8192, rank=1, size=4, base2k=12, key_base2k=12, gals=[-1, 5, 25],
                                  k_key=48, seed=8192),
    "trace-n8192-rank2": _route(trace_case, n=8192, rank=2, size=3, base2k=14, key_base2k=14, gals=[-1, 5], k_key=42, seed=8193),
    # N = 2^16, 8 limbs, base2k 12: the shift rides on the spectral tail, 16-bit body operand
    "trace-n65536-first4": _route(trace_case, host=False, n=65536, rank=1, size=8, base2k=12, key_base2k=12, gals=[-1, 5, 25, 625], k_key=96,
                                  seed=65536),
    # the result in another base than the keys: the reference's own bases (trace.rs:36-39 at base2k 14), and the last three steps at N = 4096
    "trace-bases-n256-full": _route(trace_case, n=256, rank=1, size=5, base2k=14, key_base2k=13, gals=trace_gals(256), k=57, seed=256),
    "trace-bases-n4096-last3": _route(trace_case, n=4096, rank=1, size=5, base2k=13, key_base2k=12, gals=trace_gals(4096)[-3:], k=53, seed=4098),
    "pack-n64-dense-gap4": _route(pack_case, n=64, rank=1, size=3, ct_base2k=13, key_base2k=13, indices=list(range(0, 64, 4)), log_gap_out=2, seed=64),
    "pack-n64-sparse": _route(pack_case, n=64, rank=1, size=3, ct_base2k=13, key_base2k=13, indices=[0, 5, 17, 32, 33, 63], log_gap_out=0, seed=65),
    "pack-n256-rank2": _route(pack_case, n=256, rank=2, size=3, ct_base2k=13, key_base2k=13, indices=[0, 8, 16, 128, 136], log_gap_out=3, seed=257),
    "pack-n4096-fused": _route(pack_case, n=4096, rank=1, size=3, ct_base2k=13, key_base2k=13, indices=[0, 512, 1024, 2048, 3584], log_gap_out=9,
                               seed=4099),
    # the reference's own bases (glwe_packing.rs:40-49 at base2k 13): ciphertexts base2k - 1, keys base2k, rank 3, every 5th
    "pack-bases-n64-rank3": _route(pack_case, n=64, rank=3, size=5, ct_base2k=12, key_base2k=13, indices=list(range(0, 64, 5)), log_gap_out=0,
                                   k_ct=53, bound=-45.82, seed=66),
}


def route_case(name, batch):
    builder, kw, knobs = ROUTES[name]
    return builder(batch=batch, **kw), knobs
