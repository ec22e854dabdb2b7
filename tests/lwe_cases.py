"""Cases for the LWE side under real keys (tests/ only): LWE key switch, LWE <-> GLWE conversion, CGGI blind rotation, the gate
bootstrap chain and circuit bootstrapping, restated from poulpy-core's test_suite/keyswitch/lwe_ct.rs and test_suite/conversion.rs and from
poulpy-bin-fhe's blind_rotation/tests/test_suite/generic_blind_rotation.rs and circuit_bootstrapping/tests/circuit_bootstrapping.rs, with
their negative controls.  As in tests/core_cases.py the builders call neither
the oracle nor the device: secrets, keys, ciphertexts and tables come from tests/fhe_sk.py, and a case carries what every output must decrypt
to and a bound.  tests/test_lwe_semantics.py runs the cases on the oracle, tests/test_gpu_lwe_semantics.py through the batched entry points.

Every case is a batch of 3 inputs with their own messages.  An LWE has one coefficient, so its noise is the root mean square of the batch's
errors; a GLWE's is the deviation over its coefficients, the worst of the batch.

Bounds.  The conversions take the reference's key-switch bound (fs.keyswitch_bound, rank_in of the key in question).  The reference's
conversion tests give their keys dnum = 2 rows for a 4-limb input, so the key switch drops the input's lower digits; the formula has no term
for that (it is why those tests assert limb 0 alone), and conversion_bound adds it: every mask coefficient loses a balanced remainder of
variance 2^(-2 dnum dsize key_base2k) / 12, times the secret's variance, over the coefficients the secret has.  Blind rotation: each of the
n_lwe steps adds (X^a - 1) (acc [.] BRK_i), that is twice the variance of one GGSW product (fs.noise_ggsw_product with a noise-free
accumulator, the message variance of a binary key bit, P(1) / n); where the key has more limbs than the accumulator every step also rounds
the accumulator, 2^(-2 k_res) / 12 per column against the secret; the sum, plus the reference's usual bit.  The standard variant (block
size 1) normalizes once, at the end, so the digits it decomposes grow with the step and its variance goes with n_lwe^2 instead of n_lwe
(rotation_variance).  The chain adds the key switch's variance to the rotation's."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from poulpy_amd.layouts import MatZnx, VecZnx
from tests import fhe_sk as fs
from tests.helpers import seeded

N = 256
BASE2K = 17          # poulpy-cpu-ref/src/tests.rs:154-158
K_PT = 8             # lwe_ct.rs:36, conversion.rs:121
MESSAGES = (17, -45, 101)   # 17 is the reference's; the others make a mixed-up batch index show


# ---- bounds ----
def conversion_bound(n, k_ksk, dnum, dsize, key_base2k, rank_in, k_in, secret_coeffs):
    """fs.keyswitch_bound plus the digits a key of dnum rows does not reach (module docstring); secret_coeffs: non-zero positions the input
    secret can have (n_lwe for an embedded LWE secret, rank n for a GLWE secret)."""
    var = 4.0 ** (fs.keyswitch_bound(n, k_ksk, dnum, dsize, key_base2k, rank_in) - 1.0)
    reach = dnum * dsize * key_base2k
    if reach < k_in:
        var += secret_coeffs * 0.5 * 4.0 ** -reach / 12.0
    return 0.5 * math.log2(var) + 1.0


def rotation_variance(n, rank, n_lwe, block_size, base2k, k_res, k_brk):
    p_one = 1.0 / (block_size + 1)      # binary_block_secret: one of block_size + 1 outcomes per position; block 1: a fair bit
    step = 4.0 ** fs.noise_ggsw_product(n, base2k, 0.5, p_one / n, 0.0, 1.0 / 12.0, fs.SIGMA * fs.SIGMA, 0.0, rank, k_res, k_brk)
    if block_size == 1:
        # execute_standard (cggi/algorithm.rs:429-442) normalizes at the end only: step t decomposes an accumulator that is the table plus
        # 2 t normalized terms, digits of variance (1 + 2 t) times a normalized one's, and the gadget noise grows with it; sum over t: n_lwe^2
        return 2.0 * step * n_lwe * n_lwe
    var = 2.0 * step * n_lwe
    if k_brk > k_res:
        var += (n_lwe // block_size) * (1.0 + rank * n * 0.5) * 4.0 ** -k_res / 12.0
    return var


# ---- conversions ----
def _lwe_batch(sk, base2k, k, rng):
    pts = [fs.encode_int(m, base2k, K_PT) for m in MESSAGES]
    return pts, np.stack([fs.lwe_encrypt(sk, pt, base2k, k, rng) for pt in pts])


def lwe_keyswitch_case(n, n_in, n_out, in_b, key_b, out_b, k_ct, seed, dsize=1):
    """keyswitch/lwe_ct.rs:27-127: k_ksk = k_ct + key_b dsize, dnum = ceil(k_ct / (key_b dsize)); the output decrypts under sk_out to the
    message re-expressed in the output base."""
    rng = seeded(seed)
    k_ksk = k_ct + key_b * dsize
    dnum = -(-k_ct // (key_b * dsize))
    sk_in, sk_out = fs.ternary_lwe_secret(n_in, rng), fs.ternary_lwe_secret(n_out, rng)
    key = fs.lwe_switching_key(sk_in, sk_out, n, key_b, k_ksk, dnum, rng, dsize=dsize)
    pts, cts = _lwe_batch(sk_in, in_b, k_ct, rng)
    res_size = fs.limbs_for(k_ct, out_b)
    return SimpleNamespace(op="lwe_ks", n=n, n_in=n_in, n_out=n_out, rank=1, rank_out=1, dsize=dsize, key=key, key_base2k=key_b, a=cts,
                           a_base2k=in_b, res_size=res_size, res_base2k=out_b, sk_out=sk_out,
                           want=[fs.rebase(pt, in_b, out_b, res_size) for pt in pts],
                           bound=conversion_bound(n, k_ksk, dnum, dsize, key_b, 1, k_ct, n_in))


def glwe_from_lwe_case(n, n_lwe, rank, lwe_b, key_b, glwe_b, k_lwe, k_ksk, k_glwe, dnum, seed, embed=True):
    """conversion.rs:116-219: coefficient 0 of the GLWE decrypts under sk_glwe to the LWE's message (the other coefficients hold products
    of the mask with the secret and mean nothing).  embed=False builds the key without phi_{-1} (a negative control)."""
    rng = seeded(seed)
    sk_glwe, sk_lwe = fs.ternary_secret(n, rank, rng), fs.ternary_lwe_secret(n_lwe, rng)
    key = fs.lwe_to_glwe_key(sk_lwe, sk_glwe, key_b, k_ksk, dnum, rng, embed=embed)
    pts, cts = _lwe_batch(sk_lwe, lwe_b, k_lwe, rng)
    glwe_size = fs.limbs_for(cts.shape[1] * lwe_b, key_b)       # conversion/lwe_to_glwe.rs: the rank-1 GLWE in the key's base
    res_size = fs.limbs_for(k_glwe, glwe_b)
    return SimpleNamespace(op="glwe_from_lwe", n=n, n_lwe=n_lwe, rank=1, rank_out=rank, dsize=1, key=key, key_base2k=key_b, a=cts,
                           a_base2k=lwe_b, glwe_size=glwe_size, res_size=res_size, res_base2k=glwe_b, sk_out=sk_glwe,
                           want=[fs.rebase(pt, lwe_b, glwe_b, res_size) for pt in pts],
                           bound=conversion_bound(n, k_ksk, dnum, 1, key_b, 1, k_lwe, n_lwe))


def lwe_from_glwe_case(n, n_lwe, rank, glwe_b, key_b, lwe_b, k_glwe, k_ksk, k_lwe, dnum, a_idx, seed, embed=True, read_idx=None):
    """conversion.rs:237-343: the plaintext has the message at a_idx and other non-zero values everywhere else; the LWE decrypts under sk_lwe
    to the message.  read_idx (a negative control) extracts another coefficient; embed=False builds the key without phi_{-1}."""
    rng = seeded(seed)
    sk_glwe, sk_lwe = fs.ternary_secret(n, rank, rng), fs.ternary_lwe_secret(n_lwe, rng)
    key = fs.glwe_to_lwe_key(sk_lwe, sk_glwe, key_b, k_ksk, dnum, rng, embed=embed)
    a_size, res_size = fs.limbs_for(k_glwe, glwe_b), fs.limbs_for(k_lwe, lwe_b)
    cts, wants = [], []
    for m in MESSAGES:
        data = rng.integers(1, 100, n) * np.where(rng.random(n) < 0.5, -1, 1)
        data[a_idx] = m
        other = (n - a_idx) % n
        if other != a_idx and abs(int(data[other])) == abs(m):
            data[other] += 1
        cts.append(fs.glwe_encrypt(sk_glwe, fs.encode(data, glwe_b, K_PT, a_size), glwe_b, k_glwe, rng))
        wants.append(fs.rebase(fs.encode_int(m, glwe_b, K_PT), glwe_b, lwe_b, res_size))
    return SimpleNamespace(op="lwe_from_glwe", n=n, n_lwe=n_lwe, rank=rank, rank_out=1, dsize=1, key=key, key_base2k=key_b, a=np.stack(cts),
                           a_base2k=glwe_b, a_idx=a_idx if read_idx is None else read_idx, res_size=res_size, res_base2k=lwe_b, sk_out=sk_lwe,
                           want=wants, bound=conversion_bound(n, k_ksk, dnum, 1, key_b, rank, k_glwe, rank * n))


def reference_conversions(n=N, base2k=BASE2K):
    """The three reference tests at their own parameters, (label, case); lwe_from_glwe at the reference's a_idx = 1 and at both ends."""
    k = 4 * base2k + 1
    yield "lwe_keyswitch", lwe_keyswitch_case(n, n >> 1, n >> 1, base2k - 1, base2k, base2k - 2, k, seed=11)
    yield "glwe_from_lwe", glwe_from_lwe_case(n, 22, 2, base2k - 2, base2k, base2k - 1, k, 5 * base2k + 1, k, 2, seed=12)
    for a_idx in (0, 1, n - 1):
        yield f"lwe_from_glwe a_idx {a_idx}", lwe_from_glwe_case(n, 22, 2, base2k - 1, base2k, base2k - 2, k, 5 * base2k + 1, k, 2, a_idx,
                                                                 seed=13 + a_idx)


def conversion_controls(n=N, base2k=BASE2K):
    k = 4 * base2k + 1
    yield ("LWE -> GLWE key without phi_-1",
           glwe_from_lwe_case(n, 22, 2, base2k - 2, base2k, base2k - 1, k, 5 * base2k + 1, k, 2, seed=12, embed=False))
    yield ("GLWE -> LWE key without phi_-1",
           lwe_from_glwe_case(n, 22, 2, base2k - 1, base2k, base2k - 2, k, 5 * base2k + 1, k, 2, 1, seed=14, embed=False))
    yield ("lwe_from_glwe read at N - a_idx",
           lwe_from_glwe_case(n, 22, 2, base2k - 1, base2k, base2k - 2, k, 5 * base2k + 1, k, 2, 1, seed=14, read_idx=n - 1))


def shape_conversions(n, bases, limbs):
    """The three conversions at one ring degree, bases = (input, key, output) base2k, a key that reaches every input digit, (label, case)."""
    in_b, key_b, out_b = bases
    k = limbs * in_b
    k_ksk, dnum = k + key_b, -(-k // key_b)
    yield "lwe_keyswitch", lwe_keyswitch_case(n, 300, 77, in_b, key_b, out_b, k, seed=n + 1)
    yield "glwe_from_lwe", glwe_from_lwe_case(n, 300, 2, in_b, key_b, out_b, k, k_ksk, k, dnum, seed=n + 2)
    yield "lwe_from_glwe a_idx N - 1", lwe_from_glwe_case(n, 33, 2, in_b, key_b, out_b, k, k_ksk, k, dnum, n - 1, seed=n + 3)
    yield "lwe_from_glwe a_idx 5", lwe_from_glwe_case(n, 600, 1, in_b, key_b, out_b, k, k_ksk, k, dnum, 5, seed=n + 4)


def prepare(mod, key):
    rows, cols_in, size, cols_out, n = key.shape
    pm = mod.vmp_pmat_alloc(rows, cols_in, cols_out, size)
    mod.vmp_prepare(pm, MatZnx(n, rows, cols_in, cols_out, size, np.ascontiguousarray(key)))
    return pm


def run_conversion_oracle(ref, c):
    pm = prepare(ref, c.key)
    out = []
    for ct in c.a:
        if c.op == "lwe_ks":
            out.append(ref.lwe_keyswitch(c.n_out, c.res_size, c.res_base2k, ct, c.a_base2k, pm, c.dsize, c.key_base2k))
        elif c.op == "glwe_from_lwe":
            r = VecZnx(c.n, c.rank_out + 1, c.res_size)
            ref.glwe_from_lwe(r, c.res_base2k, ct, c.a_base2k, c.glwe_size, pm, c.dsize, c.key_base2k)
            out.append(r.data.copy())
        else:
            a = VecZnx(c.n, c.rank + 1, ct.shape[0], np.ascontiguousarray(ct))
            out.append(ref.lwe_from_glwe(c.n_lwe, c.res_size, c.res_base2k, a, c.a_base2k, c.a_idx, pm, c.dsize, c.key_base2k))
    return np.stack(out)


def _log2_abs(e):
    return math.log2(abs(e)) if e != 0 else -math.inf


def check_conversion(label, c, out, fail=False):
    """The reference's assertion (limb 0 of the decryption = limb 0 of the re-expressed plaintext) and the noise against the bound; a control
    must miss: every element's error beyond the bound, or limb 0 wrong for every element."""
    errs, limb0 = [], []
    for b in range(len(out)):
        if c.op == "glwe_from_lwe":
            phase = fs.glwe_phase(out[b], c.sk_out)[:, :1]
        else:
            phase = fs.lwe_phase(out[b], c.sk_out)
        errs.append(float(fs.torus_diff(phase, c.res_base2k, c.want[b], c.res_base2k)[0]))
        limb0.append(int(fs.normalize(phase, c.res_base2k)[0, 0]) == int(c.want[b][0, 0]))
    have = fs.rms_log2(errs)
    print(f"[noise] {label}: noise_have {have:.2f} (best {min(_log2_abs(e) for e in errs):.2f}) noise_want {c.bound:.2f} limb 0 {limb0}")
    if fail:
        assert min(_log2_abs(e) for e in errs) > c.bound or not any(limb0), (label, errs, c.bound, limb0, "a negative control decrypted")
    else:
        assert all(limb0), (label, limb0)
        assert have <= c.bound, (label, errs, c.bound)
    return have


# ---- blind rotation ----
def f_table(x):
    return 2 * x + 1        # generic_blind_rotation.rs:127


def log_modulus_for(bound, log_mod=4):
    """The message modulus a rotation of this noise bound leaves room for: the table's values are 2^-(log_mod + 1) apart, and half of that
    must stay four times above the bound (itself twice the expected deviation); the reference's 16 values where there is room."""
    return max(1, min(log_mod, int(math.floor(-bound - 4.0))))


def blind_rotation_case(n, rank, n_lwe, block_size, dnum, brk_size, res_size, base2k, seed, ext=1, lwe_base2k=None, k_lwe=24, xs=(15, 6, 9),
                        tail_bit=None, reverse_rows=False, wrong_negate=False, with_drift=True, plant=None, gate=False):
    """generic_blind_rotation.rs:37-172: f(x) = 2x + 1 over 2^log_mod values in a table of one limb (k_lut = base2k), LWEs of x at
    log_mod + 1 bits under a block-binary secret, direction Left (negated exponents).  want is the whole rotated table: lut_rotate by
    b + <a, s> mod 2 N ext from the exact mod_switch_2n.

    log_mod is 4 as in the reference unless the shape's noise bound leaves no room (log_modulus_for); `limb0` says whether the bound keeps the
    noise out of limb 0 altogether, as the reference's parameters do - otherwise the comparison is on the decoded values of all N
    coefficients.  The LWE takes the rotation's base2k where mod_switch_2n rounds one limb (base2k > log2(2 N ext) + 1); else 17: the
    reference's other branch, which concatenates limbs, keeps one bit too many and negates the first limb only (test_lwe_semantics.py).

    tail_bit: n_lwe is not a multiple of block_size and the secret's last coefficient is this bit (chunks_exact drops the tail: 1 cannot
    decrypt).  reverse_rows, wrong_negate, with_drift=False: negative controls.  plant: the LWE's phase this many eighths of a table step
    away from x's (the table's half-step drift is what reads it right).  gate: add the GLWE -> LWE key of the gate bootstrap."""
    rng = seeded(seed)
    k_brk, k_res = brk_size * base2k, res_size * base2k
    var = rotation_variance(n, rank, n_lwe, block_size, base2k, k_res, k_brk)
    bound = 0.5 * math.log2(var) + 1.0
    log_mod = log_modulus_for(bound)
    mod = 1 << log_mod
    n2 = 2 * n * ext
    log2n = (n2 - 1).bit_length() + 1
    if lwe_base2k is None:
        lwe_base2k = base2k if base2k > log2n else 17
    assert lwe_base2k > log2n
    sk_glwe = fs.ternary_secret(n, rank, rng)
    if tail_bit is None:
        sk_lwe = fs.binary_block_secret(n_lwe, block_size, rng)
    else:
        full = n_lwe - n_lwe % block_size
        assert full < n_lwe
        sk_lwe = np.concatenate([fs.binary_block_secret(full, block_size, rng), np.zeros(n_lwe - full, dtype=np.int64)])
        sk_lwe[-1] = tail_bit
    brk = fs.blind_rotation_key(sk_glwe, sk_lwe, base2k, k_brk, dnum, rng)
    if reverse_rows:
        assert not np.array_equal(sk_lwe, sk_lwe[::-1])
        brk = np.ascontiguousarray(brk[::-1])
    f = [f_table(i) for i in range(mod)]
    lut, drift = fs.lut_set(f, log_mod + 1, n, ext, base2k, base2k, with_drift=with_drift)
    lut_ok, _ = fs.lut_set(f, log_mod + 1, n, ext, base2k, base2k)
    xs = [x % mod for x in xs]
    lwes, wants = [], []
    for x in xs:
        if plant is None:
            pt = fs.encode_int(x, lwe_base2k, log_mod + 1)
        else:
            pt = fs.encode_int(8 * x + plant, lwe_base2k, log_mod + 4)
        lwe = fs.lwe_encrypt(sk_lwe, pt, lwe_base2k, k_lwe, rng)
        lwe_2n = fs.mod_switch_2n(n2, lwe, lwe_base2k, True)
        rot = (int(lwe_2n[0]) + int(lwe_2n[1:] @ sk_lwe)) % n2
        lwes.append(lwe)
        wants.append(fs.lut_rotate(lut_ok, rot)[0])
    c = SimpleNamespace(op="br", n=n, rank=rank, n_lwe=n_lwe, block_size=block_size, dnum=dnum, brk_size=brk_size, res_size=res_size,
                        base2k=base2k, ext=ext, lwe=np.stack(lwes), lwe_base2k=lwe_base2k, negate=not wrong_negate, n2=n2, lut=lut, brk=brk,
                        sk_glwe=sk_glwe, sk_lwe=sk_lwe, xs=xs, log_mod=log_mod, want=wants, var=var, bound=bound,
                        limb0=bound <= -(base2k + 2.0), drift=drift)
    if gate:
        k_ksk = (res_size + 1) * base2k
        c.ksk = fs.glwe_to_lwe_key(sk_lwe, sk_glwe, base2k, k_ksk, res_size, rng)
        c.gate_want = [fs.encode_int(f_table(x) % (2 * mod), base2k, log_mod + 1, res_size) for x in xs]
        ks_var = 4.0 ** (fs.keyswitch_bound(n, k_ksk, res_size, 1, base2k, rank) - 1.0)
        c.gate_bound = 0.5 * math.log2(var + ks_var) + 1.0
    return c


# generic_blind_rotation.rs:37-46 at fft64_ref.rs:24-40: N = 512, n_lwe = 224, base2k 19, key 3 limbs x 2 rows, result 2 limbs
REF_ROTATION = dict(n=512, rank=1, n_lwe=224, dnum=2, brk_size=3, res_size=2, base2k=19)
# the controls' shape: short enough for the oracle to take a moment, the reference's bases
SMALL = dict(n=256, rank=1, n_lwe=21, block_size=7, dnum=2, brk_size=3, res_size=2, base2k=19)
ROTATION_CONTROLS = [
    ("key rows in reversed LWE order", dict(reverse_rows=True), True),
    ("mod_switch_2n negated against the table's direction", dict(wrong_negate=True), True),
    ("phase an eighth of a step below x's, table with its drift", dict(plant=-1), False),
    ("phase an eighth of a step below x's, table without its drift", dict(plant=-1, with_drift=False), True),
    ("trailing partial block, its secret bit 0", dict(n_lwe=23, tail_bit=0), False),
    ("trailing partial block, its secret bit 1 (chunks_exact drops it)", dict(n_lwe=23, tail_bit=1), True),
]


def brk_prepared(mod, c):
    """The n_lwe prepared GGSWs as one (n_lwe, doubles) array."""
    return np.stack([prepare(mod, k).data.reshape(-1) for k in c.brk])


def run_rotation_oracle(ref, c):
    """mod_switch_2n then the rotation, on the oracle: (lwe_2n (batch, n_lwe + 1), res (batch, res_size, rank + 1, n))."""
    brk = brk_prepared(ref, c)
    xpa = ref.blind_rotation_x_pow_a() if (c.block_size > 1 or c.ext > 1) else np.zeros((1, 1))
    lwe_2n = np.stack([ref.mod_switch_2n(c.n2, lwe, c.lwe_base2k, c.negate) for lwe in c.lwe])
    out = np.empty((len(c.lwe), c.res_size, c.rank + 1, c.n), dtype=np.int64)
    for b in range(len(c.lwe)):
        res = VecZnx(c.n, c.rank + 1, c.res_size)
        if c.ext > 1:
            luts = np.ascontiguousarray(c.lut[:, :, None, :])
            ref.blind_rotation_execute_extended(res, c.base2k, np.ascontiguousarray(lwe_2n[b]), luts, brk, c.dnum, c.brk_size, c.block_size, xpa)
        else:
            lut = VecZnx(c.n, 1, c.lut.shape[1], np.ascontiguousarray(c.lut[0][:, None, :]))
            ref.blind_rotation_execute(res, c.base2k, np.ascontiguousarray(lwe_2n[b]), lut, brk, c.dnum, c.brk_size, c.block_size, xpa)
        out[b] = res.data
    return lwe_2n, out


def run_gate_oracle(ref, c, acc):
    pm = prepare(ref, c.ksk)
    return np.stack([ref.lwe_from_glwe(c.n_lwe, c.res_size, c.base2k, VecZnx(c.n, c.rank + 1, c.res_size, np.ascontiguousarray(a)), c.base2k, 0,
                                       pm, 1, c.base2k) for a in acc])


def _decode_all(limbs, base2k, k):
    return np.array([fs.decode_coeff(limbs, base2k, k, i) for i in range(limbs.shape[-1])], dtype=np.int64)


def check_rotation(label, c, lwe_2n, out, fail=False):
    """The exponents against the exact mod_switch_2n; then per element: the noise over all N coefficients against the bound, limb 0 of the
    decryption against limb 0 of the rotated table (where c.limb0; else the decoded values of all N coefficients), coefficient 0 = f(x)."""
    if not fail:
        want_2n = np.stack([fs.mod_switch_2n(c.n2, lwe, c.lwe_base2k, True) for lwe in c.lwe])
        assert np.array_equal(lwe_2n, want_2n), (label, "mod_switch_2n")
    mod, bits = 1 << c.log_mod, c.log_mod + 1
    have, exact, fx = [], [], []
    for b in range(len(out)):
        have.append(fs.noise_log2(out[b], c.base2k, c.sk_glwe, c.want[b], c.base2k))
        pt = fs.normalize(fs.glwe_phase(out[b], c.sk_glwe), c.base2k)
        if c.limb0:
            exact.append(bool(np.array_equal(pt[0], c.want[b][0])))
        else:
            exact.append(bool(np.array_equal(_decode_all(pt, c.base2k, bits) % (2 * mod), _decode_all(c.want[b], c.base2k, bits) % (2 * mod))))
        fx.append(fs.decode_coeff(pt, c.base2k, bits, 0) % mod == f_table(c.xs[b]) % mod)
    print(f"[noise] {label}: noise_have {max(have):.2f} (min {min(have):.2f}) noise_want {c.bound:.2f} "
          f"{'limb 0' if c.limb0 else 'decoded table'} {exact} f(x) {fx} (modulus {mod})")
    if fail:
        assert min(have) > c.bound or not any(exact), (label, have, c.bound, exact, "a negative control decrypted")
    else:
        assert all(exact), (label, exact)
        assert all(fx), (label, fx)
        assert max(have) <= c.bound, (label, have, c.bound)
    return have


def check_gate(label, c, out, fail=False):
    """The LWE after the key switch back: decrypts under sk_lwe to f(x), noise = rotation + key switch."""
    mod, bits = 1 << c.log_mod, c.log_mod + 1
    errs = [fs.lwe_error(out[b], c.base2k, c.sk_lwe, c.gate_want[b], c.base2k) for b in range(len(out))]
    fx = [fs.decode_coeff(fs.lwe_decrypt(out[b], c.sk_lwe, c.base2k), c.base2k, bits, 0) % mod == f_table(c.xs[b]) % mod for b in range(len(out))]
    have = fs.rms_log2(errs)
    print(f"[noise] {label}: noise_have {have:.2f} noise_want {c.gate_bound:.2f} f(x) {fx} (modulus {mod})")
    if fail:
        assert min(_log2_abs(e) for e in errs) > c.gate_bound or not any(fx), (label, errs, c.gate_bound, fx)
    else:
        assert all(fx), (label, fx)
        assert have <= c.gate_bound, (label, errs, c.gate_bound)
    return have


# ---- circuit bootstrapping (poulpy-bin-fhe circuit_bootstrapping/circuit.rs:219-421, tests/circuit_bootstrapping.rs) ----
REF_CBT_BASES = (13, 11, 12, 15)      # blind-rotation key, automorphism keys, tensor keys, result: tests/circuit_bootstrapping.rs:49-53


def _cdiv(a, b):
    return -(-a // b)


def cbt_case(n, rank, n_lwe, block_size, bases, mode, seed, res_limbs=4, res_dnum=3, key_dnum=4, log_domain=None, log_gap_out=1, datas=None,
             lwe_base2k=14, plus_gap=False, swap_pairs=False):
    """tests/circuit_bootstrapping.rs:48-228 (mode "exponent": a 4-bit domain, the GGSW of X^(data 2^log_gap_out)) and :231-420 (mode
    "constant": a 1-bit domain, the GGSW of the constant data), table and gap as circuit.rs:274-342.  bases = (brk, atk, tsk, res) base2k;
    k_res = res_limbs res_base2k, each key one limb of its neighbour's base above it as the reference's test has them (its names for the
    automorphism and tensor keys' precisions crossed).  The key is the blind-rotation key, one automorphism key per trace step and the
    tensor key (key_ops_cases.tensor_key).

    want: per output row the polynomial column 0 must decrypt to, read off the exact table: the constant coefficient of
    X^(-i gap) (X^(+-phase) table) in constant mode (asserted here to be data at limb i), X^(data 2^log_gap_out) at limb i in exponent mode.
    plus_gap turns the table by +i gap instead (a control on the expectation; row 0 cannot tell).  swap_pairs exchanges the tensor key's
    input columns (rank 2)."""
    from tests import key_ops_cases as kc
    from tests import trace_cases as tc
    rng = seeded(seed)
    brk_b, atk_b, tsk_b, res_b = bases
    to_exponent = mode == "exponent"
    if log_domain is None:
        log_domain = 4 if to_exponent else 1
    if datas is None:
        datas = (1, 5, 11) if to_exponent else (1, 0, 1)
    k_res = res_limbs * res_b
    k_brk, k_atk, k_tsk = k_res + brk_b, k_res + tsk_b, k_res + atk_b
    sh = dict(glwe_size=_cdiv(k_brk, brk_b), atk_glwe_size=_cdiv(k_brk, atk_b), trace_size=_cdiv(max(k_brk, k_res), atk_b))
    sk_glwe = fs.ternary_secret(n, rank, rng)
    sk_lwe = fs.binary_block_secret(n_lwe, block_size, rng)
    brk = fs.blind_rotation_key(sk_glwe, sk_lwe, brk_b, k_brk, key_dnum, rng)
    gals = tc.trace_gals(n)
    atk = [fs.automorphism_key(sk_glwe, g, atk_b, k_atk, key_dnum, 1, rng) for g in gals]
    tsk = kc.tensor_key(sk_glwe, tsk_b, k_tsk, key_dnum, 1, rng)
    if swap_pairs:
        assert rank == 2
        tsk = [np.ascontiguousarray(t[:, ::-1]) for t in tsk]
    # circuit.rs:258-301
    alpha = 1 << (res_dnum - 1).bit_length()
    f = [0] * ((1 << log_domain) * alpha)
    for i in range(res_dnum):
        if to_exponent:
            f[i] = 1 << (res_b * (res_dnum - 1 - i))
        else:
            for j in range(1 << log_domain):
                f[j * alpha + i] = j << (res_b * (res_dnum - 1 - i))
    lut, drift = fs.lut_set(f, res_b * res_dnum, n, 1, brk_b, res_b * res_dnum)
    gap = 2 * drift
    log_gap_in = (gap * alpha - 1).bit_length()
    n2 = 2 * n
    assert lwe_base2k > (n2 - 1).bit_length() + 1
    k_lwe = max(13, log_domain + 18)
    lwes, wants = [], []
    for data in datas:
        lwe = fs.lwe_encrypt(sk_lwe, fs.encode_int(data, lwe_base2k, log_domain + 1), lwe_base2k, k_lwe, rng)
        lwe_2n = fs.mod_switch_2n(n2, lwe, lwe_base2k, not to_exponent)
        rot = (int(lwe_2n[0]) + int(lwe_2n[1:] @ sk_lwe)) % n2
        rows = []
        for i in range(res_dnum):
            msg = np.zeros(n, dtype=np.int64)
            if to_exponent:
                msg[0] = 1
                rows.append(fs._row_plaintext(fs.rotate(msg, data << log_gap_out), res_limbs, i, res_b))
            else:
                turned = fs.lut_rotate(lut, rot + (i * gap if plus_gap else -i * gap))[0]
                top = fs.rebase(turned[:, :1], brk_b, res_b, res_dnum)        # the table's values are multiples of 2^-(res_b res_dnum)
                pt = np.zeros((res_limbs, n), dtype=np.int64)
                pt[:res_dnum, 0] = top[:, 0]
                msg[0] = data
                if not plus_gap:
                    assert np.array_equal(pt, fs._row_plaintext(msg, res_limbs, i, res_b)), (data, i)
                rows.append(pt)
        lwes.append(lwe)
        wants.append(rows)
    # bounds.  Column 0: the rotation, then the trace (trace.rs:133-147, tests/trace_cases.py).  The reference's keys have 4 rows, which in
    # their bases reach 44 (automorphism) and 48 (tensor) bits of ciphertexts of 73 and 60: as in conversion_bound every key switch loses the
    # digits below, rank n / 2 secret coefficients times 2^(-2 reach) / 12; a trace step halves what it has and adds one such loss, and the
    # halved sum with its image keeps half the variance, so the losses add up to twice one.  The other columns: the expansion on top
    # (noise_ggsw_keyswitch, noise/mod.rs:140-188, with column 0's variance in the key switch's place), its own loss against the
    # tensor key's messages s_i s_j (variance n / 4).
    def lost(reach, k_in, var_msg):
        return rank * n * var_msg * 4.0 ** -reach / 12.0 if reach < k_in else 0.0
    var0 = rotation_variance(n, rank, n_lwe, block_size, brk_b, k_brk, k_brk) + 4.0 ** tc.trace_noise_want(n, rank, atk_b, k_brk, k_atk)
    var0 += 2.0 * lost(key_dnum * atk_b, k_brk, 0.5)
    if to_exponent:      # post_process (circuit.rs:392-417): a partial trace, then glwe_pack, whose steps are trace steps again
        var0 += 4.0 ** tc.trace_noise_want(n, rank, atk_b, k_brk, k_atk) + 2.0 * lost(key_dnum * atk_b, k_brk, 0.5)
    var1 = var0 + kc.var_noise_gglwe_product(n, tsk_b, 0.5, n * 0.25, var0 * 4.0 ** k_res + 1.0 / 12.0, fs.SIGMA * fs.SIGMA, 0.0, rank, k_res, k_tsk)
    var1 += lost(key_dnum * tsk_b, k_res, n * 0.25)
    var1 += n * var1 * 0.5 * 0.5
    bounds = [0.5 * math.log2(v) + 1.0 for v in [var0] + [var1] * rank]
    pt_bits = res_b - 2 if to_exponent else res_b - log_domain - 1
    return SimpleNamespace(op="cbt", mode=mode, to_exponent=to_exponent, n=n, rank=rank, n_lwe=n_lwe, block_size=block_size, bases=bases,
                           brk_dnum=key_dnum, atk_dnum=key_dnum, tsk_dnum=key_dnum, res_dnum=res_dnum, res_size=res_limbs, sh=sh, lwe=np.stack(lwes),
                           lwe_base2k=lwe_base2k, negate=not to_exponent, n2=n2, lut=lut, gap=gap, log_gap_in=log_gap_in, log_gap_out=log_gap_out,
                           log_domain=log_domain, brk=brk, gals=gals, atk=atk, tsk=tsk, sk_glwe=sk_glwe, sk_lwe=sk_lwe, datas=list(datas),
                           want=wants, bounds=bounds, pt_bits=pt_bits, k_res=k_res, rows_checked=range(1, res_dnum) if plus_gap else range(res_dnum))


def run_cbt_oracle(ref, c):
    """(lwe_2n, GGSWs (batch, res_dnum, cols, res_size, cols, n)) through circuit_bootstrap_bases (one base2k per object)."""
    brk = brk_prepared(ref, c)
    atk = [prepare(ref, k) for k in c.atk]
    tsk = [prepare(ref, k) for k in c.tsk]
    xpa = ref.blind_rotation_x_pow_a() if c.block_size > 1 else np.zeros((1, 1))
    lwe_2n = np.stack([ref.mod_switch_2n(c.n2, lwe, c.lwe_base2k, c.negate) for lwe in c.lwe])
    cols = c.rank + 1
    out = np.empty((len(c.lwe), c.res_dnum, cols, c.res_size, cols, c.n), dtype=np.int64)
    lut = VecZnx(c.n, 1, c.lut.shape[1], np.ascontiguousarray(c.lut[0][:, None, :]))
    for b in range(len(c.lwe)):
        g = MatZnx(c.n, c.res_dnum, cols, cols, c.res_size)
        ref.circuit_bootstrap_bases(g, c.bases, c.to_exponent, np.ascontiguousarray(lwe_2n[b]), lut, brk, c.brk_dnum, c.sh["glwe_size"],
                                    c.sh["glwe_size"], c.sh["atk_glwe_size"], c.sh["trace_size"], c.block_size, xpa, c.gals, atk, tsk, c.gap,
                                    c.log_gap_in if c.to_exponent else 0, c.log_gap_out if c.to_exponent else 0,
                                    c.log_domain if c.to_exponent else 0)
        out[b] = g.data
    return lwe_2n, out


def cbt_end_inputs(c, seed=0):
    """The reference's end check (tests/circuit_bootstrapping.rs:202-228, :392-419): per element a fresh GLWE of 2^pt_bits at coefficient 0
    of limb 0, and limb 0 of what its external product with the element's GGSW must decrypt to."""
    rng = seeded(9000 + seed)
    res_b = c.bases[3]
    cts, wants = [], []
    for data in c.datas:
        pt = np.zeros((c.res_size, c.n), dtype=np.int64)
        pt[0, 0] = 1 << c.pt_bits
        cts.append(fs.glwe_encrypt(c.sk_glwe, pt, res_b, c.k_res, rng))
        cts[-1] = np.ascontiguousarray(cts[-1])
        wants.append(fs.rotate(pt[0], data << c.log_gap_out) if c.to_exponent else pt[0] * data)
    return np.stack(cts), wants


def run_cbt_end_oracle(ref, c, ggsw, cts):
    res_b = c.bases[3]
    out = np.empty_like(cts)
    for b in range(len(cts)):
        pm = prepare(ref, ggsw[b])
        a = VecZnx(c.n, c.rank + 1, c.res_size, np.ascontiguousarray(cts[b]))
        res = VecZnx(c.n, c.rank + 1, c.res_size)
        ref.glwe_external_product(res, res_b, a, res_b, pm, 1, res_b)
        out[b] = res.data
    return out


def check_cbt(label, c, lwe_2n, ggsw, end, end_want, fail=False):
    """GGSW noise of every (row, column) against its bound; then the end check: limb 0 exact.  A control must miss: every element has an
    entry beyond its bound, or the end check fails for every element."""
    res_b = c.bases[3]
    if not fail:
        want_2n = np.stack([fs.mod_switch_2n(c.n2, lwe, c.lwe_base2k, c.negate) for lwe in c.lwe])
        assert np.array_equal(lwe_2n, want_2n), (label, "mod_switch_2n")
    worst, best, end_ok, have = -math.inf, math.inf, [], [-math.inf] * (c.rank + 1)
    for b in range(len(ggsw)):
        worst_b = -math.inf
        for row in c.rows_checked:
            for col in range(c.rank + 1):
                pt = c.want[b][row]
                if col > 0:
                    pt = fs.normalize(fs.mul_small(pt, c.sk_glwe[col - 1]), res_b)
                d = fs.noise_log2(ggsw[b, row, col], res_b, c.sk_glwe, pt, res_b) - c.bounds[col]
                worst_b = max(worst_b, d)
                have[col] = max(have[col], d + c.bounds[col])
        worst, best = max(worst, worst_b), min(best, worst_b)      # a GGSW is as good as its worst entry
        pt = fs.normalize(fs.glwe_phase(end[b], c.sk_glwe), res_b)
        end_ok.append(bool(np.array_equal(pt[0], end_want[b])))
    print(f"[noise] {label}: noise_have per column {['%.2f' % x for x in have]} noise_want {['%.2f' % x for x in c.bounds]} "
          f"(noise_have - noise_want of the worst entry: worst element {worst:.2f}, best element {best:.2f}), "
          f"end check limb 0 {end_ok}")
    if fail:
        assert best > 0 or not any(end_ok), (label, best, end_ok, "a negative control decrypted")
    else:
        assert all(end_ok), (label, end_ok)
        assert worst <= 0, (label, worst)


ONE_BASE = (13, 13, 13, 13)
# (label, keyword arguments of cbt_case, must fail): each control next to its positive twin
CBT_CONTROLS = [
    ("constant mode, rows expected at -gap", dict(n=256, rank=1, n_lwe=14, block_size=7, bases=ONE_BASE, mode="constant", log_domain=2,
                                                   datas=(1, 2, 3)), False),
    ("constant mode, rows expected at +gap", dict(n=256, rank=1, n_lwe=14, block_size=7, bases=ONE_BASE, mode="constant", log_domain=2,
                                                   datas=(1, 2, 3), plus_gap=True), True),
    ("rank 2, tensor key pairs in order", dict(n=256, rank=2, n_lwe=14, block_size=7, bases=ONE_BASE, mode="constant"), False),
    ("rank 2, tensor key pairs swapped", dict(n=256, rank=2, n_lwe=14, block_size=7, bases=ONE_BASE, mode="constant", swap_pairs=True), True),
]


def check_cbt_on(run, run_end, label, c, fail=False):
    """run(c) -> (lwe_2n, ggsw), run_end(c, ggsw, cts) -> external products: the whole procedure on one executor."""
    lwe_2n, ggsw = run(c)
    cts, end_want = cbt_end_inputs(c)
    check_cbt(label, c, lwe_2n, ggsw, run_end(c, ggsw, cts), end_want, fail=fail)
    return ggsw
