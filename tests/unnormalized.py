"""Un-normalized inputs for the batched entry points: what a ciphertext holds after additions without a normalize
(poulpy-core api/operations.rs glwe_add_into / _sub / _negate call vec_znx_add / _sub / _negate and never normalize).

Every generator checks that its output really has the property it promises, so that a later edit cannot turn a case quietly back into
a normalized one.  Arrays are int64 [..., size, cols, n] (a VecZnx, or a batch of them); the helpers below write in place and return
the array.

  1. sums(s):        digits uniform in [-2^(base2k-1+s), 2^(base2k-1+s)) - 2^s additions without a normalize
  2. one_wide:       one ciphertext of a normalized batch wide (place it in the second wave, or in wave 0 with normalized ones after it)
  3. wide_at(where): wide digits in one place only - the body column, a mask column, the top limb or the bottom limb
  4. full_range:     any int64, INT64_MIN, INT64_MAX and +-2^62 included - for the entry points that do no FFT
"""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min
INT64_MAX = np.iinfo(np.int64).max
EDGES = np.array([INT64_MIN, INT64_MAX, 1 << 62, -(1 << 62), INT64_MIN + 1, 0, -1, 1], dtype=np.int64)
PLACES = ("body", "mask", "top", "bottom")


def wide_digits(rng, shape, base2k, s):
    """Digits uniform in [-2^(base2k-1+s), 2^(base2k-1+s)); s >= 1.  Asserts that some digit is outside the balanced base2k range and,
    where the width reaches past 16 bits, that some digit is at least 2^15 in magnitude (the reach of the 16-bit copies)."""
    assert s >= 1
    half = 1 << (base2k - 1 + s)
    v = rng.integers(-half, half, shape, dtype=np.int64)
    # the extremes of the range, so that the width is what the name says whatever the draw
    flat = v.reshape(-1)
    flat[0] = -half
    flat[-1] = half - 1
    check_unnormalized(v, base2k)
    if base2k - 1 + s >= 16:
        check_beyond_16_bits(v)
    return v


def check_unnormalized(v, base2k):
    """Some digit lies outside [-2^(base2k-1), 2^(base2k-1)): the array is not a normalized VecZnx at this base."""
    half = 1 << (base2k - 1)
    assert ((v < -half) | (v >= half)).any(), "input is normalized"


def check_beyond_16_bits(v):
    """Some value is outside [-32767, 32767]: a 16-bit copy of it cannot hold it (-32768 included: its negation does not fit)."""
    assert ((v > 32767) | (v < -32767)).any(), "input fits 16 bits"


def sums(base2k, s):
    """Class 1 as a fill for the test runners: fill(index, data, rng) overwrites the whole VecZnx."""
    def fill(_, data, rng):
        data[...] = wide_digits(rng, data.shape, base2k, s)
    fill.label = f"sum-of-2^{s}"
    return fill


def one_wide(index, base2k, s):
    """Class 2: only ciphertext `index` of the batch gets class-1 digits; the others keep what the runner drew (normalized)."""
    def fill(i, data, rng):
        if i == index:
            data[...] = wide_digits(rng, data.shape, base2k, s)
    fill.label = f"ct{index}-wide-2^{s}"
    return fill


def wide_at(where, base2k, s, index=None):
    """Class 3: wide digits in `where` only (PLACES) of data [size, cols, n]: column 0 (body), column 1 (a mask), limb 0 (top) or the
    last limb (bottom); everything else keeps its normalized digits.  index: only that ciphertext of the batch (None: all of them)."""
    assert where in PLACES

    def fill(i, data, rng):
        if index is not None and i != index:
            return
        sel = {"body": (slice(None), 0), "mask": (slice(None), 1), "top": (0,), "bottom": (data.shape[0] - 1,)}[where]
        before = data.copy()
        data[sel] = wide_digits(rng, data[sel].shape, base2k, s)
        changed = np.zeros(data.shape, dtype=bool)
        changed[sel] = True
        assert np.array_equal(data[~changed], before[~changed])
        check_unnormalized(data[sel], base2k)
    fill.label = f"{where}-wide-2^{s}"
    return fill


def full_range(rng, shape):
    """Class 4: uniform int64 over the whole range, with every value of EDGES planted at the front.  Asserts they are there."""
    v = rng.integers(INT64_MIN, INT64_MAX, shape, dtype=np.int64, endpoint=True)
    flat = v.reshape(-1)
    assert flat.size >= EDGES.size
    flat[:EDGES.size] = EDGES
    check_full_range(v)
    return v


def full_range_fill():
    """Class 4 as a fill for the test runners"""
    def fill(_, data, rng):
        data[...] = full_range(rng, data.shape)
    fill.label = "full-range"
    return fill


def check_full_range(v):
    assert (v == INT64_MIN).any() and (v == INT64_MAX).any() and (v == 1 << 62).any() and (v == -(1 << 62)).any()
    assert (np.abs(v.astype(np.float64)) > 2.0 ** 53).any(), "no value beyond f64's exact integers"
