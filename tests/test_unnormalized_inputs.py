"""CPU: the generators of tests/unnormalized.py give inputs of the width they claim, and their checks refuse normalized ones."""
import numpy as np
import pytest

from tests import unnormalized as un
from tests.helpers import seeded


@pytest.mark.parametrize("base2k", [10, 12, 14, 16])
@pytest.mark.parametrize("s", [1, 2, 4, 6])
def test_sums_span_their_range(base2k, s):
    rng = seeded(base2k * 10 + s)
    data = np.zeros((3, 2, 256), dtype=np.int64)
    un.sums(base2k, s)(0, data, rng)
    half = 1 << (base2k - 1 + s)
    assert data.min() == -half and data.max() == half - 1
    assert (np.abs(data) >= 1 << (base2k - 1)).mean() > 0.4     # most digits outside the normalized range
    if base2k - 1 + s >= 16:
        assert (np.abs(data) >= 1 << 15).any()


def test_one_wide_touches_one_ciphertext():
    rng = seeded(3)
    batch = np.stack([rng.integers(-2048, 2048, (3, 2, 64), dtype=np.int64) for _ in range(4)])
    before = batch.copy()
    fill = un.one_wide(2, 12, 4)
    for b in range(4):
        fill(b, batch[b], rng)
    assert np.array_equal(batch[[0, 1, 3]], before[[0, 1, 3]])
    assert np.abs(batch[2]).max() >= 1 << 14


@pytest.mark.parametrize("where", un.PLACES)
def test_wide_at_touches_one_place(where):
    rng = seeded(5)
    data = rng.integers(-2048, 2048, (4, 3, 64), dtype=np.int64)
    before = data.copy()
    un.wide_at(where, 12, 5)(0, data, rng)
    sel = {"body": (slice(None), 0), "mask": (slice(None), 1), "top": (0,), "bottom": (3,)}[where]
    mask = np.zeros(data.shape, dtype=bool)
    mask[sel] = True
    assert np.array_equal(data[~mask], before[~mask])
    assert np.abs(data[sel]).max() >= 1 << 15 and np.abs(data[~mask]).max() <= 1 << 11


def test_wide_at_one_ciphertext_only():
    rng = seeded(6)
    data = rng.integers(-2048, 2048, (3, 2, 64), dtype=np.int64)
    before = data.copy()
    un.wide_at("body", 12, 5, index=1)(0, data, rng)
    assert np.array_equal(data, before)


def test_full_range_has_the_edges():
    v = un.full_range(seeded(7), (2, 3, 64))
    for e in (un.INT64_MIN, un.INT64_MAX, 1 << 62, -(1 << 62)):
        assert (v == e).any()
    assert (np.abs(v.astype(np.float64)) > 2.0 ** 62).mean() > 0.3


def test_checks_refuse_normalized_input():
    rng = seeded(8)
    normalized = rng.integers(-2048, 2048, (3, 2, 64), dtype=np.int64)
    with pytest.raises(AssertionError):
        un.check_unnormalized(normalized, 12)
    with pytest.raises(AssertionError):
        un.check_beyond_16_bits(normalized)
    with pytest.raises(AssertionError):
        un.check_full_range(normalized)
    with pytest.raises(AssertionError):
        un.check_beyond_16_bits(np.full(8, -32767, dtype=np.int64))
    un.check_beyond_16_bits(np.full(8, -32768, dtype=np.int64))    # its negation does not fit 16 bits
