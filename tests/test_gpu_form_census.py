"""The census on the device: every instantiated form of the middle kernel, the fused tail and the blind-rotation kernels (the rows of
tests/form_census_cases.py, which tests/test_form_census_host.py holds against the X-macro lists) runs once through a public batched entry
point; the dispatch notes must name the form, and the bytes must be the oracle's.

The GPU suite is organised by operation; which instantiation a call lands on is incidental there.  Here it is the subject: the note is
asserted first (a miss means the case's parameters are wrong, not the kernel), then bit-equality.  Every fused-tail case runs once more
under the rounding-margin probe: the note carries " PROBE" (the same form's probing instantiation, launch_tail_probe.hip), the bytes are
the same, and the margin - the device's and, on the same inputs, the oracle's - stays under tests.helpers.MARGIN_MAX."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from tests import form_census_cases as fc
from tests.device import mods, on_device  # noqa: F401
from tests.helpers import MARGIN_MAX

pytestmark = pytest.mark.gpu

CASES = fc.device_cases()


def _cu() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch(key, case):
    if case.batch is None:
        return fc.mid_batch(fc.ct_of(key), fc.m1_of(case.n), _cu())
    if isinstance(case.batch, str):
        return {"cu+1": _cu() + 1, "2cu+1": 2 * _cu() + 1}[case.batch]
    return case.batch


def _call(mods, case, batch, seed):
    """one call of the case's runner: (got, want)"""
    from tests.test_gpu_cnv import _run_mul_relinearize, _run_tensor
    from tests.test_gpu_parity import _run_blind_rotation, _run_glwe_op, _trace_shifted_stores
    p, n = case.p, case.n
    ref, hip = mods(n)
    sw = dict(case.sw)
    chunk, fuse = sw.pop("chunk", 0), sw.pop("fuse", (True, True))
    with on_device(hip, **sw):
        if case.run == "glwe":
            return _run_glwe_op(hip, ref, p["ks"], n, p["rank"], p["rank_out"], p["a"], p["k"], p["key"], p["k"], p["dnum"], p["dsize"], p["res"], p["k"],
                                batch=batch, seed=seed, chunk=chunk, fuse=fuse, auto=p["auto"])
        if case.run == "br":
            return _run_blind_rotation(hip, ref, n, p["rank"], p["n_lwe"], p["blk"], p["dnum"], p["bsz"], p["rsz"], p["k"], batch=batch, seed=seed,
                                       lwe_span=p["span"])
        if case.run == "tensor":
            return _run_tensor(hip, ref, n, p["rank"], p["a"], p["b"], p["res"], p["k"], p["k"], p["off"], p["mode"], batch=batch, seed=seed, chunk=chunk)
        if case.run == "mulrelin":
            return _run_mul_relinearize(hip, ref, n, p["rank"], p["a"], p["b"], p["t"], p["k"], p["off"], p["key"], p["k"], p["dnum"], 1, p["res"], p["k"],
                                        p["mode"], batch=batch, seed=seed, chunk=chunk)
        assert case.run == "trace" and batch == 2   # (the trace runner's own batch and seed)
        return _trace_shifted_stores(mods, n, p["size"], p["key"], p["gals"], p["k"])


_RECORDS = {}


def _record(mods, key, case):
    """The case run once - and, for a fused-tail row, once more under the probe - whichever of the rows that share it asks first."""
    from tests.test_gpu_margin import probing
    tail = key.startswith("k_inv_tail<")
    batch = _batch(key, case)
    ident = repr((case._replace(probe=None), batch, tail))
    if ident in _RECORDS:
        return _RECORDS[ident]
    ref, hip = mods(case.n)
    seed = zlib.crc32(ident.encode()) & 0x7FFFFFFF
    r = SimpleNamespace(batch=batch)
    hip.dispatch_notes(reset=True)
    box = {}
    r.oracle_margin = ref.rounding_margin_of(lambda: box.update(out=_call(mods, case, batch, seed)))
    r.notes = hip.dispatch_notes(reset=True).split("; ")
    got, want = box["out"]
    r.equal = bool(np.array_equal(got, want))
    if tail:
        with probing(hip) as pb:
            got1, _ = _call(mods, case, batch, seed)
            r.probe_notes = hip.dispatch_notes(reset=True).split("; ")
        r.probe_equal, r.margin = bool(np.array_equal(got1, got)), pb.margin
    _RECORDS[ident] = r
    return r


@pytest.mark.parametrize("cid,key,case", CASES, ids=[c[0] for c in CASES])
def test_form_is_dispatched_and_matches_the_oracle(mods, cid, key, case):
    r = _record(mods, key, case)
    tail = key.startswith("k_inv_tail<")
    named = (key in r.notes) if tail else any(note.startswith(key) for note in r.notes)
    assert named, f"{cid} (batch {r.batch}): the call did not land on this form; notes: {r.notes}"
    assert r.equal, f"{cid} (batch {r.batch}): the device's bytes differ from the oracle's"
    if not tail:
        return
    assert r.oracle_margin < MARGIN_MAX, f"{cid}: the oracle's own margin on these inputs is {r.oracle_margin} (lower the case's base2k)"
    want_note = case.probe or key + " PROBE"
    assert want_note in r.probe_notes, f"{cid}: under the probe the call left {r.probe_notes}"
    if case.probe:   # a form the API layer keeps away from the probe: its probing instantiation must stay unreached, or this row needs its own leg
        assert key + " PROBE" not in r.probe_notes, r.probe_notes
    assert r.probe_equal, f"{cid}: the probing instantiation changed the bytes"
    assert 0.0 < r.margin < MARGIN_MAX, (cid, r.margin)


def test_every_probe_note_is_a_product_note_with_the_suffix(mods):
    """on one shape, plainly: the same launches in the same order, each note with ' PROBE' behind it and nothing else changed"""
    from tests.test_gpu_margin import probing
    key, case = "k_inv_tail<4,8,16> PLAIN(1,1)", fc.CENSUS["k_inv_tail<4,8,16> PLAIN(1,1)"][0]
    ref, hip = mods(case.n)
    hip.dispatch_notes(reset=True)
    _call(mods, case, 3, 1)
    notes = [x for x in hip.dispatch_notes(reset=True).split("; ") if x.startswith("k_inv_tail<")]
    with probing(hip):
        _call(mods, case, 3, 1)
        probed = [x for x in hip.dispatch_notes(reset=True).split("; ") if x.startswith("k_inv_tail<")]
    assert key in notes and "k_inv_tail<4,8,16> PLAIN(1,0)" in notes
    assert probed == [x + " PROBE" for x in notes]
