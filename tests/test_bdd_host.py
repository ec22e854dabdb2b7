"""CPU: the BDD circuit entry points are declared, exported, typed and bound; pz_bdd_circuit_new - host only, no module, no device - refuses
every malformed circuit with a message that names the output bit and the node; the compiled schedule keeps its invariants (read back through
the query functions and the level tables); and the schedule compiler alone, linked into a stand-alone program built with the host
sanitizers, passes its own checks.  (Execution needs a device: tests/test_gpu_bdd.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from poulpy_amd import bdd
from tests import bdd_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pz_bdd_circuit_new", "pz_bdd_circuit_free", "pz_bdd_circuit_input_size", "pz_bdd_circuit_output_size", "pz_bdd_circuit_max_state_size",
           "pz_bdd_circuit_levels", "pz_bdd_circuit_gates", "pz_bdd_circuit_moved_copies", "pz_bdd_circuit_slots", "pz_bdd_circuit_output_slots",
           "pz_bdd_circuit_level_gates", "pz_bdd_circuit_execute_tmp_bytes", "pz_bdd_circuit_execute_batched")
OUT = 0x80000000
N, C_, X = bdd.NONE, bdd.COPY, bdd.CMUX
NONE, COPY = (N, 0, 0, 0), (C_, 0, 0, 0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from poulpy_amd.hal import load_library
    return load_library()


def _params(**kw):
    from poulpy_amd.hal import GlweOpParams
    d = dict(rank=1, dnum=3, dsize=1, key_size=3, key_base2k=12, a_size=3, a_base2k=12, res_size=3, res_base2k=12, rank_out=1)
    d.update(kw)
    return GlweOpParams(**d)


def test_header_declares_and_library_exports_the_entry_points(lib):
    from poulpy_amd import abi
    from poulpy_amd.hal import GlweOpParams
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poulpy_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in abi.PROTOTYPES, s
    node = abi.pz_bdd_node
    assert list(abi.TAGGED_STRUCTS) == ["pz_bdd_node"] and "pz_bdd_node" not in abi.STRUCTS   # typed from the header, not a parameter struct
    assert [f for f, _ in node._fields_] == ["kind", "sel", "hi", "lo"] and C.sizeof(node) == 16
    assert (abi.PZ_BDD_NONE, abi.PZ_BDD_COPY, abi.PZ_BDD_CMUX) == (bdd.NONE, bdd.COPY, bdd.CMUX) == (0, 1, 2)
    new = lib.pz_bdd_circuit_new
    assert new.restype is C.c_void_p and len(new.argtypes) == 5 and new.argtypes[3] is C.c_size_t and new.argtypes[4] is C.c_size_t
    ex = lib.pz_bdd_circuit_execute_batched
    assert ex.restype is C.c_int and len(ex.argtypes) == 10
    assert ex.argtypes[3] is C.c_size_t and ex.argtypes[5] is C.c_size_t and ex.argtypes[6] is C.POINTER(GlweOpParams) and ex.argtypes[8] is C.c_size_t
    for q in ("input_size", "output_size", "max_state_size", "levels", "gates", "moved_copies", "slots"):
        f = getattr(lib, "pz_bdd_circuit_" + q)
        assert f.restype is C.c_size_t and len(f.argtypes) == 1 and f(None) == 0
    assert lib.pz_bdd_circuit_execute_tmp_bytes.restype is C.c_size_t and len(lib.pz_bdd_circuit_execute_tmp_bytes.argtypes) == 4
    lib.pz_bdd_circuit_free(None)


def test_bindings_exist_in_every_language():
    from poulpy_amd import hal
    for m in ("bdd_circuit_new", "bdd_circuit_free", "bdd_circuit_execute_batched", "bdd_circuit_execute_tmp_bytes"):
        assert callable(getattr(hal.Module, m)), m
    assert callable(hal.bdd_circuit_new) and callable(bdd.execute_bdd_circuit)
    mirror = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "batched.rs")).read()
    ffi = open(os.path.join(ROOT, "rust", "poulpy-hip-mi355x", "src", "ffi.rs")).read()
    assert "pz_bdd_circuit_execute_batched(m_," in mirror and "pz_bdd_circuit_new(" in mirror
    assert "ffi::pz_bdd_circuit_execute_batched(" in rust
    for s in SYMBOLS:
        assert "fn %s(" % s in ffi, s


def test_node_struct_matches_the_c_compiler(tmp_path):
    """sizeof and every field offset of the ctypes node, against g++ on the same header"""
    from poulpy_amd import abi
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    node = abi.pz_bdd_node
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "poulpy_hip.h"', 'int main() {', '    std::printf("%zu\\n", sizeof(pz_bdd_node));']
    lines += ['    std::printf("%%zu\\n", offsetof(pz_bdd_node, %s));' % f for f, _ in node._fields_] + ['    return 0;', '}']
    src, exe = tmp_path / "node.cpp", tmp_path / "node"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(node)] + [getattr(node, f).offset for f, _ in node._fields_]


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
BAD = [
    ("hi out of range", 2, [([(X, 0, 2, 0), NONE], 2)], "output 0 node 0: hi index 2"),
    ("lo out of range, second output", 2, [([(X, 0, 1, 0), NONE], 2), ([NONE, NONE, NONE, (X, 1, 0, 1), NONE, NONE, (X, 0, 0, 3), NONE, NONE], 3)],
     "output 1 node 6: lo index 3"),
    ("selector out of range", 2, [([(X, 2, 1, 0), NONE], 2)], "output 0 node 0: selector 2"),
    ("ragged node count", 2, [([(X, 0, 1, 0), NONE, NONE], 2)], "output 0: 3 nodes are not whole chunks of state_size 2"),
    ("no chunk at all", 2, [([(X, 0, 1, 0), NONE], 2), ([], 2)], "output 1: 0 nodes"),
    ("last chunk starts with a copy", 2, [([COPY, NONE], 2)], "output 0 node 0: the last chunk must start with a cmux"),
    ("last chunk with a second gate", 2, [([(X, 0, 1, 0), NONE, (X, 0, 1, 0), (X, 1, 1, 0)], 2)], "output 0 node 3: the last chunk is [cmux, none"),
    ("nodes on a width-0 output", 2, [([(X, 0, 0, 0)], 0)], "output 0 has state_size 0 and 1 nodes"),
    ("unknown kind", 2, [([(7, 0, 0, 0), NONE], 2)], "output 0 node 0: unknown kind 7"),
]


@pytest.mark.parametrize("label,n_in,outputs,msg", BAD, ids=[b[0] for b in BAD])
def test_malformed_circuits_are_refused_with_the_output_and_the_node(lib, label, n_in, outputs, msg):
    from poulpy_amd import hal
    with pytest.raises(hal.PoulpyHipError) as e:
        hal.bdd_circuit_new(bdd.Circuit(n_in, outputs), lib)
    assert msg in str(e.value), (label, str(e.value))


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------------
def _levels(lib, h):
    out = []
    for lv in range(lib.pz_bdd_circuit_levels(h)):
        cnt = lib.pz_bdd_circuit_level_gates(h, lv, None, 0)
        buf = (C.c_uint32 * (4 * max(cnt, 1)))()
        assert lib.pz_bdd_circuit_level_gates(h, lv, buf, cnt) == cnt
        out.append([tuple(buf[4 * i:4 * i + 4]) for i in range(cnt)])
    return out


def _run_schedule(lib, h, circuit, bits):
    """the level tables on clear bits, every read of a level before any of its writes; a slot nothing wrote reads as None"""
    slots = [None] * lib.pz_bdd_circuit_slots(h)
    slots[0], slots[1] = 0, 1
    out = [0 if s == 0 else None for _, s in circuit.outputs]
    for gates in _levels(lib, h):
        vals = [slots[t] if bits[sel] else slots[f] for t, f, _, sel in gates]
        for (_, _, res, _), v in zip(gates, vals):
            assert v is not None
            if res & OUT:
                out[res & ~OUT] = v
            else:
                slots[res] = v
    return out


HAND = bo.hand_circuit()
CIRCUITS = {"hand": HAND, "adder32": bdd.adder(32), "adder5c": bdd.adder(5, carry_out=True), "sub6": bdd.sub(6), "ltu7": bdd.ltu(7),
            "mul3": bdd.from_truth_table(lambda x: (x & 7) * (x >> 3), 6, 6),
            "width1": bdd.Circuit(2, [([(X, 0, 0, 0)], 1), ([NONE, (X, 1, 0, 0)], 1), ([COPY, (X, 1, 0, 0)], 1)])}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_schedule_invariants(lib, name):
    import random
    from poulpy_amd import hal
    c = CIRCUITS[name]
    h = hal.bdd_circuit_new(c, lib)
    try:
        assert lib.pz_bdd_circuit_input_size(h) == c.input_size and lib.pz_bdd_circuit_output_size(h) == c.output_size
        assert lib.pz_bdd_circuit_max_state_size(h) == c.max_state_size and lib.pz_bdd_circuit_levels(h) == c.max_depth
        assert lib.pz_bdd_circuit_gates(h) == c.count(bdd.CMUX)
        assert lib.pz_bdd_circuit_moved_copies(h) == 0                  # a Copy renames
        nslots, at = lib.pz_bdd_circuit_slots(h), 2
        owner = {}
        for o, (_, s) in enumerate(c.outputs):
            first, count = C.c_size_t(), C.c_size_t()
            assert lib.pz_bdd_circuit_output_slots(h, o, C.byref(first), C.byref(count)) == 0
            assert first.value == at and count.value <= 2 * s, (o, first.value, count.value, s)
            owner.update({sl: o for sl in range(at, at + count.value)})
            at += count.value
        assert at == nslots and lib.pz_bdd_circuit_output_slots(h, c.output_size, None, None) == -1
        levels = _levels(lib, h)
        assert sum(len(g) for g in levels) == lib.pz_bdd_circuit_gates(h)
        written_outputs = []
        for lv, gates in enumerate(levels):
            reads = {s for t, f, _, _ in gates for s in (t, f)}
            writes = [res for _, _, res, _ in gates if not res & OUT]
            assert len(set(writes)) == len(writes) and not reads & set(writes), (lv, "a gate writes a slot read or written in its level")
            assert all(2 <= w < nslots for w in writes) and all(r < nslots for r in reads)
            assert [g[3] for g in gates] == sorted(g[3] for g in gates), (lv, "not sorted by selector")
            for t, f, res, sel in gates:
                o = res & ~OUT if res & OUT else owner[res]
                assert sel < c.input_size and all(s < 2 or owner[s] == o for s in (t, f)), (lv, "a gate reads another output's slot")
            written_outputs += [res & ~OUT for _, _, res, _ in gates if res & OUT]
        assert sorted(written_outputs) == [o for o, (_, s) in enumerate(c.outputs) if s], "every output is written by exactly one root gate"
        rng = random.Random(7)
        for _ in range(40):
            bits = [rng.getrandbits(1) for _ in range(c.input_size)]
            assert _run_schedule(lib, h, c, bits) == bdd.eval_plain(c, bits)
    finally:
        hal.bdd_circuit_free(h, lib)


def test_tmp_bytes_query_without_a_module_is_zero(lib):
    """No module: nothing to size.  (With a module, monotone in the batch: tests/test_gpu_bdd.py::test_refusals_launch_nothing.)"""
    from poulpy_amd import hal
    h = hal.bdd_circuit_new(HAND, lib)
    try:
        assert lib.pz_bdd_circuit_execute_tmp_bytes(None, h, C.byref(_params()), 4) == 0
    finally:
        hal.bdd_circuit_free(h, lib)


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """No module is passed: a call that got past its argument checks fails with "null module" - the checks below fire before that."""
    from poulpy_amd import abi, hal
    h = hal.bdd_circuit_new(HAND, lib)
    f = lib.pz_bdd_circuit_execute_batched
    out, key, tmp = 0x10000, 0x40000, 0x50000      # never dereferenced
    bits = (C.c_void_p * 8)(*([key] * 8))

    def err():
        return lib.pz_last_error().decode()
    try:
        for bad in (dict(a_base2k=13), dict(res_base2k=11), dict(key_base2k=14)):
            assert f(None, h, out, 4, bits, 4, C.byref(_params(**bad)), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "one base2k" in err(), err()
        assert f(None, h, out, 4, bits, 4, C.byref(_params(a_size=2)), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "a_size == p->res_size" in err(), err()
        assert f(None, h, out, 3, bits, 4, C.byref(_params()), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "n_out 3 < output_size 4" in err(), err()
        assert f(None, h, out, 4, bits, 3, C.byref(_params()), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "nbits 3 < input_size 4" in err(), err()
        holed = (C.c_void_p * 8)(*([key] * 8))
        holed[4 + 2] = None
        assert f(None, h, out, 4, holed, 4, C.byref(_params()), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "input bit 2 of input 1 is null" in err(), err()
        assert f(None, h, out, 4, bits, 4, None, tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "null params" in err()
        assert f(None, None, out, 4, bits, 4, C.byref(_params()), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "null circuit" in err()
        assert f(None, h, out, 4, bits, 4, C.byref(_params()), tmp, 1 << 30, 2) == abi.PZ_ERR_INVALID and "null module" in err()
    finally:
        hal.bdd_circuit_free(h, lib)


# ---- the schedule compiler alone, under the host sanitizers ---------------------------------------------------------------------------------
def _write_circuit(path, c):
    with open(path, "w") as f:
        f.write("%d %d\n" % (c.input_size, c.output_size))
        for nodes, s in c.outputs:
            f.write("%d %d\n" % (s, len(nodes)))
            f.write("".join("%d %d %d %d\n" % nd for nd in nodes))


def test_schedule_compiler_stand_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/test_bdd_schedule.cpp + poulpy_amd/csrc/bdd_schedule.cpp, no HIP, its own main: compiles adder(32) (handed over as a file)
    and its adversarial circuits, re-checks the invariants and evaluates every schedule against the two-bank walk.  Built with
    -fsanitize=address,undefined with the sanitizer runtimes linked INTO the program (-static-libasan -static-libubsan: it then starts in
    whatever environment the suite runs in, which is passed on unchanged) where the host compiler has them, plain otherwise; run as a child
    process."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    src = [os.path.join(ROOT, "tests", "cpp", "test_bdd_schedule.cpp"), os.path.join(ROOT, "poulpy_amd", "csrc", "bdd_schedule.cpp")]
    exe = str(tmp_path / "test_bdd_schedule")
    base = [cxx, "-std=c++17", "-O1", "-g", *src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[bdd] host compiler without sanitizer runtimes: built plain")
    circuit = str(tmp_path / "adder32.txt")
    _write_circuit(circuit, bdd.adder(32))
    r = subprocess.run([exe, circuit], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "all schedule checks passed" in r.stdout and "ok circuit from file: 32 outputs, 64 levels, 1584 gates, 961 copies renamed" in r.stdout, r.stdout[-2000:]
