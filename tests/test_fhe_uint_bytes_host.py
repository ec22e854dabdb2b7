"""The FheUint byte operations, host side: the entry points in the header and the ctypes view, the stage plan of
pz_fhe_uint_word_plan against a walk of the reference's calls, its stand-alone check under the host sanitizers, and the oracle's literal
restatement (tests/fhe_uint_bytes_oracle.py) under real keys with the values of the reference's own tests.  Nothing here needs a GPU."""
import os
import shutil
import subprocess

import pytest

from tests import fhe_sk as fs
from tests import fhe_uint_bytes_oracle as bo
from tests import fhe_uint_cases as fc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CALLS = ("pz_fhe_uint_word_op_tmp_bytes", "pz_fhe_uint_get_batched", "pz_fhe_uint_zero_byte_batched", "pz_fhe_uint_splice_batched",
         "pz_fhe_uint_sext_batched")
HOST = ("pz_fhe_uint_word_plan", "pz_fhe_uint_bit_coefficient")
WIDTHS = [8, 16, 32, 64, 128]


def test_entry_points_declared_typed_and_exported():
    import ctypes as C
    from poulpy_amd import abi, bdd, hal
    header = open(os.path.join(ROOT, "include", "poulpy_hip.h")).read()
    hpp = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    lib = hal.load_library()
    for name in CALLS + HOST:
        assert name + "(" in header, name
        assert name in abi.PROTOTYPES, name
        assert getattr(lib, name) is not None, name
    for name in CALLS:
        assert name + "(" in hpp, name
        assert hasattr(hal.Module, name[3:]), name
    p = C.POINTER(abi.pz_glwe_op_params)
    v, z, i, u = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
    assert abi.PROTOTYPES["pz_fhe_uint_word_op_tmp_bytes"] == (z, [v, p, z, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_get_batched"] == (i, [v, v, v, z, i, z, v, v, v, p, v, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_zero_byte_batched"] == (i, [v, v, v, z, z, v, v, p, v, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_splice_batched"] == (i, [v, v, v, v, z, z, z, z, v, v, p, v, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_sext_batched"] == (i, [v, v, z, z, v, v, p, v, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_bit_coefficient"] == (z, [z, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_word_plan"] == (z, [z, z, u, v, z, v, z, v])
    assert (abi.PZ_WORD_BIT, abi.PZ_WORD_BYTE) == (0, 1)
    assert [abi.PZ_WORD_OP_GET_BIT, abi.PZ_WORD_OP_GET_BYTE, abi.PZ_WORD_OP_ZERO_BYTE, abi.PZ_WORD_OP_SPLICE_U8, abi.PZ_WORD_OP_SPLICE_U16,
            abi.PZ_WORD_OP_SEXT] == list(range(6))
    # no new struct
    assert list(abi.STRUCTS) == ["pz_glwe_op_params", "pz_glwe_tensor_params", "pz_glwe_mul_const_params", "pz_glwe_term",
                                 "pz_blind_rotation_params", "pz_circuit_bootstrapping_params"]
    for name in ("fhe_uint_get_bits", "fhe_uint_get_bytes", "fhe_uint_zero_byte", "fhe_uint_splice", "fhe_uint_sext"):
        assert callable(getattr(bdd, name)), name


@pytest.mark.parametrize("word_bits", WIDTHS)
def test_bit_coefficient_is_the_interleaved_index(word_bits):
    from poulpy_amd import hal
    for n in (word_bits, 2048):
        assert [hal.fhe_uint_bit_coefficient(n, word_bits, i) for i in range(word_bits)] == [fc.coefficient(i, word_bits, n) for i in range(word_bits)]
        with pytest.raises(ValueError):
            hal.fhe_uint_bit_coefficient(n, word_bits, word_bits)
    for n, w in ((1024, 12), (64, 128), (96, 32), (0, 8)):
        with pytest.raises(ValueError):
            hal.fhe_uint_bit_coefficient(n, w, 0)


def check_plan(n, w, op, args, walk, stages_want, traces_ref):
    """the plan's traces are the walk's (sext's shared trace of s' once), its closing rotations the walk's in order, its stage count and the
    reference's trace count those of the table in DESIGN.md 4.4i"""
    from poulpy_amd import hal
    plan = hal.fhe_uint_word_plan(n, w, op, args)
    traces, closings = bo.plan_traces(plan)
    assert len(plan) == stages_want, (n, w, op, args, len(plan))
    assert len(walk.traces) == traces_ref, (n, w, op, args, len(walk.traces))
    assert sorted(set(map(repr, traces))) == sorted(set(map(repr, walk.traces))), (n, w, op, args)
    assert len(traces) == len(set(map(repr, walk.traces))), (n, w, op, args, "a trace runs twice")
    assert closings == walk.closings, (n, w, op, args)
    for st in plan:
        slots = [slot for _, _, slot in st["items"]]
        assert slots == list(range(slots[0], slots[0] + len(slots))), (n, w, op, args, "the items of a stage are one dense array")
        assert all(exp < n for _, exp, _ in st["items"]) and st["r"] < n
    return plan


@pytest.mark.parametrize("word_bits", WIDTHS)
def test_plan_is_the_walk_of_the_reference_calls(word_bits):
    """Two ring degrees each: n = word_bits (log_gap = 0) and a large one.  Every (dst, src) of both splice widths, every zero_byte, every
    sext(byte) - the last byte is the empty plan -, a get of all bits and of all bytes."""
    from poulpy_amd import abi, hal
    w, nbytes = word_bits, word_bits // 8
    for n in (w, 2048):
        wk = bo.Walk(n, w)
        for i in range(w):
            wk.get_bit(i)
        plan = check_plan(n, w, abi.PZ_WORD_OP_GET_BIT, list(range(w)), wk, 1, w)
        assert plan[0]["skip"] == 0 and plan[0]["close"] == 0 and [s for _, _, s in plan[0]["items"]] == list(range(w))
        wk = bo.Walk(n, w)
        for i in range(nbytes):
            wk.get_byte(i)
        plan = check_plan(n, w, abi.PZ_WORD_OP_GET_BYTE, list(range(nbytes)), wk, 1, nbytes)
        assert plan[0]["skip"] == 3
        for byte in range(nbytes):
            wk = bo.Walk(n, w)
            wk.zero_byte("a", byte)
            plan = check_plan(n, w, abi.PZ_WORD_OP_ZERO_BYTE, [byte], wk, 1, 1)
            assert plan[0]["plus"] is None and plan[0]["minus"] == 0 and plan[0]["base"] == 0
            k = nbytes - 1 - byte
            if k == 0:
                assert hal.fhe_uint_word_plan(n, w, abi.PZ_WORD_OP_SEXT, [byte]) == []
            else:
                wk = bo.Walk(n, w)
                wk.sext(byte)
                plan = check_plan(n, w, abi.PZ_WORD_OP_SEXT, [byte], wk, 1 + k, 1 + 2 * k)
                assert plan[0]["skip"] == 0 and plan[0]["close"] == 2 and [len(st["items"]) for st in plan] == [1, 2] + [1] * (k - 1)
        for dst in range(nbytes):
            for src in range(nbytes):
                wk = bo.Walk(n, w)
                wk.splice_u8(dst, src, "a", "b")
                plan = check_plan(n, w, abi.PZ_WORD_OP_SPLICE_U8, [dst, src], wk, 1, 2)
                assert len(plan[0]["items"]) == 2
                if dst < nbytes // 2 and src < nbytes // 2:
                    wk = bo.Walk(n, w)
                    wk.splice_u16(dst, src)
                    plan = check_plan(n, w, abi.PZ_WORD_OP_SPLICE_U16, [dst, src], wk, 2, 4)
                    assert [len(st["items"]) for st in plan] == [3, 1]
                    assert all(s == 2 for s, _, _ in plan[1]["items"]), "b is consumed by the first stage (res may be b)"


def test_plan_refusals():
    from poulpy_amd import abi, hal
    bad = [(1024, 12, abi.PZ_WORD_OP_ZERO_BYTE, [0]), (1024, 256, abi.PZ_WORD_OP_ZERO_BYTE, [0]), (1024, 0, abi.PZ_WORD_OP_ZERO_BYTE, [0]),
           (64, 128, abi.PZ_WORD_OP_ZERO_BYTE, [0]), (96, 32, abi.PZ_WORD_OP_ZERO_BYTE, [0]),
           (1024, 32, abi.PZ_WORD_OP_ZERO_BYTE, [4]), (1024, 32, abi.PZ_WORD_OP_SEXT, [4]), (1024, 32, abi.PZ_WORD_OP_GET_BYTE, [0, 4]),
           (1024, 32, abi.PZ_WORD_OP_GET_BIT, [32]), (1024, 32, abi.PZ_WORD_OP_SPLICE_U8, [4, 0]), (1024, 32, abi.PZ_WORD_OP_SPLICE_U8, [0, 4]),
           (1024, 32, abi.PZ_WORD_OP_SPLICE_U16, [2, 0]), (1024, 32, abi.PZ_WORD_OP_SPLICE_U16, [0, 2]), (1024, 8, abi.PZ_WORD_OP_SPLICE_U16, [0, 0]),
           (1024, 32, abi.PZ_WORD_OP_SPLICE_U8, [0]), (1024, 32, 6, [0]), (1024, 128, abi.PZ_WORD_OP_GET_BIT, [0] * 129)]
    for n, w, op, args in bad:
        with pytest.raises(ValueError):
            hal.fhe_uint_word_plan(n, w, op, args)
    assert hal.fhe_uint_word_plan(1024, 32, abi.PZ_WORD_OP_GET_BIT, []) == []


def test_plan_stand_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/test_word_ops.cpp + poulpy_amd/csrc/word_ops.cpp, no HIP, its own main: every word width at every ring degree from word_bits
    to 2^16, every operation with every argument, against a walk of the reference's calls; damaged plans; bad arguments.  Built with
    -fsanitize=address,undefined with the sanitizer runtimes linked INTO the program where the host compiler has them, plain otherwise; run
    as a child process."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    src = [os.path.join(ROOT, "tests", "cpp", "test_word_ops.cpp"), os.path.join(ROOT, "poulpy_amd", "csrc", "word_ops.cpp")]
    exe = str(tmp_path / "test_word_ops")
    base = [cxx, "-std=c++17", "-O1", "-g", *src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[fhe_uint_word] host compiler without sanitizer runtimes: built plain")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "all word plan checks passed" in r.stdout, r.stdout[-2000:]


# ---- the oracle's literal restatement under real keys ------------------------------------------------------------------------------------------
SHAPES = {"one_base": fc.ONE_BASE_SHAPE, "ref": fc.REF_SHAPE}
_cases = {}


def case(name, word_bits, index=fc.coefficient):
    """-> (c, ctx): the key case of a shape (made once) and the oracle context of one word width"""
    from oracle.ref import RefModule
    from tests import lwe_cases as lc
    if name not in _cases:
        c = fc.bdd_key_case(SHAPES[name], 48000 + len(name))
        ref = RefModule(c.n)
        _cases[name] = (c, ref, [lc.prepare(ref, k) for k in c.atk])
    c, ref, keys = _cases[name]
    return c, bo.Ctx(ref, c.n, word_bits, c.word_b, c.gals, keys, key_base2k=c.atk_b, conv_size=fs.limbs_for(c.k_word, c.atk_b), index=index)


A32, B32 = 0xFFFFFFFF, 0xAABBCCDD


@pytest.mark.parametrize("name", ["one_base", "ref"])
def test_oracle_splice_u8_and_u16_decrypt_to_the_reference_tests_values(name):
    """test_fhe_uint_splice_u8 / _u16 (tests/test_suite/fheuint.rs:88-205): every (dst, src)"""
    c, ctx = case(name, 32)
    a, b = fc.words_case(c, 32, [A32, B32], 48100)
    for dst in range(4):
        for src in range(4):
            assert fc.decrypt_word(c, bo.splice_u8(ctx, dst, src, a, b), 32) == bo.want_splice(A32, B32, dst, src, 8), (dst, src)
    for dst in range(2):
        for src in range(2):
            assert fc.decrypt_word(c, bo.splice_u16(ctx, dst, src, a, b), 32) == bo.want_splice(A32, B32, dst, src, 16), (dst, src)


@pytest.mark.parametrize("name", ["one_base", "ref"])
def test_oracle_sext_decrypts_to_the_reference_tests_values(name):
    """test_fhe_uint_sext (:20-80): j = 0..2 on a word whose bytes have their sign bits set and on one whose bytes have them clear"""
    c, ctx = case(name, 32)
    for value in (0x84838281, 0x44434241):
        word = fc.words_case(c, 32, [value], 48200 + (value & 0xFF))[0]
        for j in range(3):
            assert fc.decrypt_word(c, bo.sext(ctx, word, j), 32) == bo.want_sext(value, 8 * (j + 1) - 1), (hex(value), j)
        assert fc.decrypt_word(c, bo.sext(ctx, word, 3), 32) == value


@pytest.mark.parametrize("name,word_bits,value", [("one_base", 32, 0xC35A0F96), ("one_base", 16, 0xC35A), ("ref", 32, 0x3CA5F069)])
def test_oracle_get_bit_get_byte_and_zero_byte(name, word_bits, value):
    """test_fhe_uint_get_bit_glwe (:207-250): every bit is the constant coefficient of its GLWE; every byte is a word holding that byte alone
    at byte 0; zero_byte clears its byte and nothing else"""
    c, ctx = case(name, word_bits)
    word = fc.words_case(c, word_bits, [value], 48300 + word_bits)[0]
    for i in range(word_bits):
        pt = fs.normalize(fs.glwe_phase(bo.get_bit_glwe(ctx, word, i), c.sk_glwe), c.word_b)
        assert fs.decode_coeff(pt, c.word_b, 2, 0) & 1 == (value >> i) & 1, i
    for j in range(word_bits // 8):
        assert fc.decrypt_word(c, bo.get_byte(ctx, word, j), word_bits) == (value >> (8 * j)) & 0xFF, j
        assert fc.decrypt_word(c, bo.zero_byte(ctx, word, j), word_bits) == value & ~(0xFF << (8 * j)), j


def test_oracle_controls_decrypt_to_another_word():
    """A splice at the un-interleaved coefficients (index = i -> i << log_gap) and a splice with src off by one are other words."""
    c, ctx = case("one_base", 32)
    a, b = fc.words_case(c, 32, [A32, B32], 48400)
    want = bo.want_splice(A32, B32, 1, 2, 8)
    assert fc.decrypt_word(c, bo.splice_u8(ctx, 1, 2, a, b), 32) == want
    _, plain = case("one_base", 32, index=lambda i, wb, n: i * (n // wb))
    assert fc.decrypt_word(c, bo.splice_u8(plain, 1, 2, a, b), 32) != want
    assert fc.decrypt_word(c, bo.splice_u8(ctx, 1, 3, a, b), 32) != want
