"""FheUint words to word, host side: the four entry points in the header and the ctypes view, the level map of
pz_fhe_uint_pack_batched against a walk of glwe_pack_default's loop, its stand-alone check under the host sanitizers, and the oracle's
statement of FheUint::pack under real keys.  Nothing here needs a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fhe_sk as fs
from tests import fhe_uint_cases as fc
from tests import fhe_uint_pack_oracle as po
from tests.helpers import seeded

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW = ("pz_fhe_uint_pack_tmp_bytes", "pz_fhe_uint_pack_batched", "pz_fhe_uint_execute_tmp_bytes", "pz_fhe_uint_execute_batched")


def test_entry_points_declared_and_typed_without_a_new_struct():
    import ctypes as C
    from poulpy_amd import abi
    header = open(os.path.join(ROOT, "include", "poulpy_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in abi.PROTOTYPES, name
    p = C.POINTER(abi.pz_glwe_op_params)
    v, z = C.c_void_p, C.c_size_t
    assert abi.PROTOTYPES["pz_fhe_uint_pack_tmp_bytes"] == (z, [v, p, z, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_pack_batched"] == (C.c_int, [v, v, v, z, v, v, p, z, v, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_execute_tmp_bytes"] == (z, [v, v, p, p, z, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_execute_batched"] == (C.c_int, [v, v, v, z, v, z, p, v, v, p, z, v, z, z])
    assert abi.PROTOTYPES["pz_fhe_uint_pack_level_pairs"] == (z, [z, z, z, v, z])
    # the struct lists are what they were (tests/test_abi_and_host.py, tests/test_abi_fhe_uint.py pin their contents)
    assert list(abi.STRUCTS) == ["pz_glwe_op_params", "pz_glwe_tensor_params", "pz_glwe_mul_const_params", "pz_glwe_term",
                                 "pz_blind_rotation_params", "pz_circuit_bootstrapping_params"]
    assert list(abi.TAGGED_STRUCTS) == ["pz_bdd_node"] and list(abi.COMPOSITE_STRUCTS) == ["pz_fhe_uint_prepare_params"]
    # the C++ mirror and the Python layers
    hpp = open(os.path.join(ROOT, "include", "poulpy_hip.hpp")).read()
    from poulpy_amd import bdd, hal
    for name in NEW:
        assert name + "(" in hpp, name
        assert hasattr(hal.Module, name[3:]), name
    assert callable(bdd.fhe_uint_pack_words) and callable(bdd.fhe_uint_execute)


@pytest.mark.parametrize("word_bits", [8, 16, 32, 64, 128])
def test_level_map_is_the_walk_of_glwe_pack(word_bits):
    """The library's per-level (lo slot, hi slot, t) list = glwe_packing.rs:147-168 walked over {bit_index(s) << log_gap: s}, which meets the
    both-present branch of pack_internal only and leaves its survivor at index 0 in slot 0.  Two ring degrees each: n = word_bits
    (log_gap = 0) or its double, and a large one."""
    from poulpy_amd import hal
    for n in (max(word_bits, 32), 2048):
        want, branches, last = po.walk_levels(n, word_bits)
        assert branches == {"both"} and last == 0, (n, word_bits, branches, last)
        log_bits = word_bits.bit_length() - 1
        assert len(want) == log_bits
        got = [hal.fhe_uint_pack_level_pairs(n, word_bits, lv) for lv in range(log_bits)]
        assert got == want, (n, word_bits)
        assert [len(g) for g in got] == [word_bits >> (lv + 1) for lv in range(log_bits)]
        assert [g[0][2] for g in got] == [n >> (lv + 1) for lv in range(log_bits)]
        assert hal.fhe_uint_pack_level_pairs(n, word_bits, log_bits) == []
    # the un-interleaved map is another tree: the walk then pairs other slots
    assert po.walk_levels(2048, word_bits, index=lambda s, wb: s)[0] != po.walk_levels(2048, word_bits)[0] or word_bits == 8


def test_level_map_refuses_bad_shapes():
    from poulpy_amd import hal
    for n, w in ((1024, 12), (1024, 256), (1024, 0), (64, 128), (96, 32)):
        assert hal.fhe_uint_pack_level_pairs(n, w, 0) == [], (n, w)


def test_level_map_stand_alone_under_the_host_sanitizers(tmp_path):
    """tests/cpp/test_pack_levels.cpp + poulpy_amd/csrc/pack_levels.cpp, no HIP, its own main: every word width at every ring degree from
    word_bits to 2^16 against a walk of the reference's loop, the table check, damaged tables, bad shapes.  Built with
    -fsanitize=address,undefined with the sanitizer runtimes linked INTO the program where the host compiler has them, plain otherwise; run
    as a child process."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    src = [os.path.join(ROOT, "tests", "cpp", "test_pack_levels.cpp"), os.path.join(ROOT, "poulpy_amd", "csrc", "pack_levels.cpp")]
    exe = str(tmp_path / "test_pack_levels")
    base = [cxx, "-std=c++17", "-O1", "-g", *src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])
        print("[fhe_uint_pack] host compiler without sanitizer runtimes: built plain")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "all pack level checks passed" in r.stdout, r.stdout[-2000:]


def test_eight_bit_interleaving_is_the_identity():
    """(why the negative control above excludes u8: with one byte, bit_index(i) = i)"""
    assert [fc.bit_index(i, 8) for i in range(8)] == list(range(8))
    assert [fc.bit_index(i, 16) for i in range(16)] != list(range(16))


# ---- the oracle's statement under real keys ----------------------------------------------------------------------------------------------------
def bit_ciphertexts(c, value, word_bits, base2k, size, k, seed):
    """(word_bits, size, cols, n): bit s of `value` encrypted at coefficient 0, encoded at k = 2 - what the evaluator hands to FheUint::pack."""
    rng = seeded(seed)
    out = []
    for s in range(word_bits):
        data = np.zeros(c.n, dtype=np.int64)
        data[0] = (value >> s) & 1
        out.append(fs.glwe_encrypt(c.sk_glwe, fs.encode(data, base2k, 2, size), base2k, k, rng))
    return np.ascontiguousarray(np.stack(out))


@pytest.mark.parametrize("word_bits,value", [(8, 0xA6), (16, 0xC35A)])
def test_oracle_pack_of_single_bit_encryptions_decrypts_to_the_word(word_bits, value):
    from oracle.ref import RefModule
    from tests import lwe_cases as lc
    c = fc.bdd_key_case(fc.ONE_BASE_SHAPE, 45000 + word_bits)
    ref = RefModule(c.n)
    keys = [lc.prepare(ref, k) for k in c.atk]
    bits = bit_ciphertexts(c, value, word_bits, c.word_b, c.word_size, c.k_word, 45100 + word_bits)
    word = po.pack_word(ref, bits, word_bits, c.word_b, c.gals, keys)
    assert fc.decrypt_word(c, word, word_bits) == value
    if word_bits > 8:   # (u8: the interleaving is the identity)
        plain = po.pack_word(ref, bits, word_bits, c.word_b, c.gals, keys, index=lambda s, wb: s)
        assert fc.decrypt_word(c, plain, word_bits) != value, "packing at the un-interleaved indices decrypted to the value"
    else:   # the control a u8 can have: the bits in reverse order are another word
        rev = po.pack_word(ref, bits, word_bits, c.word_b, c.gals, keys, index=lambda s, wb: wb - 1 - s)
        assert fc.decrypt_word(c, rev, word_bits) != value
