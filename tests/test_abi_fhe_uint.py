"""CPU: pz_fhe_uint_prepare_params, the one struct of include/poulpy_hip.h that is made of parameter structs (declared `struct name {...};`
with its typedef apart, listed in poulpy_amd.abi.COMPOSITE_STRUCTS): typed from the header, and laid out as the C compiler lays it out."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_composite_structs_are_typed_from_the_header():
    from poulpy_amd import abi
    from poulpy_amd.hal import FheUintPrepareParams
    assert list(abi.COMPOSITE_STRUCTS) == ["pz_fhe_uint_prepare_params"]
    assert not set(abi.COMPOSITE_STRUCTS) & (set(abi.STRUCTS) | set(abi.TAGGED_STRUCTS))
    assert FheUintPrepareParams is abi.pz_fhe_uint_prepare_params
    fields = dict(FheUintPrepareParams._fields_)
    assert fields["cbt"] is abi.pz_circuit_bootstrapping_params and fields["ks_glwe"] is abi.pz_glwe_op_params and fields["ks_lwe"] is abi.pz_glwe_op_params
    assert [f for f, _ in FheUintPrepareParams._fields_] == ["cbt", "ks_glwe", "ks_lwe", "n_lwe", "lwe_size", "lwe_base2k", "word_bits", "bit_start",
                                                             "bit_count"]
    # the three new entry points are declared, and typed like every other one
    for name in ("pz_lwe_from_glwe_many_batched", "pz_lwe_from_glwe_many_tmp_bytes", "pz_ggsw_prepare_batched", "pz_fhe_uint_prepare_batched",
                 "pz_fhe_uint_prepare_tmp_bytes"):
        assert name in abi.PROTOTYPES
    assert abi.PROTOTYPES["pz_lwe_from_glwe_many_batched"][1][7] is C.POINTER(abi.pz_glwe_op_params)


def test_composite_structs_match_the_c_compiler(tmp_path):
    """sizeof and every field offset, against g++ on the same header (as test_abi_and_host.py does for the parameter blocks)"""
    from poulpy_amd import abi
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "poulpy_hip.h"', 'int main() {']
    want = []
    for name, cls in abi.COMPOSITE_STRUCTS.items():
        lines.append(f'    std::printf("%zu\\n", sizeof({name}));')
        want.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'    std::printf("%zu\\n", offsetof({name}, {f}));')
            want.append(getattr(cls, f).offset)
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want and len(want) == 10


def test_header_compiles_as_c(tmp_path):
    """the `struct name {...};` + typedef form is C as well as C++"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "poulpy_hip.h"\nint main(void) { pz_fhe_uint_prepare_params p; (void)p; return (int)sizeof(struct pz_fhe_uint_prepare_params) == 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "hdr")], check=True)
