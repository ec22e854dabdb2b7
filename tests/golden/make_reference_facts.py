#!/usr/bin/env python3
"""Generates tests/golden/reference_facts.json: what tests/test_rust_shim.py needs to know about the reference (Rust) checkout, recorded
once so that the tests run without it.  Only derived data is stored - names, yes / no answers to the tests' regexes, digests - no source.

  * the required fns of `HalImpl` / `CoreImpl`, the fns each `impl_core_*_default_methods!` macro writes, the `Znx*` impls of
    poulpy-cpu-ref, the cross-backend tests of the HAL suite and the tests poulpy-cpu-avx instantiates;
  * the answer to every (file, regex) query in tests/test_rust_shim.py::REF_QUERIES;
  * the SHA-256 of tools/gen_rust_shim.py and of the two files it writes from the reference (run here, so they are current).

    python tests/golden/make_reference_facts.py --reference PATH_TO_REFERENCE_CHECKOUT
"""
import argparse
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_facts.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GENERATED = ("tools/gen_rust_shim.py", "rust/poulpy-hip-mi355x/src/hal_impl.rs", "rust/poulpy-hip-mi355x/src/core_impl.rs")


def sha256(rel):
    return hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (poulpy-hal/, poulpy-core/, ...)")
    ref = ap.parse_args().reference
    read = lambda *p: open(os.path.join(ref, *p)).read()
    import gen_rust_shim as g
    from tests.test_rust_shim import REF_QUERIES

    # the committed shim is what the generator writes from this checkout
    sys.argv = [sys.argv[0], "--reference", ref]
    g.main()
    g.core_main(ref)

    macro_fns = {}
    for fam in ("decryption", "conversion", "operations", "encryption"):
        s = read("poulpy-core", "src", "oep", fam + ".rs")
        macro_fns[fam] = re.findall(r"\n        fn (\w+)", s[s.index("macro_rules!"):])
    hal_suite = {}
    for mod_ in ("vec_znx", "vec_znx_big", "vec_znx_dft", "svp", "vmp"):
        s = read("poulpy-hal", "src", "test_suite", mod_ + ".rs")
        hal_suite[mod_] = [m.group(1) for m in re.finditer(r"pub fn (test_\w+)(?:<[^>]*>)?\s*\(\s*params", s)]
    avx = read("poulpy-cpu-avx", "src", "fft64", "tests.rs")
    avx_suite = {m.group(1): sorted(set(re.findall(r"(test_\w+)\s*=>", m.group(2))))
                 for m in re.finditer(r"mod (\w+),.*?tests = \{(.*?)\n    \}", avx, re.S)}
    facts = {
        "reference": {"poulpy-hal": re.search(r'^version = "([^"]+)"', read("poulpy-hal", "Cargo.toml"), re.M).group(1),
                      "poulpy-core": re.search(r'^version = "([^"]+)"', read("poulpy-core", "Cargo.toml"), re.M).group(1)},
        "hal_trait_fns": [m[0] for m in g.parse_trait(os.path.join(ref, "poulpy-hal", "src", "oep", "hal_impl.rs"))],
        "core_trait_fns": [m[0] for m in g.parse_trait_named(os.path.join(ref, "poulpy-core", "src", "oep", "core_impl.rs"), "pub unsafe trait CoreImpl")],
        "core_macro_fns": macro_fns,
        "cpu_ref_znx_impls": re.findall(r"\nimpl (Znx\w+) for FFT64Ref", read("poulpy-cpu-ref", "src", "fft64", "znx.rs")),
        "hal_suite_cross_backend_tests": hal_suite,
        "avx_suite_tests": avx_suite,
        "avx_mentions": {w: w in avx for w in ("test_convolution", "test_convolution_by_const", "test_convolution_pairwise")},
        "queries": {f"{path} :: {pat}": bool(re.search(pat, read(path))) for path, pat in REF_QUERIES},
        "sha256": {rel: sha256(rel) for rel in GENERATED},
    }
    with open(OUT, "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
