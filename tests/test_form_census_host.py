"""The census table (tests/form_census_cases.py) against the lists of instantiated forms, host side: tests/cpp/list_forms.cpp expands the
X-macro lists of mid_forms.hpp, tail_plan.hpp and br_forms.hpp with the host compiler, and the table must name exactly those forms - a new
instantiation without a device case fails here, and so does a case for a form that no longer exists.  Nothing here needs a GPU."""
import os
import shutil
import subprocess

import pytest

from tests import form_census_cases as fc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def list_forms(tmp_path_factory):
    """tests/cpp/list_forms.cpp built as test_mid_forms.cpp is: under the host sanitizers where the compiler has their runtimes, plain otherwise"""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("list_forms") / "list_forms")
    base = [cxx, "-std=c++17", "-O1", "-g", os.path.join(ROOT, "tests", "cpp", "list_forms.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, (san.stderr[-1500:], plain.stderr[-1500:])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-1000:])
        return r.stdout.splitlines()
    return run


def test_table_and_lists_agree_entry_for_entry(list_forms):
    listed = list_forms()
    assert len(listed) == len(set(listed)) == 37 + 85 + 28 + 13, len(listed)
    assert sum(k.startswith("k_mid128<") for k in listed) == 19 and sum(k.startswith("k_mid128r<") for k in listed) == 18
    assert sum(k.startswith("k_inv_tail<") for k in listed) == 85
    assert sum(k.startswith("k_br_fused<") for k in listed) == 28 and sum(k.startswith("k_br_block") for k in listed) == 13
    table = set(fc.CENSUS)
    assert not set(listed) - table, f"instantiated forms without a census row: {sorted(set(listed) - table)}"
    assert not table - set(listed), f"census rows for forms that are not instantiated: {sorted(table - set(listed))}"


def test_every_row_has_a_case_or_a_reason_the_lists_bear_out(list_forms):
    """A row is a non-empty list of cases or Unreachable(reason).  The one reason the host can check in full: tail_supported() - the gate in
    front of every launch of the fused tail - is tail_plan_whole_waves (tail_plan.hpp), and it is false for exactly the plans whose rows say so."""
    gate = {line.split(" | ")[0]: line.split(" | ")[1] == "1" for line in list_forms("tail-gate")}
    assert len(gate) == 10
    for key, row in fc.CENSUS.items():
        if isinstance(row, fc.Unreachable):
            assert key.startswith("k_inv_tail<") and " PLAIN(" in key, f"{key}: only plain tails on plans no caller reaches may go without a case"
            assert len(row.reason) > 20
            if row.reason == fc._GATED:
                assert gate[key.split(" ")[0]] is False, key
            continue
        assert len(row) >= 1 and all(isinstance(c, fc.Case) for c in row), key
        if key.startswith("k_inv_tail<"):
            assert gate[key.split(" ")[0]] is True, f"{key}: a case on a plan tail_supported() refuses"
    unreachable = sorted(k for k, r in fc.CENSUS.items() if isinstance(r, fc.Unreachable))
    assert len(unreachable) == 20, unreachable   # 4 plans x 4 plain variants behind the gate, 4 of the plan no ring degree has


def test_middle_kernel_cases_land_on_their_form_by_the_host_chooser(list_forms):
    """the shape launch_mid derives from each case's parameters, through mid128_form itself: the note it chooses is the row's key"""
    for _id, key, case in fc.device_cases():
        if key.startswith("k_mid128"):
            assert list_forms("mid", *fc.glwe_mid_shape(case)) == [key], (_id, fc.glwe_mid_shape(case))


def test_block_step_cases_land_on_their_form_by_the_host_chooser(list_forms):
    for key, cases in fc.BR_BLOCK.items():
        row_max, ncols = fc.block_shape(cases)
        assert list_forms("brblock", row_max, ncols, int(key.startswith("k_br_block_lds"))) == [key], (key, row_max, ncols)
    assert list_forms("brblock", 9, 12, 0) == ["none"]


def test_middle_kernel_batches_leave_one_ciphertext_in_the_last_tile_of_a_grid_that_wraps():
    """the figures the rule gives on 256 CUs, and its two properties on other CU counts"""
    assert [fc.mid_batch(ct, fc.m1_of(8192), 256) for ct in (8, 4, 2)] == [65, 33, 17]
    for cu in (64, 104, 228, 256, 304):
        for n in (8192, 16384, 32768):
            for ct in (8, 4, 2):
                batch, m1 = fc.mid_batch(ct, fc.m1_of(n), cu), fc.m1_of(n)
                n_ct = -(-batch // ct)
                assert batch % ct == 1 and m1 * n_ct > min(cu, 256) and m1 * (n_ct - 1) <= cu
