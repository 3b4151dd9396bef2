"""The ctypes table (omldm_amd/ops/native.py: HIP_SIGS) against the HIP library's exports.

The loader skips a table row whose symbol is missing, so a stale row — or an entry point
nobody listed — goes unnoticed until a call fails. Needs the built library, not a GPU."""
import os
import shutil
import subprocess

import pytest

from omldm_amd.ops import native


@pytest.fixture(scope="module")
def exported():
    if not os.path.exists(native.HIP_LIB_PATH):
        pytest.skip("libomldm_hip.so is not built")
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    if nm is None:
        pytest.skip("no nm to list the library's exports")
    out = subprocess.run([nm, "-D", "--defined-only", native.HIP_LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    return {n for n in names if n.startswith("omldm_")}


def test_every_table_row_is_exported(exported):
    missing = sorted(name for name, _, _ in native.HIP_SIGS if name not in exported)
    assert not missing, f"HIP_SIGS rows without an export: {missing}"


def test_every_scan3_export_is_in_the_table(exported):
    listed = {name for name, _, _ in native.HIP_SIGS}
    unlisted = sorted(n for n in exported if n.startswith("omldm_scan3") and n not in listed)
    assert not unlisted, f"omldm_scan3* exports missing from HIP_SIGS: {unlisted}"


def test_table_has_no_duplicate_rows():
    names = [name for name, _, _ in native.HIP_SIGS]
    assert len(names) == len(set(names))
