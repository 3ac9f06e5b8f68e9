"""Host test of the compact power-law records and the unit decode that the
fixed-form spectrum prologue of chol_mfma_kernel reads (csrc/ewarp_spec.h:
pl_pack, PlRec, unit_decode).  `make -C enterprise_warp_amd/csrc spec-test`
builds tests/hip/spec_pack_test.cpp with plain g++ under ASan and UBSan;
compiling it evaluates the header's static_asserts on the record's size and
offsets.  The program runs here as a child process: which jobs qualify (a
turnover, free-spectrum or constant entry, more than three entries, no theta
row: not), one to three entries with constants and sampled parameters in
either slot, the 16-byte pieces at the offsets the kernel loads, the padding
that adds an exact +0.0, and the decode against u / B and u % B for every unit
of several launches (B = 1, B no power of two, u0 no multiple of B).  No
GPU."""
import os
import subprocess

from conftest import ROOT

BINARY = os.path.join(ROOT, "build", "spec_pack_test")


def test_spec_pack_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "spec-test"],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and " checks, 0 failed" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("decode ")]
    assert len(lines) == 11 and all(ln.endswith(": 0 wrong") for ln in lines)
    assert any(" B 1:" in ln for ln in lines) and any(" B 7:" in ln for ln in lines)
