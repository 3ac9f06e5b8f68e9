"""Host test of the factorisation route (csrc/ewarp_route.h: route_for,
partial_route_for, refine_after).  `make -C enterprise_warp_amd/csrc
route-test` builds tests/hip/route_table_test.cpp with plain g++; compiling it
evaluates the header's static_asserts (the route table of the product modes,
and equality with the routing code the header replaced for every mode and
width).  The program runs here as a child process and prints the table.  No
GPU."""
import os
import subprocess

from conftest import ROOT

BINARY = os.path.join(ROOT, "build", "route_table_test")


def test_route_table_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "route-test"],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=60)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "42 rows, 0 failed" in r.stdout
    lines = {tuple(ln.split()[:2]): ln.split() for ln in r.stdout.splitlines()[1:-1]}
    # mode 0: fixed white noise leaves the register kernels for the verify route at 10 blocks
    assert lines[("0", "9")][2] == "register" and lines[("0", "10")][2] == "dd-verify"
    assert lines[("0", "16")][4] == "big" and lines[("0", "17")][4] == "dd-verify"
    assert lines[("0", "65")][2] == "unsupported"
