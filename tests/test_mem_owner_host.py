"""Host test of the memory owner (csrc/ewarp_mem.h: Buf, Arena, the
reallocation hook).  `make -C enterprise_warp_amd/csrc mem-test` builds
tests/hip/mem_owner_test.cpp -- a stand-alone program that supplies
mem_alloc / mem_free itself on malloc / free -- with
-fsanitize=address,undefined; it runs here as a child process.  No GPU."""
import os
import subprocess

from conftest import ROOT

BINARY = os.path.join(ROOT, "build", "mem_owner_test")


def test_mem_owner_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "mem-test"],
                   check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([BINARY], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
