"""Host side of the Distinct kernel's register transpose (K26,
kernels/distinct_kernels.hip).

``kernels/bit_transpose.h`` is plain ``__host__ __device__`` C++: a stand-alone
program (native/selftest/bit_transpose_selftest.cpp) includes it, is built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly.  It compares the 32 x 32 transpose with the naive bit loop on random,
all-zero, all-one and every single-bit matrix, and on bit planes built from 32
column values.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pilosa_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_bit_transpose32_matches_the_naive_loop_under_asan_ubsan():
    assert os.path.exists(os.path.join(PKG, "kernels", "bit_transpose.h"))
    out = os.path.join(tempfile.mkdtemp(), "bit_transpose_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(PKG, "native", "selftest", "bit_transpose_selftest.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r =subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    last = r.stderr.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 failures"), last
    assert int(last.split()[0]) >= 1024 + 2 + 2000
