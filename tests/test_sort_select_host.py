"""Host side of the Sort kernel's word comparator and tie cut (K29,
kernels/sort_kernels.hip).

``kernels/sort_select.h`` is plain ``__host__ __device__`` C++: a stand-alone
program (native/selftest/sort_select_selftest.cpp) includes it, is built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly.  It compares the bit-sliced comparator (the ``before`` and ``equal``
words, both directions) and the "first q set bits of a word" helper with a
naive per-column loop on random, all-zero and all-one planes, with the
threshold at 0, +-1 and +- the largest magnitude of depths 1, 11 and 32, and q
from 0 to 32.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pilosa_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_comparator_and_tie_cut_match_the_naive_loop_under_asan_ubsan():
    assert os.path.exists(os.path.join(PKG, "kernels", "sort_select.h"))
    out = os.path.join(tempfile.mkdtemp(), "sort_select_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(PKG, "native", "selftest", "sort_select_selftest.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    last = r.stderr.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 failures"), last
    # 7 depths x (6 fixed words + 600 random ones) x >= 10 thresholds x 2 directions, and 604 words x 36 cuts
    assert int(last.split()[0]) >= 7 * 606 * 10 * 2 + 604 * 36
