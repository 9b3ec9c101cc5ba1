"""Host side of the set-like Extract kernel's position and hit arithmetic
(K28, kernels/extract_rows_kernels.hip).

``kernels/filter_rank.h`` is plain ``__host__ __device__`` C++: a stand-alone
program (native/selftest/filter_rank_selftest.cpp) includes it, is built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly.  It compares the output position of a filter column and the hit
enumerations of array chunks (0, 1, 8, 9 and 4,096 values), bitmap words and
runs (inside one word, ending on bit 31 or 63, over many words, the whole key)
with a naive bit loop, on random, empty, full and single-bit filters.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pilosa_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_filter_rank_matches_the_naive_loop_under_asan_ubsan():
    assert os.path.exists(os.path.join(PKG, "kernels", "filter_rank.h"))
    out = os.path.join(tempfile.mkdtemp(), "filter_rank_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(PKG, "native", "selftest", "filter_rank_selftest.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    last = r.stderr.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 failures"), last
    # 16 filters x (positions + 10 arrays + 4 bitmaps + 60 runs)
    assert int(last.split()[0]) == 16 * (1 + 10 + 4 + 60)
