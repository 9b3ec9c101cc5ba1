"""Host side of the ConstRow kernel's unit range search, location split and
meta word (K30, kernels/const_row_kernels.hip).

``kernels/const_row.h`` is plain ``__host__ __device__`` C++: a stand-alone
program (native/selftest/const_row_selftest.cpp) includes it, is built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run
directly.  It compares the lower-bound search of a unit's range, the (unit,
word, bit) split and the meta packing with a naive loop over the whole vector
on random vectors (with duplicates), the empty vector, single elements, every
column in one unit (a full container too) and a unit whose range ends exactly
at the vector's end; the vectors are heap blocks of exactly their length, so
a read past either end is a sanitizer error.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pilosa_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_range_search_split_and_meta_match_the_naive_loop_under_asan_ubsan():
    assert os.path.exists(os.path.join(PKG, "kernels", "const_row.h"))
    out = os.path.join(tempfile.mkdtemp(), "const_row_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(PKG, "native", "selftest", "const_row_selftest.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    last = r.stderr.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 failures"), last
    # 3 checks (range, bitmap, meta) per unit: 12 fixed vectors over 16 .. 48 units and 40 random
    # ones over at least 16, plus one split check per listed column
    assert int(last.split()[0]) >= 3 * 16 * (12 + 40) + 65536
