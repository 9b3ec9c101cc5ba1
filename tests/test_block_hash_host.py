"""Host side of the device block checksums (K22, kernels/sync_kernels.hip).

* The XXH64 state functions the kernel calls (kernels/xxh64_state.h: round,
  merge, tail, finalise) are exercised by a stand-alone program
  (native/selftest/block_hash_selftest.cpp) built with AddressSanitizer +
  UndefinedBehaviorSanitizer and run directly; the expected digests come from
  the ``xxhash`` module over the same words as big-endian bytes.
* Without a GPU, ``API.fragment_blocks`` / ``fragment_block_data`` answer
  exactly what the fragments' host path answers.
"""
import base64
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import xxhash

from tests.helpers import SW

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(os.path.dirname(HERE), "pilosa_amd", "native")


def _case(words: np.ndarray, piece: int) -> str:
    want = xxhash.xxh64(words.astype(">u8").tobytes()).hexdigest()
    return f"{len(words)} {want} {piece}\n" + " ".join(f"{int(w):x}" for w in words) + "\n"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_xxh64_state_functions_match_xxhash_under_asan_ubsan():
    out = os.path.join(tempfile.mkdtemp(), "block_hash_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(NATIVE, "selftest", "block_hash_selftest.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    rng = np.random.default_rng(22)
    cases = []
    for n in list(range(10)) + [31, 32, 33, 2500, 4099, 20001]:
        words = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        for piece in (0, 3, 5):
            cases.append(_case(words, piece))
    # positions as the kernel sees them: row << 20 | column, a row id past 2^40
    pos = (np.uint64(2**40 + 3) << np.uint64(20)) + np.arange(0, 7000, 7, dtype=np.uint64)
    cases.append(_case(pos, 0))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], input="".join(cases), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert f"{len(cases)} cases, 0 failures" in r.stderr


def test_api_blocks_without_gpu_are_the_host_path():
    from pilosa_amd.server.server import Server
    from pilosa_amd.utils.logger import CaptureLogger

    s = Server(tempfile.mkdtemp(), bind="127.0.0.1:0", gpu="off", logger=CaptureLogger()).open()
    try:
        s.api.create_index("i")
        s.api.create_field("i", "f")
        rng = np.random.default_rng(4)
        rows = rng.integers(0, 450, 6000)
        cols = rng.integers(0, 2 * SW, 6000)
        s.api.import_bits("i", "f", 0, row_ids=rows[cols < SW].tolist(), col_ids=cols[cols < SW].tolist())
        s.api.import_bits("i", "f", 1, row_ids=rows[cols >= SW].tolist(), col_ids=cols[cols >= SW].tolist())
        assert s.executor.gpu is None
        for shard in (0, 1):
            frag = s.holder.fragment("i", "f", "standard", shard)
            vals = frag.storage.slice()
            # the host path, written out: XXH64 over each block's positions as big-endian u64
            want = []
            for bid in np.unique(vals // np.uint64(100 * SW)).tolist():
                part = vals[vals // np.uint64(100 * SW) == np.uint64(bid)]
                want.append({"id": bid, "checksum": base64.b64encode(
                    xxhash.xxh64(part.astype(">u8").tobytes()).digest()).decode()})
            assert len(want) == 5
            assert s.api.fragment_blocks("i", "f", "standard", shard) == want
            assert [(b["id"], base64.b64decode(b["checksum"])) for b in want] == frag.blocks()
            r, c = s.api.fragment_block_data("i", "f", "standard", shard, 2)
            part = vals[vals // np.uint64(100 * SW) == np.uint64(2)]
            assert r.tolist() == (part // np.uint64(SW)).tolist() and c.tolist() == (part % np.uint64(SW)).tolist()
    finally:
        s.close()
