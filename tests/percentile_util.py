"""Shared pieces of the Percentile() tests: the numpy oracle, decimal ``nth``
literals that land on a chosen rank, and the case list run on the host
(tests/test_percentile.py) and on the device (tests/test_gpu_percentile.py)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def rank(nth_text: str, n: int) -> int:
    """Nearest rank k = max(1, ceil(nth * N / 100)) in exact arithmetic."""
    x = Fraction(nth_text) * n / 100
    return max(1, -((-x.numerator) // x.denominator))


def oracle(values, nth_text: str):
    """(k-th smallest of ``values``, entries equal to it); (0, 0) when empty."""
    values = np.asarray(values, dtype=np.int64)
    if len(values) == 0:
        return 0, 0
    s = np.sort(values)
    x = int(s[rank(nth_text, len(s)) - 1])
    return x, int((s == x).sum())


def nth_for_rank(k: int, n: int) -> str:
    """A decimal literal (at most 6 decimals, so a float literal's repr keeps
    it) whose nearest rank over n values is exactly k (1 <= k <= n < 1e7)."""
    t = Fraction(k * 100 * 10 ** 6 // n, 10 ** 6)      # in ((k-1) * 100 / n, k * 100 / n]
    assert Fraction((k - 1) * 100, n) < t <= Fraction(k * 100, n)
    whole, frac = divmod(t.numerator * (10 ** 6 // t.denominator), 10 ** 6)
    text = f"{whole}.{frac:06d}".rstrip("0")
    text = text + "0" if text.endswith(".") else text   # always a float literal
    assert rank(text, n) == k
    return text


NTHS = ["0", "0.0", "0.1", "25", "25.0", "50", "50.0", "99.9", "100", "100.0"]


def boundary_nths(values):
    """nth literals landing on k == Nneg, k == Nneg + 1 (the sign boundary)
    and first / inside / last of the longest run of equal values."""
    s = np.sort(np.asarray(values, dtype=np.int64))
    n = len(s)
    out = []
    nneg = int((s < 0).sum())
    for k in (nneg, nneg + 1):
        if 1 <= k <= n:
            out.append(nth_for_rank(k, n))
    uniq, first, counts = np.unique(s, return_index=True, return_counts=True)
    i = int(np.argmax(counts))
    a, c = int(first[i]), int(counts[i])
    assert c >= 3, "the fixture needs a run of at least 3 equal values"
    for k in (a + 1, a + 1 + c // 2, a + c):
        out.append(nth_for_rank(k, n))
    return out


def call_text(field: str, nth_text: str, filt: str = "") -> str:
    return f"Percentile({filt + ', ' if filt else ''}field={field}, nth={nth_text})"
