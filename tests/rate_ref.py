"""Reference of the rate report (csrc/rate.hip, DESIGN.md 6 "Rate report") in numpy float64 - shared by test_rate_ref.py and test_gpu_rate.py.

Per coded row, from the float32 logits x, the coded symbol s and the coder's integer pair (c_low, c_high):
  ideal_bits = (m - x[s] + log(sum_j exp(x[j] - m))) / ln 2     m = max_j x[j]; np.exp / np.log on float64(x) - float64(m)
  table_bits = 16 - log2(c_high - c_low)                        from the integers
  top1       = (x[s] == m)
Segment sums are math.fsum over the rows (correctly rounded: no summation order to argue about).
"""
import math

import numpy as np


def softmax_f32(logits):
    """The float32 PMF this library defines (csrc/cdf.hip): exp(x - m) in float32, the row sum a SERIAL float32 sum in column order, a
    correctly rounded float32 division.  (np.cumsum is serial.)"""
    x = np.ascontiguousarray(logits, np.float32)
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / np.cumsum(e, axis=1, dtype=np.float32)[:, -1:]).astype(np.float32)


def cdf_ints(pmf):
    """numpyAc's integer CDF (numpyAc.py:109-114, :80-107) as plain integers [n, nsym + 1], the last column 65536: serial float32 prefix
    sums, divided by the last in float32, times 65536 - nsym in float64, rounded half to even, plus the column index."""
    pmf = np.ascontiguousarray(pmf, np.float32)
    n, nsym = pmf.shape
    c = np.cumsum(pmf, axis=1, dtype=np.float32)
    c = (c / c[:, -1:]).astype(np.float32)
    q = np.rint(np.hstack((np.zeros((n, 1)), c.astype(np.float64))) * (65536 - nsym)).astype(np.int64)
    return q + np.arange(nsym + 1)


def pairs(pmf, sym):
    """(c_low, c_high) of every row's symbol as int64 arrays; c_high of the top symbol is 65536."""
    F = cdf_ints(pmf)
    r, s = np.arange(len(F)), np.asarray(sym, np.int64)
    return F[r, s], F[r, s + 1]


def pack(lo, hi):
    """The pair as scp_softmax_cdf stores it: lo | hi << 16 in a uint32, 65536 stored as 0."""
    return (np.asarray(lo, np.uint32) | ((np.asarray(hi, np.int64) & 0xFFFF).astype(np.uint32) << 16)).astype(np.uint32)


def unpack(lohi):
    lohi = np.asarray(lohi).view(np.uint32).astype(np.int64)
    hi = lohi >> 16
    return lohi & 0xFFFF, np.where(hi == 0, 65536, hi)


def table_bits(lo, hi):
    return 16.0 - np.log2((np.asarray(hi, np.int64) - np.asarray(lo, np.int64)).astype(np.float64))


def ideal_bits(logits, sym):
    x = np.asarray(logits, np.float32).astype(np.float64)
    m = x.max(1)
    xs = x[np.arange(len(x)), np.asarray(sym, np.int64)]
    return (m - xs + np.log(np.exp(x - m[:, None]).sum(1))) / math.log(2.0)


def top1(logits, sym):
    x = np.asarray(logits, np.float32)
    return x[np.arange(len(x)), np.asarray(sym, np.int64)] == x.max(1)


def rows(logits, sym, lohi):
    """Everything per row: dict(ideal, table, width, top1, bad) - a row whose width is below 1 is `bad` and carries 0 in both columns; a row
    whose cross-entropy is not finite (the symbol's logit is -inf) is `bad` with 0 ideal bits, and keeps the table bits of its pair."""
    lo, hi = unpack(lohi)
    w = hi - lo
    with np.errstate(invalid="ignore"):
        ideal = ideal_bits(logits, sym)
    table = np.where(w < 1, 0.0, 16.0 - np.log2(np.maximum(w, 1).astype(np.float64)))
    bad = (w < 1) | ~np.isfinite(ideal)
    return dict(ideal=np.where(bad, 0.0, ideal), table=table, width=w, top1=top1(logits, sym), bad=bad)


def segments(r, seg_off):
    """Per segment [seg_off[i], seg_off[i + 1]) of the row dict `r`: (rows, fsum ideal, fsum table, top1, bad rows)."""
    out = []
    for a, b in zip(seg_off[:-1], seg_off[1:]):
        out.append((int(b - a), math.fsum(r["ideal"][a:b]), math.fsum(r["table"][a:b]), int(r["top1"][a:b].sum()), int(r["bad"][a:b].sum())))
    return out


def segment_tolerance(n_rows, total):
    """What a float64 sum in any order may differ from fsum by, with margin: the rows carry up to 1e-9 bits of error each
    (test_gpu_rate.py: the row bound), and n terms of one sign summed in float64 stay within n * 2^-53 of the exact sum relatively -
    1e-12 covers segments of a few thousand rows."""
    return 1e-9 * n_rows + 1e-12 * abs(total)
