"""Reference of the per-level temperature (csrc/temper.hip, DESIGN.md 6 "Temperature") in numpy - shared by test_temper_ref.py and
test_gpu_temper.py.

A scaled row is np.float32(beta) * x in float32 (one multiply); its bits are rate_ref.ideal_bits of that row.  A segment's bits are
math.fsum over its rows (as in rate_ref); a GROUP's bits are the serial float64 sum of its segments in segment-index order - the order
the library fixes, so group sums compare bit for bit when they start from the same segment values.
"""
import math

import numpy as np

import rate_ref


def default_grid():
    return np.array([2.0 ** (j / 8) for j in range(-12, 13)], np.float64).astype(np.float32)


def scale(x, beta):
    """fl32(beta * x): float32 times float32, rounded once."""
    return (np.float32(beta) * np.asarray(x, np.float32)).astype(np.float32)


def row_bits(x, sym, betas):
    """-> (bits float64 [n, nt], bad bool [n, nt]): a row whose cross-entropy at beta_j is not finite is bad at j and carries 0 there."""
    x = np.asarray(x, np.float32)
    bits = np.zeros((len(x), len(betas)))
    bad = np.zeros((len(x), len(betas)), bool)
    for j, b in enumerate(betas):
        if len(x):
            with np.errstate(invalid="ignore", over="ignore"):
                v = rate_ref.ideal_bits(scale(x, b), sym)
            bad[:, j] = ~np.isfinite(v)
            bits[:, j] = np.where(bad[:, j], 0.0, v)
    return bits, bad


def segments(bits, bad, seg_off):
    """-> (seg_bits float64 [S, nt] by math.fsum, seg_bad int [S, nt])."""
    S, nt = len(seg_off) - 1, bits.shape[1]
    sb, sd = np.zeros((S, nt)), np.zeros((S, nt), np.int64)
    for s, (a, b) in enumerate(zip(seg_off[:-1], seg_off[1:])):
        for j in range(nt):
            sb[s, j] = math.fsum(bits[a:b, j])
            sd[s, j] = int(bad[a:b, j].sum())
    return sb, sd


def group_sums(seg_bits, group, ngroup):
    """Serial float64 sums in segment-index order; group ids are clamped to 0 .. ngroup - 1.  -> float64 [ngroup, nt]"""
    seg_bits = np.asarray(seg_bits, np.float64)
    out = np.zeros((ngroup, seg_bits.shape[1]))
    for s, g in enumerate(np.clip(np.asarray(group, np.int64), 0, ngroup - 1)):
        out[g] = out[g] + seg_bits[s]
    return out


def pick(sums, unit, min_gain, bad=False, rows=1):
    """One group's choice from its nt sums: the smallest; a tie goes to the index nearest `unit`, then to the lower index.  The group keeps
    `unit` unless the best sum beats the unit sum by MORE than min_gain, and always when it has a bad row or no rows."""
    best = min(range(len(sums)), key=lambda k: (sums[k], abs(k - unit), k))
    if bad or rows == 0 or not (sums[unit] - sums[best] > min_gain):
        best = unit
    return best


def choose(seg_bits, seg_bad, seg_off, group, ngroup, betas, unit, min_gain=8.0):
    """-> dict(choice int [G], group_bits float64 [G, 2] (at unit, at the choice), seg_beta float32 [S], sums float64 [G, nt])."""
    g = np.clip(np.asarray(group, np.int64), 0, ngroup - 1)
    sums = group_sums(seg_bits, g, ngroup)
    rows = np.diff(np.asarray(seg_off, np.int64))
    choice = np.zeros(ngroup, np.int64)
    for k in range(ngroup):
        mine = g == k
        choice[k] = pick(sums[k], unit, min_gain, bad=bool(np.asarray(seg_bad)[mine].any()), rows=int(rows[mine].sum()))
    gb = np.stack((sums[:, unit], sums[np.arange(ngroup), choice]), 1)
    return dict(choice=choice, group_bits=gb, seg_beta=np.asarray(betas, np.float32)[choice[g]], sums=sums)
