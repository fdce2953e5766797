"""Ring LOD in numpy ("Ring LOD"): the integer rule that gives every range ring its own truncation depth, restated from its
definition for the tests - thresholds from ring edges, J, the snap, the implied mask and the cell centres.  int64 throughout.

A cell of size 2^j is cut out of the leaf lattice: its origin is a multiple of 2^j on every axis.  Its doubled radial centre is
c2 = 2 * origin[0] + 2^j - 1, its ring the number of thresholds t_i with c2 >= 2 * t_i, and it is terminal iff drops[ring] >= j.
J(x, s) is the largest j in max(s, 1) .. max(drops) whose cell around x is terminal, 0 if there is none."""
import math

import numpy as np

T_MAX = 2 ** 31 - 1
ROW_TABLE_BITS = 16.0 - math.log2(65282.0)      # a forced row under round(c * (65536 - 255)) + arange: (c_low, c_high) = (0, 65282)


def thresholds(edges, qs0, offset0):
    """t_i = clamp(ceil((edge_i - offset0) / qs0), 0, 2^31 - 1) for edges[1:], float64."""
    out = []
    for e in list(edges)[1:]:
        v = math.ceil((np.float64(e) - np.float64(offset0)) / np.float64(qs0))
        out.append(int(min(max(v, 0), T_MAX)))
    return out


def ring_of(c2, thr):
    c2 = np.asarray(c2, np.int64)
    r = np.zeros(c2.shape, np.int64)
    for t in thr:
        r += c2 >= 2 * int(t)
    return r


def J(x0, s, thr, drops):
    """x0: radial integer positions, s: one start exponent or one per position -> int64 J per position."""
    x0 = np.asarray(x0, np.int64)
    s = np.broadcast_to(np.asarray(s, np.int64), x0.shape)
    drops = np.asarray(drops, np.int64)
    best = np.zeros(x0.shape, np.int64)
    for j in range(1, int(drops.max()) + 1):
        origin = x0 - np.mod(x0, 2 ** j)
        c2 = 2 * origin + 2 ** j - 1
        terminal = drops[ring_of(c2, thr)] >= j
        best = np.where(terminal & (j >= np.maximum(s, 1)), j, best)
    return best


def snap(q, thr, drops):
    """Quantised points int [P,3] -> (snapped points int64 [P,3], j int64 [P])."""
    q = np.asarray(q, np.int64)
    j = J(q[:, 0], 0, thr, drops)
    m = 2 ** j[:, None]
    return q - np.mod(q, m), j


def implied(origins, size_exp, thr, drops):
    """Node origins [n,3] (leaf units) with their size exponents -> bool [n]: the node lies inside (or is) a terminal cell."""
    return J(np.asarray(origins, np.int64)[:, 0], size_exp, thr, drops) > 0


def centres(origins, j):
    """Cell origins [n,3] and exponents [n] -> float64 centres origin + (2^j - 1) / 2 per axis (exact half-integers)."""
    return np.asarray(origins, np.int64).astype(np.float64) + ((2.0 ** np.asarray(j, np.int64) - 1.0) / 2.0)[:, None]


def unique_rows(a):
    """Sorted unique rows of an integer [n,3] array."""
    return np.unique(np.asarray(a, np.int64), axis=0)
