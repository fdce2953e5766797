"""Reference of the rate per ring (csrc/ringrate.hip, DESIGN.md 6 "Rate per ring") in numpy float64 - shared by test_ringrate_ref.py
and test_gpu_ringrate.py.  Plain loops over parents and levels.

One tree: nodes in BFS order with occ (1 .. 255), level (1 .. D), parent (0-based index, -1 for the root); bits = what every node cost.
  leaves(i) = popcount(occ_i) for a node of level D, the sum over the node's children otherwise
  share(i)  = bits(i) / float64(leaves(i))
  cost(p)   = ((share(a_1) + share(a_2)) + ..) + share(a_D), a_l = the ancestor of leaf p at level l: root first
  leaf p    = level-D node j owns the popcount(occ_j) consecutive leaves that start at the exclusive prefix sum of the popcounts before it
  bin       = group * n_rings + ring, ring = the largest r with rho2 >= edge_r^2, rho2 = (x*x + y*y) + z*z of (point - view)
Bin records: leaves (a count), ideal_bits / table_bits (math.fsum: correctly rounded, no order to argue about), max_ideal_bits.
"""
import math

import numpy as np

POP = np.array([bin(v).count("1") for v in range(256)], np.int64)


def leaves_per_node(occ, level, parent, depth):
    """int64 [n]: children come after their parent in BFS order, so one walk from the back finishes every node before it is handed up."""
    n = len(occ)
    out = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        if level[i] == depth:
            out[i] = POP[occ[i]]
        if parent[i] >= 0:
            out[parent[i]] += out[i]
    return out


def leaf_cost(occ, level, parent, depth, bits):
    """float64 [n_leaves] in the order of the tree's leaves: level by level, a node's sum is its parent's plus its own share."""
    n = len(occ)
    share = np.asarray(bits, np.float64) / leaves_per_node(occ, level, parent, depth).astype(np.float64)
    acc = np.empty(n, np.float64)
    for lv in range(1, depth + 1):
        for i in np.flatnonzero(np.asarray(level) == lv):
            acc[i] = share[i] if parent[i] < 0 else acc[parent[i]] + share[i]
    last = np.flatnonzero(np.asarray(level) == depth)
    return np.repeat(acc[last], POP[np.asarray(occ)[last]])


def leaf_cost_brute(occ, level, parent, depth, bits):
    """The definition read literally: for every leaf, climb `parent` from its level-D node to the root, then add the shares root first."""
    n = len(occ)
    cnt = np.zeros(n, np.int64)
    for i in range(n):                                      # leaves(i) by climbing from every level-D node
        if level[i] == depth:
            j = i
            while j >= 0:
                cnt[j] += POP[occ[i]]
                j = parent[j]
    out = []
    for i in range(n):
        if level[i] != depth:
            continue
        chain, j = [], i
        while j >= 0:
            chain.append(j)
            j = parent[j]
        assert len(chain) == depth
        total = None
        for j in reversed(chain):                           # root first
            s = np.float64(bits[j]) / np.float64(cnt[j])
            total = s if total is None else total + s
        out += [total] * int(POP[occ[i]])
    return np.array(out, np.float64)


def ring(rho2, edges):
    esq = np.asarray(edges, np.float64) * np.asarray(edges, np.float64)
    return np.searchsorted(esq, rho2, side="right") - 1


def bins(xyz, edges, group=None, n_groups=1, view=(0.0, 0.0, 0.0)):
    a = np.asarray(xyz, np.float64) - np.asarray(view, np.float64)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    rho2 = (x * x + y * y) + z * z
    g = np.zeros(len(a), np.int64) if group is None else np.asarray(group, np.int64)
    return (g * len(edges) + ring(rho2, edges)).astype(np.int32)


def record(cost_ideal, cost_table):
    return dict(leaves=int(len(cost_ideal)), ideal_bits=math.fsum(cost_ideal), table_bits=math.fsum(cost_table),
                max_ideal_bits=float(cost_ideal.max()) if len(cost_ideal) else 0.0)


def records(cost_ideal, cost_table, bin_of, n_bins):
    return [record(cost_ideal[bin_of == k], cost_table[bin_of == k]) for k in range(n_bins)]


def node_bits(level_counts, drop_last, context_size, row_bits):
    """Per-node bits from per-row bits in CODING order (encode.py:109-136: every level cut into windows of context_size rows, inside a
    window the even positions first, then the odd ones).  level_counts: nodes per level of ONE tree; drop_last: its last BFS node has no
    row.  -> float64 [n_nodes], 0 for the dropped node."""
    sizes = list(level_counts)
    if drop_last:
        sizes[-1] -= 1
    out = np.zeros(int(sum(level_counts)), np.float64)
    k, row = 0, 0
    for n in sizes:
        for i in range(0, n, context_size):
            c = min(context_size, n - i)
            for pos in list(range(0, c, 2)) + list(range(1, c, 2)):
                out[row + i + pos] = row_bits[k]
                k += 1
        row += n
    assert k == len(row_bits)
    return out
