"""Reference of the depth report (csrc/ringrate.hip, DESIGN.md 6 "Depth report") in numpy float64, built on ringrate_ref - shared by
test_depth_ref.py and test_gpu_depth.py.  Plain loops over parents.

One tree of depth D (nodes in BFS order, occ / level / parent as in ringrate_ref), leaves in the order of the tree's leaves:
  cost_k(p) = ((share(a_1) + share(a_2)) + ..) + share(a_{D-k}) for 0 <= k < D, a_l = the ancestor of leaf p at level l: the chain of
              ringrate_ref.leaf_cost_brute cut short; +0.0 for k >= D
  cells of LOD k (1 <= k <= D - 1) = the nodes of level D - k + 1; a cell's origin is (leaf >> k) << k of every leaf below it, its
              centre origin + (2^k - 1) / 2; LOD 0 = the leaves
"""
import numpy as np

import ringrate_ref as rr


def prefix_cost(occ, level, parent, depth, bits, k):
    """float64 [n_leaves]: for every leaf, climb `parent` from its level-D node to the root, then add the shares of levels 1 .. D - k,
    root first - the literal chain."""
    n = len(occ)
    cnt = rr.leaves_per_node(occ, level, parent, depth).astype(np.float64)
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
        for j in list(reversed(chain))[:max(depth - k, 0)]:             # root first, the first D - k levels
            s = np.float64(bits[j]) / cnt[j]
            total = s if total is None else total + s
        out += [np.float64(0.0) if total is None else total] * int(rr.POP[occ[i]])
    return np.array(out, np.float64)


def planes(occ, level, parent, depth, bits, max_drop):
    """float64 [max_drop + 1, n_leaves]: plane k = prefix_cost(.., k), from ONE climb per level-D node - the partial sums of the chain
    are the chains cut short (the same operations in the same order), so every plane is read off the same walk."""
    n = len(occ)
    cnt = rr.leaves_per_node(occ, level, parent, depth).astype(np.float64)
    cols = []
    for i in range(n):
        if level[i] != depth:
            continue
        chain, j = [], i
        while j >= 0:
            chain.append(j)
            j = parent[j]
        assert len(chain) == depth
        partial, total = [np.float64(0.0)], None                         # partial[m] = the first m levels added up
        for j in reversed(chain):
            s = np.float64(bits[j]) / cnt[j]
            total = s if total is None else total + s
            partial.append(total)
        col = [partial[max(depth - k, 0)] for k in range(max_drop + 1)]
        cols += [col] * int(rr.POP[occ[i]])
    return np.array(cols, np.float64).reshape(-1, max_drop + 1).T.copy()


def cell_origins(leaves, k):
    """The distinct cell origins of integer leaves [n,3] at LOD k, in the order of their first leaf, and the cell of every leaf."""
    o = (np.asarray(leaves).astype(np.int64) >> k) << k
    uniq, first, inverse = np.unique(o, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return uniq[order], rank[np.asarray(inverse).reshape(-1)]


def centres(cells_or_leaves, k):
    """float64 [n,3]: origin + (2^k - 1) / 2 in leaf units - exact (half-integers)."""
    o = (np.asarray(cells_or_leaves).astype(np.int64) >> k) << k
    return o.astype(np.float64) + (2 ** k - 1) / 2.0
