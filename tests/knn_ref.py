"""Reference of the k-nearest-neighbour searches (scp_amd/csrc/knn.hip) in numpy float64 / int64: the exact list under (squared distance
ascending, index ascending), an emulation of the kernel's fp32 arithmetic that says whether a window's distances are exact in it, a
derived worst-case bound per PAIR on |device value - float64 value|, and the validity check built on that bound.

The kernel's value of a pair is pd = 2 x_i.x_j - |x_j|^2 - |x_i|^2 = -D(i, j); everything here speaks of D = |x_i - x_j|^2 >= 0 and of
lists in ascending D, which is the kernel's descending pd."""
import numpy as np

U = 2.0 ** -24                                             # unit roundoff of fp32, round to nearest
MODES = ("f32", "f16x3")


def _f64(x):
    x = np.asarray(x)
    assert x.ndim == 2
    return x.astype(np.float64)


def sqdist_rows(x, i0, i1):
    """D[i0:i1, :] in float64 by the kernel's own formula (|x_i|^2 + |x_j|^2) - 2 x_i.x_j.  For windows whose coordinates are
    integers times one power of two, small enough that every sum below stays under 2^53 quanta, it is exact."""
    x = _f64(x)
    xx = (x * x).sum(1)
    return (xx[i0:i1, None] + xx[None, :]) - 2.0 * (x[i0:i1] @ x.T)


def _topk_block(D, k):
    """The k first columns of every row of D under (value ascending, column ascending), ties included: all columns below the k-th
    smallest value, then the lowest-numbered columns that equal it."""
    kth = np.partition(D, k - 1, axis=1)[:, k - 1:k]
    below = D < kth
    ties = D == kth
    room = k - below.sum(1)
    sel = below | (ties & (np.cumsum(ties, axis=1) <= room[:, None]))
    cols = np.nonzero(sel)[1].reshape(D.shape[0], k)       # ascending column inside a row
    vals = np.take_along_axis(D, cols, 1)
    order = np.argsort(vals, axis=1, kind="stable")        # stable: equal values keep ascending columns
    return np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)


def topk_f64(x, k, block=256):
    """(idx int64 [n, k], D float64 [n, k]) of the float64 distances under (D ascending, index ascending), blockwise."""
    x = _f64(x)
    n = x.shape[0]
    assert 1 <= k <= n
    idx, val = np.empty((n, k), np.int64), np.empty((n, k), np.float64)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        idx[i0:i1], val[i0:i1] = _topk_block(sqdist_rows(x, i0, i1), k)
    return idx, val


def dyadic_quantum(x):
    """The power of two q with x / q all integers, or None (x not dyadic within 2^-40 .. 2^40 of its largest entry)."""
    x = _f64(x)
    m = np.abs(x).max()
    if m == 0:
        return 1.0
    q = 2.0 ** (np.floor(np.log2(m)) + 1)
    for _ in range(64):
        if np.array_equal(np.rint(x / q), x / q):
            return q
        q *= 0.5
    return None


def exact_topk(x, k, block=256):
    """THE list of an exactly representable window: int64 [n, k].  The coordinates are integers times one power of two q, so every
    squared distance is an integer number of q^2; it is computed in int64 and the list taken under the unique keys D * n + j."""
    x = _f64(x)
    n = x.shape[0]
    assert 1 <= k <= n
    q = dyadic_quantum(x)
    assert q is not None, "exact_topk wants dyadic coordinates"
    xi = np.rint(x / q)                                    # integers held in float64: the matrix product below runs in BLAS and is exact
    xx = (xi * xi).sum(1)
    assert float(np.abs(xi).max()) ** 2 * x.shape[1] * 4 * n < 2.0 ** 52
    out = np.empty((n, k), np.int64)
    j = np.arange(n, dtype=np.int64)[None, :]
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        D = ((xx[i0:i1, None] + xx[None, :]) - 2 * (xi[i0:i1] @ xi.T)).astype(np.int64)
        key = D * n + j
        part = np.argpartition(key, k - 1, axis=1)[:, :k] if k < n else np.broadcast_to(j, key.shape).copy()
        pk = np.take_along_axis(key, part, 1)
        out[i0:i1] = np.take_along_axis(part, np.argsort(pk, axis=1), 1)
    return out


def is_exact_in_fp32(x, block=256):
    """The kernel's documented arithmetic, emulated in float32 with every rounding of its own:
        xx_i = sum_c fl(x_ic * x_ic), added in feature order, one rounding per product and one per sum (sqnorm_kernel),
        dot  = a k-ordered chain acc = fl(acc + x_ic * x_jc), one rounding per step (the fp32 MFMA chain),
        d    = fl(fl(2 dot - xx_j) - xx_i).
    True when xx, every step of the chain and d equal the same quantities in float64 (where they are exact for the windows this is
    meant for), i.e. when no rounding ever happened.  The product of two fp32 numbers is exact in float64, so fl(acc + a * b) is the
    float64 sum rounded once more; the double rounding cannot matter for the answer, which is False as soon as any step rounds."""
    x32 = np.asarray(x, np.float32)
    if not np.array_equal(x32.astype(np.float64), _f64(x)):
        return False
    x = x32.astype(np.float64)
    n, C = x.shape
    xx32 = np.zeros(n, np.float32)
    xx64 = np.zeros(n, np.float64)
    for c in range(C):
        p = x32[:, c] * x32[:, c]
        if not np.array_equal(p.astype(np.float64), x[:, c] * x[:, c]):
            return False
        xx32 = xx32 + p
        xx64 = xx64 + x[:, c] * x[:, c]
        if not np.array_equal(xx32.astype(np.float64), xx64):
            return False
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        acc32 = np.zeros((i1 - i0, n), np.float32)
        acc64 = np.zeros((i1 - i0, n), np.float64)
        for c in range(C):
            acc64 += x[i0:i1, c:c + 1] * x[None, :, c]
            acc32 = (acc32.astype(np.float64) + x[i0:i1, c:c + 1] * x[None, :, c]).astype(np.float32)
            if not np.array_equal(acc32.astype(np.float64), acc64):
                return False
        a32 = np.float32(2.0) * acc32 - xx32[None, :]
        d32 = a32 - xx32[i0:i1, None]
        if not np.array_equal(d32.astype(np.float64), (2.0 * acc64 - xx64[None, :]) - xx64[i0:i1, None]):
            return False
    return True


def _gamma(m):
    return m * U / (1.0 - m * U)


def bound_terms(S, Ni, Nj, C, mode):
    """E(i, j) from S = sum_c |x_ic||x_jc|, Ni = |x_i|^2, Nj = |x_j|^2 of the pair and the feature count C; see `bound`."""
    assert mode in MODES
    g = _gamma(C)
    if mode == "f32":
        edot = g * S
    else:
        G = np.sqrt(Ni * Nj)
        rc = np.sqrt(float(C))
        p, f0 = 1.0 + 2.0 ** -11, 2.0 ** -38
        e1, f1 = 2.0 ** -11 * p, (2.0 + 2.0 ** -11) * 2.0 ** -38
        e2, f2 = 2.0 ** -22, p * 2.0 ** -38
        dropped = (e1 * e1 * S + 2 * e1 * f1 * rc * G + f1 * f1 * C * G) \
            + (e2 * S + f2 * rc * G) \
            + ((1 + e2) * e2 * S + ((1 + e2) * f2 + e2 * f2) * rc * G + f2 * f2 * C * G)
        prods = (p * p * S + 2 * p * f0 * rc * G + f0 * f0 * C * G) + 2 * (p * e1 * S + (p * f1 + e1 * f0) * rc * G + f0 * f1 * C * G)
        edot = dropped + _gamma(3 * C) * prods
    r = (1.0 + U) ** 2
    return 2.0 * edot * r + g * (Ni + Nj) * r + (r - 1.0) * (2.0 * (S + edot) + (1.0 + g) * (Ni + Nj))


def bound(x, i, j, mode):
    """Worst-case E(i, j) >= |device value - float64 value| of the pair (i, j) (arrays broadcast), from the arithmetic the header of
    knn.hip documents.  u = 2^-24, gamma_m = m u / (1 - m u) (m roundings in a row), S = sum_c |x_ic||x_jc|, Ni = |x_i|^2, Nj = |x_j|^2.

    Shared by both modes.
      xx: C rounded products and C - 1 rounded sums of non-negative terms: |xx_fl - N| <= gamma_C N.
      d = fl(fl(2 P - xx_j) - xx_i), P the computed dot product with |P - x_i.x_j| <= Edot (2 P and the power-of-two scales are
      exact).  Each of the two roundings is relative u of its result, so
          E = (1 + u)^2 (2 Edot + gamma_C (Ni + Nj)) + ((1 + u)^2 - 1) (2 (S + Edot) + (1 + gamma_C)(Ni + Nj)).
    f32: P is one k-ordered chain acc = fl(acc + x_ic x_jc) of C steps (any other order of C fused or unfused steps, the generic
      kernel's included, puts at most C roundings on a term as well; zero padding adds exact zeros): Edot = gamma_C S.
    f16x3: a row is scaled by a power of two (exact) so that its largest |entry| lies in [2^13, 2^14), then split t = ta + tb + rho
      with ta = f16(t), tb = f16(t - ta) (t - ta is exact in fp32).  An f16 rounding errs by 2^-11 relative in the normal range and by
      at most 2^-25 absolute below 2^-14, which is phi = 2^-38 of the row's largest entry after un-scaling.  Per entry a of a row
      with largest entry A:
          |xa| <= (1 + 2^-11) a + phi A,      |xb| <= 2^-11 (1 + 2^-11) a + (2 + 2^-11) phi A,      |rho| <= 2^-22 a + (1 + 2^-11) phi A.
      (The header's "residual < 2^-22 |x|" is this without the phi term: it holds for entries within 2^16 of the row's largest,
      i.e. |t| >= 2^-3, where the 2^-25 floor is no more than 2^-22 |t|.)
      x y - (xa ya + xa yb + xb ya) = xb yb + rho_x y + (xa + xb) rho_y exactly; summed over c with sum_c a_c <= sqrt(C Ni),
      A <= sqrt(Ni), i.e. sum_c a_c B <= sqrt(C) G, sum_c A B <= C G, G = sqrt(Ni Nj), this gives `dropped` of bound_terms: 3 * 2^-22 S
      (7.2e-7 S) plus phi terms.  The 3 C products are exact in fp32 (11 x 11 bits) and accumulated in fp32, at most 3 C roundings
      on a term whatever the order inside the MFMA: gamma_3C sum |products|, sum |products| <= ((1 + 2^-11)^2 + 2^-10 (1 + 2^-11)^2) S
      plus phi terms.  Edot = dropped + gamma_3C sum |products|.
    Nothing here is fitted to device output.  Underflow of the distances themselves (entries below 2^-60) is not modelled."""
    x = _f64(x)
    i, j = np.broadcast_arrays(np.asarray(i), np.asarray(j))
    ax = np.abs(x)
    xx = (x * x).sum(1)
    S = (ax[i] * ax[j]).sum(-1)
    return bound_terms(S, xx[i], xx[j], x.shape[1], mode)


def _bound_lists(x, idx, mode, block=512):
    """E(i, idx[i, t]) for lists idx [n, m]."""
    x = _f64(x)
    ax = np.abs(x)
    xx = (x * x).sum(1)
    out = np.empty(idx.shape, np.float64)
    for i0 in range(0, x.shape[0], block):
        i1 = min(x.shape[0], i0 + block)
        S = np.einsum("ic,imc->im", ax[i0:i1], ax[idx[i0:i1]])
        out[i0:i1] = bound_terms(S, xx[i0:i1, None], xx[idx[i0:i1]], x.shape[1], mode)
    return out


def _dist_lists(x, idx, block=512):
    """D(i, idx[i, t]) in float64 by the same formula as sqdist_rows."""
    x = _f64(x)
    xx = (x * x).sum(1)
    out = np.empty(idx.shape, np.float64)
    for i0 in range(0, x.shape[0], block):
        i1 = min(x.shape[0], i0 + block)
        out[i0:i1] = (xx[i0:i1, None] + xx[idx[i0:i1]]) - 2.0 * np.einsum("ic,imc->im", x[i0:i1], x[idx[i0:i1]])
    return out


def row_tolerance(x, lists, mode):
    """tol_i = 2 max E(i, m) over the columns m of `lists` [n, m]."""
    return 2.0 * _bound_lists(x, lists, mode).max(1)


def check_valid(x, idx, k, mode, truth=None):
    """Is idx [n, k] (indices local to the window x [n, C]) a valid answer of a search whose values err by at most `bound`?
      - indices are in 0 .. n - 1, i.e. inside the row's own sequence; the k indices of a row are distinct;
      - D(i, j) <= D_k(i) + tol_i for every returned j, tol_i = 2 max E(i, m) over m in (returned | true top-k): a returned j beat,
        on the device, some true neighbour m that was left out, both values off by at most their E;
      - the returned values do not decrease by more than tol_i from one column to the next.
    Every row is judged.  Returns (None, worst) when valid, worst = the largest excess / tol_i seen (0 when nothing exceeds);
    else (message, worst).  truth = topk_f64(x, k) when the caller has it already."""
    x = _f64(x)
    n = x.shape[0]
    idx = np.asarray(idx).astype(np.int64)
    if idx.shape != (n, k):
        return f"shape {idx.shape}, wanted {(n, k)}", np.inf
    bad = (idx < 0) | (idx >= n)
    if bad.any():
        r = int(np.nonzero(bad.any(1))[0][0])
        return f"row {r}: index outside its sequence: {idx[r].tolist()}", np.inf
    if k > 1 and (np.diff(np.sort(idx, 1), axis=1) == 0).any():
        r = int(np.nonzero((np.diff(np.sort(idx, 1), axis=1) == 0).any(1))[0][0])
        return f"row {r}: repeated index: {idx[r].tolist()}", np.inf
    tidx, tval = truth if truth is not None else topk_f64(x, k)
    tol = np.maximum(row_tolerance(x, idx, mode), row_tolerance(x, tidx, mode))
    got = _dist_lists(x, idx)
    over = (got - tval[:, -1:]).max(1)
    if k > 1:
        over = np.maximum(over, (-np.diff(got, axis=1)).max(1))
    over = np.maximum(over, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(over > 0, over / tol, 0.0)
    worst = float(ratio.max())
    if (over > tol).any():
        r = int(np.argmax(ratio))
        return (f"row {r}: excess {over[r]:.6g} over tol {tol[r]:.6g} (D_k {tval[r, -1]:.9g}; returned {got[r].tolist()}, idx {idx[r].tolist()})", worst)
    return None, worst


def check_exact(x, idx, k, want=None):
    """Entry-for-entry equality with exact_topk; None or a message naming the first wrong row."""
    want = exact_topk(x, k) if want is None else want
    idx = np.asarray(idx).astype(np.int64)
    if idx.shape != want.shape:
        return f"shape {idx.shape}, wanted {want.shape}"
    diff = (idx != want).any(1)
    if diff.any():
        r = int(np.nonzero(diff)[0][0])
        return f"{int(diff.sum())} rows differ; row {r}: got {idx[r].tolist()}, wanted {want[r].tolist()}"
    return None
