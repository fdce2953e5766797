"""A numpy float64 restatement of the D2 (point-to-plane) path (csrc/normals.hip, scp_amd/metrics.py), for tests that hold the device to
it: the neighbour lists and the tie-set reductions bit for bit, the normals to the accuracy of an eigenvector.

Every operation is written out elementwise in the device's order - d2 = (dx*dx + dy*dy) + dz*dz, projections (dx*nx + dy*ny) + dz*nz,
sums accumulated one term at a time in index (or list) order - because `dot` / `einsum` / `sum` are free to reorder or fuse.  Only the
eigenvectors come from another algorithm (numpy.linalg.eigh against the device's Jacobi sweeps).

The second half is what the MPEG `pc_error` tool computes for "mseF,PSNR (p2plane)" when file A carries normals and file B does not
(tests/golden/d2_metrics.json pins that): with T_A(i) = every b_j at the minimum distance from a_i,
    n_B[j] = mean of n_A[i] over {i : j in T_A(i)},  e_AB[i] = mean_{j in T_A(i)} ((a_i - b_j) . n_B[j])^2,
    e_BA[j] = mean_{i in T_B(j)} ((b_j - a_i) . n_A[i])^2,  mseF = max(mean e_AB, mean e_BA),  PSNR = 10 log10(3 peak^2 / mseF)."""
import math
from collections import namedtuple

import numpy as np

CHUNK = 512

Normals = namedtuple("Normals", "normals count idx lam")


def _sqdist_rows(q, p):
    """[len(q), len(p)] squared distances, the device's expression with dx = q - p."""
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nn_sqdist(q, p):
    """min_j |q_i - p_j|^2: scp_nn_sqdist_f64."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    return np.concatenate([_sqdist_rows(q[s:s + CHUNK], p).min(1) for s in range(0, len(q), CHUNK)])


def neighbours(xyz, radius=1.0, max_nn=30):
    """-> (idx int32 [n, max_nn], -1 padded; count int32 [n]): the up to max_nn nearest points with d2 <= radius^2, the point itself
    included, ordered by (d2, index) - a stable sort on d2 of candidates listed in index order."""
    xyz = np.asarray(xyz, np.float64)
    n, r2 = len(xyz), np.float64(radius) * np.float64(radius)
    idx = np.full((n, max_nn), -1, np.int32)
    count = np.zeros(n, np.int32)
    for s in range(0, n, CHUNK):
        d = _sqdist_rows(xyz[s:s + CHUNK], xyz)
        order = np.argsort(d, axis=1, kind="stable")[:, :max_nn]
        ok = np.take_along_axis(d, order, 1) <= r2
        idx[s:s + CHUNK, :order.shape[1]] = np.where(ok, order, -1)
        count[s:s + CHUNK] = ok.sum(1)
    return idx, count


def estimate_normals(xyz, radius=1.0, max_nn=30, view=(0.0, 0.0, 0.0)):
    """-> Normals(normals [n,3], count, idx, lam [n,3] ascending eigenvalues of the covariance; NaN below 3 neighbours).  Centred
    two-pass covariance summed in list order, unit eigenvector of the smallest eigenvalue, (0,0,1) below 3 neighbours, flipped where
    n . (view - p) < 0."""
    xyz = np.asarray(xyz, np.float64)
    n = len(xyz)
    idx, count = neighbours(xyz, radius, max_nn)
    k = count.astype(np.float64)
    valid = idx >= 0
    pts = xyz[np.where(valid, idx, 0)]                      # [n, max_nn, 3]
    mean = np.zeros((n, 3))
    for s in range(max_nn):
        mean = mean + np.where(valid[:, s, None], pts[:, s], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = mean / k[:, None]
        cov = np.zeros((n, 3, 3))
        for s in range(max_nn):
            c = np.where(valid[:, s, None], pts[:, s] - mean, 0.0)
            for a in range(3):
                for b in range(a, 3):
                    cov[:, a, b] = cov[:, a, b] + c[:, a] * c[:, b]
        for a in range(3):
            for b in range(a, 3):
                cov[:, a, b] = cov[:, a, b] / k
                cov[:, b, a] = cov[:, a, b]
    enough = count >= 3
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    lam = np.full((n, 3), np.nan)
    if enough.any():
        w, v = np.linalg.eigh(cov[enough])
        lam[enough] = w
        v0 = v[:, :, 0]
        normals[enough] = v0 / np.sqrt((v0[:, 0] * v0[:, 0] + v0[:, 1] * v0[:, 1]) + v0[:, 2] * v0[:, 2])[:, None]
    flip = orientation(normals, xyz, view) < 0.0
    normals[flip] = -normals[flip]
    return Normals(normals, count, idx, lam)


def orientation(normals, xyz, view=(0.0, 0.0, 0.0)):
    """n . (view - p), the quantity whose sign orients a normal."""
    v = np.asarray(view, np.float64)
    t = v[None, :] - np.asarray(xyz, np.float64)
    return (normals[:, 0] * t[:, 0] + normals[:, 1] * t[:, 1]) + normals[:, 2] * t[:, 2]


def comparable(ref, xyz, view=(0.0, 0.0, 0.0)):
    """Points whose normal is determined well enough to compare two eigen solvers at 1e-9: the two smallest eigenvalues are separated,
    (lam1 - lam0) / lam2 >= 1e-3, and the orientation test is not at its threshold, |n . (view - p)| > 1e-9 |p|.  Points below 3
    neighbours have a fixed normal and are compared exactly elsewhere."""
    xyz = np.asarray(xyz, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (ref.lam[:, 1] - ref.lam[:, 0]) / ref.lam[:, 2]
    norm = np.sqrt((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2])
    return (ref.count >= 3) & (gap >= 1e-3) & (np.abs(orientation(ref.normals, xyz, view)) > 1e-9 * norm)


def _tie_pairs(q, p, dmin, of_p):
    """(i, j, dx, dy, dz) of every pair whose d2(q_i, p_j) equals the stored minimum (dmin[j] of the streamed cloud if of_p, else
    dmin[i] of the queries), ordered by i and then j."""
    out = []
    for s in range(0, len(q), CHUNK):
        qc = q[s:s + CHUNK]
        dx = qc[:, None, 0] - p[None, :, 0]
        dy = qc[:, None, 1] - p[None, :, 1]
        dz = qc[:, None, 2] - p[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        i, j = np.nonzero(d == (dmin[None, :] if of_p else dmin[s:s + CHUNK, None]))
        out.append((i + s, j, dx[i, j], dy[i, j], dz[i, j]))
    return [np.concatenate(c) for c in zip(*out)]


def tie_mean_normal(q, p, dmin_p, nrm_p):
    """SCP_TIE_MEAN_NORMAL: [nq,3] mean of nrm_p[j] over {j : q_i is a nearest neighbour of p_j}, summed in index order; 0 if none."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    i, j, _, _, _ = _tie_pairs(q, p, np.asarray(dmin_p, np.float64), True)
    s = np.zeros((len(q), 3))
    np.add.at(s, i, np.asarray(nrm_p, np.float64)[j])             # unbuffered: one term at a time, in the order of the pairs
    c = np.bincount(i, minlength=len(q)).astype(np.float64)
    return np.where(c[:, None] > 0, s / np.maximum(c, 1.0)[:, None], 0.0)


def tie_plane_error(q, p, dmin_q, nrm_p):
    """SCP_TIE_PLANE_ERROR: [nq] mean over the nearest neighbours p_j of q_i of ((q_i - p_j) . nrm_p[j])^2."""
    q, p, nrm_p = np.asarray(q, np.float64), np.asarray(p, np.float64), np.asarray(nrm_p, np.float64)
    i, j, dx, dy, dz = _tie_pairs(q, p, np.asarray(dmin_q, np.float64), False)
    pr = (dx * nrm_p[j, 0] + dy * nrm_p[j, 1]) + dz * nrm_p[j, 2]
    s = np.zeros(len(q))
    np.add.at(s, i, pr * pr)
    c = np.bincount(i, minlength=len(q)).astype(np.float64)
    return np.where(c > 0, s / np.maximum(c, 1.0), 0.0)


def d2_terms(a, n_a, b):
    """-> (n_B [nb,3], e_AB [na], e_BA [nb]); no duplicate handling."""
    a, n_a, b = np.asarray(a, np.float64), np.asarray(n_a, np.float64), np.asarray(b, np.float64)
    dab, dba = nn_sqdist(a, b), nn_sqdist(b, a)
    n_b = tie_mean_normal(b, a, dab, n_a)
    return n_b, tie_plane_error(a, b, dab, n_b), tie_plane_error(b, a, dba, n_a)


def merge_duplicates(a, n_a):
    """Exactly duplicated points -> one point (np.unique's order) with the mean of their normals, summed in index order; a cloud
    without duplicates is returned as it is."""
    a, n_a = np.asarray(a, np.float64), np.asarray(n_a, np.float64)
    u = np.unique(a, axis=0)
    if len(u) == len(a):
        return a, n_a
    return u, tie_mean_normal(u, a, np.zeros(len(a)), n_a)


def mean_seq(x):
    """Not the device's reduction order (torch's mean is a tree): the tests compare means at 1e-12 relative."""
    return float(np.mean(x))


def d2_psnr(a, n_a, b, peak, dropdups=True):
    """-> dict(mse_ab, mse_ba, psnr_d2): scp_amd.metrics.d2_psnr."""
    b = np.asarray(b, np.float64)
    if dropdups:
        a, n_a = merge_duplicates(a, n_a)
        ub = np.unique(b, axis=0)
        b = b if len(ub) == len(b) else ub
    _, e_ab, e_ba = d2_terms(a, n_a, b)
    m_ab, m_ba = mean_seq(e_ab), mean_seq(e_ba)
    mse = max(m_ab, m_ba)
    return dict(mse_ab=m_ab, mse_ba=m_ba, psnr_d2=10.0 * math.log10(3.0 * peak * peak / mse) if mse > 0 else float("inf"))
