"""Distortion of the quantiser, on the device.

`chamfer_psnr(pc, quant, peak)` = what the reference obtains from `pointCloud.distChamfer(pc, quantized_pc)`
(data_preproc/pt.py:88-95: max of the two mean nearest-neighbour distances, KD-tree in float64) and from the MPEG `pc_error`
tool it shells out to with `-r peak` (pt.py:13-85; `get_psnr`, utils/__init__.py:3-15 reads "mseF,PSNR (p2point)"):
    mse_ab = mean_i min_j |a_i - b_j|^2,  mseF = max(mse_ab, mse_ba),  PSNR = 10 log10(3 peak^2 / mseF)
peak = 59.70 (KITTI) / 30000 (Ford) (encode_dataset_ehem.py:115-117).  pc_error merges exactly duplicated input points
before measuring (--dropdups=2, its default): `chamfer_psnr(..., dropdups=True)` does the same for the PSNR only.

`estimate_normals` + `d2_psnr` = the D2 (point-to-plane) column: data_preproc/gene_normals.py (open3d hybrid search, radius 1.0, at most
30 neighbours, normals turned towards the sensor) and the "mseF,PSNR (p2plane)" lines of the same pc_error run.  With A the cloud that
carries normals and B the other one, T_A(i) = every b_j at the minimum distance from a_i (all equal-distance neighbours, not the first):
    n_B[j]  = mean of n_A[i] over {i : j in T_A(i)}            (plain mean, not renormalised; an unreferenced b_j never enters)
    e_AB[i] = mean over j in T_A(i) of ((a_i - b_j) . n_B[j])^2,   e_BA[j] = mean over i in T_B(j) of ((b_j - a_i) . n_A[i])^2
    mseF = max(mean e_AB, mean e_BA),  PSNR = 10 log10(3 peak^2 / mseF)
which reproduces the tool to its six printed digits on tie-free and tie-laden clouds (tests/golden/d2_metrics.json).  Exactly duplicated
points of A are merged as for D1 and take the mean of their normals; the tool's own rule for duplicates that carry DIFFERENT normals was
not identified (a probe printed 0.919601 / 1.98458, which none of keep-all / mean / first / last / sum / normalised mean gives).
The normals are not open3d's bit for bit: the neighbour sets agree except at exact distance ties, but the covariance is the centred
two-pass one and the eigenvector comes from Jacobi sweeps - D2 on estimated normals is this project's number, D2 on given normals the tool's.

`distortion_report` = where the D1 error goes (csrc/distreport.hip; no counterpart in the reference): the nearest-neighbour error of both
directions per range ring and, for the reconstructed cloud, per rho shell, split along the sensor's (r, phi, theta) axes.
"""
import math

import numpy as np
import torch

from . import native

PEAK = {"kitti": 59.70, "ford": 30000.0, "obj": 1.0}


def _unique_rows(x):
    return torch.unique(x, dim=0)


def chamfer_psnr(pc, quant, peak, dropdups=True):
    """pc [P,3], quant [U,3] device tensors (any float dtype; compared in float64).  Returns dict(chamfer, psnr, mse_ab, mse_ba)."""
    a = pc.to(torch.float64).contiguous()
    b = quant.to(torch.float64).contiguous()
    dab = native.nn_sqdist(a, b)
    dba = native.nn_sqdist(b, a)
    chamfer = max(float(dab.sqrt().mean().item()), float(dba.sqrt().mean().item()))
    if dropdups and (a.shape[0] != _unique_rows(a).shape[0] or b.shape[0] != _unique_rows(b).shape[0]):
        ua, ub = _unique_rows(a), _unique_rows(b)
        m_ab = float(native.nn_sqdist(ua, ub).mean().item())
        m_ba = float(native.nn_sqdist(ub, ua).mean().item())
    else:
        m_ab, m_ba = float(dab.mean().item()), float(dba.mean().item())
    mse = max(m_ab, m_ba)
    psnr = 10.0 * math.log10(3.0 * peak * peak / mse) if mse > 0 else float("inf")
    return dict(chamfer=chamfer, psnr=psnr, mse_ab=m_ab, mse_ba=m_ba)


def estimate_normals(xyz, radius=1.0, max_nn=30, view=(0.0, 0.0, 0.0)):
    """xyz [n,3] device tensor -> unit normals float64 [n,3], oriented towards `view` (gene_normals.py:43-44)."""
    return native.estimate_normals(xyz, radius, max_nn, view)[0]


def _merge_duplicates(a, normals):
    """Exactly duplicated points -> one point with the mean of their normals (summed in index order by the tie-set kernel: the
    duplicates of u are the points at distance 0).  Clouds without duplicates come back untouched, in their own order."""
    u = _unique_rows(a)
    if u.shape[0] == a.shape[0]:
        return a, normals
    zero = torch.zeros((a.shape[0],), dtype=torch.float64, device=a.device)
    return u, native.nn_tieset(native.TIE_MEAN_NORMAL, u, a, zero, normals)


def d2_terms(a, normals, b):
    """Per-point terms of the p2plane metric, float64 device tensors, no duplicate handling: (n_B [nb,3], e_AB [na], e_BA [nb])."""
    dab = native.nn_sqdist(a, b)
    dba = native.nn_sqdist(b, a)
    n_b = native.nn_tieset(native.TIE_MEAN_NORMAL, b, a, dab, normals)
    e_ab = native.nn_tieset(native.TIE_PLANE_ERROR, a, b, dab, n_b)
    e_ba = native.nn_tieset(native.TIE_PLANE_ERROR, b, a, dba, normals)
    return n_b, e_ab, e_ba


def d2_psnr(pc, normals, quant, peak, dropdups=True):
    """pc [P,3] with normals [P,3], quant [U,3]: device tensors (compared in float64).  Returns dict(mse_ab, mse_ba, psnr_d2)."""
    a = pc.to(torch.float64).contiguous()
    n_a = normals.to(torch.float64).contiguous()
    b = quant.to(torch.float64).contiguous()
    if n_a.shape != a.shape:
        raise native.ScpError(f"d2_psnr: {tuple(n_a.shape)} normals for a cloud of shape {tuple(a.shape)}")
    if dropdups:
        a, n_a = _merge_duplicates(a, n_a)
        b = b if _unique_rows(b).shape[0] == b.shape[0] else _unique_rows(b)
    _, e_ab, e_ba = d2_terms(a, n_a, b)
    m_ab, m_ba = float(e_ab.mean().item()), float(e_ba.mean().item())
    mse = max(m_ab, m_ba)
    psnr = 10.0 * math.log10(3.0 * peak * peak / mse) if mse > 0 else float("inf")
    return dict(mse_ab=m_ab, mse_ba=m_ba, psnr_d2=psnr)


DIST_SUMS = ("sum_sq", "sum_r2", "sum_phi2", "sum_theta2", "sum_r")
DEFAULT_EDGES = {"kitti": (0.0, 5.0, 10.0, 15.0, 20.0, 30.0, 40.0, 60.0, 80.0)}          # metres; Ford counts millimetres
DEFAULT_EDGES["ford"] = tuple(1000.0 * e for e in DEFAULT_EDGES["kitti"])


def default_edges(data_type):
    """The ring edges the report uses when none are given: KITTI 0, 5, 10, 15, 20, 30, 40, 60, 80 m, Ford the same in its millimetres."""
    if data_type not in DEFAULT_EDGES:
        raise native.ScpError(f"distortion report: no default ring edges for --type {data_type} (its unit of length is the file's own): "
                              "give edges, e.g. --distortion_report 0,0.5,1,2")
    return DEFAULT_EDGES[data_type]


def _dist_entry(rows, axis_rows, sums, max_sq, hist):
    """One entry of the report from raw sums (plain Python numbers).  mse = sum_sq / rows; mse_r, mse_phi, mse_theta = the component sums
    over the same rows, so they add up to mse less what the axis points (which have no frame) carry; bias_r = sum_r / (rows - axis_rows);
    max = sqrt(max_sq).  An entry without rows has zeros there."""
    e = dict(rows=int(rows), axis_rows=int(axis_rows), max_sq=float(max_sq), hist=[int(h) for h in hist])
    e.update({k: float(v) for k, v in zip(DIST_SUMS, sums)})
    n, framed = e["rows"], e["rows"] - e["axis_rows"]
    e["mse"] = e["sum_sq"] / n if n else 0.0
    e["mse_r"] = e["sum_r2"] / n if n else 0.0
    e["mse_phi"] = e["sum_phi2"] / n if n else 0.0
    e["mse_theta"] = e["sum_theta2"] / n if n else 0.0
    e["bias_r"] = e["sum_r"] / framed if framed else 0.0
    e["max"] = math.sqrt(e["max_sq"])
    return e


def dist_entries(raw):
    """scp_dist_seg records on the host (numpy int64 [n_bins, 72], native.dist_segments(...)["raw"].cpu().numpy()) -> one entry per bin."""
    rec = native.dist_record_views(np.ascontiguousarray(raw, np.int64))
    return [_dist_entry(rec["rows"][k], rec["axis_rows"][k], [rec[name][k] for name in DIST_SUMS], rec["max_sq"][k], rec["hist"][k])
            for k in range(raw.shape[0])]


def dist_total(entries):
    """The entry of several bins together: counts and histograms add, the maximum is the largest, every sum is math.fsum over the bins."""
    hist = [sum(e["hist"][k] for e in entries) for k in range(native.DIST_HIST)]
    return _dist_entry(sum(e["rows"] for e in entries), sum(e["axis_rows"] for e in entries),
                       [math.fsum(e[name] for e in entries) for name in DIST_SUMS], max([e["max_sq"] for e in entries] + [0.0]), hist)


def distortion_dict(edges, raw_ab, raw_ba, n_groups=1):
    """The report from the two directions' records on the host (no device needed): raw_ab int64 [R, 72] (pc -> quant, one bin per ring),
    raw_ba int64 [n_groups * R, 72] (quant -> pc, bin = group * R + ring), R = len(edges).  Plain Python throughout (json.dumps takes it)."""
    edges = list(native.dist_edges(edges))
    R = len(edges)
    if raw_ab.shape[0] != R or raw_ba.shape[0] != n_groups * R:
        raise native.ScpError(f"distortion report: {raw_ab.shape[0]} and {raw_ba.shape[0]} records for {R} rings and {n_groups} groups")
    ab, ba = dist_entries(raw_ab), dist_entries(raw_ba)
    return dict(edges=edges, a_to_b=dict(rings=ab, total=dist_total(ab)),
                b_to_a=dict(groups=[ba[g * R:(g + 1) * R] for g in range(n_groups)], total=dist_total(ba)))


def _dist_direction(a, b, edges, group, n_groups, view):
    s = native.nn_error_split(a, b, edges, group, n_groups, view)
    return native.dist_segments(s["d2"], s["comp"], s["flag"], s["bin"], n_groups * len(edges))["raw"]


def distortion_report(pc, quant, edges, quant_group=None, n_groups=1, view=(0.0, 0.0, 0.0)):
    """Where the D1 error of `quant` [U,3] against `pc` [P,3] goes (device tensors, compared in float64), both directions:
        a_to_b  every point of pc against its nearest point of quant, binned by the ORIGINAL point's range ring:   a_to_b["rings"][r]
        b_to_a  every point of quant against its nearest point of pc, binned by (quant_group, ring of the RECONSTRUCTED point):
                b_to_a["groups"][g][r]   (quant_group: device int32 [U], 0 <= g < n_groups - the encoder passes the rho shell; None: one group)
    and a_to_b["total"], b_to_a["total"].  Ring r holds edges[r] <= rho < edges[r+1] as seen from `view`, the last ring is open-ended.
    Every entry holds the raw sums of include/scp.h's scp_dist_seg (rows, axis_rows, sum_sq, sum_r2, sum_phi2, sum_theta2, sum_r, max_sq,
    hist[64]) and mse, mse_r, mse_phi, mse_theta, bias_r, max derived from them (_dist_entry); the totals' sums are math.fsum over the
    bins.  The nearest neighbour is the lowest index among equals and the sums run in a fixed order, so the report is the same bits in
    every run.  No duplicate merging is done: a_to_b["total"]["sum_sq"] / P is the mse_ab of chamfer_psnr(..., dropdups=False).
    Returns plain Python (one device -> host copy per direction)."""
    a = pc.to(torch.float64).contiguous()
    b = quant.to(torch.float64).contiguous()
    edges = native.dist_edges(edges)
    raw_ab = _dist_direction(a, b, edges, None, 1, view)
    raw_ba = _dist_direction(b, a, edges, quant_group, n_groups, view)
    return distortion_dict(edges, raw_ab.cpu().numpy(), raw_ba.cpu().numpy(), n_groups)


def _share_entry(leaves, ideal, table, mx):
    """One entry of the rate-per-ring report from raw sums (plain Python numbers); an entry without leaves has zeros per leaf."""
    n = int(leaves)
    return dict(leaves=n, ideal_bits=float(ideal), table_bits=float(table), max_ideal_bits=float(mx),
                ideal_bits_per_leaf=float(ideal) / n if n else 0.0, table_bits_per_leaf=float(table) / n if n else 0.0)


def _share_total(entries):
    """Several bins together: counts add, the maximum is the largest, both sums are math.fsum over the bins."""
    return _share_entry(sum(e["leaves"] for e in entries), math.fsum(e["ideal_bits"] for e in entries),
                        math.fsum(e["table_bits"] for e in entries), max([e["max_ideal_bits"] for e in entries] + [0.0]))


def ring_rate_dict(edges, raw, points, n_groups=1):
    """The rate-per-ring report from the scp_share_seg records on the host (no device needed): raw int64 [n_groups * R, 4] (bin = group *
    R + ring, native.share_segments(...)["raw"].cpu().numpy()), points = the R counts of input points per ring, R = len(edges).  -> edges,
    groups[g][r], rings[r] (the groups added, plus `points` and the bits per input point), total.  Plain Python (json.dumps takes it)."""
    edges = list(native.dist_edges(edges))
    R = len(edges)
    raw = np.ascontiguousarray(raw, np.int64)
    if raw.ndim != 2 or raw.shape != (n_groups * R, len(native.SHARE_FIELDS)) or len(points) != R:
        raise native.ScpError(f"rate per ring: {raw.shape} records and {len(points)} point counts for {R} rings and {n_groups} groups")
    rec = native.share_record_views(raw)
    flat = [_share_entry(rec["leaves"][k], rec["ideal_bits"][k], rec["table_bits"][k], rec["max_ideal_bits"][k]) for k in range(n_groups * R)]
    groups = [flat[g * R:(g + 1) * R] for g in range(n_groups)]

    def with_points(e, n):
        n = int(n)
        return dict(e, points=n, ideal_bits_per_point=e["ideal_bits"] / n if n else 0.0, table_bits_per_point=e["table_bits"] / n if n else 0.0)
    rings = [with_points(_share_total([g[r] for g in groups]), points[r]) for r in range(R)]
    return dict(edges=edges, groups=groups, rings=rings, total=with_points(_share_total(flat), sum(int(n) for n in points)))


def lod_centres(cells_or_leaves, k):
    """The centres of the LOD-k cells ("Depth report") of integer leaves or cell origins [n,3] (a device or host torch
    tensor, or a numpy array): origin = (x >> k) << k per axis, centre = origin + (2^k - 1) / 2 in leaf units -> float64 [n,3], exact
    (half-integers).  One row per input row: leaves of one cell give the same centre.  k = 0: the leaves themselves."""
    k = int(k)
    if k < 0 or k > native.MAX_DEPTH:
        raise native.ScpError(f"lod_centres: k = {k} outside 0 .. {native.MAX_DEPTH}")
    half = (2 ** k - 1) / 2.0
    if isinstance(cells_or_leaves, torch.Tensor):
        x = cells_or_leaves.to(torch.int64)
        return (torch.bitwise_left_shift(torch.bitwise_right_shift(x, k), k)).to(torch.float64) + half
    x = np.asarray(cells_or_leaves).astype(np.int64)
    return ((x >> k) << k).astype(np.float64) + half


def depth_dict(edges, raw, points, n_groups, cells, distortion, d1, shell_leaves, shell_depths):
    """The depth report from its raw parts on the host (no device needed): raw int64 [K + 1, n_groups * R, 4] = the scp_share_seg records
    of planes k = 0 .. K (native.share_segments_depth(...)["raw"].cpu().numpy()), points = the R counts of input points per ring, and per
    k: cells (one count per shell), distortion (a metrics.distortion_report dict), d1 (a metrics.chamfer_psnr dict).  -> edges,
    shell_leaves, shell_depths, levels[k] = dict(drop, cells, rate = ring_rate_dict on plane k, distortion, d1).  Plain Python."""
    edges = list(native.dist_edges(edges))
    raw = np.ascontiguousarray(raw, np.int64)
    K1 = len(cells)
    if raw.ndim != 3 or raw.shape[0] != K1 or len(distortion) != K1 or len(d1) != K1 or K1 < 1:
        raise native.ScpError(f"depth report: {raw.shape} records, {len(distortion)} distortion reports and {len(d1)} PSNRs for {K1} depths")
    if len(shell_leaves) != n_groups or len(shell_depths) != n_groups or any(len(c) != n_groups for c in cells):
        raise native.ScpError(f"depth report: {len(shell_leaves)} leaf counts, {len(shell_depths)} depths and cell counts {cells} for {n_groups} shells")
    levels = [dict(drop=k, cells=[int(c) for c in cells[k]], rate=ring_rate_dict(edges, raw[k], points, n_groups), distortion=distortion[k],
                   d1={name: float(v) for name, v in d1[k].items()}) for k in range(K1)]
    return dict(edges=edges, shell_leaves=[int(n) for n in shell_leaves], shell_depths=[int(d) for d in shell_depths], levels=levels)


def dequantize(leaves, qs, offset, spher=False, cylin=False, f32=False):
    """leaves int [U,3] (device) -> de-quantised Cartesian points [U,3]: `pt * qs + offset` in float64, then spher2cart /
    cylin2cart (data_preprocess.py:186-229).  f32=True: the same-level path rounds to float32 before the inverse transform
    (data_preprocess.py:85-91), the multi-level path stays in float64 (:160-167)."""
    q = torch.as_tensor([float(x) for x in qs], dtype=torch.float64, device=leaves.device)
    o = torch.as_tensor([float(x) for x in offset], dtype=torch.float64, device=leaves.device)
    p = leaves.to(torch.float64) * q + o
    if f32:
        p = p.to(torch.float32)
    if cylin:
        rho, phi, z = p[:, 0], p[:, 1], p[:, 2]
        return torch.stack((rho * torch.cos(phi), rho * torch.sin(phi), z), 1)
    if spher:
        rho, phi, th = p[:, 0], p[:, 1], p[:, 2]
        return torch.stack((rho * torch.sin(th) * torch.cos(phi), rho * torch.sin(th) * torch.sin(phi), rho * torch.cos(th)), 1)
    return p
