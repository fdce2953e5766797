#!/usr/bin/env python3
"""Cost of the D2 (point-to-plane) PSNR on a full frame: normals + D2 of the 120 000-point synth_frame(0) at level 12 --spher.

Device: estimate_normals, d2_psnr and (for scale) chamfer_psnr, each timed with device events over --reps calls after a warm-up.
Host: the same computation with a scipy KD-tree on this machine's CPU (hybrid search radius 1.0 / 30 neighbours, covariance + eigh;
nearest neighbours both ways and the plane errors - the first nearest neighbour only, exact ties are not collected), wall clock.
Writes one JSON document (--out, by default profiles/d2_metrics.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def host_threads():
    """Threads for the KD-tree queries: what the machine grants this process (OMP_NUM_THREADS where it is set), not every core it has."""
    return max(1, int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))))


def host_normals(xyz, radius=1.0, max_nn=30, workers=-1):
    from scipy.spatial import cKDTree
    d, idx = cKDTree(xyz).query(xyz, k=max_nn, distance_upper_bound=radius, workers=workers)
    valid = np.isfinite(d)
    cnt = valid.sum(1)
    pts = xyz[np.where(valid, idx, 0)]
    mean = np.where(valid[:, :, None], pts, 0.0).sum(1) / cnt[:, None]
    c = np.where(valid[:, :, None], pts - mean[:, None], 0.0)
    cov = np.einsum("nka,nkb->nab", c, c) / cnt[:, None, None]
    n = np.linalg.eigh(cov)[1][:, :, 0]
    n[cnt < 3] = (0.0, 0.0, 1.0)
    flip = (n * -xyz).sum(1) < 0
    n[flip] = -n[flip]
    return n


def host_d2(a, n_a, b, peak, workers=-1):
    from scipy.spatial import cKDTree
    _, jab = cKDTree(b).query(a, workers=workers)
    _, iba = cKDTree(a).query(b, workers=workers)
    s = np.zeros((len(b), 3))
    np.add.at(s, jab, n_a)
    c = np.bincount(jab, minlength=len(b))
    n_b = s / np.maximum(c, 1)[:, None]
    e_ab = (((a - b[jab]) * n_b[jab]).sum(1) ** 2).mean()
    e_ba = (((b - a[iba]) * n_a[iba]).sum(1) ** 2).mean()
    return 10.0 * np.log10(3.0 * peak * peak / max(e_ab, e_ba))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d2_metrics.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=12)
    args = ap.parse_args()
    from cfgs import ehem_cfg
    from scp_amd import metrics, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    native.lib()
    dev = torch.device("cuda:0")
    xyz = synth_frame(0)
    x = torch.from_numpy(xyz).to(dev)
    enc = FrameEncoder(EHEM(ehem_cfg()).to(dev), "kitti", args.level, spher=True, device=dev)
    enc.preprocess(x)
    info = enc._infos[0]
    quant = metrics.dequantize(enc.geom.leaves(0), info.qs, info.offset, spher=True, f32=True).double()
    normals = metrics.estimate_normals(x)
    res = dict(frame="synth_frame(0)", points=int(x.shape[0]), leaves=int(quant.shape[0]), level=args.level, mode="spher", reps=args.reps,
               device=torch.cuda.get_device_name(0))
    res["device_ms"] = dict(estimate_normals=device_ms(lambda: metrics.estimate_normals(x), args.reps),
                            d2_psnr=device_ms(lambda: metrics.d2_psnr(x, normals, quant, 59.70), args.reps),
                            chamfer_psnr=device_ms(lambda: metrics.chamfer_psnr(x, quant, 59.70), args.reps))
    cnt = native.estimate_normals(x)[1]
    res["below_3_neighbours"] = int((cnt < 3).sum().item())
    res["values"] = dict(metrics.d2_psnr(x, normals, quant, 59.70), **{"psnr_d1": metrics.chamfer_psnr(x, quant, 59.70)["psnr"]})
    a64, b64 = xyz.astype(np.float64), quant.cpu().numpy()
    t0 = time.perf_counter()
    hn = host_normals(a64, workers=host_threads())
    t1 = time.perf_counter()
    hp = host_d2(a64, hn, b64, 59.70, workers=host_threads())
    t2 = time.perf_counter()
    res["host_kdtree_ms"] = dict(estimate_normals=(t1 - t0) * 1e3, d2_psnr=(t2 - t1) * 1e3, threads=host_threads(),
                                 psnr_d2=float(hp), note="first nearest neighbour only, host normals")
    dn = normals.cpu().numpy()
    res["host_vs_device_normals"] = dict(median_abs_cos=float(np.median(np.abs((dn * hn).sum(1)))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
