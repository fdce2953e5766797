#!/usr/bin/env python3
"""Cost of the distortion report (csrc/distreport.hip) on a full frame: the 120 000-point synth_frame(0) at level 12 --spher and as the
level-16 multi-level workload.

Per workload the frame is quantised once (FrameEncoder.preprocess) and its reconstructed cloud built; metrics.distortion_report (both
directions: minimum, neighbour index, error split, the stable sort and the per-bin reduction, the records' copy to the host) and, as the
yardstick, metrics.chamfer_psnr on the same pair are timed with device events over --reps calls after a warm-up.  The split between the
report's kernels comes from timing native.nn_error_split and native.dist_segments of the first direction alone.
Writes one JSON document (--out, by default profiles/distortion_report.json).  A measurement tool, not a product path; the cost is
recorded, it is not a target.
"""
import argparse
import json
import os
import sys

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


def workload(model, dev, level, mullevel, reps):
    from scp_amd import metrics, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    x = torch.from_numpy(synth_frame(0)).to(dev)
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev)
    enc.preprocess(x)
    pts = enc._reconstructed()
    quant = torch.cat(pts)
    group = torch.cat([torch.full((p.shape[0],), g, dtype=torch.int32, device=dev) for g, p in enumerate(pts)])
    edges = metrics.default_edges("kitti")
    a = x.double().contiguous()
    res = dict(level=level, mullevel=mullevel, points=int(x.shape[0]), leaves=[int(p.shape[0]) for p in pts], rings=len(edges))
    split = native.nn_error_split(a, quant, edges)
    res["device_ms"] = dict(
        distortion_report=device_ms(lambda: metrics.distortion_report(x, quant, edges, quant_group=group, n_groups=len(pts)), reps),
        chamfer_psnr=device_ms(lambda: metrics.chamfer_psnr(x, quant, 59.70), reps),
        nn_error_split_a_to_b=device_ms(lambda: native.nn_error_split(a, quant, edges), reps),
        nn_sqdist_a_to_b=device_ms(lambda: native.nn_sqdist(a, quant), reps),
        dist_segments_a_to_b=device_ms(lambda: native.dist_segments(split["d2"], split["comp"], split["flag"], split["bin"], len(edges)), reps))
    rep = enc.distortion_report(x)
    t = rep["a_to_b"]["total"]
    res["values"] = dict(mse_ab=t["mse"], share_r=t["mse_r"] / t["mse"], share_phi=t["mse_phi"] / t["mse"], share_theta=t["mse_theta"] / t["mse"],
                         bias_r=t["bias_r"], max=t["max"], mse_ba=rep["b_to_a"]["total"]["mse"],
                         ring_mse_ab=[e["mse"] for e in rep["a_to_b"]["rings"]], ring_rows_ab=[e["rows"] for e in rep["a_to_b"]["rings"]],
                         shell_mse_ba=[metrics.dist_total(g)["mse"] for g in rep["b_to_a"]["groups"]])
    d1 = metrics.chamfer_psnr(x, quant, 59.70, dropdups=False)
    res["values"]["chamfer_psnr_mse_ab"] = d1["mse_ab"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_report.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from cfgs import ehem_cfg
    from scp_amd import native
    from scp_amd.models import EHEM
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    native.lib()
    dev = torch.device("cuda:0")
    model = EHEM(ehem_cfg()).to(dev)
    res = dict(frame="synth_frame(0)", reps=args.reps, device=torch.cuda.get_device_name(0),
               workloads=dict(L12_spher=workload(model, dev, 12, False, args.reps), L16_multi_level=workload(model, dev, 16, True, args.reps)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
