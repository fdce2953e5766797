#!/usr/bin/env python3
"""Cost of the depth report (csrc/ringrate.hip) and of the decoders' --lod on full frames: synth_frame(0) at level 12 --spher and as the
level-16 multi-level workload.

Per workload the frame is encoded once (synchronously, rate=True, rate_rows=True); then, with device events over --reps calls after a
warm-up - microseconds per call:
    depth_share           scp_rate_depth_share with max_drop = --max_drop: validation, leaves bottom-up, sums top-down, one plane launch
                          for max_drop >= 1 (2 * depth + 2 kernels, one small read-back); next to leaf_share (scp_rate_leaf_share) on the
                          same inputs
    share_segments_depth  the stable sort of the bins (torch) + scp_share_segments_depth_f64 on the max_drop + 1 planes; next to
                          share_segments on plane 0
    depth_report          the whole method - the max_drop + 1 distortion reports and PSNRs, read-backs and host work included (wall clock
                          as well); next to ring_rate
Then the stream is written to a temporary directory as the encode CLIs write it and decoder.decode_file is timed at lod = 0, 1, 2, 4
(wall clock, synchronised, --decode_reps calls after a warm-up), with the points each returns.  Writes one JSON document (--out, by default
profiles/depth_report.json).  A measurement tool, not a product path; the figures are records, not targets.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LODS = (0, 1, 2, 4)


def device_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, r


def workload(model, dev, level, mullevel, args, tmp):
    from scp_amd import native
    from scp_amd.decoder import decode_file, write_sidecar
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    xyz = synth_frame(0)
    x = torch.from_numpy(xyz).to(dev)
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev, rate=True, rate_rows=True)
    res = enc.encode(xyz)
    g = enc.geom
    edges = native.dist_edges([0.0, 5.0, 10.0, 15.0, 20.0, 30.0, 40.0, 60.0, 80.0])
    share_args = enc._share_args()
    K = args.max_drop
    share = native.rate_leaf_share(*share_args)
    planes = native.rate_depth_share(*share_args, K)
    pts = enc._reconstructed()
    group = torch.cat([torch.full((p.shape[0],), k, dtype=torch.int32, device=dev) for k, p in enumerate(pts)])
    bins = native.ring_bins(torch.cat(pts), edges, group, len(pts))
    n_bins = len(pts) * len(edges)
    t = dict(
        leaf_share_us=device_us(lambda: native.rate_leaf_share(*share_args), args.reps),
        depth_share_us=device_us(lambda: native.rate_depth_share(*share_args, K), args.reps),
        share_segments_us=device_us(lambda: native.share_segments(share["cost_ideal"], share["cost_table"], bins, n_bins), args.reps),
        share_segments_depth_us=device_us(lambda: native.share_segments_depth(planes["cost_ideal"], planes["cost_table"], bins, n_bins), args.reps),
        ring_rate_us=device_us(lambda: enc.ring_rate(x, edges), args.reps),
        depth_report_us=device_us(lambda: enc.depth_report(x, K, edges), args.reps))
    wall, rep = wall_ms(lambda: enc.depth_report(x, K, edges), args.reps)
    # the stream as the encode CLIs write it, then the decoder at every LOD
    out = enc.outfile(os.path.join(tmp, f"L{level}"), res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), out + ".dat")
    write_sidecar(out, enc, res, "EHEM")
    decode = []
    for lod in LODS:
        ms, got = wall_ms(lambda: decode_file(out, model, mullevel=mullevel, device=dev, lod=lod), args.decode_reps)
        decode.append(dict(lod=lod, wall_ms=ms, points=int(got["points"].shape[0]), levels_decoded=int(got.get("levels_decoded", res["n_levels"]))))
    depths = [int(i.depth) for i in g.info]
    return dict(level=level, mullevel=mullevel, points=int(x.shape[0]), nodes=int(g.total_nodes), leaves=sum(int(i.n_leaves) for i in g.info),
                segments=len(g.info), shell_depths=depths, max_drop=K, depth_share_kernels=2 * max(depths) + (2 if K >= 1 else 1), depth_report_wall_ms=wall, **t,
                decode=decode,
                report=[dict(drop=lv["drop"], cells=lv["cells"], ideal_bits=lv["rate"]["total"]["ideal_bits"],
                             ideal_bits_per_point=lv["rate"]["total"]["ideal_bits_per_point"], psnr_d1=lv["d1"]["psnr"],
                             mse_ab=lv["d1"]["mse_ab"], mse_ba=lv["d1"]["mse_ba"]) for lv in rep["levels"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_report.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decode_reps", type=int, default=3)
    ap.add_argument("--max_drop", type=int, default=4)
    args = ap.parse_args()
    from cfgs import ehem_cfg
    from scp_amd import native
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    native.lib()
    dev = torch.device("cuda:0")
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval()
    with tempfile.TemporaryDirectory() as tmp:
        res = dict(frame="synth_frame(0)", weights="fill_weights seed 0", reps=args.reps, decode_reps=args.decode_reps,
                   device=torch.cuda.get_device_name(0),
                   workloads=dict(L12_spher=workload(model, dev, 12, False, args, tmp), L16_mullevel_spher=workload(model, dev, 16, True, args, tmp)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
