#!/usr/bin/env python3
"""Cost and accuracy of the step sweep of the attribute layers (csrc/lift.h: scp_attr_sweep / scp_color_sweep; DESIGN.md 6, "Step sweep")
on the workloads of measure_attr.py and measure_color.py: synth_frame(0) with synth_reflectance at level 12 --spher and as the level-16
multi-level workload, synth_object(0, n) with synth_colors for n = 4 096 and n = 800 000; RANDOM weights (the layers read the octree's
leaves, not the model).

Timed with device events over --reps calls after a warm-up, in microseconds per call and summed over the shells of the frame, the two
alternating in the same run: the sweep entry at the default grid of 16 steps, and the loop it replaces on the same trees - 16 x (the
forward entry + the inverse entry) of the existing library, the root handed over from a call outside the timed region.  No ratio is fixed
in advance; the loop is the yardstick.  Recorded per step: est_bits of the sweep table next to the bits of the file that encode_attr /
encode_color writes at that step (version 1, the host coder), and the leaf PSNR - over leaf values, not the point-wise PSNR of
--metrics.  The synthetic attributes say nothing about real data; these are recorded values, not thresholds.  Writes one JSON document
(--out, by default profiles/attr_sweep.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def alternate_us(fns, reps):
    """{name: fn} -> {name: [microseconds per call]}: one warm-up each, then reps rounds that time every fn once, in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3)
    return out


def table_against_files(table, encode):
    """Per step of the table: est_bits, the bits of the file written at that step, their difference, the leaf PSNR and the largest error."""
    rows = []
    for r in table["rows"]:
        rep = encode(r["Q"])[1]
        rows.append(dict(Q=r["Q"], est_bits=r["est_bits"], written_bits=rep["bits"], written_minus_est=rep["bits"] - r["est_bits"],
                         table_bits=r["table_bits"], leaf_psnr=r["psnr"], linf=r["linf"]))
    return rows


def model(dev):
    from cfgs import ehem_cfg
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    return fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval()


def measure_attr(level, mullevel, reps, dev):
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame, synth_reflectance
    xyz = synth_frame(0)
    refl = synth_reflectance(xyz, 0)
    enc = FrameEncoder(model(dev), "kitti", level, spher=True, mullevel=mullevel, device=dev)
    enc.encode(xyz)
    x, r = torch.from_numpy(xyz).to(dev), torch.from_numpy(refl).to(dev)
    leaves, depths = enc.attr_leaves(), [int(i.depth) for i in enc.geom.info]
    qs = [q.contiguous() for q in enc.quantize(x)[0]]
    vals = [native.attr_leaf_values(q, r, lv, D, 255)[0] for q, lv, D in zip(qs, leaves, depths)]
    roots = [int(native.attr_forward(lv, a, D, 1)["root"].item()) for lv, a, D in zip(leaves, vals, depths)]
    grid = native.sweep_steps()

    def loop():
        for Q in grid:
            for lv, a, D, root in zip(leaves, vals, depths, roots):
                native.attr_inverse(lv, D, int(Q), root, native.attr_forward(lv, a, D, int(Q))["k"])

    out = dict(level=level, mullevel=mullevel, n_points=int(len(xyz)), leaves=[int(lv.shape[0]) for lv in leaves], depths=depths, steps=grid.tolist())
    out["us"] = alternate_us(dict(sweep=lambda: [native.attr_sweep(lv, a, D, grid) for lv, a, D in zip(leaves, vals, depths)], loop=loop), reps)
    out["loop_over_sweep"] = min(out["us"]["loop"]) / min(out["us"]["sweep"])
    out["rows"] = table_against_files(enc.attr_sweep(x, r), lambda Q: enc.encode_attr(x, r, Q))
    return out


def measure_color(n, reps, dev):
    from scp_amd import cli, color, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_colors, synth_object
    xyz = synth_object(0, n).astype(np.float32)
    rgb = synth_colors(xyz, 0)
    enc = FrameEncoder(model(dev), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev)
    q, _ = cli.obj_ints(xyz, "synth_object", dev)
    enc.encode_ints([q], 0, 0.0, len(xyz))
    c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev))
    lv, D = enc.attr_leaves()[0], int(enc.geom.info[0].depth)
    mean, ycc, _ = native.color_leaf_values(q, c, lv, D)
    roots = native.color_forward(lv, ycc, D, 1)["root"].cpu().tolist()
    grid = native.sweep_steps()

    def loop():
        for Q in grid:
            native.color_inverse(lv, D, int(Q), roots, native.color_forward(lv, ycc, D, int(Q))["k"])

    out = dict(n_points=int(len(xyz)), leaves=int(lv.shape[0]), depth=D, steps=grid.tolist())
    out["us"] = alternate_us(dict(sweep=lambda: native.color_sweep(lv, ycc, mean, D, grid), loop=loop), reps)
    out["loop_over_sweep"] = min(out["us"]["loop"]) / min(out["us"]["sweep"])
    out["rows"] = table_against_files(enc.color_sweep(q, c), lambda Q: enc.encode_color(q, c, Q))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "attr_sweep.json"))
    args = p.parse_args()
    from scp_amd import native
    native.lib()
    dev = torch.device("cuda:0")
    doc = dict(tool="tools/measure_sweep.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               note="random weights; synthetic reflectance and colours say nothing about real data; the PSNR is over leaf values; recorded "
                    "values, not thresholds; loop = 16 x (forward + inverse) of the existing entries on the same trees",
               workloads={"L12-spher": measure_attr(12, False, args.reps, dev), "L16-multi-level": measure_attr(16, True, args.reps, dev),
                          "object-4096": measure_color(4096, args.reps, dev), "object-800000": measure_color(800000, args.reps, dev)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for name, w in doc["workloads"].items():
        print(name, {k: round(min(v), 1) for k, v in w["us"].items()}, "loop / sweep", round(w["loop_over_sweep"], 2),
              "written - est bits", [r["written_minus_est"] for r in w["rows"]])


if __name__ == "__main__":
    main()
