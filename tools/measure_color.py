#!/usr/bin/env python3
"""Cost and effect of the colour layer (csrc/color.hip, scp_amd/color.py) on object clouds: synth_object(0, n) with synth_colors for n =
4 096 and n = 800 000 (distinct integer points on a bumpy sphere inside a 2^10 cube, so every leaf holds one point), RANDOM weights (the
layer reads the octree's leaves, not the model).

Timed with device events over --reps calls after a warm-up, in microseconds per call: the four entries scp_color_leaf_values,
scp_color_forward, scp_color_pairs and scp_color_inverse (Q = 4), and - the yardstick - one scp_attr_forward on the Y plane of the same
tree; forward_over_attr_forward is the ratio of the two minima (three planes through shared launches against one plane).  Timed on the
host clock, device waits included: the range coder over the pairs (native.ac_encode_lohi), color.decode_shells of the finished file and
FrameEncoder.encode_color.  Recorded per step Q = 1, 4, 16: the size of the colour file in bits, bits per input point and per leaf, the
chosen tables, and the luma / RGB PSNR of the cloud a decoder writes (color.color_psnr).  The synthetic colours say nothing about the
rate on 8i / MVUB data, and nothing here was measured on a trained checkpoint; these are recorded values, not thresholds.  Writes one JSON
document (--out, by default profiles/color.json).  A measurement tool, not a product path.
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

from measure_attr import device_us, host_us          # noqa: E402  (the same clocks as the reflectance layer's tool)

STEPS = (1, 4, 16)


def measure(n, reps, dev):
    from cfgs import ehem_cfg
    from scp_amd import attr, cli, color, metrics, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_colors, synth_object
    from scp_amd.weights import fill_weights
    xyz = synth_object(0, n).astype(np.float32)
    rgb = synth_colors(xyz, 0)
    enc = FrameEncoder(fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval(), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev)
    q, off = cli.obj_ints(xyz, "synth_object", dev)
    res = enc.encode_ints([q], 0, 0.0, len(xyz))
    x = torch.from_numpy(xyz).to(dev)
    c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev))
    lv, D = enc.attr_leaves()[0], int(enc.geom.info[0].depth)
    pts = metrics.dequantize(lv.long(), [1.0, 1.0, 1.0], off, spher=False, cylin=False)
    out = dict(n_points=int(len(xyz)), leaves=int(lv.shape[0]), depth=D, geometry_bits=int(res["bits"]))
    mean, ycc, cnt = native.color_leaf_values(q, c, lv, D)
    fwd = native.color_forward(lv, ycc, D, 4)
    tabs = torch.from_numpy(attr.tables(color.ALPHABET)[attr.choose_tables(fwd["hist"].cpu().numpy(), color.ALPHABET)[0]].view("int16").copy()).to(dev)
    pairs = native.color_pairs(fwd["k"], fwd["ctx"], tabs)
    host_pairs = pairs.cpu().numpy()
    roots = fwd["root"].cpu().tolist()
    y8 = ycc[0].to(torch.uint8).contiguous()
    data4 = color.encode_shells([lv], [D], [q], c, 4)[0]
    out["us"] = dict(
        leaf_values=device_us(lambda: native.color_leaf_values(q, c, lv, D), reps),
        forward=device_us(lambda: native.color_forward(lv, ycc, D, 4), reps),
        attr_forward_y=device_us(lambda: native.attr_forward(lv, y8, D, 4), reps),
        pairs=device_us(lambda: native.color_pairs(fwd["k"], fwd["ctx"], tabs), reps),
        inverse=device_us(lambda: native.color_inverse(lv, D, 4, roots, fwd["k"]), reps),
        host_coder=host_us(lambda: native.ac_encode_lohi(host_pairs), reps),
        decode_shells=host_us(lambda: color.decode_shells(data4, [lv], [D]), reps),
        encode_color=host_us(lambda: enc.encode_color(q, c, 4), reps))
    out["forward_over_attr_forward"] = min(out["us"]["forward"]) / min(out["us"]["attr_forward_y"])
    out["steps"] = {}
    for Q in STEPS:
        data, rep = enc.encode_color(q, c, Q)
        values = color.decode_shells(data, [lv], [D])
        assert torch.equal(values[0], rep["decoded"][0])
        psnr = color.color_psnr(x, c, pts, values[0])
        out["steps"][str(Q)] = dict(bits=rep["bits"], bits_per_point=rep["bits_per_point"], bits_per_leaf=rep["bits_per_leaf"],
                                    tables=rep["shells"][0]["tables"], level_bits=rep["shells"][0]["level_bits"],
                                    psnr_y=psnr["psnr_y"], psnr_rgb=psnr["psnr_rgb"], lossless_on_leaves=bool(torch.equal(values[0], rep["values"][0])))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "color.json"))
    args = p.parse_args()
    from scp_amd import native
    native.lib()
    dev = torch.device("cuda:0")
    doc = dict(tool="tools/measure_color.py", device=torch.cuda.get_device_name(0), reps=args.reps, cloud="synth_object(0, n) + synth_colors(., 0)",
               note="random weights; synthetic colours say nothing about 8i / MVUB rates; no trained checkpoint; recorded values, not thresholds",
               workloads={"object-4096": measure(4096, args.reps, dev), "object-800000": measure(800000, args.reps, dev)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for name, w in doc["workloads"].items():
        print(name, w["n_points"], {k: round(min(v), 1) for k, v in w["us"].items()}, round(w["forward_over_attr_forward"], 3),
              {q: (s["bits_per_point"], s["psnr_y"], s["psnr_rgb"]) for q, s in w["steps"].items()})


if __name__ == "__main__":
    main()
