#!/usr/bin/env python3
"""Cost and effect of the reflectance layer (csrc/attr.hip, scp_amd/attr.py) on full frames: synth_frame(0) with synth_reflectance at
level 12 --spher and as the level-16 multi-level workload, RANDOM weights (the layer reads the octree's leaves, not the model).

Timed with device events over --reps calls after a warm-up, in microseconds per call and summed over the shells of the frame: the four
entries scp_attr_leaf_values, scp_attr_forward, scp_attr_pairs and scp_attr_inverse (Q = 4).  Timed on the host clock, device waits
included: the range coder over the pairs (native.ac_encode_lohi) and attr.decode_shells of the finished file.  Recorded per step Q = 1,
4, 16: the size of the attribute file in bits, bits per input point and per leaf, the chosen tables, and the reflectance PSNR of the
cloud a decoder writes (attr.reflectance_psnr).  The synthetic reflectance says nothing about real KITTI rates; these are recorded
values, not thresholds.  Writes one JSON document (--out, by default profiles/attr.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (1, 4, 16)


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


def host_us(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
    return out


def measure(level, mullevel, reps, dev):
    from cfgs import ehem_cfg
    from scp_amd import attr, native
    from scp_amd.decoder import dequantise_leaves, shell_qs
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame, synth_reflectance
    from scp_amd.weights import fill_weights
    xyz = synth_frame(0)
    refl = synth_reflectance(xyz, 0)
    enc = FrameEncoder(fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval(), "kitti", level, spher=True, mullevel=mullevel, device=dev)
    res = enc.encode(xyz)
    x, r = torch.from_numpy(xyz).to(dev), torch.from_numpy(refl).to(dev)
    leaves = enc.attr_leaves()
    depths = [int(i.depth) for i in enc.geom.info]
    qs = [q.contiguous() for q in enc.quantize(x)[0]]
    pts = torch.cat([dequantise_leaves(lv.long(), q, b, float(res["z_offset"]), enc.spher, enc.cylin, enc.data_type)
                     for lv, q, b in zip(leaves, shell_qs("kitti", level, mullevel), res["bin_nums"])])
    out = dict(level=level, mullevel=mullevel, n_points=int(len(xyz)), leaves=[int(lv.shape[0]) for lv in leaves], depths=depths,
               geometry_bits=int(res["bits"]))
    vals = [native.attr_leaf_values(q, r, lv, D, 255)[0] for q, lv, D in zip(qs, leaves, depths)]
    fwd = [native.attr_forward(lv, a, D, 4) for lv, a, D in zip(leaves, vals, depths)]
    tabs = [torch.from_numpy(attr.tables()[attr.choose_tables(f["hist"].cpu().numpy())[0]].view("int16").copy()).to(dev) for f in fwd]
    pairs = [native.attr_pairs(f["k"], f["ctx"], t) for f, t in zip(fwd, tabs)]
    host_pairs = [p.cpu().numpy() for p in pairs]
    data4 = attr.encode_shells(leaves, depths, qs, r, 4, 255)[0]
    out["us"] = dict(
        leaf_values=device_us(lambda: [native.attr_leaf_values(q, r, lv, D, 255) for q, lv, D in zip(qs, leaves, depths)], reps),
        forward=device_us(lambda: [native.attr_forward(lv, a, D, 4) for lv, a, D in zip(leaves, vals, depths)], reps),
        pairs=device_us(lambda: [native.attr_pairs(f["k"], f["ctx"], t) for f, t in zip(fwd, tabs)], reps),
        inverse=device_us(lambda: [native.attr_inverse(lv, D, 4, int(f["root"].item()), f["k"]) for lv, D, f in zip(leaves, depths, fwd)], reps),
        host_coder=host_us(lambda: [native.ac_encode_lohi(p) for p in host_pairs], reps),
        decode_shells=host_us(lambda: attr.decode_shells(data4, leaves, depths), reps),
        encode_attr=host_us(lambda: enc.encode_attr(x, r, 4), reps))
    out["steps"] = {}
    for Q in STEPS:
        data, rep = enc.encode_attr(x, r, Q)
        values = attr.decode_shells(data, leaves, depths)
        assert all(torch.equal(v, d) for v, d in zip(values, rep["decoded"]))
        psnr = attr.reflectance_psnr(x, r, pts, torch.cat(values), 255)
        out["steps"][str(Q)] = dict(bits=rep["bits"], bits_per_point=rep["bits_per_point"], bits_per_leaf=rep["bits_per_leaf"],
                                    tables=[s["tables"] for s in rep["shells"]], level_bits=[s["level_bits"] for s in rep["shells"]],
                                    psnr=psnr["psnr"], mse_ab=psnr["mse_ab"], mse_ba=psnr["mse_ba"],
                                    lossless_on_leaves=all(torch.equal(v, a) for v, a in zip(values, rep["values"])))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "attr.json"))
    args = p.parse_args()
    from scp_amd import native
    native.lib()
    dev = torch.device("cuda:0")
    doc = dict(tool="tools/measure_attr.py", device=torch.cuda.get_device_name(0), reps=args.reps, frame="synth_frame(0) + synth_reflectance(., 0)",
               note="random weights; synthetic reflectance; recorded values, not thresholds",
               workloads={"L12-spher": measure(12, False, args.reps, dev), "L16-multi-level": measure(16, True, args.reps, dev)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for name, w in doc["workloads"].items():
        print(name, {k: round(min(v), 1) for k, v in w["us"].items()}, {q: (s["bits_per_point"], s["psnr"]) for q, s in w["steps"].items()})


if __name__ == "__main__":
    main()
