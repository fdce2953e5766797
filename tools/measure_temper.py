#!/usr/bin/env python3
"""Cost and effect of the per-level temperature (csrc/temper.hip) on full frames: synth_frame(0) at level 12 --spher and as the level-16
multi-level workload, RANDOM weights.

Per workload the frame's coding-order logits table is built once.  Timed with device events over --reps calls after a warm-up, in
microseconds per call: scp_temper_sweep at nt = 25 (both kernels, the frame's own segments), scp_temper_choose, scp_scale_rows in place
(with the chosen inverse temperatures; the table is restored afterwards), and in the same run as yardsticks scp_rate_segments,
scp_softmax_cdf and the packed forward that fills the table.  Then one synchronous encode with rate=True, with and without
temper="code": ideal, coded-table and coded bits, the side bits, the groups that moved.
Random weights say nothing about a trained model: the bit counts show the mechanism at work, not what it buys on a checkpoint.
Writes one JSON document (--out, by default profiles/temper.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def workload(model, dev, level, mullevel, args):
    from scp_amd import native
    from scp_amd.encoder import EncodePlan, FrameEncoder, _temper_layout
    from scp_amd.synth import synth_frame
    frame = torch.from_numpy(synth_frame(0)).to(dev)
    kw = dict(spher=True, mullevel=mullevel, device=dev)
    enc = FrameEncoder(model, "kitti", level, **kw)
    pre = enc.preprocess(frame)
    plan = EncodePlan(pre["level_sizes"], enc.context_size)
    pre["packed_plans"] = enc.packed_plans(plan)
    table = enc.logits_in_coding_order(pre, plan)
    sym = enc._sym_coded(pre, plan)
    lohi = native.softmax_cdf(table, sym)["lohi"]
    off, group, meta = _temper_layout(plan.level_sizes, enc.context_size)
    seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
    group_d = torch.from_numpy(group).to(dev)
    grid, unit = native.temper_grid()
    n, nt, G = int(table.shape[0]), len(grid), len(meta)
    forward_us = device_us(lambda: enc.logits_in_coding_order(pre, plan), args.reps)
    sweep_us = device_us(lambda: native.temper_sweep(table, sym, seg_off, grid), args.reps)
    sweep1_us = device_us(lambda: native.temper_sweep(table, sym, seg_off, grid[unit:unit + 1]), args.reps)
    sw = native.temper_sweep(table, sym, seg_off, grid)
    choose_us = device_us(lambda: native.temper_choose(sw["seg_bits"], sw["seg_bad"], seg_off, n, group_d, G, grid, unit), args.reps)
    ch = native.temper_choose(sw["seg_bits"], sw["seg_bad"], seg_off, n, group_d, G, grid, unit)
    inv = (1.0 / ch["seg_beta"].double()).float()           # (timing only: every call scales the table, the next one roughly back)
    keep = table.clone()
    scale_us = device_us(lambda: (native.scale_rows(table, seg_off, ch["seg_beta"]), native.scale_rows(table, seg_off, inv)), args.reps)
    scale_us = [u / 2 for u in scale_us]
    table.copy_(keep)
    rate_us = device_us(lambda: native.rate_segments(table, sym, lohi, seg_off), args.reps)
    cdf_us = device_us(lambda: native.softmax_cdf(table, sym), args.reps)
    res = dict(level=level, mullevel=mullevel, rows=n, segments=len(off) - 1, groups=G, nt=nt, table_row_stride=int(table.stride(0)),
               sweep_us=sweep_us, sweep_nt1_us=sweep1_us, choose_us=choose_us, scale_rows_us=scale_us, rate_us=rate_us, cdf_us=cdf_us,
               packed_forward_us=forward_us, sweep_costs_more_than_the_forward=min(sweep_us) > min(forward_us),
               exp_f64_per_call=n * 255 * nt, exp_f64_per_s=n * 255 * nt / (min(sweep_us) * 1e-6),
               sweep_table_gbps=n * 4.0 * 256 / (min(sweep_us) * 1e-6) / 1e9)
    del table, keep, lohi, sw
    bits = {}
    for tag, temper in (("plain", None), ("temper", "code")):
        r = FrameEncoder(model, "kitti", level, rate=True, temper=temper, **kw).encode(frame)
        bits[tag] = dict(ideal_bits=r["rate"]["ideal_bits"], table_bits=r["rate"]["table_bits"], coded_bits=r["bits"], n_points=r["n_points"],
                         bpp=r["bpp"], bad_rows=r["rate"]["bad_rows"])
        if temper:
            t = r["temper"]
            bits[tag].update(side_bits=t["side_bits"], moved=t["moved"], ideal_bits_unit=t["ideal_bits_unit"],
                             ideal_bits_chosen=t["ideal_bits_chosen"], coded_plus_side_bits=r["bits"] + t["side_bits"],
                             index=[g["index"] for g in t["groups"]])
    res["bits"] = bits
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temper.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from cfgs import ehem_cfg
    from scp_amd import native
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    native.lib()
    dev = torch.device("cuda:0")
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval()
    res = dict(frame="synth_frame(0)", weights="fill_weights seed 0", reps=args.reps, device=torch.cuda.get_device_name(0),
               note="RANDOM weights: the bit counts show the mechanism at work and say nothing about a trained model; what the option buys on a "
                    "trained checkpoint used off its training distribution has not been measured",
               workloads=dict(L12_spher=workload(model, dev, 12, False, args), L16_mullevel_spher=workload(model, dev, 16, True, args)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
