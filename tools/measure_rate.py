#!/usr/bin/env python3
"""Cost of the rate report (csrc/rate.hip) on full frames: synth_frame(0) at level 12 --spher and as the level-16 multi-level workload.

Per workload: the frame's coding-order logits table is built once; scp_rate_segments (both kernels, the frame's own segment list) and,
for scale, scp_softmax_cdf on the same table are timed with device events over --reps calls after a warm-up - microseconds per call and
the GB/s that is of the bytes each must move (table once + 5 resp. 4 bytes per row).  Then the pipelined encoder (encode_async, three
frames in flight) with and without rate=True: milliseconds per frame over --steps frames after --warmup.
Writes one JSON document (--out, by default profiles/rate_report.json).  A measurement tool, not a product path.
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


def frame_ms(enc, frames, steps, warmup, depth=3):
    """Wall milliseconds per frame of the pipelined encoder, `depth` frames in flight."""
    pending, t0 = [], None
    for k in range(warmup + steps):
        if k == warmup:
            while pending:
                enc.finish(pending.pop(0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        pending.append(enc.encode_async(frames[k % len(frames)]))
        if len(pending) > depth:
            enc.finish(pending.pop(0))
    while pending:
        last = enc.finish(pending.pop(0))
    return (time.perf_counter() - t0) * 1e3 / steps, last


def workload(model, dev, level, mullevel, args):
    from scp_amd import native
    from scp_amd.encoder import EncodePlan, FrameEncoder, _rate_layout
    from scp_amd.synth import synth_frame
    frames = [torch.from_numpy(synth_frame(s)).to(dev) for s in range(4)]
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev)
    pre = enc.preprocess(frames[0])
    plan = EncodePlan(pre["level_sizes"], enc.context_size)
    table = enc.logits_in_coding_order(pre, plan)
    sym = enc._sym_coded(pre, plan)
    lohi = native.softmax_cdf(table, sym)["lohi"]
    off, _ = _rate_layout(plan.level_sizes, enc.context_size)
    seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
    n = int(table.shape[0])
    dense = table.contiguous()                      # row stride 255: the scalar-load path
    rate_us = device_us(lambda: native.rate_segments(table, sym, lohi, seg_off), args.reps)
    rate255_us = device_us(lambda: native.rate_segments(dense, sym, lohi, seg_off), args.reps)
    cdf_us = device_us(lambda: native.softmax_cdf(table, sym), args.reps)
    with native.launch_profile() as p:
        native.rate_segments(table, sym, lohi, seg_off)
        native.softmax_cdf(table, sym)
        brackets = {tag: ms * 1e3 for tag, ms, _ in p.records()}
    rate_bytes, cdf_bytes = n * (4.0 * 255 + 5), n * (4.0 * 255 + 4)
    res = dict(level=level, mullevel=mullevel, rows=n, segments=len(off) - 1, table_row_stride=int(table.stride(0)),
               rate_us=rate_us, rate_us_stride255=rate255_us, cdf_us=cdf_us, launch_bracket_us=brackets,
               rate_gbps=rate_bytes / (min(rate_us) * 1e-6) / 1e9, cdf_gbps=cdf_bytes / (min(cdf_us) * 1e-6) / 1e9,
               exp_f64_per_call=n * 255, exp_f64_per_s=n * 255 / (min(rate_us) * 1e-6))
    del table, dense, lohi
    off_ms, plain = frame_ms(enc, frames, args.steps, args.warmup)
    enc_r = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev, rate=True)
    on_ms, rated = frame_ms(enc_r, frames, args.steps, args.warmup)
    off2_ms, _ = frame_ms(enc, frames, args.steps, args.warmup)
    assert plain["bytes"] == rated["bytes"]
    r = rated["rate"]
    res.update(frame_ms_rate_off=[off_ms, off2_ms], frame_ms_rate_on=on_ms,
               report=dict(bpp=rated["bpp"], bpp_table=r["bpp_table"], bpp_ideal=r["bpp_ideal"], bits_per_node_ideal=r["bits_per_node_ideal"],
                           coder_overhead_bits=r["coder_overhead_bits"], bad_rows=r["bad_rows"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_report.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from cfgs import ehem_cfg
    from scp_amd import native
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    native.lib()
    dev = torch.device("cuda:0")
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval()
    res = dict(frame="synth_frame(0..3)", weights="fill_weights seed 0", reps=args.reps, steps=args.steps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0),
               workloads=dict(L12_spher=workload(model, dev, 12, False, args), L16_mullevel_spher=workload(model, dev, 16, True, args)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
