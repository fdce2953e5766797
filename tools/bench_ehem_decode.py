#!/usr/bin/env python3
"""The lockstep EHEM decoder against the one-stream decoder, measured (bench.py is not involved).

    python tools/bench_ehem_decode.py [--streams 1,2,4,8] [--repeats 3] [--configs L16_spher_mul,L12_spher] [--out profiles/ehem_decode_batch.json]

For each workload - L16 --spher multi-level (the bench workload) and L12 --spher single-level - and each S: S different seeded synthetic
frames (seeds 0 .. S - 1, whole frames) encoded into --work, then, alternating in one process and --repeats times each: all S files in
lockstep on S slots (decoder.decode_files), and the same files one after the other through decoder.decode_file - the yardstick, whose code
the lockstep decoder does not touch; decoded codes asserted equal.  Per S: wall seconds of every repeat of both, aggregate frames/s
(medians), rounds and steps of the lockstep run, and the stage split of one further stamped lockstep run (a device synchronisation per
stamp, so its total is not a wall time).  For S > 1 the lockstep decoder is also timed, in the same alternation, with the range-decoder
calls of a step on a thread pool of min(S, 16) threads (`lockstep_pool_s`, and its stamped split).  Seeded random weights
(scp_amd/weights.py): the model's arithmetic does not depend on the weights' values.  One JSON line on stdout, also written to --out.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {"L16_spher_mul": dict(level=16, mullevel=True), "L12_spher": dict(level=12, mullevel=False)}


def _frames(model, dev, n, name, work):
    """n whole synthetic frames (seeds 0 .. n - 1) of a workload encoded into `work`, with the `.dat` and side-info files the encode CLIs
    write -> [(stream file, nodes)]."""
    import numpy as np
    import torch
    from scp_amd.decoder import write_sidecar
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    cfg = CONFIGS[name]
    os.makedirs(work, exist_ok=True)
    enc = FrameEncoder(model, "kitti", cfg["level"], spher=True, mullevel=cfg["mullevel"], device=dev)
    out = []
    for seed in range(n):
        res = enc.encode(synth_frame(seed))
        path = enc.outfile(os.path.join(work, f"{name}_f{seed:02d}"), res)
        with open(path, "wb") as f:
            f.write(res["bytes"])
        torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), path + ".dat")
        write_sidecar(path, enc, res, "EHEM")
        out.append((path, int(res["n_nodes"])))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=str, default="1,2,4,8")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", type=str, default=",".join(CONFIGS))
    ap.add_argument("--work", type=str, default=os.path.join(tempfile.gettempdir(), "scp_ehem_decode_batch"))
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ehem_decode_batch.json"))
    args = ap.parse_args()
    import torch
    from cfgs import ehem_cfg
    from scp_amd import native
    from scp_amd.decoder import EhemBatchDecoder, _ehem_job, _ehem_result, decode_file, decode_files
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev)
    counts = [int(x) for x in args.streams.split(",") if x]
    if args.repeats < 3 or not counts or not 1 <= min(counts) <= max(counts) <= 64:
        raise SystemExit("--repeats >= 3 and stream counts in 1 .. 64 expected")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    med = lambda v: sorted(v)[len(v) // 2]

    def pooled(names, S, mul):
        jobs = [_ehem_job(b, mullevel=mul) for b in names]
        d = EhemBatchDecoder(model, S, device=dev, coder_threads=min(S, 16))
        return [_ehem_result(j, sh) for j, sh in zip(jobs, d.decode(jobs))]

    same = lambda got, ref: all(len(a["codes"]) == len(b["codes"]) and all(torch.equal(x, y) for x, y in zip(a["codes"], b["codes"]))
                                and torch.equal(a["points"], b["points"]) for a, b in zip(got, ref))
    line = dict(tool="bench_ehem_decode", profile=native.numeric_profile("EHEM"), device=torch.cuda.get_device_name(0),
                frames="synthetic seeds 0.., whole frames, --spher", repeats=args.repeats, configs={})
    for name in [c for c in args.configs.split(",") if c]:
        mul = CONFIGS[name]["mullevel"]
        files = _frames(model, dev, max(counts), name, args.work)
        decode_files([files[0][0]], model, streams=1, mullevel=mul, device=dev)        # warm-up of both paths (weight planes, plans, allocator)
        decode_file(files[0][0], model, mullevel=mul, device=dev)
        rows = {}
        for S in counts:
            sub = files[:S]
            names = [f[0] for f in sub]
            row = dict(files=S, nodes=sum(f[1] for f in sub), lockstep_s=[], one_stream_s=[], lockstep_pool_s=[])
            for _ in range(args.repeats):
                t, got = wall(lambda: decode_files(names, model, streams=S, mullevel=mul, device=dev))
                row["lockstep_s"].append(t)
                t, ref = wall(lambda: [decode_file(b, model, mullevel=mul, device=dev) for b in names])
                row["one_stream_s"].append(t)
                assert same(got, ref), "the lockstep decoder's output differs from the one-stream decoder's"
                if S > 1:
                    t, got = wall(lambda: pooled(names, S, mul))
                    row["lockstep_pool_s"].append(t)
                    assert same(got, ref), "the lockstep decoder's output (coder threads) differs from the one-stream decoder's"
            d = EhemBatchDecoder(model, S, device=dev)
            d.stats = {}
            d.decode([_ehem_job(b, mullevel=mul) for b in names])
            counters = dict(rounds=d.stats.pop("rounds"), steps=d.stats.pop("steps"))
            row.update(counters, lockstep_fps=S / med(row["lockstep_s"]), one_stream_fps=S / med(row["one_stream_s"]),
                       speedup_median=med(row["one_stream_s"]) / med(row["lockstep_s"]),
                       lockstep_spread_s=max(row["lockstep_s"]) - min(row["lockstep_s"]),
                       one_stream_spread_s=max(row["one_stream_s"]) - min(row["one_stream_s"]),
                       stamped_stage_s_per_frame={k: v / S for k, v in d.stats.items()})
            if S > 1:
                d = EhemBatchDecoder(model, S, device=dev, coder_threads=min(S, 16))
                d.stats = {}
                d.decode([_ehem_job(b, mullevel=mul) for b in names])
                row.update(lockstep_pool_fps=S / med(row["lockstep_pool_s"]),
                           stamped_stage_s_per_frame_pool={k: v / S for k, v in d.stats.items() if k not in ("rounds", "steps")})
            rows[str(S)] = row
            print(name, S, json.dumps(row), file=sys.stderr, flush=True)
        line["configs"][name] = rows
    out = json.dumps(line)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
