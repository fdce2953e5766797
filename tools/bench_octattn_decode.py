#!/usr/bin/env python3
"""OctAttention decoder and the decodable encoder profile, measured (bench.py is not involved).

    python tools/bench_octattn_decode.py [--frames 3] [--decode-levels 12,14] [--out profiles/octattn_decode.json]

For L12 --spher (synthetic frame seed 0, 115 568 nodes) and L14 --cylin: encoder frames/s of the default profile (octattn/1) and of the
decodable one (octattn/1d), the same frame encoded decodable and decoded back (occupancy asserted equal), decode seconds per frame and
microseconds per node split by stage (model step, CDF + D2H, range decoder, expansion; the split adds one device synchronisation per
stage stamp, so `decode_s_per_frame` comes from an unstamped run).  Seeded random weights (scp_amd/weights.py): the model's arithmetic
does not depend on the weights' values.  One JSON line on stdout, also written to --out.

    python tools/bench_octattn_decode.py --streams 1,4,16 [--nodes 3000] [--repeats 3] [--out profiles/octattn_decode_batch.json]

The lockstep decoder (decoder.decode_octattn_files) against the one-stream decoder (decoder.decode_octattn_file) on the same files in
the same process: for each S, S different seeded L12 --spher frames, decimated until a frame has about --nodes nodes (a whole frame
is 115 k nodes = minutes of steps whatever S is; the record says by how much), encoded decodable into --work.  Alternating and
--repeats times each: all S files in lockstep on S slots, then the same files one after the other through the one-stream decoder;
decoded codes asserted equal.  Per S: wall seconds of both (every repeat), nodes per second over all streams, microseconds per
lockstep step, and the stage split of one further stamped lockstep run.

    python tools/bench_octattn_decode.py --streams 16 --trace-steps 300 [--trace-single]

A short run for a kernel trace (run it under the profiler, after a --streams run has left the files in --work): only the first
--trace-steps lockstep steps of the S files (or, --trace-single, that many nodes of the first file through the one-stream decoder).
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


def encode_rate(enc, xyz, frames):
    import torch
    enc.encode(xyz)                       # warm-up (weight planes, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        res = enc.encode(xyz)
    torch.cuda.synchronize()
    return frames / (time.perf_counter() - t0), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--decode-levels", type=str, default="12", help="comma list of the configurations (12 = L12 --spher, 14 = L14 --cylin) to decode")
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--streams", type=str, default="", help="comma list of stream counts: measure the lockstep decoder instead")
    ap.add_argument("--nodes", type=int, default=3000, help="--streams: decimate each frame until it has about this many nodes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--work", type=str, default=os.path.join(tempfile.gettempdir(), "scp_octattn_decode_batch"), help="--streams: where the encoded streams are kept")
    ap.add_argument("--trace-steps", type=int, default=0, help="--streams S: run only this many lockstep steps (for a kernel trace)")
    ap.add_argument("--trace-single", action="store_true", help="with --trace-steps: the one-stream decoder on the first file instead")
    args = ap.parse_args()
    if args.streams:
        return lockstep_main(args)
    import numpy as np
    import torch
    from cfgs import octattn_cfg
    from scp_amd import native
    from scp_amd.decoder import OctAttnFrameDecoder
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights

    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    xyz = synth_frame(0)
    dec_levels = [int(x) for x in args.decode_levels.split(",") if x]
    line = dict(tool="bench_octattn_decode", points=int(len(xyz)), profile_default=native.numeric_profile("OctAttention"),
                profile_decodable=native.numeric_profile("OctAttention", decodable=True), configs={})
    for level, spher, cylin, name in ((12, True, False, "L12_spher"), (14, False, True, "L14_cylin")):
        row = {}
        e0 = OctAttnFrameEncoder(model, "kitti", level, spher=spher, cylin=cylin, device=dev)
        e1 = OctAttnFrameEncoder(model, "kitti", level, spher=spher, cylin=cylin, device=dev, decodable=True)
        row["encode_fps_default"], _ = encode_rate(e0, xyz, args.frames)
        row["encode_fps_decodable"], res = encode_rate(e1, xyz, args.frames)
        row["decodable_over_default"] = row["encode_fps_decodable"] / row["encode_fps_default"]
        row["n_nodes"] = int(res["n_nodes"])
        row["bits_decodable"] = int(res["bits"])
        if level in dec_levels:
            sym = res["_debug"]["sym_coded"].cpu().numpy().astype(np.int64)
            d = OctAttnFrameDecoder(model, res["depth"], device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            codes, _ = d.decode(res["bytes"], res["n_nodes"])
            torch.cuda.synchronize()
            row["decode_s_per_frame"] = time.perf_counter() - t0
            assert np.array_equal(codes.cpu().numpy().astype(np.int64) - 1, sym), "decoded occupancy differs from the encoder's"
            row["decode_us_per_node"] = 1e6 * row["decode_s_per_frame"] / row["n_nodes"]
            # stage split on the first 4096 nodes of a second decode (stamped: a synchronisation per stage)
            d.stats = {}
            n_split = min(4096, row["n_nodes"])
            try:
                d.decode(res["bytes"][:], row["n_nodes"]) if n_split == row["n_nodes"] else _split(d, res, n_split)
            except _Stop:
                pass
            row["stage_us_per_node"] = {k: 1e6 * v / n_split for k, v in d.stats.items()}
            row["stage_split_nodes"] = n_split
        line["configs"][name] = row
        print(name, json.dumps(row), file=sys.stderr)
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


class _Stop(Exception):
    pass


def _stop_after(n_calls):
    """Context: the range decoders stop (by raising _Stop out of `next`) after n_calls symbols."""
    import contextlib
    from scp_amd import native

    @contextlib.contextmanager
    def cm():
        orig, count = native.AcDecoder.next, [0]

        def nxt(self, row):
            count[0] += 1
            if count[0] > n_calls:
                raise _Stop()
            return orig(self, row)
        native.AcDecoder.next = nxt
        try:
            yield
        except _Stop:
            pass
        finally:
            native.AcDecoder.next = orig
    return cm()


def _frames(model, dev, n, target, work):
    """n decimated L12 --spher frames (synthetic seeds 0 .. n - 1) encoded decodable into `work` (kept: a later run reuses them) ->
    [(stream file, nodes, decimation stride)]."""
    import torch
    from scp_amd.decoder import SIDECAR, write_sidecar
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.synth import synth_frame
    os.makedirs(work, exist_ok=True)
    index = os.path.join(work, f"index_{target}.json")
    have = json.load(open(index)) if os.path.exists(index) else []
    have = [h for h in have if os.path.exists(h[0]) and os.path.exists(h[0] + SIDECAR)]
    enc = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev, decodable=True)
    for seed in range(len(have), n):
        xyz, stride = synth_frame(seed), 16
        while True:
            res = enc.encode(xyz[seed % stride::stride].copy())
            if res["n_nodes"] <= 1.25 * target or stride >= 4096:
                break
            stride = int(stride * max(1.3, res["n_nodes"] / target))
        out = enc.outfile(os.path.join(work, f"t{target}_f{seed:02d}"), res)
        with open(out, "wb") as f:
            f.write(res["bytes"])
        write_sidecar(out, enc, res, "OctAttention")
        have.append([out, int(res["n_nodes"]), stride])
        with open(index, "w") as f:
            json.dump(have, f)
    torch.cuda.synchronize()
    return [tuple(h) for h in have[:n]]


def _jobs(files):
    from scp_amd.decoder import read_sidecar
    jobs = []
    for b, _, _ in files:
        side = read_sidecar(b)
        jobs.append(dict(name=b, stream=open(b, "rb").read(), n_nodes=side["n_nodes"], depth=side["depth"], level_wise=side["level_wise"]))
    return jobs


def lockstep_main(args):
    import torch
    from cfgs import octattn_cfg
    from scp_amd import native
    from scp_amd.decoder import OctAttnBatchDecoder, decode_octattn_file, decode_octattn_files
    from scp_amd.models import OctAttention
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    counts = [int(x) for x in args.streams.split(",") if x]
    files = _frames(model, dev, max(counts), args.nodes, args.work)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if args.trace_steps:
        S = counts[0]
        names = [f[0] for f in files[:S]]
        with _stop_after(args.trace_steps * (1 if args.trace_single else S)):
            if args.trace_single:
                decode_octattn_file(names[0], model, dev)
            else:
                decode_octattn_files(names, model, streams=S, device=dev)
        torch.cuda.synchronize()
        print(json.dumps(dict(tool="bench_octattn_decode", trace="single" if args.trace_single else "lockstep", streams=1 if args.trace_single else S,
                              steps=args.trace_steps)))
        return
    line = dict(tool="bench_octattn_decode", mode="lockstep", profile=native.numeric_profile("OctAttention", decodable=True),
                frames="synthetic seeds 0.., L12 --spher, every stride-th point", target_nodes=args.nodes, repeats=args.repeats, streams={})
    decode_octattn_files([files[0][0]], model, streams=1, device=dev)          # warm-up of both paths (weight planes, pad cache, allocator)
    decode_octattn_file(files[0][0], model, dev)
    for S in counts:
        sub = files[:S]
        names, nodes = [f[0] for f in sub], sum(f[1] for f in sub)
        row = dict(files=S, nodes=nodes, nodes_per_file=[f[1] for f in sub], decimation_stride=[f[2] for f in sub], lockstep_s=[], one_stream_s=[])
        for _ in range(args.repeats):
            t, got = wall(lambda: decode_octattn_files(names, model, streams=S, device=dev))
            row["lockstep_s"].append(t)
            t, ref = wall(lambda: [decode_octattn_file(b, model, dev) for b in names])
            row["one_stream_s"].append(t)
            assert all(torch.equal(a["codes"][0], b["codes"][0]) and torch.equal(a["points"], b["points"]) for a, b in zip(got, ref)), \
                "the lockstep decoder's output differs from the one-stream decoder's"
        d = OctAttnBatchDecoder(model, S, device=dev)
        d.stats = {}
        d.decode(_jobs(sub))
        steps = d.steps
        ls = sorted(row["lockstep_s"])
        so = sorted(row["one_stream_s"])
        row.update(steps=steps, lockstep_us_per_step=1e6 * ls[len(ls) // 2] / steps, lockstep_nodes_per_s=nodes / ls[len(ls) // 2],
                   one_stream_nodes_per_s=nodes / so[len(so) // 2], one_stream_us_per_node=1e6 * so[len(so) // 2] / nodes,
                   speedup_median=so[len(so) // 2] / ls[len(ls) // 2], lockstep_spread_s=ls[-1] - ls[0], one_stream_spread_s=so[-1] - so[0],
                   stage_us_per_step={k: 1e6 * v / steps for k, v in d.stats.items()})
        line["streams"][str(S)] = row
        print(S, json.dumps(row), file=sys.stderr, flush=True)
    out = json.dumps(line)
    print(out)
    with open(args.out or os.path.join(ROOT, "profiles", "octattn_decode_batch.json"), "w") as f:
        f.write(out + "\n")


def _split(d, res, n_split):
    """Decode with stage stamps until n_split nodes are done (the range decoder is stopped by raising out of its `next`)."""
    from scp_amd import native
    orig = native.AcDecoder.next
    count = [0]

    def nxt(self, row):
        count[0] += 1
        if count[0] > n_split:
            raise _Stop()
        return orig(self, row)
    native.AcDecoder.next = nxt
    try:
        d.decode(res["bytes"], res["n_nodes"])
    finally:
        native.AcDecoder.next = orig


if __name__ == "__main__":
    main()
