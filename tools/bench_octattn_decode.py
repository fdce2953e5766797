#!/usr/bin/env python3
"""OctAttention decoder and the decodable encoder profile, measured (bench.py is not involved).

    python tools/bench_octattn_decode.py [--frames 3] [--decode-levels 12,14] [--out profiles/octattn_decode.json]

For L12 --spher (synthetic frame seed 0, 115 568 nodes) and L14 --cylin: encoder frames/s of the default profile (octattn/1) and of the
decodable one (octattn/1d), the same frame encoded decodable and decoded back (occupancy asserted equal), decode seconds per frame and
microseconds per node split by stage (model step, CDF + D2H, range decoder, expansion; the split adds one device synchronisation per
stage stamp, so `decode_s_per_frame` comes from an unstamped run).  Seeded random weights (scp_amd/weights.py): the model's arithmetic
does not depend on the weights' values.  One JSON line on stdout, also written to --out.
"""
import argparse
import json
import os
import sys
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
    args = ap.parse_args()
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
