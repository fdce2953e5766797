#!/usr/bin/env python3
"""Cost and effect of the chunked payloads (csrc/ac_chunks.hip; DESIGN.md 6, "Chunked payloads") on the workloads of measure_attr.py and
measure_color.py: synth_frame(0) with synth_reflectance at level 12 --spher and as the level-16 multi-level workload, synth_object(0, n)
with synth_colors for n = 4 096 and n = 800 000; RANDOM weights (the layers read the octree's leaves, not the model), step Q = 4.

Timed with device events over --reps calls after a warm-up, in microseconds per call and summed over the shells: the two new entries on
buffers made beforehand - scp_ac_chunks_encode_lohi on the layer's pairs and scp_ac_chunks_decode_ctx on the chunks it wrote, N = 4096
(`us`), and the same two for N = 256, 1024, 4096 and 16384 (`entry_us_by_chunk`: one lane codes one chunk, so the chunk size sets both the
serial length of a lane's work and the number of lanes).
Timed on the host clock, device waits included, version 1 (the host coder: the code without the option) and version 2 (chunk = 4096)
alternating call by call in the same run: FrameEncoder.encode_attr / encode_color and the layer's decode_shells; beside them the host
coder and the host decoder alone on the same pairs.  Recorded for N = 1024, 4096 and 16384: the size of the version-2 file minus the
version-1 file in bytes (the length tables and a flush per chunk), from the host coder on slices of the pairs, and for N = 4096 that
the device's file has exactly that size.  Recorded values, not thresholds.  Writes one JSON document (--out, by default
profiles/ac_chunks.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from measure_attr import device_us, host_us          # noqa: E402  (the same clocks as the layers' tools)

CHUNK, SIZES, ENTRY_SIZES, Q = 4096, (1024, 4096, 16384), (256, 1024, 4096, 16384), 4


def alternating_us(a, b, reps):
    """host_us of a and b, one call of each in turn."""
    a()
    b()
    out = ([], [])
    for _ in range(reps):
        for fn, dst in ((a, out[0]), (b, out[1])):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dst.append((time.perf_counter() - t) * 1e6)
    return out


def raw_entries(pairs, ctxs, table_ofs, alphabet, dev, CHUNK=4096):
    """The two C entries on buffers made beforehand (per shell): -> (encode closure, decode closure, the symbols a decode returns)."""
    from scp_amd import attr, native
    L = native.lib()
    tabs = torch.from_numpy(attr.tables(alphabet).view(np.int16).copy()).to(dev)
    enc_bufs, dec_bufs = [], []
    for lohi, ctx, table_of in zip(pairs, ctxs, table_ofs):
        n = int(lohi.shape[0])
        C = -(-n // CHUNK)
        nb = L.scp_ac_chunks_workspace_bytes(n, CHUNK)
        enc_bufs.append(dict(lohi=lohi, n=n, nb=nb, ws=torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev), out=torch.empty(nb // 4 + 1, dtype=torch.int32, device=dev),
                             head=torch.empty(C + 1, dtype=torch.int32, device=dev)))
        lengths, data = native.ac_chunks_encode(lohi, CHUNK)
        off = np.zeros(C + 1, np.int64)
        np.cumsum(lengths, out=off[1:])
        dec_bufs.append(dict(n=n, bytes=torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev), off=torch.from_numpy(off).to(dev), ctx=ctx,
                             map=torch.tensor(table_of, dtype=torch.uint8, device=dev), nctx=len(table_of), sym=torch.empty(n, dtype=torch.int16, device=dev)))

    def encode():
        for b in enc_bufs:
            native._check(L.scp_ac_chunks_encode_lohi(b["lohi"].data_ptr(), b["n"], CHUNK, b["head"].data_ptr(), b["out"].data_ptr(), b["nb"],
                                                      b["head"].data_ptr() + 4 * (b["head"].shape[0] - 1), b["ws"].data_ptr(), b["nb"], native._stream()), "encode")

    def decode():
        for b in dec_bufs:
            native._check(L.scp_ac_chunks_decode_ctx(b["bytes"].data_ptr(), b["off"].data_ptr(), b["n"], CHUNK, tabs.data_ptr(), 16, alphabet + 1, b["map"].data_ptr(),
                                                     b["nctx"], b["ctx"].data_ptr(), b["sym"].data_ptr(), native._stream()), "decode")

    return encode, decode


def sizes(host_pairs):
    """Per N: the bytes version 2 adds to version 1 over the shells - 4 for the chunk size, the length tables, the chunks minus the serial
    payload - from the host coder on slices."""
    from scp_amd import native
    serial = sum(len(native.ac_encode_lohi(p)) for p in host_pairs)
    out = {}
    for N in SIZES:
        chunks = sum(-(-len(p) // N) for p in host_pairs)
        coded = sum(len(native.ac_encode_lohi(p[i:i + N])) for p in host_pairs for i in range(0, len(p), N))
        out[str(N)] = dict(chunks=chunks, v2_minus_v1_bytes=4 + 4 * chunks + coded - serial, v1_payload_bytes=serial)
    return out


def layer(mod, shells_v1, leaves, depths, channels, alphabet, pairs, dev):
    """What both layers share once the pairs exist: contexts and maps from the version-1 file, the entries, the host coder and decoder alone."""
    from scp_amd import attr, color, native
    ctxs, table_ofs = [], []
    for s, lv, D in zip(shells_v1, leaves, depths):
        level = torch.from_numpy(attr.level_contexts(native.attr_level_counts(lv, D).cpu().numpy())).to(dev)
        ctxs.append(torch.cat([level + c * D for c in range(channels)]).contiguous())
        if channels == 1:
            table_ofs.append([s["tables"][D - 1 - c] for c in range(D)])
        else:
            by_ctx = dict(zip(color._file_order(D), s["tables"]))
            table_ofs.append([by_ctx[c] for c in range(3 * D)])
    encode, decode = raw_entries(pairs, ctxs, table_ofs, alphabet, dev)
    by_chunk = {N: raw_entries(pairs, ctxs, table_ofs, alphabet, dev, N) for N in ENTRY_SIZES}
    host_pairs = [p.cpu().numpy() for p in pairs]
    host_ctx = [c.cpu().numpy() for c in ctxs]
    rows = [attr.tables(alphabet)[t] for t in table_ofs]
    return encode, decode, by_chunk, host_pairs, lambda: [native.AcDecoder(s["payload"], Lp=alphabet + 1).run_ctx(r, c) for s, r, c in zip(shells_v1, rows, host_ctx)]


def measure_attr_workload(level, mullevel, reps, dev):
    from cfgs import ehem_cfg
    from scp_amd import attr, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame, synth_reflectance
    from scp_amd.weights import fill_weights
    xyz = synth_frame(0)
    refl = synth_reflectance(xyz, 0)
    enc = FrameEncoder(fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval(), "kitti", level, spher=True, mullevel=mullevel, device=dev)
    enc.encode(xyz)
    x, r = torch.from_numpy(xyz).to(dev), torch.from_numpy(refl).to(dev)
    leaves, depths = enc.attr_leaves(), [int(i.depth) for i in enc.geom.info]
    data1, rep1 = enc.encode_attr(x, r, Q)
    data2, rep2 = enc.encode_attr(x, r, Q, chunk=CHUNK)
    shells = [s for s in attr.unpack(data1)[2]]
    assert all(s["U"] >= 2 for s in shells)
    pairs = []
    for lv, D, a, s in zip(leaves, depths, rep1["values"], shells):
        f = native.attr_forward(lv, a, D, Q)
        t = torch.from_numpy(attr.tables()[[s["tables"][D - 1 - c] for c in range(D)]].view(np.int16).copy()).to(dev)
        pairs.append(native.attr_pairs(f["k"], f["ctx"], t))
    encode, decode, by_chunk, host_pairs, host_decode = layer(attr, shells, leaves, depths, 1, attr.ALPHABET, pairs, dev)
    assert [native.ac_encode_lohi(p) for p in host_pairs] == [s["payload"] for s in shells]
    v1 = attr.decode_shells(data1, leaves, depths)
    assert all(torch.equal(a, b) for a, b in zip(v1, attr.decode_shells(data2, leaves, depths)))
    out = dict(level=level, mullevel=mullevel, n_points=int(len(xyz)), leaves=[int(lv.shape[0]) for lv in leaves], symbols=[int(p.shape[0]) for p in pairs],
               v1_file_bytes=len(data1), v2_file_bytes=len(data2), sizes=sizes(host_pairs))
    e1, e2 = alternating_us(lambda: enc.encode_attr(x, r, Q), lambda: enc.encode_attr(x, r, Q, chunk=CHUNK), reps)
    d1, d2 = alternating_us(lambda: attr.decode_shells(data1, leaves, depths), lambda: attr.decode_shells(data2, leaves, depths), reps)
    out["us"] = dict(chunks_encode_entry=device_us(encode, reps), chunks_decode_entry=device_us(decode, reps),
                     host_coder=host_us(lambda: [native.ac_encode_lohi(p) for p in host_pairs], reps), host_decoder=host_us(host_decode, reps),
                     encode_v1=e1, encode_v2=e2, decode_shells_v1=d1, decode_shells_v2=d2)
    out["entry_us_by_chunk"] = {str(N): dict(encode=device_us(e, reps), decode=device_us(d, reps)) for N, (e, d) in by_chunk.items()}
    return out


def measure_color_workload(n, reps, dev):
    from cfgs import ehem_cfg
    from scp_amd import attr, cli, color, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_colors, synth_object
    from scp_amd.weights import fill_weights
    xyz = synth_object(0, n).astype(np.float32)
    rgb = synth_colors(xyz, 0)
    enc = FrameEncoder(fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval(), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev)
    q, _ = cli.obj_ints(xyz, "synth_object", dev)
    enc.encode_ints([q], 0, 0.0, len(xyz))
    c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev))
    leaves, depths = enc.attr_leaves(), [int(enc.geom.info[0].depth)]
    lv, D = leaves[0], depths[0]
    data1, rep1 = enc.encode_color(q, c, Q)
    data2, rep2 = enc.encode_color(q, c, Q, chunk=CHUNK)
    shells = color.unpack(data1)[1]
    by_ctx = dict(zip(color._file_order(D), shells[0]["tables"]))
    f = native.color_forward(lv, native.color_leaf_values(q, c, lv, D)[1], D, Q)
    t = torch.from_numpy(attr.tables(color.ALPHABET)[[by_ctx[k] for k in range(3 * D)]].view(np.int16).copy()).to(dev)
    pairs = [native.color_pairs(f["k"], f["ctx"], t)]
    encode, decode, by_chunk, host_pairs, host_decode = layer(color, shells, leaves, depths, 3, color.ALPHABET, pairs, dev)
    assert native.ac_encode_lohi(host_pairs[0]) == shells[0]["payload"]
    assert torch.equal(color.decode_shells(data1, leaves, depths)[0], color.decode_shells(data2, leaves, depths)[0])
    out = dict(n_points=int(len(xyz)), leaves=[int(lv.shape[0])], symbols=[int(pairs[0].shape[0])], v1_file_bytes=len(data1), v2_file_bytes=len(data2),
               sizes=sizes(host_pairs))
    e1, e2 = alternating_us(lambda: enc.encode_color(q, c, Q), lambda: enc.encode_color(q, c, Q, chunk=CHUNK), reps)
    d1, d2 = alternating_us(lambda: color.decode_shells(data1, leaves, depths), lambda: color.decode_shells(data2, leaves, depths), reps)
    out["us"] = dict(chunks_encode_entry=device_us(encode, reps), chunks_decode_entry=device_us(decode, reps),
                     host_coder=host_us(lambda: native.ac_encode_lohi(host_pairs[0]), reps), host_decoder=host_us(host_decode, reps),
                     encode_v1=e1, encode_v2=e2, decode_shells_v1=d1, decode_shells_v2=d2)
    out["entry_us_by_chunk"] = {str(N): dict(encode=device_us(e, reps), decode=device_us(d, reps)) for N, (e, d) in by_chunk.items()}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ac_chunks.json"))
    args = p.parse_args()
    from scp_amd import native
    native.lib()
    dev = torch.device("cuda:0")
    doc = dict(tool="tools/measure_chunks.py", device=torch.cuda.get_device_name(0), reps=args.reps, chunk=CHUNK, Q=Q,
               note="random weights; synthetic reflectance and colours; version 1 and version 2 alternate call by call in the same run; "
                    "encode_* / decode_shells_* / host_* on the host clock with device waits, *_entry by device events; recorded values, not thresholds",
               workloads={"L12-spher": measure_attr_workload(12, False, args.reps, dev), "L16-multi-level": measure_attr_workload(16, True, args.reps, dev),
                          "object-4096": measure_color_workload(4096, args.reps, dev), "object-800000": measure_color_workload(800000, args.reps, dev)})
    for w in doc["workloads"].values():
        assert w["v2_file_bytes"] - w["v1_file_bytes"] == w["sizes"][str(CHUNK)]["v2_minus_v1_bytes"]      # the device wrote the host coder's sizes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for name, w in doc["workloads"].items():
        print(name, w["symbols"], {k: (round(min(v), 1), round(max(v), 1)) for k, v in w["us"].items()}, {n: s["v2_minus_v1_bytes"] for n, s in w["sizes"].items()},
              {n: (round(min(v["encode"]), 1), round(min(v["decode"]), 1)) for n, v in w["entry_us_by_chunk"].items()})


if __name__ == "__main__":
    main()
