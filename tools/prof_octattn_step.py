#!/usr/bin/env python3
"""Where the OctAttention decoder's per-node time goes: kernel time against wall time of the step.

    python tools/prof_octattn_step.py encode DIR              # a small decodable frame (L10 --spher, synthetic seed 5, every 12th point) -> DIR/f.bin
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_octattn_step.py decode DIR [--nodes 3000]

`decode` decodes the first --nodes nodes of DIR/f.bin (the range decoder is stopped there) and prints one JSON line: nodes, wall seconds,
wall microseconds per node.  Divided by the same node count, the kernel statistics of the traced run give the GPU time per node and the
launches per node; the difference to the wall time is the host's (Python, ctypes, launch) share.  The traced decode also contains the one
batched forward that fills the front-pad cache (`OctAttnStepper.prefill_pad`).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


class _Stop(Exception):
    pass


def main():
    import torch
    from cfgs import octattn_cfg
    from scp_amd import native
    from scp_amd.decoder import OctAttnFrameDecoder, read_sidecar, write_sidecar
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    mode, d = sys.argv[1], sys.argv[2]
    nodes = int(sys.argv[sys.argv.index("--nodes") + 1]) if "--nodes" in sys.argv else 3000
    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    out = os.path.join(d, "f.bin")
    if mode == "encode":
        os.makedirs(d, exist_ok=True)
        enc = OctAttnFrameEncoder(model, "kitti", 10, spher=True, device=dev, decodable=True)
        res = enc.encode(synth_frame(5)[::12].copy())
        with open(out, "wb") as f:
            f.write(res["bytes"])
        write_sidecar(out, enc, res, "OctAttention")
        print(json.dumps(dict(n_nodes=res["n_nodes"])))
        return
    side = read_sidecar(out)
    with open(out, "rb") as f:
        stream = f.read()
    dec = OctAttnFrameDecoder(model, side["depth"], device=dev)
    orig, count = native.AcDecoder.next, [0]

    def nxt(self, row):
        count[0] += 1
        if count[0] > nodes:
            raise _Stop()
        return orig(self, row)
    native.AcDecoder.next = nxt
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        dec.decode(stream, side["n_nodes"])
    except _Stop:
        pass
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    n = min(nodes, side["n_nodes"])
    print(json.dumps(dict(nodes=n, wall_s=t, wall_us_per_node=1e6 * t / n)))


if __name__ == "__main__":
    main()
