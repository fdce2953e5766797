#!/usr/bin/env python3
"""Row-chain kernels (csrc/rowchain.hip) against the launches they replace, on one MI355X: correctness against float64 and time.
    python tools/mb_rowchain.py [rows]
The two forms of the LayerNorm + projection kernel (rc_ln_linear_kernel, one workgroup per CU, against ln2_proj_kernel of csrc/lnlin2.hip,
two per CU), plain rows (N = 256) and q|k|v / k|v planes (N = 768 / 512), at the frame's own row counts or the ones given:
    python tools/mb_rowchain.py --ab [--rounds R] [rows ...]
SCP_LNLIN is read once per process, so every measurement is a fresh child process (--forms), old and new interleaved; the table shows the
median over the rounds.  Rows 32768 and 65536 are one tile for each of 256 / 512 workgroups: with two workgroups resident per CU the second
lasts clearly less than twice the first."""
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scp_amd import native  # noqa: E402
from scp_amd.ops import linear_s, _split  # noqa: E402


def timeit(f, n=10):
    f(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n


FRAME_ROWS = (590848, 303616, 159232, 87040, 51200)


def forms(rows):
    """child of --ab: times of this process's form (SCP_LNLIN) as one JSON line"""
    dev = torch.device("cuda:0")
    native.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    gamma = (1 + 0.1 * torch.randn(256, generator=g)).to(dev)
    beta = (0.1 * torch.randn(256, generator=g)).to(dev)
    fw, b = {}, {}
    for N in (768, 512, 256):
        fw[N] = native.LnFoldedWeight((torch.randn((N, 256), generator=g) * 0.05).to(dev), gamma, beta)
        b[N] = (torch.randn(N, generator=g) * 0.1).to(dev)
    res = {}
    for M in rows:
        x = (torch.randn((M, 256), generator=g) * 1.5 + 0.3).to(dev)
        valid = (torch.rand(M, generator=g) > 0.1).float().to(dev)
        out = torch.empty((M, 256), dtype=torch.float32, device=dev)
        for N in (768, 512):
            res[f"{M} {N}"] = timeit(lambda: native.swin_ln_qkv(x, fw[N], b[N], 1e-5, valid), 20)
        res[f"{M} 256"] = timeit(lambda: native.swin_ln_linear(x, fw[256], b[256], 1e-5, valid, out=out), 20)
        del x, valid, out
    print("FORMS " + json.dumps(res), flush=True)


def ab(rows, rounds):
    got = {1: [], 2: []}
    for _ in range(rounds):
        for mode in (1, 2):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"] + [str(m) for m in rows], env=dict(os.environ, SCP_LNLIN=str(mode)),
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child SCP_LNLIN={mode} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            got[mode].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("FORMS ")][-1][6:]))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"{'rows':>8} {'N':>4}  {'old ms':>8} {'new ms':>8}  new/old   (median of {rounds}; min - max old | new)")
    for M in rows:
        for N in (768, 512, 256):
            k = f"{M} {N}"
            o, n = [g[k] for g in got[1]], [g[k] for g in got[2]]
            print(f"{M:8d} {N:4d}  {med(o):8.4f} {med(n):8.4f}  {med(n) / med(o):7.3f}   ({min(o):.4f} - {max(o):.4f} | {min(n):.4f} - {max(n):.4f})", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--forms":
        return forms([int(a) for a in sys.argv[2:]])
    if len(sys.argv) > 1 and sys.argv[1] == "--ab":
        args = sys.argv[2:]
        rounds = 3
        if args and args[0] == "--rounds":
            rounds, args = int(args[1]), args[2:]
        return ab([int(a) for a in args] or list(FRAME_ROWS) + [32768, 65536], rounds)
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 590848
    dev = torch.device("cuda:0")
    native.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    x = (torch.randn((M, 256), generator=g) * 1.5 + 0.3).to(dev)
    gamma = (1 + 0.1 * torch.randn(256, generator=g)).to(dev)
    beta = (0.1 * torch.randn(256, generator=g)).to(dev)
    valid = (torch.rand(M, generator=g) > 0.1).float().to(dev)
    for N in (768, 512, 256):
        W = (torch.randn((N, 256), generator=g) * 0.05).to(dev)
        b = (torch.randn(N, generator=g) * 0.1).to(dev)
        fw = native.LnFoldedWeight(W, gamma, beta)
        out = native.swin_ln_linear(x, fw, b, 1e-5, valid)
        torch.cuda.synchronize()
        # float64 reference on a sample of rows
        idx = torch.cat((torch.arange(0, min(M, 300)), torch.randint(0, M, (2000,), generator=g), torch.arange(max(0, M - 300), M))).to(dev)
        xs = x[idx].double()
        ln = torch.nn.functional.layer_norm(xs, (256,), gamma.double(), beta.double(), 1e-5) * valid[idx].double()[:, None]
        ref = ln @ W.double().T + b.double()
        err = (out[idx].double() - ref).abs().max().item()
        # the launches it replaces
        def old():
            h = native.layernorm_rows(x, gamma, beta, 1e-5, valid=valid[:, None].contiguous(), split=True)
            return linear_s(h, W, b)
        o2 = old()
        err_old = (o2[idx].double() - ref).abs().max().item()
        t_new = timeit(lambda: native.swin_ln_linear(x, fw, b, 1e-5, valid, out=out))
        t_old = timeit(old)
        t_ln = timeit(lambda: native.layernorm_rows(x, gamma, beta, 1e-5, valid=valid[:, None].contiguous(), split=True))
        fl = 2.0 * M * N * 256
        print(f"N={N:4d} M={M}: rowchain {t_new:.3f} ms ({fl / t_new / 1e9:.0f} TF/s alg)  |  LN {t_ln:.3f} + gemm_split {t_old - t_ln:.3f} = {t_old:.3f} ms"
              f"   max err vs f64: new {err:.2e} old {err_old:.2e}", flush=True)
    # ragged M and invalid rows
    for Mr in (1, 31, 129, 1000):
        xr = x[:Mr].contiguous()
        W = (torch.randn((256, 256), generator=g) * 0.05).to(dev)
        fw = native.LnFoldedWeight(W, gamma, beta)
        o = native.swin_ln_linear(xr, fw, None, 1e-5, None)
        ref = torch.nn.functional.layer_norm(xr.double(), (256,), gamma.double(), beta.double(), 1e-5) @ W.double().T
        print(f"M={Mr}: max err {(o.double() - ref).abs().max().item():.2e}")


if __name__ == "__main__":
    main()
