#!/usr/bin/env python3
"""The attention -> post-attention hand-over, rows against fragment order (include/scp.h: SCP_LDO_FRAG): the window attention (shift 0 / 256,
planes out), scp_swin_post_attn, and the two back to back, four interleaved rounds each, us per launch.
    python tools/mb_attn_o.py TREE ROWS [ROWS...]      TREE: a checkout with a built library (one without the fragment order times the rows form only)"""
import json, os, sys, torch
tree = os.path.abspath(sys.argv[1]); sys.path.insert(0, tree)
from scp_amd import native
dev = torch.device("cuda:0"); native.lib()
HAS_FRAG = hasattr(native, "FragAct")

def timeit(f, n):
    f(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3

out = {"tree": tree, "frag": HAS_FRAG, "cases": {}}
for M in [int(a) for a in sys.argv[2:]]:
    nw = M // 512; T = nw * 512
    g = torch.Generator().manual_seed(1)
    qkv = (torch.randn((T, 768), generator=g) * 2.0).to(dev)
    table = (torch.randn((1023, 4), generator=g) * 0.5).to(dev)
    lens, left = [], nw
    while left > 0:
        n = min(left, 1 + len(lens) % 5); lens.append(n); left -= n
    rows, base = [], 0
    for n in lens:
        rows += [[base, n * 512]] * n; base += n * 512
    wtab = torch.tensor(rows, dtype=torch.int32, device=dev)
    q = qkv[:, :256]
    kv = native.KvPlanes(qkv[:, 256:512], qkv[:, 512:])
    rn = lambda *sh, s=1.0: (torch.randn(sh, generator=g) * s).to(dev)
    x = rn(T, 256)
    pw = native.PostAttnWeights(rn(256, 256, s=0.05), rn(256, s=0.1), 1 + rn(256, s=0.1), rn(256, s=0.1), rn(1024, 256, s=0.05), rn(1024, s=0.1), rn(256, 1024, s=0.03), rn(256, s=0.1))
    y = torch.empty_like(x)
    modes = [("rows", True)] + ([("frag", "frag")] if HAS_FRAG else [])
    o = {m: native.swin_attention_packed_planes(q, kv, table, wtab, 0, split=s) for m, s in modes}
    if HAS_FRAG:
        a, b = native.swin_post_attn(o["rows"], x, pw), native.swin_post_attn(o["frag"], x, pw)
        print(M, "post-attn identical:", torch.equal(a, b), flush=True)
    res = {}
    # settle the clocks under load first
    for _ in range(30): native.swin_post_attn(o["rows"], x, pw, out=y)
    torch.cuda.synchronize()
    for rep in range(4):
        for m, s in modes:
            res.setdefault(f"attn0_{m}", []).append(timeit(lambda: native.swin_attention_packed_planes(q, kv, table, wtab, 0, split=s), 10))
            res.setdefault(f"attn256_{m}", []).append(timeit(lambda: native.swin_attention_packed_planes(q, kv, table, wtab, 256, split=s), 10))
        for m, s in modes:
            res.setdefault(f"post_{m}", []).append(timeit(lambda: native.swin_post_attn(o[m], x, pw, out=y), 10))
        for m, s in modes:      # the pair back to back, as a block runs them
            def pair():
                oo = native.swin_attention_packed_planes(q, kv, table, wtab, 256, split=s)
                native.swin_post_attn(oo, x, pw, out=y)
            res.setdefault(f"pair_{m}", []).append(timeit(pair, 10))
    out["cases"][str(T)] = {k: [round(v, 1) for v in vs] for k, vs in res.items()}
    for k, vs in res.items(): print(T, k, " ".join(f"{v:.1f}" for v in vs), "us", flush=True)
print("MBAB " + json.dumps(out))
