"""The OctAttention decoder's two HIP entry points, each against an independent reference (-m gpu):
- scp_decode_expand_octattn against a numpy construction of the encode_dataset.py:32-55 layout, and against the encoder's own context
  rows (Geom.context_octattn) level by level on real trees - decoder inputs pinned to encoder inputs with no model or coder in the loop;
- scp_octattn_attention_rowinv against a float64 evaluation of attention_model.py:58-95 at the head widths, window lengths, strides
  and score regimes where a flash-style kernel goes wrong, and with NaN in every row a launch promises not to read."""
import numpy as np
import pytest
import torch

from conftest import parity_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ scp_decode_expand_octattn
def _expand_np(sym, ctx, apos, L, depth):
    """One decoded level's children in numpy (encode_dataset.py:32-55): children of parent i in octant order d = 0..7 (x bit 2, y bit 1,
    z bit 0); a child's context row is its parent's slots 1..3 moved up one slot, the parent's own occupancy field set to its symbol s,
    then (255, L + 1, d + 1); its origins are the parent's three ancestor origins and p + (x, y, z) << (depth - L); positions are the
    origins over 2^depth in float64, rounded to float32 once."""
    sym = np.asarray(sym, np.int64)
    occ = np.where(sym < 0, 0, sym + 1)
    par, d = np.nonzero((occ[:, None] >> np.arange(8)) & 1)          # row-major: parent order, then octant order
    cctx = np.empty((len(par), 12), np.uint8)
    cctx[:, :9] = ctx[par, 3:]
    cctx[:, 6] = sym[par]
    cctx[:, 9], cctx[:, 10], cctx[:, 11] = 255, L + 1, d + 1
    capos = np.empty((len(par), 4, 3), np.int64)
    capos[:, :3] = apos[par, 1:]
    capos[:, 3] = apos[par, 3] + (np.stack(((d >> 2) & 1, (d >> 1) & 1, d & 1), 1).astype(np.int64) << (depth - L))
    cpos = (capos.astype(np.float64) / 2.0 ** depth).astype(np.float32)
    return occ.astype(np.uint8), cctx, capos.astype(np.int32), cpos


def _parents(rng, n, L, depth, top=False, col9=255):
    """n parents of level L: symbols over -1 .. 254, random context bytes with 0 .. 3 pad rows (255, 0, 0) at origin 0 in front, the
    parents' own occupancy column = col9 (None: random bytes), origins on each slot's grid (top: the parents' origins in the last two
    cells of their level, so that their last children reach the top of the range)."""
    sym = rng.integers(-1, 255, n)
    ctx = rng.integers(0, 256, (n, 12)).astype(np.uint8)
    ctx[:, 9] = rng.integers(0, 256, n) if col9 is None else col9
    apos = np.empty((n, 4, 3), np.int64)
    for k in range(4):                                # slot k holds a node of level L - 3 + k: origins are multiples of 2^(depth - lvl + 1)
        lvl = max(L - 3 + k, 1)
        cells = 1 << (lvl - 1)
        apos[:, k] = rng.integers(0, cells, (n, 3)) << (depth - lvl + 1)
    if top:
        apos[:, 3] = ((1 << (L - 1)) - 1 - rng.integers(0, 2, (n, 3))) << (depth - L + 1)
    npad = rng.integers(0, 4, n)
    for k in range(3):
        pad = npad > k
        ctx[pad, 3 * k:3 * k + 3] = (255, 0, 0)
        apos[pad, k] = 0
    return sym, ctx, apos.astype(np.int32)


_EXPAND_CASES = [(1, 1, 12, False, 255), (255, 3, 12, False, None), (256, 12, 12, False, 255), (257, 1, 30, False, None),
                 (70001, 9, 17, False, None), (4099, 30, 30, True, 255), (300, 29, 30, True, None), (1000, 4, 12, False, "all -1")]


@pytest.mark.parametrize("n,L,depth,top,col9", _EXPAND_CASES,
                         ids=[f"n{n}_L{L}_depth{d}" + ("_top" if t else "") + ("_no_children" if c == "all -1" else "") for n, L, d, t, c in _EXPAND_CASES])
def test_decode_expand_octattn_vs_numpy(dev, n, L, depth, top, col9):
    from scp_amd import native
    rng = np.random.default_rng(n * 131 + L * 7 + depth)
    sym, ctx, apos = _parents(rng, n, L, depth, top, None if col9 is None else 255)
    if col9 == "all -1":
        sym[:] = -1                                   # m == 0: no children at all
    elif n == 1:
        sym[:] = 254                                  # all eight children
    else:                                             # every symbol -1 .. 254 once (as far as n goes), the rest random
        sym[:min(n, 256)] = np.arange(min(n, 256)) - 1
        rng.shuffle(sym)
    occ8, cctx, capos, cpos = native.decode_expand_octattn(torch.from_numpy(sym).to(dev), torch.from_numpy(ctx).to(dev),
                                                           torch.from_numpy(apos).to(dev), L, depth)
    w_occ, w_ctx, w_apos, w_pos = _expand_np(sym, ctx, apos, L, depth)
    assert np.array_equal(occ8.cpu().numpy(), w_occ)
    assert cctx.shape == (len(w_ctx), 12) and capos.shape == cpos.shape == (len(w_ctx), 4, 3)
    assert np.array_equal(cctx.cpu().numpy(), w_ctx)
    assert np.array_equal(capos.cpu().numpy(), w_apos)
    assert np.array_equal(cpos.cpu().numpy().view(np.int32), w_pos.view(np.int32))
    if top:                                           # the last child of the top cell
        assert w_apos[:, 3].max() == (1 << depth) - (1 << (depth - L))


def test_decode_expand_octattn_refuses_bad_levels(dev):
    """The C entry point itself: shift >= depth, L outside 1 .. 254 and depth above 30 are SCP_EINVAL, and nothing is written."""
    from scp_amd import native
    rng = np.random.default_rng(5)
    sym, ctx, apos = _parents(rng, 40, 3, 12)
    sym_d, ctx_d, apos_d = torch.from_numpy(sym).to(dev), torch.from_numpy(ctx).to(dev), torch.from_numpy(apos).to(dev)
    popc = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=dev)
    cum = torch.cumsum(popc[sym_d + 1], 0)
    m = int(cum[-1])
    outs = [torch.full((m, 12), 77, dtype=torch.uint8, device=dev), torch.full((m, 4, 3), 77, dtype=torch.int32, device=dev),
            torch.full((m, 4, 3), 77.0, device=dev), torch.full((40,), 77, dtype=torch.uint8, device=dev)]

    def rc(L, shift, depth):
        return native.lib().scp_decode_expand_octattn(sym_d.data_ptr(), cum.data_ptr(), ctx_d.data_ptr(), apos_d.data_ptr(), 40, L, shift,
                                                      depth, *[o.data_ptr() for o in outs], native._stream())

    for L, shift, depth in ((3, 12, 12), (3, 13, 12), (0, 12, 12), (255, 9, 12), (3, 28, 31), (3, 9, 31)):
        assert rc(L, shift, depth) == -1, (L, shift, depth)
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in outs)
    assert rc(3, 9, 12) == 0                          # the same buffers are accepted with a valid level
    got = _expand_np(sym, ctx, apos, 3, 12)
    assert np.array_equal(outs[0].cpu().numpy(), got[1]) and np.array_equal(outs[1].cpu().numpy(), got[2])
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):
        native.decode_expand_octattn(sym_d, ctx_d, apos_d, 0, 12)


def _tree(kind, dev):
    """(integer cloud int32 [P, 3] on the device) of the frames the decoder meets: KITTI-like frames under the three coordinate systems,
    encode.py's --type obj integers and a Ford-like millimetre frame."""
    from scp_amd import native
    from scp_amd.cli import obj_ints
    from scp_amd.encoder import level_qs
    from scp_amd.synth import ford_like, synth_frame
    if kind == "obj":
        return obj_ints((synth_frame(5)[::60] * 2).astype(np.float32), "frame", dev)[0]
    mode, level, dt, xyz = {"spher_L12": (native.SPHER, 12, "kitti", synth_frame(0)), "cylin_L14": (native.CYLIN, 14, "kitti", synth_frame(1)),
                            "cart_L10": (native.CART, 10, "kitti", synth_frame(2)),
                            "ford_L17": (native.SPHER, 17, "ford", ford_like(synth_frame(3)))}[kind]
    q, _, _ = native.quantize(torch.from_numpy(xyz).to(dev), mode, level_qs(dt, level), -200.0 if dt == "kitti" else -float(2 ** 17))
    return q


@pytest.mark.parametrize("kind", ["spher_L12", "cylin_L14", "cart_L10", "obj", "ford_L17"])
def test_decoder_contexts_equal_the_encoders_level_by_level(dev, kind):
    """The decoder's expansion fed each level's true symbols, from the decoder's root row: every level's context rows and positions are
    the encoder's (Geom.context_octattn) bit for bit, the own-occupancy column aside (255 until the decoder writes the decoded symbol
    there), and the last expansion's own origins are the tree's leaves."""
    from scp_amd import native
    q = _tree(kind, dev)
    g = native.Geom()
    g.build(q, [(0, q.shape[0], None, False)])
    depth = int(g.info[0].depth)
    ctx_e, pos_e, sym_e = g.context_octattn(0)
    counts = g.level_counts(0)
    leaves = g.leaves(0)
    assert len(counts) == depth and sum(counts) == ctx_e.shape[0]
    ctx = torch.tensor([[255, 0, 0] * 3 + [255, 1, 1]], dtype=torch.uint8, device=dev)      # OctAttnFrameDecoder.decode's root row
    apos = torch.zeros((1, 4, 3), dtype=torch.int32, device=dev)
    pos = torch.zeros((1, 4, 3), dtype=torch.float32, device=dev)
    a = 0
    for L in range(1, depth + 1):
        n = counts[L - 1]
        assert ctx.shape[0] == n, (L, ctx.shape[0], n)
        assert bool((ctx[:, 9] == 255).all()), L
        ctx[:, 9] = sym_e[a:a + n]
        bad = (ctx != ctx_e[a:a + n]).any(1).nonzero().flatten()[:5].tolist()
        assert not bad, (L, bad, ctx[bad].tolist(), ctx_e[a:a + n][bad].tolist())
        assert torch.equal(pos.view(torch.int32), pos_e[a:a + n].view(torch.int32)), L
        syms = sym_e[a:a + n].long()
        occ8, ctx, apos, pos = native.decode_expand_octattn(syms, ctx, apos, L, depth)
        assert torch.equal(occ8, (syms + 1).to(torch.uint8)), L
        a += n
    assert a == ctx_e.shape[0]
    assert torch.equal(apos[:, 3], leaves)
    assert torch.equal(torch.unique(apos[:, 3], dim=0), torch.unique(q, dim=0))
    print(f"{kind}: depth {depth}, {a} nodes, {leaves.shape[0]} leaves")


# ------------------------------------------------------------------------------------------------ scp_octattn_attention_rowinv
def _attn_f64(q, k, v, ku, vu, H):
    """attention_model.py:58-95 in float64 for one window (the evaluation of test_rowinv_attention_query_range_and_batch): q, k, v, k_u,
    v_u [c, D] -> known and unknown stream [c, D], and the largest |score| of either."""
    c, D = q.shape
    hd = D // H
    qd, kd, vd, kud, vud = (t.double().reshape(c, H, hd).transpose(0, 1) for t in (q, k, v, ku, vu))
    s = qd @ kd.transpose(1, 2) / hd ** 0.5
    mask = torch.tril(torch.ones(c, c, dtype=torch.bool, device=q.device))
    ref = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ vd
    su = s.clone()
    su.diagonal(dim1=1, dim2=2).copy_((qd * kud).sum(-1) / hd ** 0.5)
    pu = torch.softmax(su.masked_fill(~mask, float("-inf")), -1)
    refu = (pu * (~torch.eye(c, dtype=torch.bool, device=q.device))) @ vd + pu.diagonal(dim1=1, dim2=2)[..., None] * vud
    smax = max(float(s.masked_fill(~mask, 0).abs().max()), float(su.diagonal(dim1=1, dim2=2).abs().max()))
    return ref.transpose(0, 1).reshape(c, D), refu.transpose(0, 1).reshape(c, D), smax


def _scores(B, c, H, hd, profile, dev, seed):
    """q_u, k, v, k_u, v_u float32 [B, c, D].  'normal': N(0, 1) entries (scores about N(0, 1)).  The sharp profiles put every head's
    query on one unit direction u (scaled by sqrt(hd)) and the keys at f_j u, so that score (t, j) is about f_j, with |f| up to 80:
    'late'      f rises along the window: each row's largest key is its last one, in its last tile, and every tile raises the running
                maximum (the alpha rescale carries the result); the unknown diagonal sits 2 below the known one;
    'diag_high' f uniform in [-40, 40], the unknown diagonal at 80: the last merge (a2 ~ 0, p2 = 1) carries the result;
    'diag_low'  f uniform in [0, 80], the unknown diagonal at -80: far below every key (p2 underflows)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    D = H * hd
    rn = lambda *s: torch.randn(s, generator=g, device=dev, dtype=torch.float64)
    v, vu = rn(B, c, D), rn(B, c, D)
    if profile == "normal":
        return tuple(t.float() for t in (rn(B, c, D), rn(B, c, D), v, rn(B, c, D), vu))
    u = rn(H, hd)
    u = (u / u.norm(dim=1, keepdim=True)).reshape(1, 1, D)
    uni = lambda lo, hi: lo + (hi - lo) * torch.rand((B, c, 1), generator=g, device=dev, dtype=torch.float64)
    if profile == "late":
        f = torch.linspace(-80, 80, c, device=dev, dtype=torch.float64).reshape(1, c, 1).expand(B, c, 1)
        fu = f - 2
    elif profile == "diag_high":
        f, fu = uni(-40, 40), torch.full((B, c, 1), 80.0, device=dev, dtype=torch.float64)
    else:
        f, fu = uni(0, 80), torch.full((B, c, 1), -80.0, device=dev, dtype=torch.float64)
    q = hd ** 0.5 * u + 0.05 * rn(B, c, D)
    k = f * u + 0.05 * rn(B, c, D)
    ku = fu * u + 0.05 * rn(B, c, D)
    return tuple(t.float() for t in (q, k, v, ku, vu))


_SENT = 1.0e30


def _place(B, c, H, hd, ops, strided, dev):
    """The operands as the kernel reads them.  dense: contiguous [B, c, D].  strided: the stepper's cache layout - key and value as
    column slices of one buffer of 2 W columns (W = 640 for D = 600) with more rows than the window (window stride != c x row stride),
    q_u, k_u / v_u and out / out_u inside wider buffers; every float the kernel must not read is NaN.  out / out_u start at a sentinel.
    -> (q, k, v, ku, vu, out, out_u, out buffer)."""
    D = H * hd
    q, k, v, ku, vu = ops
    nan = float("nan")
    if not strided:
        ob = torch.full((2, B, c, D), _SENT, device=dev)
        return q.clone(), k.clone(), v.clone(), ku.clone(), vu.clone(), ob[0], ob[1], ob
    W = -(-(D + 8) // 128) * 128
    kv = torch.full((B, c + 5, 2 * W), nan, device=dev)
    kv[:, :c, :D], kv[:, :c, W:W + D] = k, v
    kvu = torch.full((B, c + 2, 2 * D + 12), nan, device=dev)
    kvu[:, :c, 3:3 + D], kvu[:, :c, D + 9:2 * D + 9] = ku, vu
    qb = torch.full((B, c + 3, D + 7), nan, device=dev)
    qb[:, :c, :D] = q
    ob = torch.full((2, B, c + 1, D + 5), _SENT, device=dev)
    return qb[:, :c, :D], kv[..., :D], kv[..., W:W + D], kvu[:, :, 3:3 + D], kvu[:, :, D + 9:2 * D + 9], ob[0, :, :c, :D], ob[1, :, :c, :D], ob


_ROWINV_CASES = [   # (B, c, H, hd, profile, streams, strided)
    (2, 1, 1, 1, "normal", "both", False), (2, 2, 4, 31, "late", "both", True), (1, 31, 5, 32, "diag_high", "both", False),
    (2, 32, 4, 33, "diag_low", "both", True), (2, 33, 1, 152, "late", "out", True), (1, 64, 5, 152, "normal", "out_u", True),
    (2, 65, 4, 150, "diag_high", "out_u", False), (3, 65, 1, 31, "late", "out", False), (2, 33, 5, 1, "diag_low", "out_u", True),
    (1, 1024, 4, 150, "late", "both", True), (1, 1024, 5, 152, "diag_low", "both", True), (1, 1024, 1, 1, "diag_high", "both", False),
    (2, 1024, 4, 33, "normal", "both", True), (1, 1024, 5, 32, "late", "out_u", False), (1, 1024, 4, 150, "diag_high", "out", True),
]


@pytest.mark.parametrize("B,c,H,hd,profile,streams,strided", _ROWINV_CASES,
                         ids=[f"B{b}_c{c}_H{h}_hd{d}_{p}_{s}_{'strided' if st else 'dense'}" for b, c, h, d, p, s, st in _ROWINV_CASES])
def test_rowinv_attention_vs_float64(dev, B, c, H, hd, profile, streams, strided):
    """Every row of every window against the float64 evaluation, within what an fp32 chain carries: a score of magnitude |s| over hd
    channels holds ~ sqrt(hd) |s| 2^-24 of rounding, which moves a convex combination of the v rows by that much times their spread
    (2 max |v|); the tolerance is twice that, plus 2^-19 max |v| for the sums over the keys (the largest measured error is under a
    tenth of the first term).  A one-stream launch gives the bits of the two-stream one, and nothing outside the output slices is written."""
    from scp_amd import native
    D = H * hd
    ops = _scores(B, c, H, hd, profile, dev, seed=c * 10 + hd)
    q, k, v, ku, vu, o, ou, ob = _place(B, c, H, hd, ops, strided, dev)
    want_o, want_u = streams in ("out", "both"), streams in ("out_u", "both")
    native.octattn_attention_rowinv(q, k, v, H, k_u=ku, v_u=vu, out=o if want_o else None, out_u=ou if want_u else None)
    keep = torch.ones_like(ob, dtype=torch.bool)
    (keep[0, :, :c, :D] if strided else keep[0]).fill_(not want_o)
    (keep[1, :, :c, :D] if strided else keep[1]).fill_(not want_u)
    assert bool((ob[keep] == _SENT).all())
    err = err_u = 0.0
    vmax = float(torch.maximum(ops[2].abs().max(), ops[4].abs().max()))
    smax = 0.0
    for b in range(B):
        ref, refu, sm = _attn_f64(*(t[b] for t in ops), H)
        smax = max(smax, sm)
        if want_o:
            err = max(err, float((o[b].double() - ref).abs().max()))
        if want_u:
            err_u = max(err_u, float((ou[b].double() - refu).abs().max()))
    tol = 2 * 2.0 ** -24 * hd ** 0.5 * (1 + smax) * 2 * vmax + 2.0 ** -19 * vmax
    print(f"rowinv B{B} c{c} H{H} hd{hd} {profile} {streams}: max |s| {smax:.1f}, max |v| {vmax:.2f}, float64 error out {err:.2e} "
          f"out_u {err_u:.2e} (tolerance {tol:.2e})")
    parity_record(f"rowinv_f64/B{B}_c{c}_H{H}_hd{hd}_{profile}_{streams}_{'strided' if strided else 'dense'}", max_err_out=err, max_err_out_u=err_u,
                  tol=tol, max_abs_score=smax)
    if profile != "normal":
        assert smax > 60
    assert err <= tol and err_u <= tol
    if streams != "both":                              # the same rows from a two-stream launch: the same bits
        q2, k2, v2, ku2, vu2, o2, ou2, _ = _place(B, c, H, hd, ops, strided, dev)
        native.octattn_attention_rowinv(q2, k2, v2, H, k_u=ku2, v_u=vu2, out=o2, out_u=ou2)
        assert torch.equal(o, o2) if want_o else torch.equal(ou, ou2)


def test_rowinv_reads_no_row_it_may_not(dev):
    """With NaN in every row no output row may read - with `out`: K / V rows >= q1; `out_u` alone: K / V rows >= q1 - 1 (the last query row
    reads only keys below itself, the decoder's unknown pass before row t of the cache is written) - and in q / k_u / v_u outside
    [q0, q1), each row of [q0, q1) is finite with the bits of the clean full launch, and no row outside [q0, q1) is written.  One-row
    launches at the tile edges, multi-row launches that start off the 32-row grid, full-size and row-offset operands, two windows."""
    from scp_amd import native
    B, c, H, hd = 2, 1024, 4, 150
    ops = _scores(B, c, H, hd, "late", dev, seed=3)
    q, k, v, ku, vu, o, ou, _ = _place(B, c, H, hd, ops, True, dev)
    native.octattn_attention_rowinv(q, k, v, H, k_u=ku, v_u=vu, out=o, out_u=ou)
    assert bool(torch.isfinite(o).all() and torch.isfinite(ou).all())
    nan = float("nan")
    n = 0
    for q0, q1 in ((0, 1), (31, 32), (32, 33), (33, 34), (1023, 1024), (5, 70), (33, 97), (961, 1000), (1, 1024)):
        for streams in ("out", "out_u", "both"):
            want_o, want_u = streams != "out_u", streams != "out"
            lim = q1 if want_o else q1 - 1
            for offset in ((False, True) if q1 - q0 == 1 else (False,)):
                q2, k2, v2, ku2, vu2, o2, ou2, _ = _place(B, c, H, hd, ops, True, dev)
                k2[:, lim:], v2[:, lim:] = nan, nan
                for t in (q2, ku2, vu2):
                    t[:, :q0], t[:, q1:] = nan, nan
                if offset:                           # the decoder's form: q_u / k_u / v_u / out hold rows q0 .. q1 - 1 only
                    args = dict(k_u=ku2[:, q0:q1], v_u=vu2[:, q0:q1], out=o2[:, :q1 - q0] if want_o else None,
                                out_u=ou2[:, :q1 - q0] if want_u else None, q0=q0, q1=q1, qoff=q0)
                    native.octattn_attention_rowinv(q2[:, q0:q1], k2, v2, H, **args)
                    got_o, got_u, r0 = o2[:, :q1 - q0], ou2[:, :q1 - q0], 0
                else:
                    native.octattn_attention_rowinv(q2, k2, v2, H, k_u=ku2, v_u=vu2, out=o2 if want_o else None, out_u=ou2 if want_u else None,
                                                    q0=q0, q1=q1)
                    got_o, got_u, r0 = o2[:, q0:q1], ou2[:, q0:q1], q0
                what = (q0, q1, streams, offset)
                for want, got, full, buf in ((want_o, got_o, o, o2), (want_u, got_u, ou, ou2)):
                    if want:
                        assert bool(torch.isfinite(got).all()), what
                        assert torch.equal(got, full[:, q0:q1]), what
                    written = torch.zeros(buf.shape[:2], dtype=torch.bool, device=dev)
                    if want:
                        written[:, r0:r0 + q1 - q0] = True
                    assert bool((buf[~written] == _SENT).all()), what
                n += 1
    print(f"{n} poisoned launches: bits kept")


def test_rowinv_refusals(dev):
    from scp_amd import native
    q = torch.randn((1, 4, 153), device=dev)
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):            # head width 153 > RI_MAXHD: refused by the C entry point
        native.octattn_attention_rowinv(q, q, q, 1, out=torch.empty_like(q))
    q = torch.randn((1, 8, 64), device=dev)
    k = torch.randn((1, 6, 64), device=dev)
    with pytest.raises(native.ScpError, match="beyond the key rows"):
        native.octattn_attention_rowinv(q, k, k, 2, out=torch.empty_like(q))
    with pytest.raises(native.ScpError, match="beyond the key rows"):
        native.octattn_attention_rowinv(q[:, 5:6], k, k, 2, k_u=q[:, 5:6], v_u=q[:, 5:6], out_u=torch.empty_like(q[:, :1]), q0=6, q1=7, qoff=6)
