"""The lockstep EHEM decoder (-m gpu): scp_decode_expand_batch gives the bits of scp_decode_expand run per segment, and several streams
decoded together decode to the bits the one-stream decoder gives - through decode_files and through the CLIs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfgs import ehem_cfg
from conftest import ROOT

pytestmark = pytest.mark.gpu

_SENT = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, context_size):
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    cfg = ehem_cfg()
    cfg["model"]["context_size"] = context_size
    return fill_weights(EHEM(cfg), 0).to(dev)


@pytest.fixture(scope="module")
def model1k(dev):
    return _model(dev, 1024)


@pytest.fixture(scope="module")
def model8k(dev):
    return _model(dev, 8192)


# ------------------------------------------------------------------------------------------------ scp_decode_expand_batch
def _segments(sizes, seed):
    """Per segment: parents (sym, pos, anc, octant) and decode_expand's scalars, all different from segment to segment."""
    rng = np.random.default_rng(seed)
    segs = []
    for k, n in enumerate(sizes):
        sym = rng.integers(0, 255, n).astype(np.int64)
        if k % 3 == 0:
            sym[:] = 254                                    # eight children each ...
            sym[0] = 6                                      # ... behind three: window borders fall between the children of one parent
        if k % 4 == 1 and n > 1:
            sym[-1] = -1                                    # a dropped last node
        if n == 1 and k % 2 == 1:
            sym[:] = -1                                     # a segment whose only parent is the dropped node: no children
        shift = [0, 30, 3, 11, 7][k % 5]
        L = [1, 254, 9, 12, 17][k % 5]
        polar = k % 2 == 0
        segs.append(dict(sym=sym, pos=rng.integers(0, 1 << 20, (n, 3)).astype(np.int32), anc=rng.integers(0, 256, (n, 9)).astype(np.uint8),
                         octant=rng.integers(1, 9, n).astype(np.uint8), L=L, shift=shift, lv_next=[L + 1, 0, 255, 12][k % 4] % 256,
                         lv_clamp=[255, 12, 0, 16][k % 4], polar=polar, mn=float(rng.uniform(-50, 50)) if polar else 0.0,
                         den=float(rng.uniform(0.5, 5000)) if polar else float(2 ** (k % 19 + 1)), drop=k % 4 == 2))
    return segs


def _reference(dev, segs, cs):
    """native.decode_expand per segment, re-ordered with torch -> (inputs of the batch call, its expected outputs)."""
    from scp_amd import native
    from scp_amd.decoder import EhemLockstep
    outs, coded = [], []
    for g in segs:
        t = lambda a: torch.from_numpy(a).to(dev)
        o = native.decode_expand(t(g["sym"]), t(g["pos"]), t(g["anc"]), t(g["octant"]), g["L"], g["shift"], g["lv_next"], g["lv_clamp"], g["polar"],
                                 g["mn"], g["den"])
        outs.append(o)
        m = o[1].shape[0]
        coded.append(m - 1 if (g["drop"] and m > 0) else m)
    steps, wbase = EhemLockstep.layout(coded, cs)
    T = sum(coded)
    cctx = torch.full((T, 12), _SENT, dtype=torch.uint8, device=dev)
    cposn = torch.full((T, 3), float("nan"), dtype=torch.float32, device=dev)
    for k, step in enumerate(steps):
        for col, c in step:
            r = int(wbase[k, col])
            cctx[r:r + c] = outs[col][4][k * cs:k * cs + c]
            cposn[r:r + c] = outs[col][5][k * cs:k * cs + c]
    ns = np.array([len(g["sym"]) for g in segs], np.int64)
    ms = np.array([o[1].shape[0] for o in outs], np.int64)
    seg = np.zeros(len(segs), native.EXPAND_SEG)
    for k, g in enumerate(segs):
        seg[k] = (ns[:k].sum(), ns[k], ms[:k].sum(), coded[k], g["L"], g["shift"], g["lv_next"], g["lv_clamp"], 1 if g["polar"] else 0, 0, g["mn"], g["den"])
    cat = lambda key, dt: torch.from_numpy(np.concatenate([g[key] for g in segs]).astype(dt)).to(dev)
    inputs = dict(sym=cat("sym", np.int64), pos=cat("pos", np.int32), anc=cat("anc", np.uint8), octant=cat("octant", np.uint8), seg=seg,
                  wbase=wbase, M=int(ms.sum()), T=T, cs=cs)
    want = dict(occ8=torch.cat([o[0] for o in outs]), cpos=torch.cat([o[1] for o in outs]), canc=torch.cat([o[2] for o in outs]),
                coct=torch.cat([o[3] for o in outs]), cctx=cctx, cposn=cposn)
    return inputs, want, coded, ms


_TAIL = 5      # sentinel rows behind every output


def _buffers(dev, n, M, T):
    def f(shape, dt):     # every BYTE at the sentinel
        return torch.full((int(np.prod(shape)) * torch.empty((), dtype=dt).element_size(),), _SENT, dtype=torch.uint8, device=dev).view(dt).reshape(shape)
    return dict(occ8=f((n + _TAIL,), torch.uint8), cpos=f((M + _TAIL, 3), torch.int32), canc=f((M + _TAIL, 9), torch.uint8),
                coct=f((M + _TAIL,), torch.uint8), cctx=f((T + _TAIL, 12), torch.uint8), cposn=f((T + _TAIL, 3), torch.float32))


def _call(dev, inp, buf, **over):
    """The C entry point on caller-owned buffers -> its return code.  `over`: arguments replaced (refusal cases)."""
    from scp_amd import native
    tab = native.popcount_table(dev)
    cum = torch.cumsum(tab[inp["sym"] + 1], 0)
    seg, wbase = np.ascontiguousarray(inp["seg"]), np.ascontiguousarray(inp["wbase"], np.int64)
    off = 64 * native.EXPAND_SEG.itemsize                   # the caller's device copy of both tables: seg at byte 0, wbase behind 64 records
    host = np.zeros(off + 8 * wbase.size + 64, np.uint8)
    host[:seg.nbytes] = seg.view(np.uint8)
    host[off:off + wbase.nbytes] = wbase.reshape(-1).view(np.uint8)
    scratch = torch.from_numpy(host).to(dev)
    a = dict(sym=inp["sym"].data_ptr(), cum=cum.data_ptr(), pos=inp["pos"].data_ptr(), anc=inp["anc"].data_ptr(), octant=inp["octant"].data_ptr(),
             n=inp["sym"].shape[0], seg=seg.ctypes.data, S=seg.shape[0], cs=inp["cs"], wbase=wbase.ctypes.data, K=wbase.shape[0], M=inp["M"], T=inp["T"],
             table=scratch.data_ptr(), cpos=buf["cpos"].data_ptr(), canc=buf["canc"].data_ptr(), coct=buf["coct"].data_ptr(),
             cctx=buf["cctx"].data_ptr(), cposn=buf["cposn"].data_ptr(), occ8=buf["occ8"].data_ptr())
    a.update(over)
    rc = native.lib().scp_decode_expand_batch(*[a[k] for k in ("sym", "cum", "pos", "anc", "octant", "n", "seg", "S", "cs", "wbase", "K", "M", "T", "table",
                                                                "cpos", "canc", "coct", "cctx", "cposn", "occ8")], native._stream())
    torch.cuda.synchronize()
    return rc, (seg, wbase, cum, scratch)


_CASES = {   # segment sizes, cs
    "mixed_cs1024": ([1, 255, 256, 3000, 257, 1, 40, 700, 1], 1024),
    "mixed_cs8192": ([1, 255, 256, 3000, 257, 1, 40, 700, 1], 8192),
    "one_segment": ([3000], 1024),
    "S64": ([1 + (37 * k) % 150 for k in range(64)], 1024),
}


@pytest.mark.parametrize("case", list(_CASES))
def test_expand_batch_equals_decode_expand_per_segment(dev, case):
    """Bit for bit (positions as int32 views), every output row written and nothing behind them: the buffers start at a sentinel and are
    compared whole, their tails included."""
    sizes, cs = _CASES[case]
    segs = _segments(sizes, seed=len(sizes) + cs)
    inp, want, coded, ms = _reference(dev, segs, cs)
    n, M, T = sum(sizes), inp["M"], inp["T"]
    assert M > T > 0 or case == "one_segment"
    if case.startswith("mixed"):
        assert n > 4500 and any(m == 0 for m in ms) and any(c == m - 1 for c, m in zip(coded, ms) if m)
        assert {g["shift"] for g in segs} >= {0, 30} and {g["polar"] for g in segs} == {True, False}
    if case == "mixed_cs1024":
        # a parent whose eight children lie on both sides of a window border
        g = segs[3]
        occ = np.array([bin(int(s) + 1).count("1") for s in g["sym"]])
        end = np.cumsum(occ)
        assert ((end - occ) // cs != (end - 1) // cs)[occ == 8].any() and coded[3] > 2 * cs
    if case == "S64":
        assert len(segs) == 64
    buf = _buffers(dev, n, M, T)
    rc, _keep = _call(dev, inp, buf)
    assert rc == 0
    for key, rows in (("occ8", n), ("cpos", M), ("canc", M), ("coct", M), ("cctx", T), ("cposn", T)):
        got = buf[key].view(torch.int32) if key == "cposn" else buf[key]
        ref = want[key].view(torch.int32) if key == "cposn" else want[key]
        assert torch.equal(got[:rows], ref), key
        assert bool((got[rows:] == (_SENT if got.dtype == torch.uint8 else int.from_bytes(bytes([_SENT] * 4), "little", signed=True))).all()), key
    if T:
        assert not bool(torch.isnan(want["cposn"]).any()), "the reference layout covers every input row"
    # the Python wrapper: the same arrays
    from scp_amd import native
    cum = torch.cumsum(native.popcount_table(dev)[inp["sym"] + 1], 0)
    got = native.decode_expand_batch(inp["sym"], inp["pos"], inp["anc"], inp["octant"], cum, inp["seg"], cs, inp["wbase"], M, T)
    for g, key in zip(got, ("occ8", "cpos", "canc", "coct", "cctx", "cposn")):
        assert torch.equal(g.view(torch.int32) if key == "cposn" else g, want[key].view(torch.int32) if key == "cposn" else want[key]), key
    if case == "one_segment":
        # S = 1: scp_decode_expand outright (one column: window k starts at row k * cs)
        t = lambda a: torch.from_numpy(a).to(dev)
        g0 = segs[0]
        one = native.decode_expand(t(g0["sym"]), t(g0["pos"]), t(g0["anc"]), t(g0["octant"]), g0["L"], g0["shift"], g0["lv_next"], g0["lv_clamp"],
                                   g0["polar"], g0["mn"], g0["den"])
        assert coded[0] == ms[0] and all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                     b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, one))


def test_expand_batch_refusals_launch_nothing(dev):
    sizes, cs = [5, 300, 1], 64
    segs = _segments(sizes, seed=3)
    inp, want, coded, ms = _reference(dev, segs, cs)
    n, M, T = sum(sizes), inp["M"], inp["T"]
    buf = _buffers(dev, n, M, T)

    def seg_with(k, **kw):
        s = inp["seg"].copy()
        for key, v in kw.items():
            s[key][k] = v
        return s

    bad = [dict(sym=None), dict(cum=None), dict(pos=None), dict(anc=None), dict(octant=None), dict(seg=None), dict(wbase=None), dict(table=None),
           dict(cpos=None), dict(canc=None), dict(coct=None), dict(cctx=None), dict(cposn=None), dict(occ8=None),
           dict(S=0), dict(S=65), dict(cs=0), dict(cs=-1), dict(K=0), dict(n=0), dict(n=n + 1), dict(M=M - 2), dict(M=0), dict(T=-1), dict(T=T - 1)]
    keep = []
    for over in bad:
        rc, k = _call(dev, inp, buf, **over)
        keep.append(k)
        assert rc == -1, over
    for kw in (dict(L=0), dict(L=255), dict(shift=-1), dict(shift=31), dict(lv_next=-1), dict(lv_next=256), dict(lv_clamp=-1), dict(lv_clamp=256),
               dict(den=0.0), dict(den=float("nan")), dict(first=1), dict(count=0), dict(cfirst=3), dict(coded=-1), dict(coded=int(ms[1]) + 1)):
        s = np.ascontiguousarray(seg_with(1, **kw))
        rc, k = _call(dev, inp, buf, seg=s.ctypes.data)
        keep.append((k, s))
        assert rc == -1, kw
    wb = inp["wbase"].copy()
    wb[0, 1] = -1                                             # a window of coded children without a place
    rc, k = _call(dev, inp, buf, wbase=wb.ctypes.data)
    assert rc == -1
    wb2 = inp["wbase"].copy()
    wb2[wb2 >= 0] += 1                                        # the last window would end behind the inputs
    rc, k = _call(dev, inp, buf, wbase=wb2.ctypes.data)
    assert rc == -1
    for key, b in buf.items():
        assert bool((b.view(torch.uint8) == _SENT).all()), key
    assert _call(dev, inp, buf)[0] == 0 and torch.equal(buf["cctx"][:T], want["cctx"])


# ------------------------------------------------------------------------------------------------ round trips
def _encode(model, dev, tmp_path, stem, xyz, level, spher=False, cylin=False, mullevel=False):
    """FrameEncoder -> stream, `.dat` and side-info files as the encode CLIs write them -> (stream file, result, occupancies per shell,
    leaves per shell)."""
    from scp_amd.decoder import write_sidecar
    from scp_amd.encoder import FrameEncoder
    enc = FrameEncoder(model, "kitti", level, spher=spher, cylin=cylin, mullevel=mullevel, device=dev)
    res = enc.encode(xyz)
    out = enc.outfile(str(tmp_path / stem), res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), out + ".dat")
    write_sidecar(out, enc, res, "EHEM")
    occ = enc.geom.nodes(("occ",))["occ"]
    occs = [occ[i.node_base:i.node_base + i.n_nodes].clone() for i in enc.geom.info]
    return out, res, occs, [enc.geom.leaves(s).clone() for s in range(len(enc.geom.info))]


def _same(a, b):
    return (len(a["codes"]) == len(b["codes"]) and all(torch.equal(x, y) for x, y in zip(a["codes"], b["codes"]))
            and all(torch.equal(x, y) for x, y in zip(a["leaves"], b["leaves"])) and torch.equal(a["points"], b["points"]))


def test_round_trip_five_frames_on_three_slots(model1k, dev, tmp_path):
    """Five frames of different sizes, depths and coordinate systems, context_size 1024 (levels of several windows with short and odd tails
    beside one-node windows): streams=3 decodes every frame to the encoder's occupancies and leaves and to decode_file's result;
    streams=1 and streams=8 give the same."""
    from scp_amd.decoder import decode_file, decode_files
    from scp_amd.synth import synth_frame
    frames = [_encode(model1k, dev, tmp_path, "a", synth_frame(5)[::20].copy(), 12, spher=True),
              _encode(model1k, dev, tmp_path, "b", synth_frame(4)[::40].copy(), 11, cylin=True),
              _encode(model1k, dev, tmp_path, "c", synth_frame(3)[::60].copy(), 10),
              _encode(model1k, dev, tmp_path, "d", synth_frame(2)[::90].copy(), 9, spher=True),
              _encode(model1k, dev, tmp_path, "e", np.array([[10.0, 3.0, -1.0]], np.float32), 12, spher=True)]
    files = [f[0] for f in frames]
    sizes = [f[1]["level_sizes"] for f in frames]
    print("nodes per frame:", [f[1]["n_nodes"] for f in frames], "largest levels:", [max(s) for s in sizes])
    assert any(max(s) > 2 * 1024 for s in sizes) and len({f[1]["n_nodes"] for f in frames}) == 5
    got = decode_files(files, model1k, streams=3, device=dev)
    for f, (out, res, occs, leaves) in enumerate(frames):
        assert len(got[f]["codes"]) == 1
        assert torch.equal(got[f]["codes"][0].long(), occs[0].long()), f
        assert torch.equal(got[f]["leaves"][0], leaves[0].to(got[f]["leaves"][0].dtype)), f
        assert _same(got[f], decode_file(out, model1k, device=dev)), f
    one = decode_files(files, model1k, streams=1, device=dev)
    many = decode_files(files, model1k, streams=8, device=dev)
    for f in range(5):
        assert _same(got[f], one[f]) and _same(got[f], many[f]), f


def test_multi_level_frames_on_two_slots(model1k, dev, tmp_path):
    """Three multi-level frames, one of them three one-leaf shells (every shell's last level is the dropped node alone: rounds with 0
    coded rows, a launch-free expansion), decoded with streams=2 = decode_file(..., mullevel=True)."""
    from scp_amd.decoder import decode_file, decode_files
    from scp_amd.synth import synth_frame
    leaf = np.array([[r * 0.8, r * 0.6, -1.0] for r in (5, 30, 70)], np.float32)
    frames = [_encode(model1k, dev, tmp_path, "a", synth_frame(6)[::50].copy(), 12, spher=True, mullevel=True),
              _encode(model1k, dev, tmp_path, "b", leaf, 12, spher=True, mullevel=True),
              _encode(model1k, dev, tmp_path, "c", synth_frame(7)[::80].copy(), 11, spher=True, mullevel=True)]
    files = [f[0] for f in frames]
    got = decode_files(files, model1k, streams=2, mullevel=True, device=dev)
    for f, (out, res, occs, _) in enumerate(frames):
        assert len(got[f]["codes"]) == 3
        for k in range(3):
            c = got[f]["codes"][k]
            assert c[-1] == 0 and torch.equal(c[:-1].long(), occs[k][:-1].long()), (f, k)          # the last BFS node is not coded
        assert _same(got[f], decode_file(out, model1k, mullevel=True, device=dev)), f
    assert all(lv.shape[0] == 0 for lv in got[1]["leaves"])


def test_production_window_length(model8k, dev, tmp_path):
    """context_size 8192: two frames of about 10 000 points whose deepest levels span two windows."""
    from scp_amd.decoder import decode_file, decode_files
    from scp_amd.synth import synth_frame
    frames = [_encode(model8k, dev, tmp_path, f"f{i}", synth_frame(i)[::12].copy(), 12, spher=True) for i in range(2)]
    assert all(8192 < max(f[1]["level_sizes"]) <= 2 * 8192 for f in frames), [max(f[1]["level_sizes"]) for f in frames]
    got = decode_files([f[0] for f in frames], model8k, streams=2, device=dev)
    for f, (out, res, occs, leaves) in enumerate(frames):
        assert torch.equal(got[f]["codes"][0].long(), occs[0].long()), f
        assert _same(got[f], decode_file(out, model8k, device=dev)), f


def test_rounds_cut_into_several_phase1_runs_and_coder_threads(model1k, dev, tmp_path):
    """Bounds of 3 000 tokens per phase-1 forward: the rounds of the larger levels are cut into several runs of whole steps (each with its
    own plan, preparation and row offsets); the same once more with the range decoders of a step on a thread pool.  Both = decode_file."""
    from scp_amd.decoder import EhemBatchDecoder, _ehem_job, chunk_steps, decode_file
    from scp_amd.synth import synth_frame
    frames = [_encode(model1k, dev, tmp_path, "a", synth_frame(5)[::20].copy(), 12, spher=True),
              _encode(model1k, dev, tmp_path, "b", synth_frame(4)[::40].copy(), 11, cylin=True),
              _encode(model1k, dev, tmp_path, "c", synth_frame(3)[::60].copy(), 10)]
    want = [decode_file(f[0], model1k, device=dev) for f in frames]
    runs = []
    for kw in (dict(max_tokens=3000), dict(max_rows=2048), dict(coder_threads=3)):
        d = EhemBatchDecoder(model1k, 3, device=dev, **kw)
        orig = d._plan
        d._plan = lambda lengths, orig=orig: runs.append(sum(lengths)) or orig(lengths)
        got = d.decode([_ehem_job(f[0]) for f in frames])
        for g, w in zip(got, want):
            assert len(g) == 1 and torch.equal(torch.cat(g[0][0]), w["codes"][0]) and torch.equal(g[0][1], w["leaves"][0]), kw
        if "max_tokens" in kw:
            big = max(f[1]["level_sizes"][-1] for f in frames)
            assert big > 3000 and len(chunk_steps([[1024] * 3] * 5, max_tokens=3000)) > 1
    assert frames[0][1]["level_sizes"][-1] + frames[1][1]["level_sizes"][-1] > 2 * 3000


_STAGES = ("tree_expansion", "phase1_model", "cdf_d2h", "range_decoder", "index_ops", "phase2_model")


@pytest.mark.parametrize("points,tail", [(4097, (1025, 2049)), (4101, (1026, 2051)), (2, (1,))])
def test_one_stream_tail_windows_of_one_two_and_three_nodes(model1k, dev, points, tail):
    """Integer clouds on a line, context_size 1024: the last two levels end in a tail window of one node (1024 + 1, 2 x 1024 + 1: no phase
    2 for it, yet its rows in the level's phase-1 state, the preparation and the CDF rows are stepped over) or of two and three nodes;
    two points are one level of one node (no phase 2 at all).  FrameDecoder as constructed, without the preparation ahead and with stage
    stamps, and EhemBatchDecoder on one slot, all decode to the encoder's occupancies and leaves."""
    from scp_amd.decoder import EhemBatchDecoder, FrameDecoder
    from scp_amd.encoder import FrameEncoder
    q = np.zeros((points, 3), np.int32)
    q[:, 0] = np.arange(points)
    enc = FrameEncoder(model1k, "kitti", 12, spher=False, cylin=False, mullevel=False, device=dev)
    res = enc.encode_ints([q], 0, 0.0, points)
    assert tuple(res["level_sizes"][-len(tail):]) == tail, res["level_sizes"]
    occ = enc.geom.nodes(("occ",))["occ"].long()
    leaves = enc.geom.leaves(0).long()
    assert occ.shape[0] == res["n_nodes"] == sum(res["level_sizes"])

    def check(shells, what):
        assert len(shells) == 1, what
        codes, lv = shells[0]
        assert torch.equal(torch.cat(codes).long(), occ), what
        assert torch.equal(lv.long(), leaves), what

    def one_stream(**attrs):
        d = FrameDecoder(model1k, 12, mullevel=False, polar=False, device=dev)
        for k, v in attrs.items():
            setattr(d, k, v)
        check(d.decode(res["bytes"], res["n_levels"], res["pos_mm"]), attrs)
        return d

    one_stream()
    one_stream(prepare_ahead=False)
    stats = one_stream(stats={}).stats
    if points == 2:                                           # one node: nothing goes up, no phase 2
        assert all(k in stats for k in _STAGES[:4]) and stats.get("phase2_model", 0) == 0, stats
    else:
        assert all(k in stats for k in _STAGES) and stats["phase2_model"] > 0, stats
    job = dict(name="line", stream=res["bytes"], n_levels=res["n_levels"], pos_mm=res["pos_mm"], polar=False, mullevel=False, lidar_level=12)
    check(EhemBatchDecoder(model1k, 1, device=dev).decode([job])[0], "lockstep, one slot")


def test_a_stream_of_another_profile_is_refused_before_anything_is_decoded(model1k, dev, tmp_path):
    from scp_amd import native
    from scp_amd.decoder import SIDECAR, EhemBatchDecoder, decode_files
    from scp_amd.synth import synth_frame
    a = _encode(model1k, dev, tmp_path, "a", synth_frame(1)[::600].copy(), 9, spher=True)
    b = _encode(model1k, dev, tmp_path, "b", synth_frame(2)[::600].copy(), 9, spher=True)
    side = json.load(open(b[0] + SIDECAR))
    json.dump(dict(side, profile="ehem/0"), open(b[0] + SIDECAR, "w"))
    made = []
    init = EhemBatchDecoder.__init__
    EhemBatchDecoder.__init__ = lambda self, *x, **k: made.append(1) or init(self, *x, **k)
    try:
        with pytest.raises(native.ScpError, match="numeric profile") as e:
            decode_files([a[0], b[0]], model1k, streams=2, device=dev)
    finally:
        EhemBatchDecoder.__init__ = init
    assert os.path.basename(b[0]) in str(e.value) and not made


@pytest.mark.parametrize("mullevel", [False, True])
def test_cli_decode_with_and_without_streams(tmp_path, mullevel):
    """encode.py on four files, decode_ehem.py with and without --streams 3: identical .ply bytes, `oct len:` and file lines (and the same
    once for encode_mullevel.py / decode_ehem_mullevel.py)."""
    from scp_amd.synth import synth_frame, write_kitti_bin
    srcs = []
    for i in range(4):
        src = tmp_path / f"00000{i}.bin"
        write_kitti_bin(str(src), synth_frame(i)[::(200 + 90 * i)].copy())
        srcs.append(str(src))
    out = tmp_path / "out"
    enc_script, dec_script = ("encode_mullevel.py", "decode_ehem_mullevel.py") if mullevel else ("encode.py", "decode_ehem.py")
    enc = [sys.executable, os.path.join(ROOT, enc_script), "--test_files", *srcs, "--type", "kitti", "--lidar_level", "10", "--spher",
           "--random_weights", "0", "--out_dir", str(out)]
    r = subprocess.run(enc, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    dec = [sys.executable, os.path.join(ROOT, dec_script), "--test_files", *srcs, "--random_weights", "0", "--out_dir", str(out)]
    plys, lines = [], []
    for extra in ([], ["--streams", "3"]):
        r = subprocess.run(dec + extra, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        names = sorted(p.name for p in out.iterdir() if p.suffix == ".ply")
        assert len(names) == 4
        plys.append([(out / n).read_bytes() for n in names])
        lines.append([ln for ln in r.stdout.splitlines() if ln.startswith(("oct len:", str(out))) or re.fullmatch(r"\d/4", ln)])
        for n in names:
            (out / n).unlink()
    assert all(len(p) > 100 for p in plys[0]) and len(set(plys[0])) == 4
    assert plys[0] == plys[1]
    assert lines[0] == lines[1] and len(lines[0]) == 12
