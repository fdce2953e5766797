"""The lockstep OctAttention decoder (-m gpu): the one-row-per-stream attention kernel gives the bits of the row-invariant kernel's one-row
launch, the batch stepper gives the rows of the batched decodable forward whatever the other slots do, and several streams decoded
together decode to the bits the one-stream decoder gives."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, parity_record
from cfgs import octattn_cfg

pytestmark = pytest.mark.gpu

_SENT = 1.0e30
_NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from scp_amd.models import OctAttention
    from scp_amd.weights import fill_weights
    return fill_weights(OctAttention(octattn_cfg()), 0).to(dev)


@pytest.fixture
def dmodel(model):
    model.decodable = True
    yield model
    model.decodable = False


# ------------------------------------------------------------------------------------------------ scp_octattn_attention_rowinv_step
_TS = (0, 1, 31, 32, 33, 64, 500, 1023)


def _step_case(dev, H, hd, ns, slot, ts, streams, strided, seed):
    """`ns` cache slots of 1024 rows (+ 5 the kernel never reaches when strided), slot s at row ts[s]; launch rows = `slot`.  Every float
    a launch row may not read is NaN: cache rows > t of a listed slot (>= t when `out` is not wanted), every row of a slot not listed,
    and the padding of the strided buffers.  -> operands, outputs (at a sentinel) and the output buffer."""
    g = torch.Generator(device=dev).manual_seed(seed)
    D, S, rows = H * hd, len(slot), 1024
    want_o = streams != "out_u"
    rn = lambda *s: torch.randn(s, generator=g, device=dev)
    W = -(-(D + 8) // 128) * 128 if strided else D
    kv = rn(ns, rows + (5 if strided else 0), 2 * W)
    for s in range(ns):
        lim = (ts[s] + 1 if want_o else ts[s]) if s in slot else 0
        kv[s, lim:] = _NAN
    if strided:
        kv[:, :, D:W] = _NAN
        kv[:, :, W + D:] = _NAN
        qb = torch.full((S, D + 7), _NAN, device=dev)
        qb[:, :D] = rn(S, D)
        kvu = torch.full((S, 2 * D + 12), _NAN, device=dev)
        kvu[:, 3:3 + D], kvu[:, D + 9:2 * D + 9] = rn(S, D), rn(S, D)
        q, ku, vu = qb[:, :D], kvu[:, 3:3 + D], kvu[:, D + 9:2 * D + 9]
        ob = torch.full((2, S + 1, D + 5), _SENT, device=dev)
        o, ou = ob[0, :S, :D], ob[1, :S, :D]
    else:
        q, ku, vu = rn(S, D), rn(S, D), rn(S, D)
        ob = torch.full((2, S, D), _SENT, device=dev)
        o, ou = ob[0], ob[1]
    return q, kv[:, :rows, :D], kv[:, :rows, W:W + D], ku, vu, o, ou, ob


def _row_f64(q, k, v, ku, vu, t, H, known):
    """attention_model.py:58-95 for ONE query row in float64: keys 0 .. t - 1 of the cache and the diagonal term (k[t], v[t] for the known
    stream; k_u, v_u for the unknown one) -> (the row [D], its largest |score|)."""
    D = q.shape[0]
    hd = D // H
    kd = torch.cat((k[:t], (k[t] if known else ku)[None])).double().reshape(t + 1, H, hd)
    vd = torch.cat((v[:t], (v[t] if known else vu)[None])).double().reshape(t + 1, H, hd)
    s = torch.einsum("hd,jhd->hj", q.double().reshape(H, hd), kd) / hd ** 0.5
    return torch.einsum("hj,jhd->hd", torch.softmax(s, -1), vd).reshape(D), float(s.abs().max())


_STEP_CASES = [   # (H, hd, cache slots, launch rows, streams, strided)
    (4, 150, 16, "perm", "both", True), (4, 152, 16, "perm", "out_u", True), (4, 152, 16, "subset", "out", True),
    (2, 64, 16, "perm", "both", False), (3, 1, 16, "subset", "both", True), (4, 150, 9, "subset", "out_u", False),
    (1, 152, 8, "perm", "out", False), (5, 64, 3, "one", "both", True),
]


@pytest.mark.parametrize("H,hd,ns,rows,streams,strided", _STEP_CASES,
                         ids=[f"H{h}_hd{d}_slots{n}_{r}_{s}_{'strided' if st else 'dense'}" for h, d, n, r, s, st in _STEP_CASES])
def test_step_kernel_equals_the_rowinv_kernels_one_row_launch(dev, H, hd, ns, rows, streams, strided):
    """Launch row s of scp_octattn_attention_rowinv_step = what scp_octattn_attention_rowinv writes for q0 = t, q1 = t + 1 on that slot's
    cache (torch.equal), with t over the tile edges mixed in ONE launch, `slot[]` a permutation / a strict subset / a single slot, NaN in
    every float no row may read, and nothing outside the output rows written.  The same rows against float64 under the bound derived
    for the row-invariant kernel: a score of magnitude |s| over hd channels holds ~ sqrt(hd) |s| 2^-24 of rounding, which moves a convex
    combination of the v rows by that much times their spread (2 max |v|); the tolerance is twice that, plus 2^-19 max |v| for the
    sums over the keys."""
    from scp_amd import native
    rng = np.random.default_rng(H * 1000 + hd + ns)
    ts = [_TS[(i * 3 + 1) % len(_TS)] for i in range(ns)]
    slot = {"perm": [int(x) for x in rng.permutation(ns)], "subset": [int(x) for x in rng.permutation(ns)[:max(ns // 2, 1)]], "one": [ns - 2]}[rows]
    assert set(ts) == set(_TS) or ns < len(_TS)
    S, D = len(slot), H * hd
    want_o, want_u = streams != "out_u", streams != "out"
    q, k, v, ku, vu, o, ou, ob = _step_case(dev, H, hd, ns, slot, ts, streams, strided, seed=hd * 7 + ns)
    t_dev = torch.tensor(ts, dtype=torch.int32, device=dev)
    slot_dev = torch.tensor(slot, dtype=torch.int32, device=dev)
    native.octattn_attention_rowinv_step(q, k, v, t_dev, slot_dev, H, k_u=ku, v_u=vu, out=o if want_o else None, out_u=ou if want_u else None)
    keep = torch.ones_like(ob, dtype=torch.bool)
    keep[0, :S, :D] = not want_o
    keep[1, :S, :D] = not want_u
    assert bool((ob[keep] == _SENT).all())
    err = err_u = smax = 0.0
    vmax = 0.0
    for r, s in enumerate(slot):
        t = ts[s]
        ro, ru = torch.full((1, D), _SENT, device=dev), torch.full((1, D), _SENT, device=dev)
        native.octattn_attention_rowinv(q[r:r + 1], k[s], v[s], H, k_u=ku[r:r + 1], v_u=vu[r:r + 1], out=ro if want_o else None,
                                        out_u=ru if want_u else None, q0=t, q1=t + 1, qoff=t)
        if want_o:
            assert bool(torch.isfinite(o[r]).all()), (r, s, t)
            assert torch.equal(o[r], ro[0]), (r, s, t, float((o[r] - ro[0]).abs().max()))
            ref, sm = _row_f64(q[r], k[s], v[s], ku[r], vu[r], t, H, True)
            err, smax = max(err, float((o[r].double() - ref).abs().max())), max(smax, sm)
            vmax = max(vmax, float(v[s, :t + 1].abs().max()))
        if want_u:
            assert bool(torch.isfinite(ou[r]).all()), (r, s, t)
            assert torch.equal(ou[r], ru[0]), (r, s, t, float((ou[r] - ru[0]).abs().max()))
            ref, sm = _row_f64(q[r], k[s], v[s], ku[r], vu[r], t, H, False)
            err_u, smax = max(err_u, float((ou[r].double() - ref).abs().max())), max(smax, sm)
            vmax = max(vmax, float(vu[r].abs().max()), float(v[s, :t].abs().max()) if t else 0.0)
    tol = 2 * 2.0 ** -24 * hd ** 0.5 * (1 + smax) * 2 * vmax + 2.0 ** -19 * vmax
    print(f"rowinv_step H{H} hd{hd} slots{ns} {rows} {streams}: max |s| {smax:.1f}, max |v| {vmax:.2f}, float64 error out {err:.2e} "
          f"out_u {err_u:.2e} (tolerance {tol:.2e})")
    parity_record(f"rowinv_step_f64/H{H}_hd{hd}_slots{ns}_{rows}_{streams}_{'strided' if strided else 'dense'}", max_err_out=err,
                  max_err_out_u=err_u, tol=tol, max_abs_score=smax)
    assert err <= tol and err_u <= tol


def test_step_kernel_refusals(dev):
    from scp_amd import native
    t = torch.zeros(2, dtype=torch.int32, device=dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    q = torch.randn((1, 153), device=dev)
    kv = torch.randn((2, 8, 153), device=dev)
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):            # head width 153: refused by the C entry point
        native.octattn_attention_rowinv_step(q, kv, kv, t, slot, 1, out=torch.empty_like(q))
    q = torch.randn((1, 64), device=dev)
    kv = torch.randn((2, 1025, 64), device=dev)
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):            # more cache rows than the kernel keeps scores for
        native.octattn_attention_rowinv_step(q, kv, kv, t, slot, 2, out=torch.empty_like(q))
    kv = torch.randn((2, 16, 64), device=dev)
    L = native.lib().scp_octattn_attention_rowinv_step
    o = torch.full((1, 64), _SENT, device=dev)
    p = lambda x: x.data_ptr()
    good = [p(q), 64, p(kv), p(kv), 16 * 64, 64, 2, 16, None, None, 0, p(o), None, 64, p(t), p(slot), 1, 2, 32, native._stream()]
    bad = {0: None, 2: None, 3: None, 14: None, 15: None, 11: None, 16: 0, 17: 0, 18: 0, 1: 63, 5: 63, 13: 63, 6: 0, 7: 0, 4: 15 * 64}
    for i, val in bad.items():
        args = list(good)
        args[i] = val
        assert L(*args) == -1, i
    args = list(good)
    args[12] = p(o)                                                       # out_u without k_u / v_u
    assert L(*args) == -1
    torch.cuda.synchronize()
    assert bool((o == _SENT).all())
    assert L(*good) == 0
    with pytest.raises(native.ScpError, match="nothing to compute"):
        native.octattn_attention_rowinv_step(q, kv, kv, t, slot, 2)
    # a slot number or a row outside the cache: the row is left alone, the others are written
    o2 = torch.full((2, 64), _SENT, device=dev)
    q2 = torch.randn((2, 64), device=dev)
    for tt, ss in (([3, 16], [0, 1]), ([3, 3], [0, 2]), ([3, -1], [0, 1]), ([3, 3], [0, -1])):
        o2.fill_(_SENT)
        native.octattn_attention_rowinv_step(q2, kv, kv, torch.tensor(tt, dtype=torch.int32, device=dev),
                                             torch.tensor(ss, dtype=torch.int32, device=dev), 2, out=o2)
        assert bool(torch.isfinite(o2[0]).all() and (o2[0] != _SENT).all() and (o2[1] == _SENT).all()), (tt, ss)


# ------------------------------------------------------------------------------------------------ OctAttnBatchStepper
def _chunks(dev, n):
    """n chunks of 1 + 2 cs rows of logits_octattn_c1024-style inputs (the fixture's rows, rolled, occupancies shuffled) -> per chunk
    (ctx uint8 [N, 12], pos [N, 4, 3])."""
    z = golden("logits_octattn_c1024")
    data, pos = torch.from_numpy(z["data"].astype(np.int64)), torch.from_numpy(z["pos"])
    g = torch.Generator().manual_seed(19)
    out = []
    for w in range(n):
        ds, ps = [], []
        for k in range(3):
            d, p = data.roll(37 * (3 * w + k) + 5, 0).clone(), pos.roll(37 * (3 * w + k) + 5, 0).clone()
            d[:, :, 0] = torch.where(d[:, :, 0] == 255, d[:, :, 0], torch.randint(0, 255, d[:, :, 0].shape, generator=g))
            ds.append(d if k else d[-1:])
            ps.append(p if k else p[-1:])
        out.append((torch.cat(ds).reshape(-1, 12).to(torch.uint8).to(dev), torch.cat(ps).to(dev)))
    return out


def _teacher_forced_batch(m, dev, poison):
    """Four slots, each teacher-forced through the first n rows of a chunk of its own (pad-prefix window, then windows that start empty),
    started at different steps, so that the set of slots a call serves, their rows t and their resets all differ from step to step; slot
    1 runs a second chunk after its first.  poison: every cache starts as NaN and after each reset the slot's cache rows >= t are NaN
    again.  -> per run (the stepper's logits rows, the batched decodable forward's rows)."""
    from scp_amd.decoder import octattn_window_of
    from scp_amd.models.oct_attention import OctAttnBatchStepper, _pad_rows
    cs = m.cfg.model.context_size
    chunks = _chunks(dev, 5)
    pc, pp = _pad_rows(cs - 1, dev)
    refs = [m(torch.cat((pc, c)).reshape(3, cs, 4, 3), torch.cat((pp, p)).reshape(3, cs, 4, 3)).reshape(-1, 255)[cs - 1:] for c, p in chunks]
    # (slot, chunk, first step, rows)
    runs = [(0, 0, 0, 1 + cs + 200), (1, 1, 37, 300), (2, 2, 500, 1 + cs + 40), (3, 3, 5, 700), (1, 4, 400, 1 + cs + 3)]
    st = OctAttnBatchStepper(m, 5)                    # slot 4 is never served
    if poison:
        st.kv.fill_(_NAN)
    got = [[] for _ in runs]
    last = max(s0 + n for _, _, s0, n in runs)
    sets = set()
    for step in range(last):
        live = sorted((slot, k, step - s0) for k, (slot, _, s0, n) in enumerate(runs) if s0 <= step < s0 + n)
        if not live:
            continue
        ids = [slot for slot, _, _ in live]
        sets.add(tuple(ids))
        for slot, k, r in live:
            w, t = octattn_window_of(r, cs)
            if r == 0 or t == 0:
                st.reset([slot], pad=(w == 0))
                if poison:
                    st.kv[slot, :, st.t[slot]:] = _NAN
            assert st.t[slot] == t
        ctx = torch.cat([chunks[runs[k][1]][0][r:r + 1] for _, k, r in live])
        pos = torch.cat([chunks[runs[k][1]][1][r:r + 1] for _, k, r in live])
        unk = ctx.clone()
        unk[:, 9] = 255
        logits = st.unknown(ids, unk, pos)
        st.known(ids, ctx, pos)
        for b, (_, k, _) in enumerate(live):
            got[k].append(logits[b])
    assert st.t_dev.tolist() == st.t
    assert len(sets) >= 6
    return [(torch.stack(g), refs[runs[k][1]][:len(g)]) for k, g in enumerate(got)]


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "nan_beyond_t"])
def test_batch_step_equals_batched_forward(dmodel, dev, poison):
    """Every logits row of every slot = that row of OctAttention.forward under the decodable profile, bit for bit, whatever the other
    slots hold or do; with NaN in every cache row at or beyond its slot's t, and in the slot never served, the rows keep their bits."""
    for k, (got, ref) in enumerate(_teacher_forced_batch(dmodel, dev, poison)):
        assert bool(torch.isfinite(got).all()), k
        bad = (got != ref).any(1).nonzero().flatten()[:10].tolist()
        assert torch.equal(got, ref), f"run {k}: rows differing: {bad}"


# ------------------------------------------------------------------------------------------------ round trips
def _encode(model, dev, tmp_path, stem, xyz, level, spher=False, cylin=False, level_wise=False, ints=None, data_type="kitti"):
    """Encode decodable, write stream + side-info -> (stream file, the encoder's result, its integers)."""
    from scp_amd.decoder import write_sidecar
    from scp_amd.encoder import OctAttnFrameEncoder
    enc = OctAttnFrameEncoder(model, data_type, level, spher=spher, cylin=cylin, level_wise=level_wise, device=dev, decodable=True)
    if ints is None:
        qs, bin_num = enc.quantize(torch.from_numpy(xyz).to(dev))
        quant = enc.quant_info()
    else:
        qs, bin_num, quant = [torch.from_numpy(np.ascontiguousarray(ints[0], np.int32)).to(dev)], ints[1], ints[2]
    res = enc.encode_ints(qs, bin_num, len(xyz), quant=quant)
    out = enc.outfile(str(tmp_path / stem), res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    write_sidecar(out, enc, res, "OctAttention")
    return out, res, qs[0]


def _five_frames(model, dev, tmp_path):
    """Five small frames of different sizes and modes: --spher, --cylin, Cartesian, level_wise, --type obj."""
    from scp_amd.cli import obj_ints
    from scp_amd.synth import synth_frame
    frames = [_encode(model, dev, tmp_path, "a", synth_frame(5)[::150].copy(), 9, spher=True),
              _encode(model, dev, tmp_path, "b", synth_frame(4)[::240].copy(), 10, cylin=True),
              _encode(model, dev, tmp_path, "c", synth_frame(3)[::100].copy(), 8),
              _encode(model, dev, tmp_path, "d", synth_frame(2)[::200].copy(), 9, spher=True, level_wise=True)]
    xyz = (synth_frame(5)[::400] * 2).astype(np.float32)
    q, off = obj_ints(xyz, "frame", dev)
    frames.append(_encode(model, dev, tmp_path, "e", xyz, 12, ints=(q.cpu().numpy(), 0.0, [dict(qs=[1.0, 1.0, 1.0], offset=off)]), data_type="obj"))
    return frames


def _same(a, b):
    return torch.equal(a["codes"][0], b["codes"][0]) and torch.equal(a["leaves"][0], b["leaves"][0]) and torch.equal(a["points"], b["points"])


def test_round_trip_five_frames_on_three_slots(model, dev, tmp_path):
    """Five frames decoded together with streams=3 (two slots are refilled; the last steps run with one active slot): per frame the
    decoded codes = the encoder's symbols, the leaves = the encoder's distinct integers, and every logits row the decoder computed =
    the encoder's table row, bit for bit - the rows are recorded on the device by wrappers of OctAttnBatchStepper.unknown and
    OctAttnLockstep.step (which row of which call is which node of which file).  Two of the frames decode to the one-stream decoder's
    codes, leaves and points; streams=1 and streams=8 (more slots than files) give the same results."""
    import time
    from scp_amd.decoder import OctAttnLockstep, decode_octattn_file, decode_octattn_files
    from scp_amd.models.oct_attention import OctAttnBatchStepper
    frames = _five_frames(model, dev, tmp_path)
    files = [f[0] for f in frames]
    nodes = [f[1]["n_nodes"] for f in frames]
    print("nodes per frame:", nodes)
    assert len(set(nodes)) == 5
    unknown, step = OctAttnBatchStepper.unknown, OctAttnLockstep.step
    calls, visits = [], []

    def rec_unknown(self, slot_ids, ctx, pos):
        logits = unknown(self, slot_ids, ctx, pos)
        calls.append(logits)
        return logits

    def rec_step(self):
        rows = step(self)
        visits.append([(f, i, self.L[s]) for s, f, i, *_ in rows])
        return rows

    OctAttnBatchStepper.unknown, OctAttnLockstep.step = rec_unknown, rec_step
    t0 = time.perf_counter()
    try:
        got = decode_octattn_files(files, model, streams=3, device=dev)
    finally:
        OctAttnBatchStepper.unknown, OctAttnLockstep.step = unknown, step
    torch.cuda.synchronize()
    wall3 = time.perf_counter() - t0
    assert not model.decodable
    assert len(calls) == len(visits) and [c.shape[0] for c in calls] == [len(v) for v in visits]
    assert max(len(v) for v in visits) == 3 and len(visits[-1]) == 1
    allrows = torch.cat(calls)
    where = [[] for _ in files]
    k = 0
    for v in visits:
        for f, _, _ in v:
            where[f].append(k)
            k += 1
    for f, (out, res, q) in enumerate(frames):
        table = res["_debug"]["table"]
        assert len(where[f]) == table.shape[0] == res["n_nodes"], f
        rows = allrows.index_select(0, torch.tensor(where[f], device=dev))
        bad = (rows != table).any(1).nonzero().flatten()[:10].tolist()
        assert torch.equal(rows, table), f"file {f}: decoder logits rows differing from the encoder's: {bad}"
        sym = res["_debug"]["sym_coded"].cpu().numpy().astype(np.int64)
        assert np.array_equal(got[f]["codes"][0].cpu().numpy().astype(np.int64) - 1, sym), f
        uniq = np.unique(q.cpu().numpy().astype(np.int64), axis=0)
        leaves = got[f]["leaves"][0].cpu().numpy()
        assert np.array_equal(np.unique(leaves, axis=0), uniq) and len(leaves) == len(uniq), f
    t0 = time.perf_counter()
    for f in (1, 3):
        assert _same(got[f], decode_octattn_file(files[f], model, dev)), f
    wall_single = time.perf_counter() - t0
    t0 = time.perf_counter()
    one = decode_octattn_files(files, model, streams=1, device=dev)
    wall1 = time.perf_counter() - t0
    many = decode_octattn_files(files, model, streams=8, device=dev)
    for f in range(5):
        assert _same(got[f], one[f]) and _same(got[f], many[f]), f
    print(f"streams=3: {wall3:.1f} s for {sum(nodes)} nodes in {len(visits)} steps; streams=1: {wall1:.1f} s; the one-stream decoder on "
          f"frames 1 and 3 ({nodes[1] + nodes[3]} nodes): {wall_single:.1f} s")
    parity_record("octattn_lockstep/five_frames", nodes=sum(nodes), steps_streams3=len(visits), wall_streams3=wall3, wall_streams1=wall1)


def test_batch_decoder_errors_name_the_file(model, dev, tmp_path):
    """A side-info file that claims fewer / more nodes than the stream's tree holds: ScpError naming that file; a refused file in the
    batch is refused before anything is decoded."""
    import json
    from scp_amd import native
    from scp_amd.decoder import SIDECAR, decode_octattn_files
    from scp_amd.models.oct_attention import OctAttnBatchStepper
    from scp_amd.synth import synth_frame
    a = _encode(model, dev, tmp_path, "a", synth_frame(1)[::600].copy(), 7, spher=True)
    b = _encode(model, dev, tmp_path, "b", synth_frame(2)[::600].copy(), 7, spher=True)
    side = json.load(open(b[0] + SIDECAR))
    for delta, what in ((-3, "more than"), (3, "decoded")):
        json.dump(dict(side, n_nodes=side["n_nodes"] + delta), open(b[0] + SIDECAR, "w"))
        with pytest.raises(native.ScpError, match=what) as e:
            decode_octattn_files([a[0], b[0]], model, streams=2, device=dev)
        assert os.path.basename(b[0]) in str(e.value)
    json.dump(dict(side, sequential=True), open(b[0] + SIDECAR, "w"))
    made = []
    init = OctAttnBatchStepper.__init__
    OctAttnBatchStepper.__init__ = lambda self, *x: made.append(1) or init(self, *x)
    try:
        with pytest.raises(native.ScpError, match="--sequential") as e:
            decode_octattn_files([a[0], b[0]], model, streams=2, device=dev)
    finally:
        OctAttnBatchStepper.__init__ = init
    assert os.path.basename(b[0]) in str(e.value) and not made


def test_cli_decode_with_and_without_streams(tmp_path):
    """encode.py --decodable on five files, decode.py with and without --streams 4: identical .ply bytes."""
    import subprocess
    import sys
    from scp_amd.synth import synth_frame, write_kitti_bin
    srcs = []
    for i in range(5):
        src = tmp_path / f"00000{i}.bin"
        write_kitti_bin(str(src), synth_frame(i)[::(300 + 60 * i)].copy())
        srcs.append(str(src))
    out = tmp_path / "out"
    enc = [sys.executable, os.path.join(ROOT, "encode.py"), "--test_files", *srcs, "--type", "kitti", "--lidar_level", "8", "--spher",
           "--random_weights", "0", "--out_dir", str(out), "--model", "OctAttention", "--decodable"]
    r = subprocess.run(enc, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    dec = [sys.executable, os.path.join(ROOT, "decode.py"), "--test_files", *srcs, "--random_weights", "0", "--out_dir", str(out)]
    plys, lines = [], []
    for extra in ([], ["--streams", "4"]):
        r = subprocess.run(dec + extra, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        plys.append([(out / f"00000{i}.ply").read_bytes() for i in range(5)])
        lines.append([ln for ln in r.stdout.splitlines() if ln.startswith(("oct len:", str(out))) or "/5" in ln])
        for i in range(5):
            (out / f"00000{i}.ply").unlink()
    assert all(len(p) > 100 for p in plys[0]) and len(set(plys[0])) == 5
    assert plys[0] == plys[1]
    assert lines[0] == lines[1] and len(lines[0]) == 15
