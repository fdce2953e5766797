"""OctAttention decoder (-m gpu): the decodable profile (octattn/1d) is row-invariant, the KV-cached step reproduces the batched forward
bit for bit, and streams encoded with decodable=True decode back to the encoder's symbols, leaves and points."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden, parity_record
from cfgs import octattn_cfg

pytestmark = pytest.mark.gpu


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


def _windows(dev, n):
    """n different 1024-row windows of logits_octattn_c1024-style inputs: the fixture's rows, rolled and with occupancies shuffled."""
    z = golden("logits_octattn_c1024")
    data = torch.from_numpy(z["data"].astype(np.int64))
    pos = torch.from_numpy(z["pos"])
    g = torch.Generator().manual_seed(7)
    ds, ps = [], []
    for w in range(n):
        d, p = data.roll(37 * w, 0).clone(), pos.roll(37 * w, 0).clone()
        if w:
            d[:, :, 0] = torch.where(d[:, :, 0] == 255, d[:, :, 0], torch.randint(0, 255, d[:, :, 0].shape, generator=g))
        ds.append(d)
        ps.append(p)
    return torch.stack(ds).to(dev), torch.stack(ps).to(dev)


def test_decodable_rows_do_not_depend_on_later_rows_or_the_batch(dmodel, dev):
    d, p = _windows(dev, 3)
    out3 = dmodel(d, p)
    for w in range(3):
        for t in (0, 1, 31, 32, 511, 1023):
            pre = dmodel(d[w:w + 1, :t + 1], p[w:w + 1, :t + 1])
            assert torch.equal(pre[0, t], out3[w, t]), (w, t)
    assert torch.equal(dmodel(d[1:2], p[1:2])[0], out3[1])
    d96, p96 = d.repeat(32, 1, 1, 1), p.repeat(32, 1, 1, 1)
    out96 = dmodel(d96, p96)
    for w in (0, 1, 2, 50, 95):
        assert torch.equal(out96[w], out3[w % 3])
    # a tail window padded behind its last real row (the encoder's batched form) against the short window alone
    k = 300
    tail_d = torch.cat((d[2, :k], d[0, :1024 - k]))[None]
    tail_p = torch.cat((p[2, :k], torch.zeros_like(p[0, :1024 - k])))[None]
    assert torch.equal(dmodel(tail_d, tail_p)[0, :k], dmodel(d[2:3, :k], p[2:3, :k])[0])


def test_default_profile_is_unchanged_and_differs_from_the_decodable_one(model, dev):
    from scp_amd import native
    assert native.numeric_profile("OctAttention").startswith("octattn/1:")
    assert native.numeric_profile("OctAttention", decodable=True).startswith("octattn/1d:")
    d, p = _windows(dev, 1)
    a = model(d, p)
    model.decodable = True
    try:
        b = model(d, p)
    finally:
        model.decodable = False
    assert torch.equal(model(d, p), a)
    assert not torch.equal(a, b) and (a - b).abs().max() < 1e-2


def test_split_f16_gemm_rows_do_not_depend_on_m(dev):
    """The dense layers of the decodable profile: one row's bits at M = 2 and at M = 131 072."""
    from scp_amd import native, ops
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn((131072, 600), device=dev, generator=g) * 4
    w = torch.randn((1280, 600), device=dev, generator=g) * 0.05
    b = torch.randn((1280,), device=dev, generator=g)
    big = native.linear_split_f16(native.SplitActF16(x), ops._split16(w), b, cfg=1)
    for r in (0, 1, 70000, 131070):
        small = native.linear_split_f16(native.SplitActF16(x[r:r + 2].contiguous()), ops._split16(w), b, cfg=1)
        assert torch.equal(small, big[r:r + 2])
    w1 = torch.randn((300, 600), device=dev, generator=g) * 0.05
    mx_big = torch.zeros(131072, dtype=torch.int32, device=dev)
    big = native.linear_split_f16(native.SplitActF16(x), ops._split16(w1), None, native.ACT_RELU, None, row_max=mx_big)
    mx = torch.zeros(2, dtype=torch.int32, device=dev)
    small = native.linear_split_f16(native.SplitActF16(x[5:7].contiguous()), ops._split16(w1), None, native.ACT_RELU, None, row_max=mx)
    assert torch.equal(small, big[5:7]) and torch.equal(mx, mx_big[5:7])


def test_rowinv_attention_query_range_and_batch(dev):
    """The kernel alone: rows [q0, q1) of a launch equal the same rows of the full launch (and of a one-window launch)."""
    from scp_amd import native
    g = torch.Generator(device=dev).manual_seed(11)
    B, c, H, hd = 3, 700, 4, 150
    D = H * hd
    q = torch.randn((B, c, D), device=dev, generator=g)
    kv = torch.randn((2, B, c, 1280), device=dev, generator=g)
    k, v, ku, vu = kv[0, ..., :D], kv[0, ..., 640:640 + D], kv[1, ..., :D], kv[1, ..., 640:640 + D]
    o, ou = torch.empty_like(q), torch.empty_like(q)
    native.octattn_attention_rowinv(q, k, v, H, k_u=ku, v_u=vu, out=o, out_u=ou)
    # float64 evaluation of attention_model.py:58-95 for window 1
    qd, kd, vd, kud, vud = (t[1].double().reshape(c, H, hd).transpose(0, 1) for t in (q, k, v, ku, vu))
    s = qd @ kd.transpose(1, 2) / hd ** 0.5
    mask = torch.tril(torch.ones(c, c, dtype=torch.bool, device=dev))
    ref = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ vd
    su = s.clone()
    su.diagonal(dim1=1, dim2=2).copy_((qd * kud).sum(-1) / hd ** 0.5)
    pu = torch.softmax(su.masked_fill(~mask, float("-inf")), -1)
    refu = (pu * (~torch.eye(c, dtype=torch.bool, device=dev))) @ vd + pu.diagonal(dim1=1, dim2=2)[..., None] * vud
    assert (o[1].double() - ref.transpose(0, 1).reshape(c, D)).abs().max() < 1e-4
    assert (ou[1].double() - refu.transpose(0, 1).reshape(c, D)).abs().max() < 1e-4
    for q0, q1 in ((0, 1), (5, 6), (31, 97), (650, 700)):
        o2, ou2 = torch.zeros_like(q), torch.zeros_like(q)
        native.octattn_attention_rowinv(q, k, v, H, k_u=ku, v_u=vu, out=o2, out_u=ou2, q0=q0, q1=q1)
        assert torch.equal(o2[:, q0:q1], o[:, q0:q1]) and torch.equal(ou2[:, q0:q1], ou[:, q0:q1])
        # one row through offset operands (the decoder's form: q / k_u / v_u / out hold row t only)
        t = q1 - 1
        o3, ou3 = torch.empty((1, D), device=dev), torch.empty((1, D), device=dev)
        native.octattn_attention_rowinv(q[2, t:t + 1], k[2], v[2], H, k_u=ku[2, t:t + 1], v_u=vu[2, t:t + 1], out=o3, out_u=ou3, q0=t, q1=t + 1, qoff=t)
        assert torch.equal(o3[0], o[2, t]) and torch.equal(ou3[0], ou[2, t])


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "logits_octattn_*.npz"))))
def test_decodable_logits_vs_reference(dmodel, dev, name):
    z = golden(name)
    data = torch.from_numpy(z["data"].astype(np.int64))[None].to(dev)
    pos = torch.from_numpy(z["pos"])[None].to(dev)
    e = float(np.abs(dmodel(data, pos)[0].cpu().numpy() - z["out"]).max())
    parity_record(f"octattn_decodable/{name}", max_dlogit=e)
    assert e <= 1e-3


def _teacher_forced(m, dev, st=None, n=None, poison=False):
    """Teacher-forced steps over a chunk's pad-prefix window and two full windows (the first n of its 1 + 2 cs rows) -> (the stepper's
    logits rows, the batched decodable forward's).  poison: after every reset the cache rows >= t are NaN (rows the window has not
    written yet: after reset(pad=False) they still hold the previous window's values)."""
    from scp_amd.decoder import octattn_window_of
    from scp_amd.models.oct_attention import OctAttnStepper, _pad_rows
    cs = m.cfg.model.context_size
    d, p = _windows(dev, 3)
    N = 1 + 2 * cs
    ctx = torch.cat((d[0, -1:], d[1], d[2])).reshape(N, 12).to(torch.uint8)
    pos = torch.cat((p[0, -1:], p[1], p[2]))
    pc, pp = _pad_rows(cs - 1, dev)
    seq_c, seq_p = torch.cat((pc, ctx)), torch.cat((pp, pos))
    ref = m(seq_c.reshape(3, cs, 4, 3), seq_p.reshape(3, cs, 4, 3)).reshape(-1, 255)[cs - 1:]
    st = OctAttnStepper(m) if st is None else st
    rows = []
    for r in range(N if n is None else n):
        w, t = octattn_window_of(r, cs)
        if r == 0 or t == 0:
            st.reset(pad=(w == 0))
            if poison:
                st.kv[:, st.t:] = float("nan")
        assert st.t == t
        unk = ctx[r:r + 1].clone()
        unk[0, 9] = 255
        rows.append(st.unknown(unk, pos[r:r + 1]))
        st.known(ctx[r:r + 1], pos[r:r + 1])
    got = torch.cat(rows)
    return got, ref[:got.shape[0]]


def _assert_rows_equal(got, ref):
    from scp_amd import native
    bad = (got != ref).any(1).nonzero().flatten()[:10].tolist()
    assert torch.equal(got, ref), f"rows differing: {bad}"
    c1 = native.softmax_cdf(got, want_lohi=False, want_cdf=True)["cdf"]
    c2 = native.softmax_cdf(ref, want_lohi=False, want_cdf=True)["cdf"]
    assert torch.equal(c1, c2)


def test_step_equals_batched_forward(dmodel, dev):
    """Teacher-forced steps over a chunk's pad-prefix window and two full windows: every logits row and every integer CDF row equals
    the batched decodable forward's."""
    _assert_rows_equal(*_teacher_forced(dmodel, dev))


def test_step_reads_no_cache_row_at_or_after_t(dmodel, dev):
    """The same steps with NaN in every cache row >= t after each reset: the unknown pass reads rows < t only, the known pass row t only
    once it has written it - every logits row keeps its bits."""
    got, ref = _teacher_forced(dmodel, dev, poison=True)
    assert bool(torch.isfinite(got).all())
    _assert_rows_equal(got, ref)


def test_stepper_follows_weight_updates(dev):
    """The stepper's derived weights (the pad rows' K / V cache, the fused key | value weight: ops.derived) follow an in-place refill of
    the parameters, in the same stepper and in a new one.  A model of its own: the module-scoped one stays untouched."""
    from scp_amd import ops
    from scp_amd.models import OctAttention
    from scp_amd.models.oct_attention import OctAttnStepper, _kv_cat, _pad_rows
    from scp_amd.weights import fill_weights
    m = fill_weights(OctAttention(octattn_cfg(), decodable=True), 0).to(dev)
    n = 1 + 64                                        # the pad window's row and the next window's first 64 rows
    st = OctAttnStepper(m)
    got0, ref0 = _teacher_forced(m, dev, st, n)
    _assert_rows_equal(got0, ref0)
    lyr = m.transformer_encoder.layers[0]
    pad0, kv0 = st.prefill_pad(), st._kv(lyr)
    fill_weights(m, 1)
    got1, ref1 = _teacher_forced(m, dev, st, n)
    assert not torch.equal(ref1, ref0)
    _assert_rows_equal(got1, ref1)
    _assert_rows_equal(*_teacher_forced(m, dev, OctAttnStepper(m), n))
    pad1, kv1 = st.prefill_pad(), st._kv(lyr)
    cap = []
    pc, pp = _pad_rows(m.cfg.model.context_size - 1, dev)
    m(pc.reshape(1, -1, 4, 3), pp.reshape(1, -1, 4, 3), capture_kv=cap)
    assert not torch.equal(pad1, pad0) and torch.equal(pad1, torch.stack([k[0] for k in cap]))
    w, b = _kv_cat(lyr.attn, m.embed_dimension)
    assert not torch.equal(kv1[0], kv0[0]) and torch.equal(kv1[0], w) and torch.equal(kv1[1], b)
    fill_weights(m, 2)
    with ops.frozen_weights():                        # the decoder's frame scope validates each derived weight at its first use
        got2, ref2 = _teacher_forced(m, dev, st, n)
    _assert_rows_equal(got2, ref2)
    assert not torch.equal(ref2, ref1)


def _round_trip(model, dev, tmp_path, xyz, level, spher=False, cylin=False, level_wise=False, stem="f", ints=None, data_type="kitti"):
    """Encode decodable, write stream + side-info, decode.  ints = (integers [P, 3], bin_num, quant) given from outside, else the encoder
    quantises.  Checks: every logits row the decoder computes = the encoder's row (and so every integer CDF row), decoded codes = the
    encoder's symbols, leaves = the encoder's distinct integers, and every ORIGINAL point lies within its quantisation cell's error bound
    of the decoded point of its leaf (an independent check of the de-quantisation: offsets, steps, the cylindrical z offset)."""
    from scp_amd import native
    from scp_amd.decoder import decode_octattn_file, write_sidecar
    from scp_amd.encoder import OctAttnFrameEncoder
    enc = OctAttnFrameEncoder(model, data_type, level, spher=spher, cylin=cylin, level_wise=level_wise, device=dev, decodable=True)
    if ints is None:
        qs, bin_num = enc.quantize(torch.from_numpy(xyz).to(dev))
        quant = enc.quant_info()
    else:
        qs, bin_num, quant = [torch.from_numpy(np.ascontiguousarray(ints[0], np.int32)).to(dev)], ints[1], ints[2]
    res = enc.encode_ints(qs, bin_num, len(xyz), quant=quant)
    assert not model.decodable                      # the encoder restores the model's own profile
    out = enc.outfile(str(tmp_path / stem), res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    side = write_sidecar(out, enc, res, "OctAttention")
    assert side["profile"].startswith("octattn/1d:") and side["context_size"] == 1024 and side["level_wise"] == level_wise
    # every logits row the decoder computes, recorded on the device (no host sync per node) by a wrapper of OctAttnStepper.unknown for
    # the length of the decode: the range decoder reads only the CDF entries around each symbol, so decoded symbols alone do not show
    # that the decoder's CDF rows are the encoder's
    from scp_amd.models.oct_attention import OctAttnStepper
    table = res["_debug"]["table"]
    rows = torch.empty_like(table)
    seen = [0]
    unknown = OctAttnStepper.unknown

    def record(self, ctx, pos):
        logits = unknown(self, ctx, pos)
        if seen[0] < rows.shape[0]:
            rows[seen[0]].copy_(logits[0])
        seen[0] += 1
        return logits

    OctAttnStepper.unknown = record
    try:
        got = decode_octattn_file(out, model, dev)
    finally:
        OctAttnStepper.unknown = unknown
    assert seen[0] == table.shape[0] == res["n_nodes"]
    bad = (rows != table).any(1).nonzero().flatten()[:10].tolist()
    assert torch.equal(rows, table), f"decoder logits rows differing from the encoder's: {bad}"
    cdf = lambda t: native.softmax_cdf(t, want_lohi=False, want_cdf=True)["cdf"]
    assert torch.equal(cdf(rows), cdf(table))
    sym = res["_debug"]["sym_coded"].cpu().numpy().astype(np.int64)
    assert np.array_equal(got["codes"][0].cpu().numpy().astype(np.int64) - 1, sym)
    q = qs[0].cpu().numpy().astype(np.int64)
    uniq = np.unique(q, axis=0)
    leaves = got["leaves"][0].cpu().numpy()
    assert np.array_equal(np.unique(leaves, axis=0), uniq) and len(leaves) == len(uniq)
    # the decoded point of every original point's leaf, against the original point
    key = lambda a: (a[:, 0] << 42) | (a[:, 1] << 21) | a[:, 2]
    kl = key(leaves)
    order = np.argsort(kl)
    idx = order[np.searchsorted(kl[order], key(q))]
    assert np.array_equal(leaves[idx], q)
    pts = got["points"].cpu().numpy()[idx]
    x = xyz.astype(np.float64)
    step = float(quant[0]["qs"][0])
    err = np.abs(pts - x)
    slack = 1e-3
    if spher or cylin:
        r = np.linalg.norm(x[:, :2] if cylin else x, axis=1)
        dang = 2 * np.pi / (bin_num - 1)
        assert (np.linalg.norm(err, axis=1) <= 0.5 * step * 1.8 + r * dang + slack).all()
        if cylin:                                   # z is quantised on its own: half a step at most
            assert err[:, 2].max() <= 0.5 * step + slack, err[:, 2].max()
    else:
        assert err.max() <= 0.5 * step + slack, err.max()
    return res, got


@pytest.mark.parametrize("mode", ["spher", "cylin", "cart", "spher_level_wise"])
def test_round_trip_small_frames(model, dev, tmp_path, mode):
    from scp_amd.synth import synth_frame
    xyz = synth_frame(5)[::12].copy()
    _round_trip(model, dev, tmp_path, xyz, 10, spher=mode.startswith("spher"), cylin=mode == "cylin", level_wise=mode.endswith("level_wise"))


def test_round_trip_obj_frame(model, dev, tmp_path):
    """--type obj as encode.py runs it (qs 1, the frame's per-axis minimum as offset, carried by the side-info's `quant`)."""
    from scp_amd.cli import obj_ints
    from scp_amd.synth import synth_frame
    xyz = (synth_frame(5)[::60] * 2).astype(np.float32)
    q, off = obj_ints(xyz, "frame", dev)
    _round_trip(model, dev, tmp_path, xyz, 12, ints=(q.cpu().numpy(), 0.0, [dict(qs=[1.0, 1.0, 1.0], offset=off)]), data_type="obj")


def test_round_trip_golden_e2e_frame(model, dev, tmp_path):
    """The e2e_octattn_spher_L12 fixture (the reference's coded symbols): encoded decodable, decoded back to the reference's symbols."""
    from scp_amd.models import OctAttention
    from scp_amd.weights import fill_weights
    z = golden("e2e_octattn_spher_L12")
    m = fill_weights(OctAttention(octattn_cfg()), int(z["wseed"])).to(dev)
    from oracle import scp_oracle as orc
    _, bin_num, _, _, pt = orc.quantise(z["xyz"], 400 / (2 ** 12 - 1), "spher")      # the reference's integers (as test_gpu_e2e does)
    quant = [dict(qs=[400 / (2 ** 12 - 1), 2 * np.pi / (bin_num - 1), np.pi / (bin_num - 1)], offset=[0.0, 0.0, 0.0])]
    res, got = _round_trip(m, dev, tmp_path, z["xyz"].astype(np.float32), 12, spher=True, ints=(np.ascontiguousarray(pt, np.int32), bin_num, quant))
    assert res["n_nodes"] == int(z["n_nodes"])
    assert np.array_equal(got["codes"][0].cpu().numpy().astype(np.int16) - 1, z["sym_coded"])


def test_default_profile_stream_is_refused(model, dev, tmp_path):
    from scp_amd import native
    from scp_amd.decoder import decode_octattn_file, write_sidecar
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.synth import synth_frame
    enc = OctAttnFrameEncoder(model, "kitti", 8, spher=True, device=dev)
    res = enc.encode(synth_frame(1)[::200].copy())
    out = enc.outfile(str(tmp_path / "d"), res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    with pytest.raises(native.ScpError, match="--decodable"):
        decode_octattn_file(out, model, dev)
    write_sidecar(out, enc, res, "OctAttention")
    with pytest.raises(native.ScpError, match="--decodable"):
        decode_octattn_file(out, model, dev)


def test_cli_encode_decodable_then_decode(tmp_path):
    import subprocess
    import sys
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.synth import synth_frame, write_kitti_bin
    xyz = synth_frame(2)[::30].copy()
    src = tmp_path / "000007.bin"
    write_kitti_bin(str(src), xyz)
    out = tmp_path / "out"
    enc = [sys.executable, os.path.join(ROOT, "encode.py"), "--test_files", str(src), "--type", "kitti", "--lidar_level", "10", "--spher",
           "--random_weights", "0", "--out_dir", str(out), "--model", "OctAttention"]
    r = subprocess.run(enc + ["--decodable"], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out / "000007.bin").exists() and (out / "000007.bin.scp.json").exists()
    dec = [sys.executable, os.path.join(ROOT, "decode.py"), "--test_files", str(src), "--random_weights", "0", "--out_dir", str(out)]
    r = subprocess.run(dec, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ply = out / "000007.ply"
    assert ply.exists()
    from scp_amd import native
    q, _, _ = native.quantize(torch.from_numpy(xyz).cuda(), native.SPHER, 400 / (2 ** 10 - 1))
    n_unique = len(np.unique(q.cpu().numpy(), axis=0))
    assert len(pointCloud.ptread(str(ply))) == n_unique
    # a default-profile stream: refused with the re-encode hint, no .ply written
    out2 = tmp_path / "out2"
    r = subprocess.run(enc[:-2] + ["--out_dir", str(out2), "--model", "OctAttention"], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (out2 / "000007.bin.scp.json").exists()
    r = subprocess.run(dec[:-2] + ["--out_dir", str(out2)], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode != 0 and "--decodable" in r.stderr
    assert not (out2 / "000007.ply").exists()


def _full_frame(tmp):
    """The full-frame round trip, run in a child process (test_round_trip_full_l12_frame gives it its own time limit)."""
    import pathlib
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    m = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    res, got = _round_trip(m, dev, pathlib.Path(tmp), synth_frame(0), 12, spher=True)
    assert res["n_nodes"] == got["codes"][0].numel() > 100000
    print("full frame ok:", res["n_nodes"], "nodes")


def test_round_trip_full_l12_frame(tmp_path):
    """One full synthetic frame at L12 --spher (115 568 nodes; about 270 s of decoding), in a child process under its
    own time limit of 900 s."""
    import subprocess
    import sys
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            f"import test_gpu_octattn_decode as t; t._full_frame({str(tmp_path)!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "full frame ok" in r.stdout
