"""Rate report on the device (csrc/rate.hip) against the float64 reference (rate_ref.py): rows, segment sums and their bit-for-bit
reproducibility, bad pairs, the encoders' `rate` entry on every entry point, the CLI flag."""
import json
import math
import os

import numpy as np
import pytest
import torch

import rate_ref
from cfgs import ehem_cfg, octattn_cfg

pytestmark = pytest.mark.gpu

N_ALL = 5200
ROW_IDEAL_TOL = 1e-9      # bits.  float32 inputs with |x| <= 1e4, float64 differences and sums, exp / log good to a few ulp: the error is
ROW_TABLE_TOL = 1e-12     # near 1e-13 (an ulp of 1.4e4 is 1.8e-12 ... of 16 is 3.6e-15); the bounds leave orders of margin


def _make_rows(n, seed=3):
    """Logit rows of every kind, by row index mod 8: 0 flat (zeros), 1 random, 2 peaked on the symbol, 3 peaked AWAY from it at scale 1e4
    (the float32 softmax of the symbol underflows: width 1, 16 table bits, ~1.4e4 ideal bits), 4 symbol 0, 5 symbol 254 (c_high stored
    as 0), 6 an exact tie of the symbol with the maximum, 7 random at scale 8."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 255)).astype(np.float32)
    sym = rng.integers(0, 255, n).astype(np.uint8)
    k = np.arange(n) % 8
    r = np.arange(n)
    x[k == 0] = 0.0
    x[r[k == 2], sym[k == 2]] += 20.0
    other = ((sym.astype(np.int64) + 1 + rng.integers(0, 253, n)) % 255)
    x[r[k == 3], other[k == 3]] = 1e4
    sym[k == 4] = 0
    sym[k == 5] = 254
    top = x.max(1) + 1.0
    x[r[k == 6], sym[k == 6]] = top[k == 6]
    x[r[k == 6], other[k == 6]] = top[k == 6]
    x[k == 7] *= 8.0
    return x, sym


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def table(dev):
    """The shared rows: logits / symbols on the host, the device copies under the three row strides, the pairs native.softmax_cdf makes of
    them, and the reference's row values - computed once, never modified."""
    from scp_amd import native
    x, sym = _make_rows(N_ALL)
    d = {}
    for ld in (255, 256, 300):
        buf = torch.zeros((N_ALL, ld), dtype=torch.float32, device=dev)
        buf[:, :255] = torch.from_numpy(x).to(dev)
        d[ld] = buf[:, :255]
    sym_d = torch.from_numpy(sym).to(dev)
    lohi = native.softmax_cdf(d[255], sym_d)["lohi"]
    for ld in (256, 300):
        assert torch.equal(native.softmax_cdf(d[ld], sym_d)["lohi"], lohi)
    ref = rate_ref.rows(x, sym, lohi.cpu().numpy())
    assert not ref["bad"].any()
    return dict(x=x, sym=sym, dev=d, sym_d=sym_d, lohi=lohi, ref=ref)


def _run(t, ld, a, b, seg_off, want_rows=False, lohi=None):
    from scp_amd import native
    r = native.rate_segments(t["dev"][ld][a:b], t["sym_d"][a:b], (t["lohi"] if lohi is None else lohi)[a:b], seg_off, want_rows=want_rows)
    torch.cuda.synchronize()
    return r


def _check_segments(raw, ref, a, seg_off):
    """raw: host records [S,5] of segments seg_off (relative to row a of the shared table)"""
    want = rate_ref.segments({k: v[a:] for k, v in ref.items()}, seg_off)
    f = raw.view(np.float64)
    assert np.isfinite(f[:, 1:3]).all()
    for i, (rows, ideal, tab, top1, bad) in enumerate(want):
        assert raw[i, 0] == rows and raw[i, 3] == top1 and raw[i, 4] == bad, (i, raw[i], want[i])
        assert abs(f[i, 1] - ideal) <= rate_ref.segment_tolerance(rows, ideal), (i, f[i, 1], ideal)
        assert abs(f[i, 2] - tab) <= rate_ref.segment_tolerance(rows, tab), (i, f[i, 2], tab)


@pytest.mark.parametrize("ld", [255, 256, 300])
def test_rows_against_the_float64_reference(table, ld):
    ref = table["ref"]
    for n in (0, 1, 63, 64, 65, 257, 1000):
        r = _run(table, ld, 0, n, [0, n], want_rows=True)
        raw = r["raw"].cpu().numpy()
        if n == 0:
            assert np.array_equal(raw, np.zeros((1, 5), np.int64))
            continue
        ideal, tab = r["row_ideal"].cpu().numpy(), r["row_table"].cpu().numpy()
        assert np.isfinite(ideal).all() and np.isfinite(tab).all()
        err_i, err_t = np.abs(ideal - ref["ideal"][:n]).max(), np.abs(tab - ref["table"][:n]).max()
        print(f"ld {ld} n {n}: max |ideal - ref| {err_i:.3e}  max |table - ref| {err_t:.3e}")
        assert err_i <= ROW_IDEAL_TOL and err_t <= ROW_TABLE_TOL
        assert np.array_equal(np.rint(np.exp2(16.0 - tab)).astype(np.int64), ref["width"][:n])       # the width the table bits imply
        assert raw[0, 0] == n and raw[0, 3] == int(ref["top1"][:n].sum()) and raw[0, 4] == 0
        _check_segments(raw, ref, 0, [0, n])
    # what the row kinds are there for
    k = np.arange(1000) % 8
    r = _run(table, ld, 0, 1000, [0, 1000], want_rows=True)
    ideal, tab = r["row_ideal"].cpu().numpy(), r["row_table"].cpu().numpy()
    want_flat = math.log2(255.0)
    assert np.all(np.abs(ideal[k == 0] - want_flat) <= np.spacing(want_flat))
    assert np.all(tab[k == 3] == 16.0) and np.all(ref["width"][:1000][k == 3] == 1) and np.all(np.abs(ideal[k == 3] - 1e4 / math.log(2.0)) < 10.0)
    assert ref["top1"][:1000][k == 6].all() and ref["top1"][:1000][k == 0].all()
    # one-row segments: every row's own top1 flag, exactly
    n = 257
    raw = _run(table, ld, 0, n, list(range(n + 1)))["raw"].cpu().numpy()
    assert np.array_equal(raw[:, 3], ref["top1"][:n].astype(np.int64)) and np.all(raw[:, 0] == 1)
    assert np.array_equal(raw.view(np.float64)[:, 1], ideal[:n]) and np.array_equal(raw.view(np.float64)[:, 2], tab[:n])


LAYOUTS = {"one": [0, 1000], "single rows": list(range(66)), "empty first / middle / last": [0, 0, 10, 10, 10, 300, 1000, 1000],
           "63 / 64 / 65": [0, 63, 127, 192, 255, 256, 321], "5000 rows": [0, 5000]}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_segment_sums_and_their_bits(table, name):
    off = LAYOUTS[name]
    got = {}
    for ld in (255, 256):
        raw = _run(table, ld, 0, off[-1], off)["raw"].cpu().numpy()
        _check_segments(raw, table["ref"], 0, off)
        again = _run(table, ld, 0, off[-1], off)["raw"].cpu().numpy()
        assert np.array_equal(raw, again)                              # two runs: identical bits
        got[ld] = raw
    assert np.array_equal(got[255], got[256])                          # either row stride: identical bits
    # the same rows at another table offset, other segments in front: identical bits
    shift = 137
    for ld in (255, 256):
        moved = _run(table, ld, shift, shift + off[-1], off)["raw"].cpu().numpy()
        inside = _run(table, ld, 0, shift + off[-1], [0, 5, 64, shift] + [shift + o for o in off[1:]])["raw"].cpu().numpy()
        assert np.array_equal(inside[3:], moved)
        _check_segments(moved, table["ref"], shift, off)


def test_bad_pairs_are_counted_and_kept_out_of_the_sums(table):
    n = 130
    lohi = table["lohi"][:n].clone()
    for r, (lo, hi) in {3: (5, 5), 64: (10, 7), 129: (0, 0)}.items():     # width 0, negative width; (0, stored 0) is the full range: fine
        lohi[r] = lo | (hi << 16)
    res = _run(table, 256, 0, n, [0, 64, n], want_rows=True, lohi=lohi)
    ref = rate_ref.rows(table["x"][:n], table["sym"][:n], lohi.cpu().numpy())
    assert ref["bad"].sum() == 2 and ref["width"][129] == 65536
    raw = res["raw"].cpu().numpy()
    ideal, tab = res["row_ideal"].cpu().numpy(), res["row_table"].cpu().numpy()
    assert np.isfinite(ideal).all() and np.isfinite(tab).all() and np.isfinite(raw.view(np.float64)[:, 1:3]).all()
    assert ideal[3] == 0 and tab[3] == 0 and ideal[64] == 0 and tab[64] == 0 and tab[129] == 0.0
    assert raw[:, 4].tolist() == [1, 1] and raw[:, 0].tolist() == [64, 66]
    _check_segments(raw, ref, 0, [0, 64, n])


# ------------------------------------------------------------------------------------------------------------------ encoders
def _check_rate(res):
    rate = res["rate"]
    assert [lv["nodes"] for lv in rate["levels"]] == list(res["level_sizes"])
    assert rate["bad_rows"] == 0
    assert 0 < res["bits"] - rate["table_bits"] <= 16 and rate["coder_overhead_bits"] == res["bits"] - rate["table_bits"]
    assert rate["bpp_ideal"] == rate["ideal_bits"] / res["n_points"] and rate["bpp_table"] == rate["table_bits"] / res["n_points"]
    assert rate["bits_per_node_ideal"] == rate["ideal_bits"] / res["n_nodes"]
    assert abs(math.fsum(lv["ideal_bits"] for lv in rate["levels"]) - rate["ideal_bits"]) <= rate_ref.segment_tolerance(res["n_nodes"], rate["ideal_bits"])
    assert abs(math.fsum(lv["table_bits"] for lv in rate["levels"]) - rate["table_bits"]) <= rate_ref.segment_tolerance(res["n_nodes"], rate["table_bits"])
    for lv in rate["levels"]:
        assert 0 <= lv["top1"] <= lv["nodes"] and lv["table_bits"] >= 0 and lv["ideal_bits"] >= 0
        if "phase1" in lv:
            a, b = lv["phase1"], lv["phase2"]
            assert a["nodes"] + b["nodes"] == lv["nodes"] and a["top1"] + b["top1"] == lv["top1"] and a["nodes"] - b["nodes"] >= 0
            for k in ("ideal_bits", "table_bits"):
                assert abs(a[k] + b[k] - lv[k]) <= rate_ref.segment_tolerance(lv["nodes"], lv[k])


def _check_against_reference_rows(res):
    """the report's totals against the reference on the frame's own table (the synchronous call keeps it in `_debug`)"""
    from scp_amd import native
    tab, sym = res["_debug"]["table"], res["_debug"]["sym_coded"]
    lohi = native.softmax_cdf(tab, sym)["lohi"].cpu().numpy()
    ref = rate_ref.rows(tab.cpu().numpy(), sym.cpu().numpy(), lohi)
    n = len(lohi)
    assert abs(math.fsum(ref["ideal"]) - res["rate"]["ideal_bits"]) <= rate_ref.segment_tolerance(n, res["rate"]["ideal_bits"])
    assert abs(math.fsum(ref["table"]) - res["rate"]["table_bits"]) <= rate_ref.segment_tolerance(n, res["rate"]["table_bits"])
    assert sum(lv["top1"] for lv in res["rate"]["levels"]) == int(ref["top1"].sum())


@pytest.mark.parametrize("mullevel,level", [(False, 12), (True, 14)])
def test_ehem_encoders_report_the_rate_on_every_entry_point(dev, mullevel, level):
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev)
    frames = [synth_frame(s)[::30].copy() for s in (4, 5)]
    plain = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev)
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev, rate=True)
    want = [plain.encode(f) for f in frames]
    assert all("rate" not in w for w in want)
    sync = [enc.encode(f) for f in frames]
    assert [s["bytes"] for s in sync] == [w["bytes"] for w in want]
    for s in sync:
        _check_rate(s)
        assert all("phase1" in lv and "phase2" in lv for lv in s["rate"]["levels"])
        _check_against_reference_rows(s)
    hs = [enc.encode_async(f) for f in frames]
    asy = [enc.finish(h) for h in hs]
    assert [a["bytes"] for a in asy] == [w["bytes"] for w in want]
    assert [a["rate"] for a in asy] == [s["rate"] for s in sync]            # bit-identical entries
    bat = enc.finish_batch(enc.encode_batch_async(frames))
    assert [b["bytes"] for b in bat] == [w["bytes"] for w in want]
    assert [b["rate"] for b in bat] == [s["rate"] for s in sync]
    hq, infos = enc.host_ints(frames[0])
    qs = [torch.from_numpy(np.ascontiguousarray(q)).to(dev) for q in hq]
    ints = enc.encode_ints(qs, infos[0].bin_num, 0.0, frames[0].shape[0])
    _check_rate(ints)
    json.dumps(sync[0]["rate"])                                               # plain numbers only


def test_octattn_encoder_reports_the_rate(dev):
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    xyz = synth_frame(6)[::30].copy()
    want = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev).encode(xyz)
    enc = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev, rate=True)
    sync = enc.encode(xyz)
    assert "rate" not in want and sync["bytes"] == want["bytes"]
    _check_rate(sync)
    assert all("phase1" not in lv for lv in sync["rate"]["levels"])
    _check_against_reference_rows(sync)
    asy = enc.finish(enc.encode_async(xyz))
    assert asy["bytes"] == want["bytes"] and asy["rate"] == sync["rate"]
    lw = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev, mullevel=True, level_wise=True, rate=True).encode(xyz)
    _check_rate(lw)
    assert len(lw["rate"]["levels"]) == len(lw["level_sizes"]) > 3


def test_cli_rate_report_writes_the_json_and_leaves_the_streams_alone(tmp_path, dev):
    import subprocess
    import sys
    from conftest import ROOT
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame, write_kitti_bin
    from scp_amd.weights import fill_weights
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    outs = {}
    for flag in ([], ["--rate_report"]):
        out = tmp_path / ("out_rate" if flag else "out_plain")
        cmd = [sys.executable, os.path.join(ROOT, "encode.py"), "--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", "12",
               "--spher", "--random_weights", "0", "--out_dir", str(out)] + flag
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("bpp ideal / table / coded" in r.stdout) == bool(flag)
        if flag:
            assert r.stdout.count("bpp ideal / table / coded   :") == 2 and "bpp ideal / table / coded (mean):" in r.stdout
        outs[bool(flag)] = out
    bins = sorted(p.name for p in outs[True].iterdir() if p.name.endswith(".bin"))
    assert len(bins) == 2 and bins == sorted(p.name for p in outs[False].iterdir() if p.name.endswith(".bin"))
    assert not [p for p in outs[False].iterdir() if p.name.endswith(".rate.json")]
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev)
    enc = FrameEncoder(model, "kitti", 12, spher=True, device=dev, rate=True)
    for i, b in enumerate(bins):
        assert (outs[True] / b).read_bytes() == (outs[False] / b).read_bytes()
        rep = json.load(open(outs[True] / (b[:-len(".bin")] + ".rate.json")))
        assert rep["model"] == "EHEM" and rep["lidar_level"] == 12 and rep["profile"] == enc.profile_string()
        res = enc.encode(pointCloud.ptread(str(seq / f"{i:06d}.bin")))
        assert res["bytes"] == (outs[True] / b).read_bytes()
        for k in ("levels", "ideal_bits", "table_bits", "bad_rows", "bpp_ideal", "bpp_table", "bits_per_node_ideal", "coder_overhead_bits"):
            assert rep[k] == res["rate"][k], k
        assert rep["bits"] == res["bits"] and rep["n_points"] == res["n_points"]
