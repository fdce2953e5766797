"""Per-level temperature on the GPU (csrc/temper.hip; DESIGN.md 6, "Temperature"): the sweep against the rate kernel on scaled tables bit
for bit and against the numpy reference (tests/temper_ref.py), the row scaling against numpy's float32 product, the chooser against the
reference on the device's own sums, a table that must move, and the encoders, decoders and command lines with the option on.

On the parent commit none of this exists: every test here fails there (no symbols, no keyword arguments, no flags)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rate_ref
import temper_ref
from cfgs import ehem_cfg, octattn_cfg
from conftest import ROOT
from test_gpu_rate import ROW_IDEAL_TOL, _make_rows

pytestmark = pytest.mark.gpu

EXTRA = (0.3, 0.6, 0.9, 1.1, 1.7, 2.3, 3.0)          # not powers of two, and beyond both ends of the default grid
GRIDS = {1: np.array([1.0], np.float32), 2: np.array([0.75, 1.0], np.float32), 25: temper_ref.default_grid(),
         32: np.concatenate((temper_ref.default_grid(), np.array(EXTRA, np.float32)))}
BETA_MAX = 3.0
N_MAX = 2049


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_ROWS = {}


def rows_for(nsym):
    """test_gpu_rate._make_rows' eight kinds on an alphabet of nsym symbols (narrow alphabets: the kinds are rebuilt on the first nsym
    columns), the 1e4 rows rescaled so that |beta x| <= 1e4 for every beta used - the premise of ROW_IDEAL_TOL.  Computed once per nsym."""
    if nsym not in _ROWS:
        x, sym = _make_rows(N_MAX)
        n, r, k = len(x), np.arange(len(x)), np.arange(len(x)) % 8
        if nsym != 255:
            rng = np.random.default_rng(nsym)
            wide = rng.standard_normal((n, nsym)).astype(np.float32)
            wide[:, :min(nsym, 255)] = x[:, :min(nsym, 255)]
            x, sym = wide, (sym.astype(np.int64) % nsym).astype(np.uint8)
            other = (sym.astype(np.int64) + 1) % nsym
            x[k == 0] = 0.0
            x[k == 1] = rng.standard_normal((int((k == 1).sum()), nsym)).astype(np.float32)
            x[r[k == 2], sym[k == 2]] = 20.0
            x[r[k == 3], other[k == 3]] = 1e4
            sym[k == 4] = 0
            sym[k == 5] = nsym - 1
            top = x.max(1) + 1.0
            x[r[k == 6], sym[k == 6]] = top[k == 6]
            x[r[k == 6], (sym[k == 6].astype(np.int64) + 1) % nsym] = top[k == 6]
        x[x == np.float32(1e4)] = np.float32(1e4 / BETA_MAX)
        assert np.abs(x).max() * BETA_MAX <= 1e4 and (np.abs(x) > 3000).any() and (sym < nsym).all()
        _ROWS[nsym] = (x, sym)
    return _ROWS[nsym]


def on_device(x, ld):
    """The rows under row stride ld (columns beyond nsym hold a marker nobody may read as a logit)."""
    buf = torch.full((len(x), ld), 777.0, dtype=torch.float32, device=dev())
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(dev())
    return buf[:, :x.shape[1]]


def seg_offsets(n):
    """Empty segments, one of 1 row and - at 2049 rows - one of 1025."""
    if n >= 2049:
        return [0, 0, 1, 1, 1026, n, n]
    if n >= 3:
        return [0, 0, 1, n // 3, n // 3, n, n]
    return [0, 0, n, n]


def pairs_of_width_one(n):
    """(c_low, c_high) = (0, 1): a pair every table could hold - the rate kernel's own bad-pair rule stays out of the comparison."""
    return torch.full((n,), 1 << 16, dtype=torch.int32, device=dev())


# ------------------------------------------------------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("nsym,ld", [(s, l) for s in (2, 7, 255, 256) for l in sorted({s, 256, 300})])
def test_sweep_equals_the_rate_kernel_on_the_scaled_table_bit_for_bit(nsym, ld):
    from scp_amd import native
    x, sym = rows_for(nsym)
    tab, sym_d = on_device(x, ld), torch.from_numpy(sym).to(dev())
    sizes = (0, 1, 63, 64, 65, 257, 2049)
    for n in sizes:
        for nt in (1, 2, 25, 32):
            betas, off = GRIDS[nt], seg_offsets(n)
            r = native.temper_sweep(tab[:n], sym_d[:n], off, betas, want_rows=True)
            seg_bits, seg_bad, row_bits = r["seg_bits"].cpu().numpy(), r["seg_bad"].cpu().numpy(), r["row_bits"].cpu().numpy()
            assert seg_bits.shape == seg_bad.shape == (len(off) - 1, nt) and row_bits.shape == (n, nt)
            assert np.isfinite(seg_bits).all() and np.isfinite(row_bits).all()
            if n == 0:
                assert not seg_bits.any() and not seg_bad.any()
                continue
            ref_bits, ref_bad = temper_ref.row_bits(x[:n], sym[:n], betas)
            ref_seg, ref_segbad = temper_ref.segments(ref_bits, ref_bad, off)
            assert not ref_bad.any()
            scaled = torch.empty((n, ld), dtype=torch.float32, device=dev())[:, :nsym]
            for j, b in enumerate(betas):
                native.scale_rows(tab[:n], [0, n], [b], out=scaled)
                rr = native.rate_segments(scaled, sym_d[:n], pairs_of_width_one(n), off, want_rows=True)
                assert rr["ideal_bits"].cpu().numpy().tobytes() == seg_bits[:, j].tobytes(), (n, nt, j)
                assert np.array_equal(rr["bad_rows"].cpu().numpy(), seg_bad[:, j])
                assert rr["row_ideal"].cpu().numpy().tobytes() == row_bits[:, j].tobytes(), (n, nt, j)
            err = np.abs(row_bits - ref_bits).max()
            print(f"nsym {nsym} ld {ld} n {n} nt {nt}: max |row - ref| {err:.3e}")
            assert err <= ROW_IDEAL_TOL
            rows = np.diff(off)
            for s in range(len(rows)):
                for j in range(nt):
                    assert abs(seg_bits[s, j] - ref_seg[s, j]) <= rate_ref.segment_tolerance(rows[s], ref_seg[s, j]), (s, j)
            assert not seg_bad.any()


def test_sweep_counts_a_row_without_a_finite_cross_entropy_and_writes_nothing_non_finite():
    from scp_amd import native
    x, sym = (a.copy() for a in rows_for(255))
    x, sym = x[:300], sym[:300]
    x[7, sym[7]] = -np.inf                                  # the symbol's logit: infinite bits at every beta
    x[9] = -np.inf                                          # nothing to normalise: NaN
    x[11, (int(sym[11]) + 1) % 255] = np.inf                # inf - inf
    betas, off = GRIDS[25], [0, 8, 100, 300]
    r = native.temper_sweep(on_device(x, 256), torch.from_numpy(sym).to(dev()), off, betas, want_rows=True)
    seg_bits, seg_bad, row_bits = r["seg_bits"].cpu().numpy(), r["seg_bad"].cpu().numpy(), r["row_bits"].cpu().numpy()
    assert np.isfinite(seg_bits).all() and np.isfinite(row_bits).all()
    assert not row_bits[[7, 9, 11]].any()
    assert np.array_equal(seg_bad, np.repeat([[1], [2], [0]], 25, 1))
    ref_bits, ref_bad = temper_ref.row_bits(x, sym, betas)
    assert np.array_equal(np.flatnonzero(ref_bad.all(1)), [7, 9, 11]) and np.abs(row_bits - ref_bits).max() <= ROW_IDEAL_TOL


# ------------------------------------------------------------------------------------------------------------------ 2. scale_rows
@pytest.mark.parametrize("nsym,ld", [(255, 256), (255, 255), (255, 300), (7, 256), (256, 256), (2, 300)])
def test_scale_rows_is_numpys_float32_product_bit_for_bit(nsym, ld):
    from scp_amd import native
    x, _ = (a.copy() for a in rows_for(nsym))
    n = 1000
    x = x[:n]
    x[3, 1] = -np.inf
    x[n - 1, 0] = -np.inf
    x[5, nsym - 1] = np.float32(1e-42)                      # a subnormal
    off = [0, 0, 1, 1, 400, 400, n - 1, n, n]               # boundaries at rows 0 and n - 1, empty segments
    beta = np.array([9.0, 0.3, 9.0, 1.7, 9.0, 1.0, 2.3, 9.0], np.float32)      # (9: the empty segments' - nobody's)
    seg = np.searchsorted(np.asarray(off), np.arange(n), side="right") - 1
    want = (beta[seg][:, None] * x).astype(np.float32)
    assert want.dtype == np.float32 and np.isneginf(want[3, 1]) and want[400:n - 1].tobytes() == x[400:n - 1].tobytes()
    src = on_device(x, ld)
    out = torch.full((n, ld), 555.0, dtype=torch.float32, device=dev())
    got = native.scale_rows(src, off, beta, out=out[:, :nsym])
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert src.cpu().numpy().tobytes() == x.tobytes()                              # the input stands
    if ld > nsym:                                                                  # out of place: the columns behind the alphabet are copied
        assert (out[:, nsym:] == 777.0).all()
    # in place: the same bits, and the columns behind the alphabet are left alone
    same = native.scale_rows(src, off, beta)
    assert same.data_ptr() == src.data_ptr() and src.cpu().numpy().tobytes() == want.tobytes()
    if ld > nsym:
        base = torch.as_strided(src, (n, ld), (ld, 1))
        assert (base[:, nsym:] == 777.0).all()
    # beta = 1 returns the input bits
    again = on_device(x, ld)
    native.scale_rows(again, [0, n], [1.0])
    assert again.cpu().numpy().tobytes() == x.tobytes()
    # a row no segment holds is copied
    part = native.scale_rows(on_device(x, ld), [10, 20], [0.3], out=out[:, :nsym])
    w2 = x.copy()
    w2[10:20] = (np.float32(0.3) * x[10:20]).astype(np.float32)
    assert part.cpu().numpy().tobytes() == w2.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 3. the chooser
def _choose_and_compare(seg_bits, seg_bad, off, n, group, ngroup, betas, unit, min_gain=8.0):
    from scp_amd import native
    off_d = torch.tensor(off, dtype=torch.int64, device=dev())
    r = native.temper_choose(seg_bits, seg_bad, off_d, n, group, ngroup, betas, unit, min_gain)
    want = temper_ref.choose(seg_bits.cpu().numpy(), seg_bad.cpu().numpy(), off, group, ngroup, betas, unit, min_gain)
    choice = r["choice"].cpu().numpy()
    assert np.array_equal(choice, want["choice"]), (choice, want["choice"])
    assert r["group_bits"].cpu().numpy().tobytes() == want["group_bits"].tobytes()            # serial order: bit for bit
    assert r["seg_beta"].cpu().numpy().tobytes() == want["seg_beta"].tobytes()
    return choice, r["group_bits"].cpu().numpy()


def test_choose_equals_the_reference_on_the_devices_own_sums():
    from scp_amd import native
    x, sym = (a.copy() for a in rows_for(255))
    n = 2049
    x[1500, sym[1500]] = -np.inf                            # its group stays at unit
    betas = GRIDS[25]
    unit = 12
    off = [0, 0, 1, 64, 200, 200, 700, 1026, 1400, 1600, 2049]
    S = len(off) - 1
    sw = native.temper_sweep(on_device(x, 256), torch.from_numpy(sym).to(dev()), off, betas)
    rng = np.random.default_rng(5)
    groups = [np.arange(S) % 4, rng.permutation(np.arange(S) % 4), rng.permutation(np.arange(S) % 5), np.zeros(S, np.int64),
              np.array([0, 1, 2, 3, 99, -7, 1, 2, 3, 0])]                            # ids out of range are clamped
    for g in groups:
        for gain in (0.0, 8.0, 1e6):
            ngroup = 6 if g.max() < 6 else 4
            choice, _ = _choose_and_compare(sw["seg_bits"], sw["seg_bad"], off, n, g.astype(np.int32), ngroup, betas, unit, gain)
            bad_group = int(np.clip(g[8], 0, ngroup - 1))                            # the segment of row 1500
            assert choice[bad_group] == unit
            assert all(choice[k] == unit for k in range(ngroup) if k not in np.clip(g, 0, ngroup - 1))      # no segment, no rows: unit
            if gain == 1e6:
                assert (choice == unit).all()
    # exact ties and a gain of exactly min_gain, on made-up sums
    nt = 5
    b5 = np.array([0.5, 0.75, 1.0, 1.5, 2.0], np.float32)
    sums = np.array([[5.0, 50.0, 100.0, 50.0, 5.0], [5.0, 50.0, 100.0, 5.0, 50.0], [92.0, 95.0, 100.0, 92.0, 99.0], [91.5, 95.0, 100.0, 92.0, 99.0],
                     [7.0, 7.0, 7.0, 7.0, 7.0]])
    sb = torch.from_numpy(sums).to(dev())
    bad = torch.zeros((5, nt), dtype=torch.int32, device=dev())
    choice, gb = _choose_and_compare(sb, bad, [0, 1, 2, 3, 4, 5], 5, np.arange(5, dtype=np.int32), 5, b5, 2, 8.0)
    assert choice.tolist() == [0, 3, 2, 0, 2]
    assert gb.tolist() == [[100.0, 5.0], [100.0, 5.0], [100.0, 100.0], [100.0, 91.5], [7.0, 7.0]]
    assert sw["seg_bits"].shape == (S, 25)


# ------------------------------------------------------------------------------------------------------------------ 4. a table that must move
def test_a_table_of_overconfident_rows_moves_to_a_lower_inverse_temperature():
    """Rows of N(0, 8^2) logits whose symbols are drawn uniformly and independently of them: far too sharp a softmax for symbols it knows
    nothing about, so every group of enough rows is cheaper under beta < 1."""
    from scp_amd import native
    rng = np.random.default_rng(17)
    n = 3000
    x = (8.0 * rng.standard_normal((n, 255))).astype(np.float32)
    sym = rng.integers(0, 255, n).astype(np.uint8)
    off = [0, 3, 10, 74, 202, 702, 1500, 1500, 2400, 3000]
    group = np.array([0, 0, 1, 2, 3, 4, 4, 5, 6], np.int32)
    betas, unit = temper_ref.default_grid(), 12
    bits, bad = temper_ref.row_bits(x, sym, betas)
    seg_bits, seg_bad = temper_ref.segments(bits, bad, off)
    want = temper_ref.choose(seg_bits, seg_bad, off, group, 7, betas, unit)
    rows = np.array([int(np.diff(off)[group == g].sum()) for g in range(7)])
    big = np.flatnonzero(rows >= 64)
    assert len(big) == 6 and (want["choice"][big] < unit).all(), want["choice"]          # the premise of the last assertion below
    sw = native.temper_sweep(on_device(x, 256), torch.from_numpy(sym).to(dev()), off, betas)
    choice, gb = _choose_and_compare(sw["seg_bits"], sw["seg_bad"], off, n, group, 7, betas, unit)
    assert np.array_equal(choice, want["choice"])
    print("rows", rows.tolist(), "choice", choice.tolist(), "bits unit / chosen", gb.tolist())
    for g in big:
        assert gb[g, 1] < gb[g, 0] - 8.0


# ------------------------------------------------------------------------------------------------------------------ 5. the encoders
_MODEL = {}


def ehem_model():
    if "ehem" not in _MODEL:
        from scp_amd.models import EHEM
        from scp_amd.weights import fill_weights
        _MODEL["ehem"] = fill_weights(EHEM(ehem_cfg()), 0).to(dev())
    return _MODEL["ehem"]


def frames():
    from scp_amd.synth import synth_frame
    if "frames" not in _MODEL:
        _MODEL["frames"] = [synth_frame(s)[::30].copy() for s in (4, 5)]
    return _MODEL["frames"]


CONFIGS = [(False, 12), (True, 14)]


def _check_temper(res, mode, grid=None):
    t = res["temper"]
    grid = temper_ref.default_grid() if grid is None else np.asarray(grid, np.float32)
    assert t["mode"] == mode and t["grid"] == [float(b) for b in grid] and t["grid_u32"] == [int(b) for b in grid.view(np.uint32)]
    assert grid[t["unit"]] == 1.0 and t["side_bits"] == 8 * len(t["groups"]) and len(t["groups"]) == 2 * len(res["level_sizes"])
    assert [(g["level"], g["phase"]) for g in t["groups"]] == [(l, p) for l in range(len(res["level_sizes"])) for p in (1, 2)]
    for l, size in enumerate(res["level_sizes"]):
        assert t["groups"][2 * l]["rows"] + t["groups"][2 * l + 1]["rows"] == size
    assert t["ideal_bits_unit"] == math.fsum(g["bits_unit"] for g in t["groups"])
    assert t["ideal_bits_chosen"] == math.fsum(g["bits_chosen"] for g in t["groups"])
    assert t["moved"] == sum(g["index"] != t["unit"] for g in t["groups"])
    for g in t["groups"]:
        assert 0 <= g["index"] < len(grid) and g["bits_chosen"] <= g["bits_unit"]
        if g["index"] != t["unit"]:
            assert g["bits_unit"] - g["bits_chosen"] > 8.0
        else:
            assert g["bits_chosen"] == g["bits_unit"]
        if "sums" in g or mode == "report":
            assert len(g["sums"]) == len(grid) and g["sums"][t["unit"]] == g["bits_unit"] and g["sums"][g["index"]] == g["bits_chosen"]
            assert temper_ref.pick(g["sums"], t["unit"], 8.0, rows=g["rows"]) == g["index"]
    json.dumps(t)                                                                  # plain numbers only
    return t


@pytest.mark.parametrize("mullevel,level", CONFIGS)
def test_ehem_encoders_temper_on_every_entry_point(mullevel, level):
    from scp_amd.encoder import FrameEncoder
    kw = dict(spher=True, mullevel=mullevel, device=dev())
    model, fr = ehem_model(), frames()
    plain = FrameEncoder(model, "kitti", level, rate=True, **kw)
    want = [plain.encode(f) for f in fr]
    assert all("temper" not in w for w in want)
    # the report and a grid of 1 alone leave the bytes as they are
    rep = FrameEncoder(model, "kitti", level, temper="report", **kw)
    reps = [rep.encode(f) for f in fr]
    assert [r["bytes"] for r in reps] == [w["bytes"] for w in want]
    one = FrameEncoder(model, "kitti", level, temper="code", temper_grid=[1.0], **kw)
    ones = [one.encode(f) for f in fr]
    assert [r["bytes"] for r in ones] == [w["bytes"] for w in want]
    for r, o in zip(reps, ones):
        _check_temper(r, "report")
        _check_temper(o, "code", [1.0])
    enc = FrameEncoder(model, "kitti", level, temper="code", rate=True, **kw)
    sync = [enc.encode(f) for f in fr]
    for s, r, w in zip(sync, reps, want):
        t = _check_temper(s, "code")
        print(f"mullevel {mullevel}: moved {t['moved']} of {len(t['groups'])} groups, ideal bits {t['ideal_bits_unit']:.1f} -> "
              f"{t['ideal_bits_chosen']:.1f}, stream bits {w['bits']} -> {s['bits']}")
        # the choice is the report's, and a frame whose groups all stay is the plain stream
        assert [g["index"] for g in t["groups"]] == [g["index"] for g in r["temper"]["groups"]]
        assert [(g["bits_unit"], g["bits_chosen"]) for g in t["groups"]] == [(g["bits_unit"], g["bits_chosen"]) for g in r["temper"]["groups"]]
        if t["moved"] == 0:
            assert s["bytes"] == w["bytes"]
        # everything behind the choice sees the table that was coded: the rate report's (level, phase) is the sweep's chosen column
        assert s["rate"]["bad_rows"] == 0 and 0 < s["rate"]["coder_overhead_bits"] <= 16
        for g in t["groups"]:
            for res, key in ((s, "bits_chosen"), (w, "bits_unit")):
                ph = res["rate"]["levels"][g["level"]]["phase%d" % g["phase"]]
                assert ph["nodes"] == g["rows"]
                assert abs(ph["ideal_bits"] - g[key]) <= rate_ref.segment_tolerance(g["rows"], g[key]), (g, key, ph)
        # ... and so does _debug["table"]
        tab, sym = s["_debug"]["table"], s["_debug"]["sym_coded"]
        from scp_amd import native
        assert native.ac_encode_lohi(native.softmax_cdf(tab, sym)["lohi"].cpu().numpy()) == s["bytes"]
    asy = [enc.finish(h) for h in [enc.encode_async(f) for f in fr]]
    assert [a["bytes"] for a in asy] == [s["bytes"] for s in sync]
    assert [a["temper"] for a in asy] == [s["temper"] for s in sync]                # bit-identical entries
    assert [a["rate"] for a in asy] == [s["rate"] for s in sync]
    bat = enc.finish_batch(enc.encode_batch_async(fr))
    assert [b["bytes"] for b in bat] == [s["bytes"] for s in sync]
    assert [b["temper"] for b in bat] == [s["temper"] for s in sync]
    rbat = rep.finish_batch(rep.encode_batch_async(fr))
    assert [b["temper"] for b in rbat] == [r["temper"] for r in reps] and [b["bytes"] for b in rbat] == [w["bytes"] for w in want]
    hq, infos = enc.host_ints(fr[0])
    qs = [torch.from_numpy(np.ascontiguousarray(q)).to(dev()) for q in hq]
    ints = enc.encode_ints(qs, infos[0].bin_num, 0.0, fr[0].shape[0])
    _check_temper(ints, "code")
    # the columns of the sums are the report's by default, and a coded choice's on request (the CLIs' --temper --temper_report)
    assert all("sums" not in g for g in sync[0]["temper"]["groups"]) and all("sums" in g for g in reps[0]["temper"]["groups"])
    enc.temper_sums = True
    cols = enc.encode(fr[0])
    assert cols["bytes"] == sync[0]["bytes"]
    assert [g["sums"] for g in _check_temper(cols, "code")["groups"]] == [g["sums"] for g in reps[0]["temper"]["groups"]]
    enc.temper_sums = False
    with pytest.raises(Exception, match="exactly one value is 1.0"):
        FrameEncoder(model, "kitti", level, temper="code", temper_grid=[0.5, 2.0], **kw)
    with pytest.raises(Exception, match="'report' or 'code'"):
        FrameEncoder(model, "kitti", level, temper="yes", **kw)


# ------------------------------------------------------------------------------------------------------------------ 6. round trips
def write_stream(enc, res, stem):
    from scp_amd.decoder import write_sidecar
    out = enc.outfile(stem, res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), out + ".dat")
    write_sidecar(out, enc, res, "EHEM")
    return out


_STREAMS = {}


def streams(mullevel, level, tmp_path_factory):
    """The tempered and the plain stream of frame 0 of a configuration, written once, and the plain stream's decode."""
    from scp_amd.decoder import decode_file
    from scp_amd.encoder import FrameEncoder
    if mullevel not in _STREAMS:
        d = tmp_path_factory.mktemp("temper%d" % level)
        kw = dict(spher=True, mullevel=mullevel, device=dev())
        enc = FrameEncoder(ehem_model(), "kitti", level, temper="code", **kw)
        plain = FrameEncoder(ehem_model(), "kitti", level, **kw)
        res = enc.encode(frames()[0])
        occ = enc.geom.nodes(("occ",))["occ"]                                        # the encoder's occupancy codes, per shell
        occ = [occ[int(i.node_base):int(i.node_base + i.n_nodes)].clone() for i in enc.geom.info]
        pres = plain.encode(frames()[0])
        t_out, p_out = write_stream(enc, res, str(d / "f")), write_stream(plain, pres, str(d / "f"))
        assert os.path.basename(t_out).startswith("f_temper_spher_") and os.path.basename(p_out).startswith("f_spher_")
        _STREAMS[mullevel] = dict(res=res, pres=pres, occ=occ, t_out=t_out, p_out=p_out,
                                  want=decode_file(p_out, ehem_model(), mullevel=mullevel, device=dev()))
    return _STREAMS[mullevel]


def _same_decode(got, want):
    assert len(got["codes"]) == len(want["codes"])
    for a, b in zip(got["codes"], want["codes"]):
        assert torch.equal(a, b)
    for a, b in zip(got["leaves"], want["leaves"]):
        assert torch.equal(a, b)
    assert torch.equal(got["points"], want["points"])


@pytest.mark.parametrize("mullevel,level", CONFIGS)
def test_tempered_streams_decode_to_the_plain_streams_tree(mullevel, level, tmp_path_factory):
    from scp_amd.decoder import decode_file, decode_files
    s = streams(mullevel, level, tmp_path_factory)
    t = s["res"]["temper"]
    print(f"mullevel {mullevel}: moved {t['moved']} of {len(t['groups'])} groups; bytes {len(s['pres']['bytes'])} -> {len(s['res']['bytes'])}")
    # (with every group at 1 the two streams would be the same bytes and the round trip would show nothing)
    assert t["moved"] > 0 and s["res"]["bytes"] != s["pres"]["bytes"]
    got = decode_file(s["t_out"], ehem_model(), mullevel=mullevel, device=dev())
    _same_decode(got, s["want"])
    # the decoded occupancy codes are the encoder's, level by level (decode_file joins a shell's levels in BFS order, as the geometry
    # holds them; the last BFS node of a multi-level shell is not coded and stays 0)
    assert len(got["codes"]) == len(s["occ"]) == (3 if mullevel else 1)
    for c, occ in zip(got["codes"], s["occ"]):
        assert c.shape == occ.shape
        if mullevel:
            assert c[-1] == 0 and torch.equal(c[:-1].long(), occ[:-1].long())
        else:
            assert torch.equal(c.long(), occ.long())
    # one tempered and one plain file in lockstep: every slot its own table
    for order in ((s["t_out"], s["p_out"]), (s["p_out"], s["t_out"])):
        for out in decode_files(order, ehem_model(), streams=2, mullevel=mullevel, device=dev()):
            _same_decode(out, s["want"])
    # a preview
    a = decode_file(s["t_out"], ehem_model(), mullevel=mullevel, device=dev(), lod=2)
    b = decode_file(s["p_out"], ehem_model(), mullevel=mullevel, device=dev(), lod=2)
    assert a["lod"] == 2 and all(torch.equal(x, y) for x, y in zip(a["cells"], b["cells"])) and torch.equal(a["points"], b["points"])


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_a_tempered_stream_without_its_table_is_refused_before_anything_is_decoded(tmp_path, tmp_path_factory, monkeypatch):
    import shutil
    from scp_amd import decoder, native
    s = streams(False, 12, tmp_path_factory)
    name = str(tmp_path / os.path.basename(s["t_out"]))
    for sfx in ("", ".dat", decoder.SIDECAR):
        shutil.copy(s["t_out"] + sfx, name + sfx)
    side = json.load(open(name + decoder.SIDECAR))

    def boom(*a, **k):
        raise AssertionError("a decoder was started")
    monkeypatch.setattr(decoder.FrameDecoder, "decode", boom)
    monkeypatch.setattr(decoder.EhemBatchDecoder, "decode", boom)

    def refused(match):
        with pytest.raises(native.ScpError, match=match):
            decoder.decode_file(name, ehem_model(), device=dev())
        with pytest.raises(native.ScpError, match=match):
            decoder.decode_files([s["p_out"], name], ehem_model(), streams=2, device=dev())

    json.dump(dict(side, temper=dict(side["temper"], index=side["temper"]["index"][:-2])), open(name + decoder.SIDECAR, "w"))
    refused("indices, a stream of")
    json.dump({k: v for k, v in side.items() if k != "temper"}, open(name + decoder.SIDECAR, "w"))
    refused("no `temper` entry")
    os.remove(name + decoder.SIDECAR)
    refused("without its side-info file")


def test_octattention_reports_but_does_not_code():
    from scp_amd import native
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev())
    with pytest.raises(native.ScpError, match="one node per step"):
        OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev(), temper="code")
    xyz = synth_frame(6)[::30].copy()
    want = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev()).encode(xyz)
    enc = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev(), mullevel=True, level_wise=True, temper="report")
    lw_plain = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev(), mullevel=True, level_wise=True).encode(xyz)
    lw = enc.encode(xyz)
    t = lw["temper"]
    assert lw["bytes"] == lw_plain["bytes"] and len(t["groups"]) == len(lw["level_sizes"]) > 3 and t["side_bits"] == 8 * len(t["groups"])
    assert [g["rows"] for g in t["groups"]] == list(lw["level_sizes"]) and all(g["phase"] is None for g in t["groups"])
    assert all(g["bits_chosen"] <= g["bits_unit"] for g in t["groups"])
    asy = enc.finish(enc.encode_async(xyz))
    assert asy["bytes"] == lw["bytes"] and asy["temper"] == t
    one = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev(), temper="report").encode(xyz)
    assert one["bytes"] == want["bytes"] and len(one["temper"]["groups"]) == 1 and "temper" not in want


# ------------------------------------------------------------------------------------------------------------------ 8. command lines
LINE = "temper bpp unit / chosen, side bits, moved :"


def run_cli(tmp_path, script, seq, tag, flags):
    out = tmp_path / ("out_" + tag)
    cmd = [sys.executable, os.path.join(ROOT, script), "--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", "12",
           "--spher", "--random_weights", "0", "--out_dir", str(out)] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stdout


def two_frames(tmp_path):
    from scp_amd.synth import synth_frame, write_kitti_bin
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    return seq


def test_cli_temper_report_writes_the_json_and_leaves_the_streams_alone(tmp_path):
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.decoder import SIDECAR
    from scp_amd.encoder import FrameEncoder
    seq = two_frames(tmp_path)
    mrep, mrep_out = run_cli(tmp_path, "encode_mullevel.py", seq, "mrep", ["--temper_report"])
    assert mrep_out.count(LINE) == 2
    names = sorted(p.name for p in mrep.iterdir())
    docs = [f for f in names if f.endswith(".temper.json")]
    bins = [f for f in names if f.endswith(".bin")]
    assert len(docs) == len(bins) == 2 and not [f for f in names if "_temper" in f]
    assert [d[:-len(".temper.json")] + ".bin" for d in docs] == bins
    kw = dict(spher=True, mullevel=True, device=dev())
    plain = FrameEncoder(ehem_model(), "kitti", 12, **kw)
    menc = FrameEncoder(ehem_model(), "kitti", 12, temper="report", **kw)
    for i, (d, b) in enumerate(zip(docs, bins)):
        doc = json.load(open(mrep / d))
        xyz = pointCloud.ptread(str(seq / f"{i:06d}.bin"))
        res, want = menc.encode(xyz), plain.encode(xyz)
        # the stream, its name and its side-info file are those of an encoder without the option
        assert (mrep / b).read_bytes() == want["bytes"] == res["bytes"] and str(mrep / b) == plain.outfile(str(mrep / b).split("_spher_")[0], want)
        assert "temper" not in json.load(open(mrep / (b + SIDECAR)))
        assert {k: doc[k] for k in res["temper"]} == res["temper"]
        assert doc["model"] == "EHEM" and doc["lidar_level"] == 12 and doc["bits"] == res["bits"] and doc["n_points"] == res["n_points"]
        line = [ln for ln in mrep_out.splitlines() if ln.startswith(LINE)][i].split(":")[1].split()
        assert [float(v) for v in line] == [res["temper"]["ideal_bits_unit"] / res["n_points"], res["temper"]["ideal_bits_chosen"] / res["n_points"],
                                             res["temper"]["side_bits"], res["temper"]["moved"]]


def test_cli_temper_writes_a_stream_the_decoder_reads_and_no_flag_changes_nothing(tmp_path):
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.decoder import SIDECAR, decode_file
    from scp_amd.encoder import FrameEncoder
    seq = two_frames(tmp_path)
    plain, plain_out = run_cli(tmp_path, "encode.py", seq, "plain", [])
    code, code_out = run_cli(tmp_path, "encode.py", seq, "code", ["--temper", "--rate_report"])
    assert LINE not in plain_out and code_out.count(LINE) == 2
    assert code_out.count("bpp ideal / table / coded   :") == 2
    names = {tag: sorted(p.name for p in d.iterdir()) for tag, d in (("plain", plain), ("code", code))}
    # without the flags: names, streams and side-info files as today
    assert not [f for f in names["plain"] if "temper" in f]
    assert all("temper" not in json.load(open(plain / f)) for f in names["plain"] if f.endswith(SIDECAR))
    penc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, device=dev())
    for i, pb in enumerate(f for f in names["plain"] if f.endswith(".bin")):
        assert (plain / pb).read_bytes() == penc.encode(pointCloud.ptread(str(seq / f"{i:06d}.bin")))["bytes"]
    assert not [f for f in names["code"] if f.endswith(".temper.json")]
    # --temper: `_temper` in every name, the table in every side-info file, the in-process encoder's bytes
    bins = [f for f in names["code"] if f.endswith(".bin")]
    assert len(bins) == 2 and all("_temper_spher_" in f for f in bins)
    assert [f.replace("_temper", "") for f in names["code"] if not f.endswith(".rate.json")] == names["plain"]
    enc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, device=dev(), temper="code")
    for i, b in enumerate(bins):
        res = enc.encode(pointCloud.ptread(str(seq / f"{i:06d}.bin")))
        assert res["bytes"] == (code / b).read_bytes()
        side = json.load(open(code / (b + SIDECAR)))
        assert side["temper"] == dict(betas_u32=res["temper"]["grid_u32"], index=[g["index"] for g in res["temper"]["groups"]])
        line = [ln for ln in code_out.splitlines() if ln.startswith(LINE)][i].split(":")[1].split()
        assert [float(v) for v in line] == [res["temper"]["ideal_bits_unit"] / res["n_points"], res["temper"]["ideal_bits_chosen"] / res["n_points"],
                                             res["temper"]["side_bits"], res["temper"]["moved"]]
    # decode_ehem.py on the tempered output reproduces the leaf set
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decode_ehem.py"), "--test_files", str(seq), "--random_weights", "0", "--out_dir", str(code)],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    plys = sorted(p for p in code.iterdir() if p.name.endswith(".ply"))
    assert len(plys) == 2
    for ply, b, pb in zip(plys, bins, [f for f in names["plain"] if f.endswith(".bin")]):
        want = decode_file(str(plain / pb), ehem_model(), device=dev())
        got = decode_file(str(code / b), ehem_model(), device=dev())
        assert torch.equal(got["leaves"][0], want["leaves"][0])
        assert torch.equal(got["points"], want["points"])
        # the file the command wrote holds the plain stream's points, byte for byte what the same writer makes of them
        ref_ply = str(tmp_path / ("want_" + ply.name))
        pointCloud.write_ply_data(ref_ply, want["points"].cpu().numpy())
        assert ply.read_bytes() == open(ref_ply, "rb").read()
        pts = np.asarray(pointCloud.ptread(str(ply)))[:, :3]
        assert pts.shape == tuple(want["points"].shape)
