"""Rate report without a GPU: the numpy reference (rate_ref.py) against the oracle's tables and coder, the exact row, the CLI flag, the
exported symbols and the argument checks of scp_rate_segments."""
import math
import os

import numpy as np
import pytest

import rate_ref
from conftest import golden


def _lib_or_skip():
    from scp_amd import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("library not built")
    return native.lib()


CHUNK = 20000         # rows per numpy pass: the 300 000-row case stays within a few hundred MB


def _symbols(rng, pmf, kind):
    n = len(pmf)
    if kind == "sampled":
        out = np.empty(n, np.int16)
        for a in range(0, n, CHUNK):
            cum = np.cumsum(pmf[a:a + CHUNK].astype(np.float64), 1)
            out[a:a + CHUNK] = np.minimum((rng.random((len(cum), 1)) * cum[:, -1:] > cum).sum(1), 254)
        return out
    if kind == "uniform":
        return rng.integers(0, 255, n).astype(np.int16)
    return pmf.argmin(1).astype(np.int16)                         # the least likely symbol of every row


def _random_pmf(rng, n, scale):
    out = np.empty((n, 255), np.float32)
    for a in range(0, n, CHUNK):
        out[a:a + CHUNK] = rate_ref.softmax_f32(rng.standard_normal((min(CHUNK, n - a), 255), dtype=np.float32) * np.float32(scale))
    return out


def _cases():
    z = golden("cdf_mixed")
    rng = np.random.default_rng(11)
    for kind in ("sampled", "uniform", "least"):
        yield f"cdf_mixed/{kind}", z["pdf"], _symbols(rng, z["pdf"], kind)
    for n in (1, 2, 7, 100, 10000, 300000):
        for scale in (0.0, 1.0, 8.0):
            pmf = _random_pmf(rng, n, scale)
            for kind in ("sampled", "uniform", "least"):
                yield f"n{n}/scale{scale:g}/{kind}", pmf, _symbols(rng, pmf, kind)


def test_reference_pairs_equal_the_oracle_and_table_bits_predict_the_stream_size(orc):
    """The reference's integer pairs are the oracle's CDF columns, no width is below one, and the table bits predict the coded size to
    within two bytes: 0 < 8 * len(stream) - sum(16 - log2(c_high - c_low)) <= 16.  The cap was set before this test existed, from a
    first measurement of 0.44 .. 8.64 bits over these case families plus one byte (the coder emits whole bytes); this test's own 57 cases - the
    300 000-row ones, the only ones near a frame's length, included - give 0.46 .. 9.00 bits (printed below)."""
    gaps = {}
    for name, pmf, sym in _cases():
        cdf = orc.pmf_to_cdf(pmf)
        parts = [rate_ref.pairs(pmf[a:a + CHUNK], sym[a:a + CHUNK]) for a in range(0, len(pmf), CHUNK)]
        lo, hi = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        s = sym.astype(np.int64)
        r = np.arange(len(pmf))
        want_hi = cdf[r, s + 1].astype(np.int64)
        assert np.array_equal(lo, cdf[r, s]) and np.array_equal(hi & 0xFFFF, want_hi) and np.all((hi == 65536) == (s == 254)), name
        assert (hi - lo).min() >= 1, name
        assert np.array_equal(np.stack(rate_ref.unpack(rate_ref.pack(lo, hi))), np.stack((lo, hi))), name
        gaps[name] = 8 * len(orc.ac_encode(cdf, sym)) - math.fsum(rate_ref.table_bits(lo, hi))
    print("coder overhead bits: min %.3f max %.3f over %d cases" % (min(gaps.values()), max(gaps.values()), len(gaps)))
    bad = {k: v for k, v in gaps.items() if not 0 < v <= 16}
    assert not bad, bad


def test_flat_row_costs_log2_255_bits():
    got = rate_ref.ideal_bits(np.zeros((3, 255), np.float32), [0, 100, 254])
    want = math.log2(255.0)
    assert np.all(np.abs(got - want) <= np.spacing(want))
    assert rate_ref.top1(np.zeros((3, 255), np.float32), [0, 100, 254]).all()           # a tie with the maximum is a hit
    # a peaked row away from the symbol, scale 1e4: the float32 softmax underflows, the table still charges 16 bits, the model ~1.4e4
    x = np.zeros((1, 255), np.float32)
    x[0, 7] = 1e4
    lo, hi = rate_ref.pairs(rate_ref.softmax_f32(x), [200])
    assert hi[0] - lo[0] == 1 and rate_ref.table_bits(lo, hi)[0] == 16.0
    assert abs(rate_ref.ideal_bits(x, [200])[0] - 1e4 / math.log(2.0)) < 1e-6


def test_rate_layout_follows_the_coding_order_of_the_windows():
    """Phase 1 = the first (c + 1) // 2 rows of each window in coding order (EncodePlan: the even positions), phase 2 the rest."""
    from scp_amd.encoder import EncodePlan, _rate_layout, _rate_report
    sizes = [1, 6, 0, 8193, 7]
    plan = EncodePlan(sizes, 8192)
    off, levels = _rate_layout(sizes, 8192)
    assert off[0] == 0 and off[-1] == plan.n_rows and all(a <= b for a, b in zip(off[:-1], off[1:]))
    order = plan.coding_order()
    row0 = np.concatenate(([0], np.cumsum(sizes)))
    for l, (p1, p2) in enumerate(levels):
        first = np.concatenate([order[off[i]:off[i + 1]] for i in p1] + [np.zeros(0, np.int64)])
        second = np.concatenate([order[off[i]:off[i + 1]] for i in p2] + [np.zeros(0, np.int64)])
        assert len(first) + len(second) == sizes[l]
        assert np.all((first - row0[l]) % 2 == 0) and np.all((second - row0[l]) % 2 == 1)      # (window starts are even: 8192)
        assert np.all((first >= row0[l]) & (first < row0[l + 1])) and np.all((second >= row0[l]) & (second < row0[l + 1]))
    off1, levels1 = _rate_layout(sizes)
    assert off1 == [0, 1, 7, 7, 8200, 8207] and levels1 == [([i],) for i in range(5)]
    # the report adds the segments up per level and phase
    raw = np.zeros((len(off) - 1, 5), np.int64)
    raw[:, 0] = np.diff(off)
    raw.view(np.float64)[:, 1] = 2.0 * np.diff(off)
    raw.view(np.float64)[:, 2] = 3.0 * np.diff(off)
    raw[:, 3] = 1
    rep = _rate_report(raw, levels, 8 * 7000, 1000)
    assert [lv["nodes"] for lv in rep["levels"]] == sizes
    assert rep["levels"][3]["phase1"]["nodes"] == 4096 + 1 and rep["levels"][3]["phase2"]["nodes"] == 4096
    assert rep["ideal_bits"] == 2.0 * sum(sizes) and rep["table_bits"] == 3.0 * sum(sizes) and rep["bad_rows"] == 0
    assert rep["bpp_ideal"] == rep["ideal_bits"] / 1000 and rep["bits_per_node_ideal"] == 2.0
    assert rep["coder_overhead_bits"] == 8 * 7000 - rep["table_bits"]
    for lv in rep["levels"]:
        assert lv["phase1"]["nodes"] + lv["phase2"]["nodes"] == lv["nodes"] and lv["phase1"]["top1"] + lv["phase2"]["top1"] == lv["top1"]


def test_cli_accepts_rate_report_and_keeps_its_refusals():
    from scp_amd import native
    from scp_amd.cli import get_args, refuse_unsupported
    base = ["--test_files", "x.bin", "--type", "kitti", "--lidar_level", "12", "--spher"]
    for mullevel in (False, True):
        off, on = get_args(base, mullevel), get_args(base + ["--rate_report"], mullevel)
        assert getattr(off, "rate_report", False) is False and on.rate_report is True
        for name in ("EHEM", "OctAttention"):
            refuse_unsupported(on, name, mullevel)
        with pytest.raises(native.ScpError, match="--metrics is available for the EHEM encoders only"):
            refuse_unsupported(get_args(base + ["--rate_report", "--metrics"], mullevel), "OctAttention", mullevel)
        with pytest.raises(native.ScpError, match="--sequential is an OctAttention mode"):
            refuse_unsupported(get_args(base + ["--rate_report", "--sequential"], mullevel), "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--preproc_path with OctAttention is not supported"):
            refuse_unsupported(get_args(base + ["--rate_report", "--preproc_path", "pp/"], mullevel), "OctAttention", mullevel)


def test_library_exports_the_rate_entry_points():
    L = _lib_or_skip()
    assert hasattr(L, "scp_rate_segments") and hasattr(L, "scp_rate_workspace_bytes")
    assert L.scp_rate_workspace_bytes(0, 3) == 0
    assert L.scp_rate_workspace_bytes(1000, 3) >= 17 * 1000 and L.scp_rate_workspace_bytes(1000, 3) % 8 == 0
    assert L.scp_rate_workspace_bytes(-1, 3) == -1 and L.scp_rate_workspace_bytes(10, -1) == -1


def test_a_symbol_with_a_minus_inf_logit_is_bad_yet_keeps_its_table_bits(orc):
    """An infinite cross-entropy: the row is bad and carries 0 ideal bits, but its pair is the oracle table's entry of width 1 - the 16
    bits the coder spends stay in the table column, so stream length minus table bits keeps its bound."""
    x = np.zeros((3, 255), np.float32)
    x[1, 7] = -np.inf
    x[2, :200] = -np.inf
    sym = np.array([7, 7, 254], np.uint8)
    lo, hi = rate_ref.pairs(rate_ref.softmax_f32(x), sym)
    r = rate_ref.rows(x, sym, rate_ref.pack(lo, hi))
    assert r["bad"].tolist() == [False, True, False] and r["width"][1] == 1
    assert r["ideal"][1] == 0.0 and r["table"][1] == 16.0 and np.isfinite(r["ideal"]).all() and np.isfinite(r["table"]).all()
    assert abs(r["ideal"][0] - math.log2(255.0)) < 1e-12 and abs(r["ideal"][2] - math.log2(55.0)) < 1e-12
    stream = orc.ac_encode(orc.pmf_to_cdf(rate_ref.softmax_f32(x)), sym.astype(np.int16))
    assert 0 < 8 * len(stream) - math.fsum(r["table"]) <= 16


def test_rate_segments_rejects_bad_arguments_without_a_gpu():
    """The argument checks come before any HIP call: SCP_EINVAL (-1), nothing launched."""
    L = _lib_or_skip()
    z, one = None, 4096            # NULL and a fake (never dereferenced) non-NULL address
    ws = L.scp_rate_workspace_bytes(10, 2)
    ok = dict(logits=one, ld=256, n=10, nsym=255, sym=one, lohi=one, seg_off=one, nseg=2, out=one, ri=z, rt=z, ws=one, ws_bytes=ws, stream=z)

    def call(**kw):
        a = dict(ok, **kw)
        return L.scp_rate_segments(a["logits"], a["ld"], a["n"], a["nsym"], a["sym"], a["lohi"], a["seg_off"], a["nseg"], a["out"], a["ri"], a["rt"],
                                   a["ws"], a["ws_bytes"], a["stream"])
    for bad in (dict(logits=z), dict(sym=z), dict(lohi=z), dict(seg_off=z), dict(out=z), dict(ws=z), dict(nsym=1), dict(nsym=257),
                dict(ld=254), dict(ws_bytes=ws - 1), dict(ws_bytes=0), dict(nseg=-1), dict(n=-1), dict(ws=4097)):
        assert call(**bad) == -1, bad
