"""csrc/cdf.hip on the rows a trained model emits (-m gpu; the rows are tests/cdf_cases.py, shown to discriminate by tests/test_cdf_cases.py).

A stream decodes only if the encoder's call (the coding-order table: row stride 256, 16-byte stage-in, only the symbol's pair kept) and the
decoders' (contiguous rows, full tables, another place in another 64-row tile) get the same integers for a row.  So: the table is the
oracle's function of the library's own PMF on every path and layout, for alphabets of 2 .. 255 symbols; that PMF is the float64 softmax to
a bound derived from the arithmetic; a row's bits depend on the row alone; the device pairs drive the host coder to the oracle's bytes;
the rate kernel charges the oracle's widths; and models sharpened until their float32 probabilities underflow still round-trip."""
import numpy as np
import pytest
import torch

import cdf_cases as CC
from cfgs import ehem_cfg, octattn_cfg

pytestmark = pytest.mark.gpu

N = 4003
SHARPEN = 32.0            # the output layers of the probability heads times this: the smallest power of two at which 10 % of a frame's rows
#                           spread over more than 104 and a coded symbol has width 1, on every frame below (_check_sharp asserts both
#                           halves of that: the conditions at this factor, and that half of it would miss them)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i32(t):
    return None if t is None else t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same_bits(got, want, rows=None, what=""):
    """Every output both dicts hold, bit for bit (`rows`: the rows of `want` that `got` holds)."""
    for k in ("pmf", "cdf", "lohi"):
        a, b = got.get(k), want.get(k)
        if a is None or b is None:
            continue
        b = b if rows is None else b[rows]
        assert torch.equal(_i32(a), _i32(b)), (what, k, (_i32(a) != _i32(b)).nonzero()[:5].tolist())


@pytest.fixture(scope="module")
def rows(dev, orc):
    """rows(nsym), filled at first use and freed with the module: the logit rows, their device copies, everything the library makes of
    them in ONE launch of the contiguous layout, and the oracle's table of the library's PMF.  Shared and never modified."""
    from scp_amd import native
    cache = {}

    def get(nsym):
        if nsym not in cache:
            x, sym = CC.logit_rows(N, nsym, 0)
            x_d, sym_d = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(sym)).to(dev)
            r = native.softmax_cdf(CC.place(x_d), sym_d, want_pmf=True, want_cdf=True)
            torch.cuda.synchronize()
            pmf = r["pmf"].cpu().numpy()
            cache[nsym] = dict(x=x, sym=sym, x_d=x_d, sym_d=sym_d, r=r, pmf=pmf, cdf=r["cdf"].cpu().numpy().view(np.uint16),
                               lohi=r["lohi"].cpu().numpy().view(np.uint32), want=orc.pmf_to_cdf(pmf))
        return cache[nsym]

    yield get
    cache.clear()


def _check_pairs(lohi, want, sym):
    lo, hi = CC.pairs(want, sym)
    lohi = np.asarray(lohi).view(np.uint32).astype(np.int64)
    assert np.array_equal(lohi & 0xFFFF, lo)
    assert np.array_equal(lohi >> 16, hi)                    # 0 for the top symbol (= 65536)


# ------------------------------------------------------------------------------------------------------- the table, on every path
@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_table_is_the_oracles_function_of_the_librarys_pmf(dev, orc, rows, nsym):
    """scp_softmax_cdf: cdf == orc.pmf_to_cdf(pmf) exactly and the pairs are its entries around the symbol; every row count, every layout of
    cdf_cases.place and every choice of outputs gives the bits of the one contiguous 4 003-row launch."""
    from scp_amd import native
    t = rows(nsym)
    assert np.isfinite(t["pmf"]).all()
    assert np.array_equal(t["cdf"], t["want"])
    _check_pairs(t["lohi"], t["want"], t["sym"])
    for n in CC.ROW_COUNTS:
        head = slice(0, n)
        for name, (ld, mis) in CC.LAYOUTS.items():
            v = CC.place(t["x_d"][:n], ld, mis)
            assert v.data_ptr() % 16 == (4 if mis else 0) and v.stride(0) == (nsym if ld is None else ld)
            s = t["sym_d"][:n]
            what = (nsym, n, name)
            _assert_same_bits(native.softmax_cdf(v, s, want_pmf=True, want_cdf=True), t["r"], head, what)
            pairs_only = native.softmax_cdf(v, s)
            assert pairs_only["cdf"] is None and pairs_only["pmf"] is None
            _assert_same_bits(pairs_only, t["r"], head, what + ("lohi alone",))
            table_only = native.softmax_cdf(v, want_lohi=False, want_cdf=True)
            assert table_only["lohi"] is None
            _assert_same_bits(table_only, t["r"], head, what + ("cdf alone",))
            _assert_same_bits(native.softmax_cdf(v, s, want_cdf=True), t["r"], head, what + ("lohi and cdf",))


@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_pmf_path_table_is_the_oracles(dev, orc, nsym):
    """scp_pmf_cdf on unnormalised rows whose float32 prefix sums depend on their order: the oracle's table and pairs, at an aligned and at a
    misaligned base, with either output alone or both."""
    from scp_amd import native
    p, sym = CC.pmf_rows(N, nsym, 0)
    want = orc.pmf_to_cdf(p)
    p_d, sym_d = torch.from_numpy(np.array(p)).to(dev), torch.from_numpy(np.array(sym)).to(dev)
    for n in CC.ROW_COUNTS:
        for mis in (False, True):
            v = CC.place(p_d[:n], None, mis)
            assert v.is_contiguous() and v.data_ptr() % 16 == (4 if mis else 0)
            r = native.pmf_cdf(v, sym_d[:n], want_cdf=True)
            cdf = r["cdf"].cpu().numpy().view(np.uint16)
            bad = np.flatnonzero((cdf != want[:n]).any(1))
            assert np.array_equal(cdf, want[:n]), (nsym, n, mis, len(bad), bad[:10].tolist())
            _check_pairs(r["lohi"].cpu().numpy(), want[:n], sym[:n])
            _assert_same_bits(native.pmf_cdf(v, sym_d[:n]), r, None, (nsym, n, mis, "lohi alone"))
            _assert_same_bits(native.pmf_cdf(v, want_cdf=True), r, None, (nsym, n, mis, "cdf alone"))


# ------------------------------------------------------------------------------------------------------- the PMF
@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_pmf_against_float64_with_a_derived_bound(dev, orc, rows, nsym):
    """|pmf - ref| <= (nsym + 4) 2^-24 ref + 2^-148, ref = exp(float64(float32(x - max))) normalised in float64.  Relative term, in half ulps:
    four for the two expf results good to 1 ulp (the entry's own and the sum's terms), nsym - 1 for the serial float32 additions, one for
    the correctly rounded division; absolute term: two subnormal roundings.  Derived, not measured - it rests on HIP's documented 1 ulp
    for expf.  The largest observed |pmf - ref| / bound on gfx950 is 0.4999 (nsym 254, an N(0,1) * 30 row: one subnormal step against
    the absolute term); on the plain N(0,1) rows, which have no subnormals, it is 0.38 at nsym 2 and 0.05 at nsym 255."""
    t = rows(nsym)
    ref = CC.softmax_f64(t["x"])
    pmf = t["pmf"].astype(np.float64)
    bound = (nsym + 4) * 2.0 ** -24 * ref + 2.0 ** -148
    ratio = np.abs(pmf - ref) / bound
    k = CC.kind_of(np.arange(N))
    worst = {CC.KINDS[i]: float(ratio[k == i].max()) for i in range(len(CC.KINDS))}
    tiny = float(np.finfo(np.float32).tiny)
    print(f"nsym {nsym}: max |pmf - ref| / bound {ratio.max():.4f}; per kind {({a: round(b, 4) for a, b in worst.items()})}; "
          f"zero share {(t['pmf'] == 0).mean():.3f}, subnormal entries {int(((t['pmf'] > 0) & (t['pmf'] < tiny)).sum())}")
    assert (ratio <= 1.0).all(), (nsym, float(ratio.max()), np.argwhere(ratio > 1.0)[:5].tolist())
    # the rows keep on the device the edges they were built for: exact zeros and (beyond two columns) subnormals reach the table code
    assert (t["pmf"] == 0).mean() >= 0.10
    assert nsym == 2 or ((t["pmf"] > 0) & (t["pmf"] < tiny)).any()


# ------------------------------------------------------------------------------------------------------- a row alone
_POSITIONS = (64 + 0, 64 + 31, 64 + 63, 128 + 1, 128 + 62, 192 + 17)      # tile positions 0, 31, 63 / 1, 62 / a partial last tile of 37 rows
_TABLE_ROWS = 192 + 37


@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_a_rows_integers_depend_on_the_row_alone(dev, orc, rows, nsym):
    """One row of every kind, at tile positions 0, 1, 31, 62 and 63, in a partial last tile and in a one-row launch: the same pmf, cdf and
    pair bits.  Its neighbours are rows of other kinds, among them an all-NaN, an all-+inf and an all--inf row next to every position
    (nothing is asserted about those rows' own output)."""
    from scp_amd import native
    t = rows(nsym)
    back = t["x_d"][(torch.arange(_TABLE_ROWS, device=dev) * 7 + 3) % N].clone()
    sym_b = t["sym_d"][(torch.arange(_TABLE_ROWS, device=dev) * 7 + 3) % N].clone()
    special = (float("nan"), float("inf"), float("-inf"))
    for i, p in enumerate(_POSITIONS):
        back[p - 1 if p % 64 else p + 2] = special[i % 3]
        back[p + 1 if p % 64 != 63 else p - 2] = special[(i + 1) % 3]
    back[0], back[1], back[63] = special
    for kind in range(len(CC.KINDS)):
        r0 = 10 * (kind % 4) + kind                           # a row of this kind; the forced symbol differs from kind to kind
        assert CC.kind_of(r0) == kind
        probe, s = t["x_d"][r0], t["sym_d"][r0]
        want = {k: v[r0:r0 + 1] for k, v in t["r"].items()}    # the row's bits in the shared 4 003-row launch (tile 0, position r0)
        tab, sy = back.clone(), sym_b.clone()
        for p in _POSITIONS:
            tab[p], sy[p] = probe, s
        for name in ("tight", "ld256"):                       # the decoders' and the encoder's stage-in
            ld, mis = CC.LAYOUTS[name]
            got = native.softmax_cdf(CC.place(tab, ld, mis), sy, want_pmf=True, want_cdf=True)
            for p in _POSITIONS:
                _assert_same_bits({k: v[p:p + 1] for k, v in got.items()}, want, None, (nsym, CC.KINDS[kind], name, p))
            one = native.softmax_cdf(CC.place(probe[None], ld, mis), s[None], want_pmf=True, want_cdf=True)
            _assert_same_bits(one, want, None, (nsym, CC.KINDS[kind], name, "one-row launch"))


# ------------------------------------------------------------------------------------------------------- into the host coder
@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_device_pairs_drive_the_host_coder_to_the_oracles_bytes(dev, orc, rows, nsym):
    """native.ac_encode_lohi(device pairs) == orc.ac_encode(orc.pmf_to_cdf(pmf), sym), and both decoders fed the device table rows return
    the symbols (native: scp_ac_dec_run for the first half, scp_ac_dec_next for the second) - the 4 003 rows followed by 1 200
    consecutive symbols of width 1 (probability an exact zero) and 300 ordinary rows."""
    from scp_amd import native
    t = rows(nsym)
    k = CC.kind_of(np.arange(N))
    huge = np.flatnonzero(k == CC.KINDS.index("huge"))
    run = np.resize(huge, 1200)
    x = np.concatenate([t["x"], t["x"][run], t["x"][:300]])
    sym = np.concatenate([t["sym"], t["sym"][run], t["sym"][:300]]).astype(np.uint8)
    hot = t["x"][run].argmax(1)
    sym[N:N + 1200] = np.where(hot == 0, nsym - 1, 0)         # a column beside the 1e30 one: probability exactly 0
    n = len(x)
    r = native.softmax_cdf(torch.from_numpy(x).to(dev), torch.from_numpy(sym).to(dev), want_pmf=True, want_cdf=True)
    pmf, cdf = r["pmf"].cpu().numpy(), r["cdf"].cpu().numpy().view(np.uint16)
    lohi = r["lohi"].cpu().numpy().view(np.uint32)
    want = orc.pmf_to_cdf(pmf)
    assert np.array_equal(cdf, want)
    lo, hi = CC.pairs(want, sym)
    width = np.where(hi == 0, 65536, hi) - lo
    assert (width[N:N + 1200] == 1).all() and (pmf[np.arange(N, N + 1200), sym[N:N + 1200]] == 0).all()
    s16 = sym.astype(np.int16)
    stream = orc.ac_encode(want, s16)
    assert native.ac_encode_lohi(lohi) == stream
    assert native.ac_encode_cdf(cdf, s16) == stream
    half = n // 2
    dec = native.AcDecoder(stream, Lp=nsym + 1)
    assert np.array_equal(dec.run(cdf[:half]), s16[:half])
    assert [dec.next(cdf[i]) for i in range(half, n)] == s16[half:].tolist()
    odec = orc.AcDecoder(stream, nsym)
    assert [odec.decode_cdf_row(row) for row in cdf] == s16.tolist()


# ------------------------------------------------------------------------------------------------------- the rate kernel
@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_rate_kernel_charges_the_oracles_widths_on_peaked_rows(dev, orc, rows, nsym):
    """scp_rate_segments on the peaked kinds with REFERENCE pairs (the oracle's table of the library's PMF, not the kernel's own output):
    row table bits == 16 - log2(width) to the bound tests/test_gpu_rate.py uses - width-1 symbols, symbols whose logit is -inf (an
    infinite cross-entropy: counted in bad_rows, 0 ideal bits, yet the 16 table bits the coder spends), 1e30 entries."""
    from scp_amd import native
    from test_gpu_rate import ROW_TABLE_TOL
    t = rows(nsym)
    k = CC.kind_of(np.arange(N))
    idx = np.flatnonzero(np.isin(k, [CC.KINDS.index(name) for name in CC.PEAKED_KINDS]))
    sym = t["sym"][idx]
    lo, hi = CC.pairs(t["want"][idx], sym)
    width = np.where(hi == 0, 65536, hi) - lo
    assert (width >= 1).all() and (width == 1).sum() >= 100
    lohi = torch.from_numpy((lo | (hi << 16)).astype(np.uint32).view(np.int32)).to(dev)
    x_sel, sym_d = t["x_d"][torch.from_numpy(idx).to(dev)], torch.from_numpy(np.array(sym)).to(dev)
    xs = t["x"][idx, sym.astype(np.int64)]
    inf_ce = np.isneginf(xs)
    want_tab = 16.0 - np.log2(width.astype(np.float64))
    n = len(idx)
    for name, (ld, mis) in CC.LAYOUTS.items():
        r = native.rate_segments(CC.place(x_sel, ld, mis), sym_d, lohi, [0, n], want_rows=True)
        torch.cuda.synchronize()
        tab, ideal = r["row_table"].cpu().numpy(), r["row_ideal"].cpu().numpy()
        err = np.abs(tab - want_tab).max()
        print(f"nsym {nsym} {name}: max |table bits - (16 - log2 width)| {err:.3e} over {n} rows, {int(inf_ce.sum())} of them with a -inf symbol logit")
        assert np.isfinite(tab).all() and np.isfinite(ideal).all()
        assert err <= ROW_TABLE_TOL, (name, np.flatnonzero(np.abs(tab - want_tab) > ROW_TABLE_TOL)[:5].tolist())
        assert int(r["bad_rows"][0]) == int(inf_ce.sum()) and (ideal[inf_ce] == 0).all() and (ideal[~inf_ce] >= 0).all()
        assert abs(float(r["table_bits"][0]) - float(np.sum(want_tab))) <= 1e-9 * n


# ------------------------------------------------------------------------------------------------------- sharp models
def _sharpen(model, layers):
    """The output layer of every probability head times SHARPEN (a power of two: every logit scales exactly)."""
    with torch.no_grad():
        for lin in layers:
            lin.weight.mul_(SHARPEN)
            lin.bias.mul_(SHARPEN)
    return model


@pytest.fixture(scope="module")
def sharp_ehem(dev):
    """A model of this module's own, sharpened BEFORE its first forward: the row-chain kernels cache their weights, and the flat
    module-scoped models of the other test files stay flat."""
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    m = fill_weights(EHEM(ehem_cfg()), 0)
    return _sharpen(m, (m.prob_pred_mlp1[-1], m.prob_pred_mlp2[-1])).to(dev)


def _check_sharp(res, orc, what):
    """An encoder result of a sharpened model: at least 10 % of its table rows spread over more than 104 and a coded symbol has width 1;
    at HALF the factor fewer than 10 % of the rows would (the sharpened layers are the last and linear, the factor a power of two: every
    logit, so every spread, halves to rounding) - SHARPEN is the smallest power of two that gets there, asserted and not only recorded;
    and the stream is the oracle coder's on the device table.  -> (share over 104, coded symbols of width 1)"""
    from scp_amd import native
    table, sym_d = res["_debug"]["table"], res["_debug"]["sym_coded"]
    assert bool(torch.isfinite(table).all())
    spread = (table.max(1).values - table.min(1).values).cpu().numpy()
    r = native.softmax_cdf(table, sym_d, want_cdf=True)
    cdf, sym = r["cdf"].cpu().numpy().view(np.uint16), sym_d.cpu().numpy()
    lo, hi = CC.pairs(cdf, sym)
    width = np.where(hi == 0, 65536, hi) - lo
    _check_pairs(r["lohi"].cpu().numpy(), cdf, sym)
    assert res["bytes"] == orc.ac_encode(cdf, sym.astype(np.int16))
    over, over_at_half, width1 = float((spread > 104).mean()), float((spread > 208).mean()), int((width == 1).sum())
    print(f"{what} sharpened x{SHARPEN:g}: {100 * over:.1f} % of {len(spread)} rows spread over more than 104 ({100 * over_at_half:.1f} % would at "
          f"x{SHARPEN / 2:g}), median spread {np.median(spread):.1f}, {width1} coded symbols of width 1")
    assert over >= 0.10 and width1 >= 1
    assert over_at_half < 0.10
    return over, width1


@pytest.mark.parametrize("mullevel", [False, True])
def test_sharp_ehem_frames_round_trip(sharp_ehem, dev, orc, mullevel):
    """synth_frame(4)[::30] at L12, same-level and multi-level, through a model whose float32 probabilities underflow: at least 10 % of
    the table rows spread over more than 104, a coded symbol has width 1, the bytes are the oracle coder's on the device table, and
    FrameDecoder regenerates the occupancy codes and the leaves exactly.  SHARPEN = 32 is the smallest power of two that gets there
    (measured on gfx950): at 16 no row of either frame spreads over 104 (medians 69 and 63); at 32, 97.7 % of the same-level frame's
    14 076 rows and 84.2 % of the multi-level one's 15 049 do.  The synthetic weights know nothing about the occupancies, so nearly
    every coded symbol (13 878 and 14 952) then has a probability that underflowed and width 1: the streams cost 16 bits a node."""
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    xyz = synth_frame(4)[::30].copy()
    enc = FrameEncoder(sharp_ehem, "kitti", 12, spher=True, mullevel=mullevel, device=dev)
    res = enc.encode(xyz)
    _check_sharp(res, orc, f"EHEM frame 4, mullevel {mullevel},")
    nodes = enc.geom.nodes(("occ", "level"))
    shells = FrameDecoder(sharp_ehem, 12, mullevel=mullevel, polar=True, device=dev).decode(res["bytes"], res["n_levels"], res["pos_mm"])
    assert len(shells) == (3 if mullevel else 1)
    for s, (codes, leaves) in enumerate(shells):
        info = enc.geom.info[s]
        want = nodes["occ"][info.node_base:info.node_base + info.n_nodes].cpu().numpy()
        got = torch.cat(codes).cpu().numpy()
        assert len(got) == len(want)
        if mullevel:
            assert got[-1] == 0 and np.array_equal(got[:-1], want[:-1])      # the last BFS node is not coded
        else:
            assert np.array_equal(got, want)
            assert np.array_equal(leaves.cpu().numpy(), enc.geom.leaves(s).cpu().numpy())


@pytest.mark.parametrize("mullevel", [False, True])
def test_sharp_ehem_streams_decode_in_lockstep_as_one_by_one(sharp_ehem, dev, orc, tmp_path, mullevel):
    """Two sharp streams (frames 4 and 5, each held to the conditions of _check_sharp) through the lockstep decoder: the encoder's
    occupancy codes and leaves, and decode_file's result for each."""
    from scp_amd.decoder import decode_file, decode_files
    from scp_amd.synth import synth_frame
    from test_gpu_ehem_decode_batch import _encode, _same
    frames = [_encode(sharp_ehem, dev, tmp_path, f"f{i}", synth_frame(i)[::30].copy(), 12, spher=True, mullevel=mullevel) for i in (4, 5)]
    for i, f in zip((4, 5), frames):
        _check_sharp(f[1], orc, f"EHEM frame {i}, mullevel {mullevel},")
    got = decode_files([f[0] for f in frames], sharp_ehem, streams=2, mullevel=mullevel, device=dev)
    for f, (out, res, occs, leaves) in enumerate(frames):
        assert len(got[f]["codes"]) == len(occs) == (3 if mullevel else 1)
        for k, occ in enumerate(occs):
            c = got[f]["codes"][k]
            if mullevel:
                assert c[-1] == 0 and torch.equal(c[:-1].long(), occ[:-1].long()), (f, k)
            else:
                assert torch.equal(c.long(), occ.long()) and torch.equal(got[f]["leaves"][k], leaves[k].to(got[f]["leaves"][k].dtype)), (f, k)
        assert _same(got[f], decode_file(out, sharp_ehem, mullevel=mullevel, device=dev)), f


def test_sharp_octattention_stream_round_trips(dev, orc, tmp_path):
    """OctAttention with its output layer sharpened the same way: a --decodable stream of the smallest frame tests/test_gpu_octattn_decode.py
    encodes (synth_frame(1)[::200], L8), decoded by decode.py's decoder - every logits row, symbol, leaf and point (that file's
    _round_trip), and the stream is the oracle coder's on the device table.  Measured on gfx950 at SHARPEN = 32: all 576 rows spread
    over 104 (median 127) and 553 coded symbols have width 1; at 16 no row does (median 64)."""
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    from test_gpu_octattn_decode import _round_trip
    m = fill_weights(OctAttention(octattn_cfg()), 0)
    m = _sharpen(m, (m.decoder1,)).to(dev)
    res, got = _round_trip(m, dev, tmp_path, synth_frame(1)[::200].copy(), 8, spher=True)
    _check_sharp(res, orc, "OctAttention")
