"""The rows of tests/cdf_cases.py, checked on the CPU through the oracle alone: they still have the edges they are named for and can tell
a subtly wrong CDF kernel from a right one, so a later edit of the generators cannot quietly take an edge away from
tests/test_gpu_cdf.py.  The thresholds are conditions on the INPUTS: if a seed misses one, change the seed, not the threshold."""
import numpy as np
import pytest

import cdf_cases as CC

N = 4003
SEEDS = (0, 1)
TINY = float(np.finfo(np.float32).tiny)                   # the smallest normal float32


@pytest.fixture(scope="module")
def tables(orc):
    """Per (nsym, seed): the rows, their float32 PMF and the oracle's table of it - computed once, read-only."""
    out = {}
    for nsym in CC.NSYMS:
        for seed in SEEDS:
            x, sym = CC.logit_rows(N, nsym, seed)
            pmf = CC.softmax_f32(x)
            out[nsym, seed] = dict(x=x, sym=sym, pmf=pmf, cdf=orc.pmf_to_cdf(pmf))
    return out


def test_the_lists_are_what_the_gpu_tests_promise():
    assert CC.NSYMS == (2, 3, 16, 64, 65, 128, 129, 254, 255) and CC.ROW_COUNTS == (1, 63, 64, 65, 129, 4003)
    assert len(CC.KINDS) == 10 and set(CC.PEAKED_KINDS) < set(CC.KINDS)
    assert {ld for ld, _ in CC.LAYOUTS.values()} == {None, 256, 300} and [m for _, m in CC.LAYOUTS.values()].count(True) == 1
    assert CC.LAYOUTS["ld256-misaligned"] == (256, True)


@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_every_kind_is_what_it_is_named_for(nsym):
    x, sym = CC.logit_rows(N, nsym, 0)
    assert x.dtype == np.float32 and x.shape == (N, nsym) and sym.dtype == np.uint8 and int(sym.max()) < nsym
    k = CC.kind_of(np.arange(N))
    rows = lambda name: x[k == CC.KINDS.index(name)]
    spread = lambda a: a.max(1) - np.where(np.isinf(a), np.inf, a).min(1)
    assert (rows("flat") == 0).all()
    assert (spread(rows("normal30")) > 87).mean() > (0.5 if nsym >= 16 else 0.01)
    assert np.median(spread(rows("normal1e4"))) > 1e3
    ramp = rows("ramp")
    assert (ramp[:, 0] == 0).all() and (ramp[:, -1] == np.float32(-104)).all() and (np.diff(ramp, axis=1) < 0).all()
    assert ((rows("huge") == np.float32(1e30)).sum(1) == 1).all()
    ninf = np.isneginf(rows("neginf")).sum(1)
    assert ninf.min() >= 1 and ninf.max() <= nsym - 1 and (nsym == 2 or len(set(ninf.tolist())) > 1)
    r = np.flatnonzero(k == CC.KINDS.index("tie"))
    assert (x[r, sym[r]] == x[r].max(1)).all() and ((x[r] == x[r].max(1, keepdims=True)).sum(1) >= 2).all()
    r = np.flatnonzero(k == CC.KINDS.index("peaked"))
    assert (x[r].argmax(1) == sym[r]).all()
    # the same call gives the same rows; another seed gives others; a prefix of a longer table is NOT assumed anywhere
    x2, sym2 = CC.logit_rows(N, nsym, 0)
    assert np.array_equal(x, x2, equal_nan=True) and np.array_equal(sym, sym2)
    assert not np.array_equal(CC.logit_rows(N, nsym, 1)[0], x)


@pytest.mark.parametrize("nsym", CC.NSYMS)
def test_forced_symbols(tables, nsym):
    """Column 0, column nsym - 1 (c_high stored as 0), the argmax and a zero-probability column are coded on fixed rows of every kind."""
    t = tables[nsym, 0]
    x, sym, pmf = t["x"], t["sym"].astype(np.int64), t["pmf"]
    r = np.arange(N)
    k, f = CC.kind_of(r), (r // 10) % 4
    assert (sym[f == 0] == 0).all() and (sym[f == 1] == nsym - 1).all()
    free = (k != CC.KINDS.index("tie")) & (k != CC.KINDS.index("peaked"))
    m = free & (f == 2)
    assert (x[r[m], sym[m]] == x[m].max(1)).all()
    m = free & (f == 3) & (pmf == 0).any(1)
    assert m.sum() >= (50 if nsym > 2 else 10) and (pmf[r[m], sym[m]] == 0).all()
    for kind in range(len(CC.KINDS)):                      # every kind meets symbol 0 and the top symbol
        assert (sym[k == kind] == 0).any() and (sym[k == kind] == nsym - 1).any()
    # a coded symbol of probability zero has width 1 in the oracle's table: the +arange term alone
    lo, hi = CC.pairs(t["cdf"], sym)
    w = np.where(hi == 0, 65536, hi) - lo
    assert (w[m] == 1).all() and (w >= 1).all()


@pytest.mark.parametrize("nsym", CC.NSYMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_zero_and_subnormal_probabilities(tables, nsym, seed):
    """At least 10 % of all entries of the float32 softmax are exact zeros and at least one is subnormal.  nsym = 2 cannot be asked for a
    subnormal: its ramp is the two end points 0 and -104 (an exact zero), and two N(0,1) * 30 logits land 87.4 .. 103.9 apart only by
    chance - the zeros are asked of it all the same."""
    pmf = tables[nsym, seed]["pmf"]
    zero = (pmf == 0).mean()
    sub = int(((pmf > 0) & (pmf < TINY)).sum())
    print(f"nsym {nsym} seed {seed}: zero share {zero:.3f}, subnormal entries {sub}")
    assert zero >= 0.10
    if nsym > 2:
        assert sub >= 1
    assert np.isfinite(pmf).all() and (np.abs(pmf.astype(np.float64).sum(1) - 1) < 1e-4).all()
    # the float32 PMF is the float64 one to rounding (the bound of tests/test_gpu_cdf.py, with numpy's exp in place of the device's)
    ref = CC.softmax_f64(tables[nsym, seed]["x"])
    assert (np.abs(pmf - ref) <= (nsym + 4) * 2.0 ** -24 * ref + 2.0 ** -148).all()


@pytest.mark.parametrize("nsym", CC.NSYMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_tables_on_logit_rows(orc, tables, nsym, seed):
    """The C loop is the numpy restatement, tables increase strictly, and the oracle coder round-trips its own table - on zeros,
    subnormals and width-1 symbols."""
    t = tables[nsym, seed]
    assert np.array_equal(t["cdf"], orc.pmf_to_cdf_numpy(t["pmf"]))
    c = CC.widen(t["cdf"])
    assert (c[:, 0] == 0).all() and (c[:, -1] == 65536).all() and (np.diff(c, axis=1) > 0).all()
    sym = t["sym"].astype(np.int16)
    bs = orc.ac_encode(t["cdf"], sym)
    dec = orc.AcDecoder(bs, nsym)
    assert [dec.decode_cdf_row(row) for row in t["cdf"]] == sym.tolist()


@pytest.mark.parametrize("nsym", CC.NSYMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_pmf_rows_depend_on_summation_order(orc, nsym, seed):
    """On pmf_rows the oracle's table (float32 serial prefix sums) differs from the table of float64 prefix sums on at least 1 % of the rows:
    a kernel that re-associates the sum (pairwise, per column quarter, in higher precision) cannot reproduce it."""
    p, sym = CC.pmf_rows(N, nsym, seed)
    assert p.dtype == np.float32 and (p > 0).all() and p.max() < 2 and sym[0] == 0 and sym[1] == nsym - 1
    cdf = orc.pmf_to_cdf(p)
    assert np.array_equal(cdf, orc.pmf_to_cdf_numpy(p))
    c = CC.widen(cdf)
    assert (np.diff(c, axis=1) > 0).all()
    differ = (cdf != CC.cdf_from_f64_prefix_sums(p)).any(1).mean()
    print(f"nsym {nsym} seed {seed}: rows differing from float64 prefix sums {100 * differ:.2f} % ({int(round(differ * N))} of {N})")
    if nsym >= 16:
        assert differ >= 0.01
    elif nsym == 3:
        # three terms: c[0] = p[0] is exact and c[1] one correctly rounded addition in either arithmetic; only the last sum rounds twice,
        # and it moves an integer only through c / c[-1]: on about 65533 * 2^-24 = 0.4 % of the rows at the very most, so 1 % is out of
        # reach for any seed.  Measured: ONE row of the 4 003 with either seed (0.02 %).  `differ > 0` rests on that one row - if an edit
        # of the generator loses it, pick a seed that has one (a condition on the inputs, as every threshold here); the 1 % is asked
        # from 16 columns on.
        assert 0 < differ < 0.01
    else:
        assert differ == 0                                  # two terms: p[0], then the last sum, and c[-1] / c[-1] == 1 whatever it is
    s = sym.astype(np.int16)
    dec = orc.AcDecoder(orc.ac_encode(cdf, s), nsym)
    assert [dec.decode_cdf_row(row) for row in cdf] == s.tolist()


def test_column_quarter_sums_would_show(orc):
    """The wrong kernel the GPU tests must catch - the prefix sums of the four 64-column quarters taken separately and added - restated on
    the host: its table differs from the oracle's from 128 columns on (a quarter of ONE column, as the second of 65, adds in serial order
    all the same)."""
    for nsym in (128, 129, 254, 255):
        p, _ = CC.pmf_rows(N, nsym, 0)
        c = np.zeros_like(p)
        base = np.zeros(N, np.float32)
        for q in range(0, nsym, 64):
            part = np.cumsum(p[:, q:q + 64], axis=1, dtype=np.float32)
            c[:, q:q + 64] = base[:, None] + part
            base = base + part[:, -1]
        f = (c / c[:, -1:]).astype(np.float32).astype(np.float64)
        q_ = np.rint(np.hstack((np.zeros((N, 1)), f)) * (65536 - nsym)).astype(np.int64)
        wrong = ((q_ + np.arange(nsym + 1)) & 0xFFFF).astype(np.uint16)
        assert (wrong != orc.pmf_to_cdf(p)).any(1).mean() >= 0.01, nsym


@pytest.mark.parametrize("name", list(CC.LAYOUTS))
def test_place_embeds_rows_without_touching_them(name):
    ld, mis = CC.LAYOUTS[name]
    for nsym in (2, 65, 255):
        for n in (1, 65):
            x, _ = CC.logit_rows(n, nsym, 0)
            v = CC.place(x, ld, mis)
            assert v.shape == (n, nsym) and v.dtype == np.float32 and np.array_equal(v, x, equal_nan=True)
            assert v.strides == (4 * (nsym if ld is None else ld), 4)
            assert v.ctypes.data % 16 == (4 if mis else 0)
            base = v.base
            while base.base is not None:
                base = base.base
            assert np.isnan(base).sum() == base.size - n * nsym        # everything around the rows is NaN
    import torch
    t = torch.from_numpy(np.array(CC.logit_rows(65, 129, 0)[0]))
    v = CC.place(t, ld, mis)
    assert tuple(v.shape) == (65, 129) and v.stride() == (129 if ld is None else ld, 1) and v.data_ptr() % 16 == (4 if mis else 0)
    assert torch.equal(v, t)
