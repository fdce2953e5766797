"""Reflectance layer, host side: the definition (attr_ref) on the hard trees, the tables, the attribute file, and the range decoder's
row-per-context entry.  No GPU."""
import hashlib
import math

import numpy as np
import pytest

import attr_ref
from attr_cases import QS, cases

TABLE_SHA = {0: "90ef837a2cb26258093f1452efbead231cd4e395bef54e0b3d7e1a3d7f8392a4",
             15: "4f62c2a100799f9ef49fe304aa1e8029d0d58fc76457de65d9125f589991fa32"}


@pytest.mark.parametrize("name", sorted(cases()))
def test_q1_inverts_exactly(name):
    c = cases()[name]
    f = attr_ref.forward(c["leaves"], c["a"], c["D"], 1)
    U = len(c["leaves"])
    assert len(f["k"]) == len(f["ctx"]) == U - 1 and f["level_counts"][0] == U and f["level_counts"][-1] == 1
    assert 0 <= f["root"] <= 255 and max((attr_ref.symbol(k) for k in f["k"]), default=0) <= 510
    assert sum(map(sum, f["hist"])) == U - 1
    assert attr_ref.inverse(c["leaves"], c["D"], 1, f["root"], f["k"]) == c["a"].tolist()


@pytest.mark.parametrize("name", sorted(cases()))
@pytest.mark.parametrize("Q", QS[1:])
def test_lossy_steps_stay_in_the_alphabet_and_decode(name, Q):
    c = cases()[name]
    f = attr_ref.forward(c["leaves"], c["a"], c["D"], Q)
    assert max((attr_ref.symbol(k) for k in f["k"]), default=0) <= 510
    back = attr_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"])
    assert len(back) == len(c["a"]) and all(0 <= v <= 255 for v in back)


def test_cases_reach_what_they_are_for():
    cs = cases()
    f = attr_ref.forward(cs["full_255_first"]["leaves"], cs["full_255_first"]["a"], 2, 1)
    assert f["hist"][0][510] == 4                                    # d = -255 four times
    f = attr_ref.forward(cs["full_0_first"]["leaves"], cs["full_0_first"]["a"], 2, 1)
    assert f["hist"][0][509] == 4
    f = attr_ref.forward(cs["full_plus_one"]["leaves"], cs["full_plus_one"]["a"], 2, 1)
    assert f["level_counts"] == [9, 2, 1] and f["k"][0] < 0         # W = 8 + 1, d < 0
    f = attr_ref.forward(cs["chain21"]["leaves"], cs["chain21"]["a"], 21, 1)
    assert f["level_counts"] == [2] + [1] * 21 and f["ctx"] == [0]
    f = attr_ref.forward(cs["heavy"]["leaves"], cs["heavy"]["a"], 5, 8)
    assert f["level_counts"] == [4103, 519, 71, 15, 8, 1]
    r = cs["random"]
    assert r["q"].shape == (6000, 3) and r["cnt"].min() >= 1 and r["cnt"].sum() < 6000
    assert not np.isfinite(r["r"]).all() and (r["r"][np.isfinite(r["r"])] < 0).any() and (r["r"][np.isfinite(r["r"])] > 1).any()
    for ax in range(3):
        f = attr_ref.forward(cs[f"axis{ax}"]["leaves"], cs[f"axis{ax}"]["a"], 3, 1)
        assert f["k"] == [191] and f["ctx"] == [2]


def _pair(lo, hi, Q):
    """Two leaves of weight 1 that differ in the last bit of axis 2 -> (k, the values a decoder gets back)."""
    leaves = np.array([[0, 0, 0], [0, 0, 1]], np.int32)
    f = attr_ref.forward(leaves, [lo, hi], 1, Q)
    return f["k"][0], f["root"], attr_ref.inverse(leaves, 1, Q, f["root"], f["k"])


def test_worked_pairs():
    assert _pair(10, 17, 1) == (7, 13, [10, 17])
    assert (-7) // 2 == -4 and _pair(17, 10, 1) == (-7, 13, [17, 10])
    assert attr_ref.step(1, 1, 8) == 11 == math.isqrt(128)
    assert _pair(10, 17, 8) == (1, 13, [8, 19])


def test_half_rounds_up_and_thirds_round_to_nearest():
    lv = np.array([[1, 1, 1]], np.int32)
    q = np.array([[1, 1, 1]] * 3, np.int32)
    assert attr_ref.leaf_values(q[:2], [10 / 255, 11 / 255], lv, 2, 255) == ([11], [2])
    assert attr_ref.leaf_values(q, [10 / 255, 10 / 255, 11 / 255], lv, 2, 255) == ([10], [3])
    assert attr_ref.leaf_values(q, [10 / 255, 11 / 255, 11 / 255], lv, 2, 255) == ([11], [3])
    assert attr_ref.leaf_values(q, [np.nan, np.inf, 2.0], lv, 2, 255) == ([85], [3])
    assert attr_ref.leaf_values(q + 1, [0.5] * 3, lv, 2, 255) == ([0], [0])


def test_tables_are_whole_and_pinned():
    from scp_amd import attr
    t = attr_ref.tables()
    assert t.shape == (16, 512) and t.dtype == np.uint16
    assert np.array_equal(attr.tables(), t)
    c = attr.table_counts()
    assert (c >= 1).all() and (c.sum(axis=1) == 65536).all()
    assert (t[:, 0] == 0).all() and (t[:, 511] == 0).all()               # 65536 wraps to 0
    wide = t.astype(np.int64)
    wide[:, 511] = 65536
    assert (np.diff(wide, axis=1) >= 1).all()
    for g, sha in TABLE_SHA.items():
        assert hashlib.sha256(t[g].astype("<u2").tobytes()).hexdigest() == sha, g


def test_choose_tables_prefers_the_cheapest_and_the_lower_index_on_ties():
    from scp_amd import attr
    hist = np.zeros((3, 511), np.int64)
    hist[0, 0] = 1000                                      # all zeros: the steepest table
    hist[1, :] = 1                                         # flat: the flattest
    choice, bits = attr.choose_tables(hist)                # row 2 is empty: every table costs 0 bits, the tie goes to table 0
    assert choice.tolist() == [0, 15, 0] and bits[2] == 0.0
    c = attr.table_counts().astype(np.float64)
    assert bits[0] == pytest.approx(1000 * (16 - np.log2(c[0, 0])))


def test_step_is_the_floor_square_root_without_overflow():
    rng = np.random.default_rng(3)
    ws = [1, 2, 3, 7, 8, 9, 4096, (1 << 21) - 1, 1 << 21] + [int(v) for v in rng.integers(1, 1 << 21, size=40)]
    for w1 in ws:
        for w2 in ws:
            for Q in (1, 2, 8, 16, 254, 255):
                x = (Q * Q * (w1 + w2)) // (w1 * w2)
                s = attr_ref.step(w1, w2, Q)
                assert s == max(1, math.isqrt(x)) and (s == 1 or s * s <= x < (s + 1) * (s + 1))
                assert x <= 2 * 255 * 255 and Q * Q * (w1 + w2) < 1 << 63 and w1 * w2 < 1 << 63
                if Q == 1:
                    assert s == 1


def _shells():
    return [dict(D=12, U=5000, root=93, tables=[3] * 6 + [9] * 6, payload=bytes(range(200)) * 3),
            dict(D=13, U=1, root=255), dict(D=14, U=0),
            dict(D=3, U=2, root=0, tables=[0, 15, 7], payload=b"\x00")]


def test_pack_round_trips():
    from scp_amd import attr
    data = attr.pack(8, 255, _shells())
    assert data[:4] == b"SCPA" and data[4] == 1 and data[5] == 8
    Q, scale, shells = attr.unpack(data)
    assert (Q, scale, len(shells)) == (8, 255, 4)
    for got, want in zip(shells, _shells()):
        assert got["D"] == want["D"] and got["U"] == want["U"] and got["root"] == want.get("root")
        assert got["tables"] == want.get("tables", []) and got["payload"] == want.get("payload", b"")
    assert attr.pack(Q, scale, shells) == data
    assert attr.unpack(attr.pack(1, 1, []))[2] == []


def test_damaged_files_are_refused():
    from scp_amd import attr, native
    data = attr.pack(8, 255, _shells())
    for cut in (0, 3, 4, 10, 12, 16, 17, 25, 40, len(data) - 1):
        with pytest.raises(native.ScpError, match="truncated|magic"):
            attr.unpack(data[:cut])
    with pytest.raises(native.ScpError, match="magic"):
        attr.unpack(b"SCPB" + data[4:])
    with pytest.raises(native.ScpError, match="version"):
        attr.unpack(data[:4] + b"\x02" + data[5:])
    with pytest.raises(native.ScpError, match="behind"):
        attr.unpack(data + b"\x00")
    with pytest.raises(native.ScpError, match="Q 0"):
        attr.unpack(data[:5] + b"\x00" + data[6:])
    with pytest.raises(native.ScpError):
        attr.pack(0, 255, [])
    with pytest.raises(native.ScpError):
        attr.pack(1, 255, [dict(D=3, U=2, root=0, tables=[0, 16, 1], payload=b"")])


def test_level_contexts_and_symbols():
    from scp_amd import attr
    assert attr.level_contexts([9, 2, 1]).tolist() == [1] + [0] * 7
    assert attr.level_contexts([1, 1, 1]).tolist() == []
    ks = list(range(-255, 256))
    assert attr.symbols_to_coefficients([attr_ref.symbol(k) for k in ks]).tolist() == ks


def test_dec_run_ctx_equals_next_in_a_loop():
    """3 contexts (the two extremes of the grid and one in between), 5 000 symbols: the row-per-context entry decodes what
    scp_ac_dec_next decodes row by row; a context beyond the table is refused before anything is decoded."""
    from scp_amd import native
    rng = np.random.default_rng(7)
    rows = attr_ref.tables()[[0, 15, 8]]
    n = 5000
    ctx = rng.integers(0, 3, size=n).astype(np.uint8)
    k = np.where(ctx == 0, rng.integers(-2, 3, size=n), rng.integers(-255, 256, size=n))
    k[:4] = (255, -255, 0, 1)
    lohi = np.array(attr_ref.pairs(k.tolist(), ctx.tolist(), rows), np.uint32)
    stream = native.ac_encode_lohi(lohi)
    want = [attr_ref.symbol(int(v)) for v in k]
    one = native.AcDecoder(stream, Lp=512)
    assert [one.next(rows[c]) for c in ctx] == want
    got = native.AcDecoder(stream, Lp=512).run_ctx(rows, ctx)
    assert got.dtype == np.int16 and got.tolist() == want
    bad = ctx.copy()
    bad[-1] = 3
    d = native.AcDecoder(stream, Lp=512)
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):
        d.run_ctx(rows, bad)
    assert d.run_ctx(rows, ctx).tolist() == want                    # nothing was consumed by the refused call
    with pytest.raises(native.ScpError):
        native.AcDecoder(stream, Lp=256).run_ctx(rows, ctx)
    assert native.AcDecoder(stream, Lp=512).run_ctx(rows, ctx[:0]).tolist() == []
