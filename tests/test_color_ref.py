"""Colour layer, host side: the colour transform over all 2^24 colours, the definition (color_ref) on the hard trees, the wide tables, the
colour file, the PLY reader and writer, the command line's refusals and the range coder under the 1021-symbol alphabet.  No GPU."""
import numpy as np
import pytest

import attr_ref
import color_ref
from color_cases import QS, cases


def test_ycocg_r_is_exact_on_all_colours():
    v = np.arange(1 << 24, dtype=np.int32)
    R, G, B = v >> 16, (v >> 8) & 255, v & 255
    Co = R - B
    t = B + (Co >> 1)
    Cg = G - t
    Y = t + (Cg >> 1)
    assert Y.min() == 0 and Y.max() == 255 and Co.min() == -255 and Co.max() == 255 and Cg.min() == -255 and Cg.max() == 255
    t2 = Y - (Cg >> 1)
    G2 = Cg + t2
    B2 = t2 - (Co >> 1)
    assert np.array_equal(G2, G) and np.array_equal(B2, B) and np.array_equal(B2 + Co, R)
    for i in np.random.default_rng(1).integers(0, 1 << 24, size=2000).tolist() + [0, (1 << 24) - 1, 0xFF0000, 0x00FF00, 0x0000FF]:
        c = (int(R[i]), int(G[i]), int(B[i]))
        assert color_ref.rgb_to_ycc(*c) == (int(Y[i]), int(Co[i]), int(Cg[i])) and color_ref.ycc_to_rgb(int(Y[i]), int(Co[i]), int(Cg[i])) == c


def test_tables_of_both_alphabets():
    from scp_amd import attr, native
    assert np.array_equal(attr.tables(511), attr_ref.tables()) and np.array_equal(attr.tables(), attr_ref.tables())
    t = color_ref.tables()
    assert t.shape == (16, 1022) and t.dtype == np.uint16 and native.COLOR_ALPHABET == 1021
    assert np.array_equal(attr.tables(1021), t)
    c = attr.table_counts(1021)
    assert c.shape == (16, 1021) and (c >= 1).all() and (c.sum(axis=1) == 65536).all()
    assert (t[:, 0] == 0).all() and (t[:, 1021] == 0).all()             # 65536 wraps to 0
    wide = t.astype(np.int64)
    wide[:, 1021] = 65536
    assert (np.diff(wide, axis=1) >= 1).all()
    with pytest.raises(native.ScpError):
        attr.tables(512)
    # the price of coding Y under the wide alphabet: 510 counts of 65536 are reserved for symbols Y never emits
    assert -np.log2(1 - 510 / 65536) < 0.0113


@pytest.mark.parametrize("name", sorted(cases()))
def test_q1_returns_the_leaf_means(name):
    c = cases()[name]
    f = color_ref.forward(c["leaves"], c["ycc"], c["D"], 1)
    U = len(c["leaves"])
    assert [len(p) for p in f["k"]] == [U - 1] * 3 and len(f["ctx"]) == U - 1 and f["level_counts"][0] == U and f["level_counts"][-1] == 1
    assert 0 <= f["root"][0] <= 255 and all(-255 <= v <= 255 for v in f["root"][1:])
    assert sum(map(sum, f["hist"])) == 3 * (U - 1) and len(f["hist"]) == 3 * c["D"]
    assert color_ref.inverse(c["leaves"], c["D"], 1, f["root"], f["k"]) == c["rgb"].tolist()
    # the Y plane is the reflectance layer's transform of the Y values
    g = attr_ref.forward(c["leaves"], c["ycc"][0], c["D"], 1)
    assert g["k"] == f["k"][0] and g["ctx"] == f["ctx"] and g["root"] == f["root"][0] and g["level_counts"] == f["level_counts"]


@pytest.mark.parametrize("name", sorted(cases()))
@pytest.mark.parametrize("Q", QS)
def test_coefficients_stay_in_the_alphabet(name, Q):
    c = cases()[name]
    f = color_ref.forward(c["leaves"], c["ycc"], c["D"], Q)
    assert max((abs(k) for k in f["k"][0]), default=0) <= 255
    assert max((abs(k) for p in f["k"] for k in p), default=0) <= 510
    assert max((attr_ref.symbol(k) for p in f["k"] for k in p), default=0) <= 1020
    back = color_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"])
    assert len(back) == len(c["rgb"]) and all(0 <= v <= 255 for p in back for v in p)


def test_cases_reach_what_they_are_for():
    cs = cases()
    assert color_ref.forward(cs["co_red_first"]["leaves"], cs["co_red_first"]["ycc"], 2, 1)["hist"][2 + 0][1020] == 4       # Co, level 1
    assert color_ref.forward(cs["co_blue_first"]["leaves"], cs["co_blue_first"]["ycc"], 2, 1)["hist"][2 + 0][1019] == 4
    assert color_ref.forward(cs["cg_green_first"]["leaves"], cs["cg_green_first"]["ycc"], 2, 1)["hist"][4 + 0][1020] == 4    # Cg, level 1
    assert color_ref.forward(cs["cg_magenta_first"]["leaves"], cs["cg_magenta_first"]["ycc"], 2, 1)["hist"][4 + 0][1019] == 4
    r = cs["random"]
    assert r["q"].shape == (6000, 3) and r["rgb8"].shape == (6000, 3) and r["cnt"].min() >= 1 and r["cnt"].sum() < 6000
    assert (r["q"] < 0).any() and (r["q"] >= 1 << 12).any()


def test_half_rounds_up_and_thirds_round_to_nearest():
    lv = np.array([[1, 1, 1]], np.int32)
    q = np.array([[1, 1, 1]] * 3, np.int32)
    mean, ycc, cnt = color_ref.leaf_values(q[:2], [(10, 0, 255), (11, 1, 254)], lv, 2)
    assert (mean, cnt) == ([[11, 1, 255]], [2]) and [p[0] for p in ycc] == list(color_ref.rgb_to_ycc(11, 1, 255))
    assert color_ref.leaf_values(q, [(10, 10, 0)] * 2 + [(11, 13, 1)], lv, 2)[0] == [[10, 11, 0]]
    assert color_ref.leaf_values(q + 1, [(9, 9, 9)] * 3, lv, 2)[::2] == ([[0, 0, 0]], [0])
    assert [color_ref.point_color(v) for v in (np.nan, np.inf, -np.inf, -3.0, 0.49, 0.5, 254.5, 300.0)] == [0, 0, 0, 0, 0, 1, 255, 255]


def _shells():
    return [dict(D=4, U=5000, root=(93, -255, 255), tables=[3] * 4 + [9] * 4 + [15] * 4, payload=bytes(range(200)) * 3),
            dict(D=13, U=1, root=(255, 0, -1)), dict(D=14, U=0),
            dict(D=1, U=2, root=(0, 7, -7), tables=[0, 15, 7], payload=b"\x00")]


def test_pack_round_trips():
    from scp_amd import color
    data = color.pack(8, _shells())
    assert data[:4] == b"SCPC" and tuple(data[4:8]) == (1, 8, 1, 4)
    Q, shells = color.unpack(data)
    assert (Q, len(shells)) == (8, 4)
    for got, want in zip(shells, _shells()):
        assert got["D"] == want["D"] and got["U"] == want["U"] and got["root"] == want.get("root")
        assert got["tables"] == want.get("tables", []) and got["payload"] == want.get("payload", b"")
    assert color.pack(Q, shells) == data
    assert color.unpack(color.pack(1, []))[1] == []


def test_damaged_files_are_refused():
    from scp_amd import color, native
    data = color.pack(8, _shells())
    for cut in (0, 3, 4, 7, 10, 13, 16, 20, 30, 40, len(data) - 1):
        with pytest.raises(native.ScpError, match="truncated|magic"):
            color.unpack(data[:cut])
    with pytest.raises(native.ScpError, match="magic"):
        color.unpack(b"SCPA" + data[4:])
    with pytest.raises(native.ScpError, match="version"):
        color.unpack(data[:4] + b"\x02" + data[5:])
    with pytest.raises(native.ScpError, match="unknown colour transform 2"):
        color.unpack(data[:6] + b"\x02" + data[7:])
    with pytest.raises(native.ScpError, match="behind"):
        color.unpack(data + b"\x00")
    with pytest.raises(native.ScpError, match="Q 0"):
        color.unpack(data[:5] + b"\x00" + data[6:])
    at = 8 + 5 + 5                                              # shell 0's first table index
    assert data[at:at + 4] == b"\x03" * 4
    with pytest.raises(native.ScpError, match="names table 16"):
        color.unpack(data[:at] + b"\x10" + data[at + 1:])
    with pytest.raises(native.ScpError):
        color.pack(0, [])
    with pytest.raises(native.ScpError):
        color.pack(1, [dict(D=1, U=2, root=(0, 0, 0), tables=[0, 16, 1], payload=b"")])
    with pytest.raises(native.ScpError):
        color.pack(1, [dict(D=1, U=2, root=(0, 0, 0), tables=[0, 1], payload=b"")])
    with pytest.raises(native.ScpError):
        color.pack(1, [dict(D=1, U=1, root=(0, 256, 0))])


def test_loadply_returns_colours_and_the_default_call_is_unchanged(tmp_path):
    from scp_amd.data_preproc import pt
    xyz = np.array([[1.5, 2.0, 3.0], [4.0, 5.0, 6.25], [7.0, 8.0, 9.0]], np.float32)
    rgb = np.array([[0, 128, 255], [1, 2, 3], [250, 251, 252]], np.uint8)
    with_c, without, short = str(tmp_path / "c.ply"), str(tmp_path / "g.ply"), str(tmp_path / "s.ply")
    pt.write_ply_colors(with_c, xyz, rgb)
    pt.write_ply_data(without, xyz)
    lines = open(with_c).read().splitlines()
    assert lines[:3] == ["ply", "format ascii 1.0", "element vertex 3"] and lines[6:10] == ["property uchar red", "property uchar green",
                                                                                            "property uchar blue", "end_header"]
    assert lines[10] == "1.5 2.0 3.0 0 128 255" and open(without).read().splitlines()[7:] == [ln.rsplit(" ", 3)[0] for ln in lines[10:]]
    p, c = pt.loadply(with_c, "rgb")
    assert p.dtype == np.float32 and c.dtype == np.float32 and np.array_equal(p, xyz) and np.array_equal(c, rgb.astype(np.float32))
    assert pt.pcread(with_c, "rgb")[1].shape == (3, 3)
    for path in (with_c, without):                             # the default call: points only
        p, c = pt.loadply(path)
        assert np.array_equal(p, xyz) and c is None
        assert pt.loadply(path, "geometry")[1] is None and np.array_equal(pt.ptread(path), xyz)
    p, c = pt.loadply(without, "rgb")
    assert np.array_equal(p, xyz) and c is None
    open(short, "w").write("\n".join(lines[:11] + ["4.0 5.0 6.25 1 2"] + lines[12:]) + "\n")
    p, c = pt.loadply(short, "rgb")                            # one short line: the whole file falls back
    assert np.array_equal(p, xyz) and c is None
    with pytest.raises(ValueError):
        pt.write_ply_colors(with_c, xyz, rgb[:2])


def test_synthetic_object_and_colours():
    from scp_amd.synth import synth_colors, synth_object
    x = synth_object(3, 4096)
    assert x.shape == (4096, 3) and x.min() >= 0 and x.max() < 1024 and len(np.unique(x, axis=0)) == 4096
    assert np.array_equal(x, synth_object(3, 4096)) and not np.array_equal(x, synth_object(4, 4096))
    c = synth_colors(x, 3)
    assert c.shape == (4096, 3) and c.dtype == np.uint8 and c.std(axis=0).min() > 20 and np.array_equal(c, synth_colors(x, 3))


def test_refusals_name_the_flag(tmp_path):
    from scp_amd import cli, native
    from scp_amd.data_preproc import pt
    good, plain = str(tmp_path / "c.ply"), str(tmp_path / "g.ply")
    pt.write_ply_colors(good, np.zeros((2, 3)), np.zeros((2, 3), np.uint8))
    pt.write_ply_data(plain, np.zeros((2, 3)))

    def refuse(argv, name="EHEM", mullevel=False):
        cli.refuse_unsupported(cli.get_args(argv, mullevel), name, mullevel)

    base = ["--test_files", good, "--type", "obj"]
    refuse(base + ["--color"])
    refuse(base + ["--color", "255"])
    assert cli.color_request(cli.get_args(base)) is None and cli.color_request(cli.get_args(base + ["--color"])) == 1
    for argv, kw, why in ((["--test_files", good, "--type", "kitti", "--color"], {}, "--type kitti.*--attr"),
                          (["--test_files", good, "--type", "ford", "--color"], {}, "--type ford.*--attr"),
                          (["--test_files", good, "--type", "kitti", "--color"], dict(mullevel=True), "--type kitti.*--attr"),
                          (base + ["--color"], dict(name="OctAttention"), "EHEM encoders only"),
                          (base + ["--color", "--preproc_path", "pp/"], {}, "--preproc_path"),
                          (base + ["--color", "0"], {}, "1 .*\\.\\. 255"), (base + ["--color", "256"], {}, "1 .*\\.\\. 255"),
                          (["--test_files", plain, "--type", "obj", "--color"], {}, "no colour columns"),
                          (["--test_files", str(tmp_path / "none.ply"), "--type", "obj", "--color"], {}, "no colour columns")):
        with pytest.raises(native.ScpError, match="--color") as e:
            refuse(argv, **kw)
        assert __import__("re").search(why, str(e.value)), (argv, str(e.value))
    with pytest.raises(native.ScpError, match="--type obj"):                     # the multi-level command line has no object form
        refuse(base + ["--color"], mullevel=True)
    with pytest.raises(native.ScpError, match="--attr.*--type obj files have points only"):
        refuse(base + ["--attr"])
    with pytest.raises(native.ScpError, match="--attr.*--type obj"):
        refuse(base + ["--attr", "--color"])
    assert cli.get_decode_args(["--color"]).color and not cli.get_decode_args([]).color


def test_range_coder_under_the_wide_alphabet():
    """ac_encode_lohi on the reference's pairs, then AcDecoder(Lp = 1022).run_ctx: three channels of two levels, the extremes of the
    alphabet, and a plane that is z = 1020 throughout."""
    from scp_amd import native
    rng = np.random.default_rng(9)
    D, n = 2, 3000
    rows = color_ref.tables()[[0, 8, 15, 3, 15, 12]]
    ctx = rng.integers(0, D, size=n).tolist()
    k = [rng.integers(-2, 3, size=n).tolist(), [-510] * n, rng.integers(-510, 511, size=n).tolist()]
    k[2][:4] = [510, -510, 0, 1]
    lohi = np.array(color_ref.pairs(k, ctx, rows, D), np.uint32)
    assert len(lohi) == 3 * n
    stream = native.ac_encode_lohi(lohi)
    want = [attr_ref.symbol(v) for p in k for v in p]
    assert want[n:2 * n] == [1020] * n and max(want) == 1020 and 1019 in want
    sym_ctx = np.array(color_ref.payload_contexts(ctx, D), np.uint8)
    got = native.AcDecoder(stream, Lp=1022).run_ctx(rows, sym_ctx)
    assert got.dtype == np.int16 and got.tolist() == want
    from scp_amd import attr
    assert attr.symbols_to_coefficients(got).reshape(3, n).tolist() == k
    with pytest.raises(native.ScpError):
        native.AcDecoder(stream, Lp=512).run_ctx(rows, sym_ctx)
