"""Ring LOD without a GPU ("Ring LOD"): the properties of the integer rule as tests/ringlod_ref.py restates it, the threshold
conversion, the command-line syntax, the side-info entry with every refusal, and the file-name token."""
import json

import numpy as np
import pytest

import ringlod_ref as ref

TABLES = [([], [3]), ([40], [2, 0]), ([100, 900, 2000], [0, 3, 1, 2]), ([7, 7, 64], [1, 4, 0, 8]), ([0, 5], [5, 2, 6]),
          ([1000, 3000], [8, 0, 3])]


def random_tables(seed, count=12):
    rng = np.random.default_rng(seed)
    out = list(TABLES)
    for _ in range(count):
        r = int(rng.integers(1, 7))
        out.append((sorted(int(v) for v in rng.integers(0, 4096, r - 1)), [int(v) for v in rng.integers(0, 9, r)]))
    return out


@pytest.mark.parametrize("k", range(len(random_tables(3))))
def test_the_snap_is_idempotent_and_lands_every_point_of_a_terminal_cell_on_its_origin(k):
    thr, drops = random_tables(3)[k]
    rng = np.random.default_rng(100 + k)
    q = rng.integers(0, 4096, (3000, 3))
    if thr:                                                  # rows next to every threshold
        near = np.concatenate([np.arange(t - 300, t + 300) for t in thr])
        q = np.concatenate((q, np.stack((np.clip(near, 0, None), rng.integers(0, 4096, near.shape), rng.integers(0, 4096, near.shape)), 1)))
    snapped, j = ref.snap(q, thr, drops)
    again, j2 = ref.snap(snapped, thr, drops)
    assert np.array_equal(again, snapped)                    # idempotent
    assert np.array_equal(j2, j)                             # J of a snapped point is J of the original
    assert j.min() >= 0 and j.max() <= max(drops)
    assert np.array_equal(snapped, (q >> j[:, None]) << j[:, None])
    # every point inside a terminal cell lands on that cell's origin: for every size, the points whose enclosing cell of that size is
    # terminal and is the largest such cell
    for size in range(1, max(drops) + 1):
        origin0 = (q[:, 0] >> size) << size
        terminal = np.asarray(drops)[ref.ring_of(2 * origin0 + 2 ** size - 1, thr)] >= size
        assert (j[terminal] >= size).all()
        inside = terminal & (j == size)
        assert np.array_equal(snapped[inside], (q[inside] >> size) << size)
    # a node of the snapped tree is implied iff it lies inside a terminal cell; its points are its origin
    for size in range(1, 10):
        origins = (snapped >> size) << size
        imp = ref.implied(origins, size, thr, drops)
        assert np.array_equal(snapped[imp], origins[imp])
        assert not imp.any() or size <= max(drops)
    assert not ref.implied(snapped, max(drops) + 1, thr, drops).any()        # a start size above kmax gives 0


def test_non_monotone_drops_take_the_largest_terminal_cell():
    thr, drops = [100, 900, 2000], [0, 3, 1, 2]
    x = np.array([0, 99, 100, 103, 104, 899, 900, 901, 1999, 2000, 2001, 4095])
    j = ref.J(x, 0, thr, drops)
    # worked by hand.  Ring 0 (drop 0) holds c2 < 200: the cell [96, 104) has c2 = 199 and is not terminal, [100, 104) has c2 = 203: ring 1
    # (drop 3), terminal at size 4.  [896, 904) has c2 = 1799 < 1800: ring 1, terminal at size 8 - it takes 900 and 901 with it, whose
    # own small cells lie in ring 2 (drop 1).  [1992, 2000) has c2 = 3991: ring 2, too large for drop 1; [2000, 2008) is ring 3 (drop 2).
    assert j.tolist() == [0, 0, 2, 2, 3, 3, 3, 3, 1, 2, 2, 2]
    assert ref.J(x, 2, thr, drops).tolist() == [0, 0, 2, 2, 3, 3, 3, 3, 0, 2, 2, 2]
    assert ref.J(x, 4, thr, drops).tolist() == [0] * len(x)
    c = ref.centres(np.array([[104, 8, 16], [5, 6, 7]]), np.array([3, 0]))
    assert c.tolist() == [[107.5, 11.5, 19.5], [5.0, 6.0, 7.0]]


def test_threshold_conversion_on_edges_that_fall_on_a_lattice_value():
    from scp_amd import native
    for f in (ref.thresholds, native.ringlod_thresholds):
        assert f([0, 10, 25], 0.5, 0.0) == [20, 50]                          # exactly on the lattice: q >= 20 is at or beyond 10
        assert f([0, 10, 25], 0.5, 0.25) == [20, 50]                         # 19.5 -> 20, 49.5 -> 50
        assert f([0, 10, 25], 0.5, -0.25) == [21, 51]
        assert f([0, 1.0], 2.0 ** -10, 0.0) == [1024]
        assert f([0, 1.0, 2.0], 1.0, 5.0) == [0, 0]                          # clamped at 0
        assert f([0, 1e30], 1e-3, 0.0) == [2 ** 31 - 1]                      # clamped at 2^31 - 1
        assert f([0], 1.0, 0.0) == []
    qs = 400 / (2 ** 12 - 1)                                                 # the L12 step: 10 / qs is not an integer
    for edges in ([0, 10, 25], [0, 5, 40, 80]):
        got = native.ringlod_thresholds(edges, qs, 0.0)
        assert got == ref.thresholds(edges, qs, 0.0)
        for e, t in zip(edges[1:], got):
            assert t * qs >= e > (t - 1) * qs


def test_cli_parsing():
    from scp_amd import cli, native
    assert cli.parse_ring_lod("0,10,25:2,1,0") == ((0.0, 10.0, 25.0), (2, 1, 0))
    assert cli.parse_ring_lod("0:3") == ((0.0,), (3,))
    args = cli.get_args(["--ring_lod", "0,10,25:2,0,1", "--type", "kitti", "--spher"])
    assert cli.ring_lod_request(args) == ((0.0, 10.0, 25.0), (2, 0, 1))
    assert cli.ring_lod_request(cli.get_args(["--type", "kitti"])) is None
    for bad, why in (("0,10,25", "EDGES:DROPS"), ("0,10:1,x", "EDGES:DROPS"), ("0,10:1", "one drop per ring"), ("0,10:1,2,3", "one drop per ring"),
                     ("5,10:1,2", "ascending from 0|start at 0"), ("0,10,10:1,2,3", "ascending from 0|start at 0"), ("0,10:1,9", "0 .. 8"),
                     ("0,10:-1,2", "0 .. 8"), ("0,a:1,2", "--ring_lod")):
        with pytest.raises(native.ScpError, match=why):
            cli.parse_ring_lod(bad)
    # refusals that need no device
    import argparse
    def ns(**kw):
        base = dict(spher=True, cylin=False, type="kitti", preproc_path="", level_wise=False, metrics=False, sequential=False,
                    ring_lod=((0.0, 10.0), (1, 0)))
        base.update(kw)
        return argparse.Namespace(**base)
    cli.refuse_unsupported(ns(), "EHEM", False)
    cli.refuse_unsupported(ns(), "EHEM", True)
    for kw, name, why in ((dict(), "OctAttention", "EHEM encoders only"), (dict(type="obj", spher=False), "EHEM", "--type obj"),
                          (dict(spher=False), "EHEM", "no radial axis"), (dict(preproc_path="x/"), "EHEM", "--preproc_path")):
        with pytest.raises(native.ScpError, match=why):
            cli.refuse_unsupported(ns(**kw), name, False)


def test_encoder_argument_checks_need_no_device():
    from scp_amd import native
    from scp_amd.encoder import parse_ring_lod
    assert parse_ring_lod(None) is None
    assert parse_ring_lod(([0, 10, 25], [0, 0, 0])) is None                  # all drops 0: the option is off
    assert parse_ring_lod(([0, 10, 25], [2, 0, 1])) == ((0.0, 10.0, 25.0), (2, 0, 1))
    for bad, why in ((([0, 10], [1]), "one drop per ring"), (([0, 10], [1, 9]), "0 .. 8"), (([0, 10], [1, 1.5]), "0 .. 8"), (([0, 10], [True, 1]), "0 .. 8"),
                     (([1, 10], [1, 1]), "not ascending from 0"), (([0, 10, 5], [1, 1, 1]), "not ascending from 0"),
                     ((list(range(33)), [1] * 33), "at most 32"), (5, "expected")):
        with pytest.raises(native.ScpError, match=why):
            parse_ring_lod(bad)


def test_the_name_token_with_and_without_temper():
    from scp_amd.decoder import is_ringlod, is_tempered
    for name, ring, temper in (("a/000001_ringlod_spher_12_4097_0.bin", True, False), ("a/000001_ringlod_temper_spher_12_4097_0.bin", True, True),
                               ("a/000001_ringlod_temper_cylin_42_4097_-3.bin", True, True), ("a/000001_temper_spher_12_4097_0.bin", False, True),
                               ("a/000001_spher_12_4097_0.bin", False, False), ("a/ringlod_spher_12_4097_0.bin", True, False),
                               ("a/ringlod_000001_spher_12_4097_0.bin", False, False), ("a/000001_temper_ringlod_spher_12_4097_0.bin", True, False),
                               ("a/000001_ringlod_12_4097_0.bin", True, False), ("a/x_ringlod_temper_12_4097_0.bin", True, True),
                               ("12_4097_0.bin", False, False)):
        assert is_ringlod(name) == ring, name
        assert is_tempered(name) == temper, name


class _Enc:
    data_type, lidar_level, mullevel, spher, cylin, profile, temper = "kitti", 12, False, True, False, None, None
    ring_lod = ((0.0, 10.0, 25.0), (2, 0, 1))

    @staticmethod
    def outfile(base, res):
        from scp_amd.encoder import FrameEncoder
        return FrameEncoder.outfile(_Enc, base, res)

    _temper_token = staticmethod(lambda base: base)
    _ring_token = staticmethod(lambda base: base + "_ringlod")


def test_side_info_entry_is_written_required_and_refused_when_malformed(tmp_path, monkeypatch):
    from scp_amd import decoder, native
    monkeypatch.setattr(native, "numeric_profile", lambda *a, **k: "ehem/test")
    res = dict(n_points=10, n_nodes=20, bin_num=4097.0, z_offset=0.0, n_levels=12,
               ring_lod=dict(edges=[0.0, 10.0, 25.0], drops=[2, 0, 1], thresholds=[[103, 256]], snapped=[1, 2, 3], implied_rows=4, leaves=[5]))
    out = _Enc.outfile(str(tmp_path / "f"), res)
    assert out.endswith("f_ringlod_spher_12_4097_0.bin")
    side = decoder.write_sidecar(out, _Enc, res, "EHEM")
    assert side["ring_lod"] == dict(drops=[2, 0, 1], thresholds=[[103, 256]]) and json.load(open(out + decoder.SIDECAR)) == side
    good = decoder.stream_ringlod(out, side, 12, False)
    assert good == dict(drops=(2, 0, 1), thresholds=[(103, 256)])
    # the entry is ignored for a name without the field
    assert decoder.stream_ringlod(str(tmp_path / "f_spher_12_4097_0.bin"), side, 12, False) is None
    assert decoder.stream_ringlod(str(tmp_path / "f_temper_spher_12_4097_0.bin"), dict(side, ring_lod="junk"), 12, False) is None
    # a plain encoder writes no entry
    class Plain(_Enc):
        ring_lod = None
    assert "ring_lod" not in decoder.write_sidecar(str(tmp_path / "g_spher_12_4097_0.bin"), Plain, res, "EHEM")

    def bad(entry, why, n_levels=12, mullevel=False, **kw):
        s = None if entry is None else dict(side, **kw)
        if entry not in (None, "missing"):
            s["ring_lod"] = entry
        elif entry == "missing":
            s.pop("ring_lod")
        with pytest.raises(native.ScpError, match=why):
            decoder.stream_ringlod(out, s, n_levels, mullevel)

    bad(None, "without its side-info file")
    bad("missing", "no `ring_lod` entry")
    bad([1, 2], "no `ring_lod` entry")
    bad(dict(drops=[2, 0, 1]), "no `ring_lod` entry")
    bad(dict(drops=[2, 0.5, 1], thresholds=[[103, 256]]), "`drops` is not a list of integers")
    bad(dict(drops=[2, True, 1], thresholds=[[103, 256]]), "`drops` is not a list of integers")
    bad(dict(drops=[2, 0, 1], thresholds=[[103.0, 256]]), r"`thresholds\[0\]` is not a list of integers")
    bad(dict(drops=[2, 0, 1], thresholds=[103, 256]), "thresholds of 2 shells")
    bad(dict(drops=[2, 0, 1], thresholds=[[256, 103]]), "descending")
    bad(dict(drops=[2, 0, 1], thresholds=[[-1, 103]]), "negative")
    bad(dict(drops=[2, 0, 1], thresholds=[[103, 2 ** 31]]), "beyond")
    bad(dict(drops=[2, 0, 1], thresholds=[[103, 256], [103, 256]]), "thresholds of 2 shells, the stream has 1")
    bad(dict(drops=[2, 0, 1], thresholds=[[103, 256]]), "thresholds of 1 shells, the stream has 3", n_levels=45, mullevel=True)
    bad(dict(drops=[2, 0], thresholds=[[103, 256]]), "one more drop than thresholds")
    bad(dict(drops=[2, 0, 1, 1], thresholds=[[103, 256]]), "one more drop than thresholds")
    bad(dict(drops=[], thresholds=[[]]), "1 .. 32 rings")
    bad(dict(drops=[2, 0, 9], thresholds=[[103, 256]]), "drop 9 out of range: 0 .. 8")
    bad(dict(drops=[2, 0, -1], thresholds=[[103, 256]]), "drop -1 out of range")
    bad(dict(drops=[2, 0, 4], thresholds=[[103, 256]]), "drop 4 out of range: 0 .. 3", n_levels=4)
    # three shells: depths m - 1, m, m + 1 with m = n_levels // 3
    three = dict(drops=[2, 0, 1], thresholds=[[103, 256], [206, 512], [412, 1024]])
    assert decoder.stream_ringlod(out, dict(side, ring_lod=three), 45, True)["thresholds"][2] == (412, 1024)
    # _ehem_job refuses before the stream is read: the stream file does not even exist
    import torch
    torch.save(torch.zeros((12, 2)), out + ".dat")
    json.dump(dict(side, ring_lod=dict(drops=[2, 0, 1], thresholds=[[256, 103]])), open(out + decoder.SIDECAR, "w"))
    with pytest.raises(native.ScpError, match="descending"):
        decoder._ehem_job(out)


def test_find_stream_takes_the_ringlod_field(tmp_path):
    from scp_amd import cli, native
    for name in ("seq000001_ringlod_temper_spher_12_4097_0.bin", "000002_ringlod_cylin_12_4097_-2.bin", "000003_spher_12_4097_0.bin"):
        (tmp_path / name).write_bytes(b"")
    root = str(tmp_path) + "/"
    assert cli.find_stream(root, "data/seq/000001.bin") == ("seq000001_ringlod_temper_spher_12_4097_0.bin", "seq000001")
    assert cli.find_stream(root, "000002.bin") == ("000002_ringlod_cylin_12_4097_-2.bin", "000002")
    assert cli.find_stream(root, "000003.bin") == ("000003_spher_12_4097_0.bin", "000003")
    (tmp_path / "000003_ringlod_spher_12_4097_0.bin").write_bytes(b"")
    with pytest.raises(native.ScpError, match="2 streams match"):
        cli.find_stream(root, "000003.bin")
