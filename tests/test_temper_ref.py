"""Per-level temperature without a GPU: the reference's chooser (temper_ref.py) against brute force, the exported symbols and every
argument check of scp_temper_sweep / scp_temper_choose / scp_scale_rows, and the file-name / side-info logic of tempered streams."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import temper_ref


def _lib_or_skip():
    from scp_amd import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("library not built")
    return native.lib()


# ------------------------------------------------------------------------------------------------------------ the choice rule
def _brute(sums, unit, min_gain, bad, rows):
    """The rule spelt out the long way: every index that attains the minimum, the nearest to unit among them, the lower of two equally
    near; then the three reasons to stay."""
    lo = min(sums)
    cands = [k for k in range(len(sums)) if sums[k] == lo]
    near = min(abs(k - unit) for k in cands)
    best = min(k for k in cands if abs(k - unit) == near)
    if bad or rows == 0:
        return unit
    if sums[unit] - sums[best] > min_gain:
        return best
    return unit


def test_reference_chooser_against_brute_force_on_random_sums():
    rng = np.random.default_rng(11)
    for trial in range(400):
        nt = int(rng.integers(1, 33))
        unit = int(rng.integers(0, nt))
        # few distinct values: exact ties are the rule, not the exception
        sums = [float(v) for v in rng.integers(0, 6, nt) * 8.0 + 100.0]
        bad, rows = bool(trial % 7 == 0), 0 if trial % 11 == 0 else 5
        for gain in (0.0, 8.0, 16.0):
            assert temper_ref.pick(sums, unit, gain, bad=bad, rows=rows) == _brute(sums, unit, gain, bad, rows), (sums, unit, gain, bad, rows)


def test_ties_go_to_the_index_nearest_unit_then_to_the_lower_one():
    assert temper_ref.pick([5.0, 50.0, 100.0, 50.0, 5.0], 2, 8.0) == 0             # equally near: the lower index
    assert temper_ref.pick([5.0, 50.0, 100.0, 5.0, 50.0], 2, 8.0) == 3             # the nearer one
    assert temper_ref.pick([5.0, 5.0, 100.0, 50.0, 50.0], 2, 8.0) == 1
    assert temper_ref.pick([7.0, 7.0, 7.0], 1, 0.0) == 1                           # nothing beats unit: unit


def test_a_gain_exactly_equal_to_min_gain_stays():
    assert temper_ref.pick([92.0, 100.0], 1, 8.0) == 1                             # exactly the byte: not MORE than it
    assert temper_ref.pick([np.nextafter(92.0, 0.0), 100.0], 1, 8.0) == 0
    assert temper_ref.pick([92.0, 100.0], 1, 8.0, bad=False, rows=3) == 1


def test_a_bad_segment_and_an_empty_group_stay_at_unit():
    betas = temper_ref.default_grid()
    unit = int(np.flatnonzero(betas == 1.0)[0])
    nt = len(betas)
    seg_bits = np.full((5, nt), 1000.0)
    seg_bits[:, 0] = 10.0                                                          # every group would move to index 0
    seg_bad = np.zeros((5, nt), np.int64)
    seg_bad[3, 7] = 1                                                              # one bad row, at a column nobody would choose
    seg_off = [0, 10, 20, 20, 30, 40]                                              # segment 2 is empty
    group = [0, 0, 2, 1, 3]                                                        # group 1: the bad one; 2: no rows; 3: fine
    r = temper_ref.choose(seg_bits, seg_bad, seg_off, group, 4, betas, unit)
    assert r["choice"].tolist() == [0, unit, unit, 0]
    assert r["group_bits"][0].tolist() == [2000.0, 20.0] and r["group_bits"][1].tolist() == [1000.0, 1000.0]
    assert r["seg_beta"].tolist() == [betas[0], betas[0], 1.0, 1.0, betas[0]]
    # group ids are clamped, never followed out of range
    r2 = temper_ref.choose(seg_bits, seg_bad, seg_off, [0, 0, 2, 1, 99], 4, betas, unit)
    assert r2["choice"].tolist() == r["choice"].tolist() and np.array_equal(r2["group_bits"], r["group_bits"])


def test_group_sums_are_serial_in_segment_order():
    seg = np.array([[1e16], [1.0], [-1e16], [1.0]])
    assert temper_ref.group_sums(seg, [0, 0, 0, 0], 1)[0, 0] == ((1e16 + 1.0) - 1e16) + 1.0 == 1.0
    assert temper_ref.group_sums(seg, [0, 1, 0, 1], 2)[:, 0].tolist() == [0.0, 2.0]


def test_default_grid_and_the_scaled_row():
    from scp_amd import native
    g, unit = native.temper_grid()
    assert np.array_equal(g, temper_ref.default_grid()) and g.dtype == np.float32 and len(g) == 25 and unit == 12 and g[unit] == 1.0
    assert abs(g[0] - 0.3535534) < 1e-6 and abs(g[-1] - 2.828427) < 1e-6 and (np.diff(g) > 0).all()
    for bad in ([], [0.5, 2.0], [1.0, 1.0], [1.0, -2.0], [1.0, float("inf")], [1.0, float("nan")], [1.0] + [2.0] * 32):
        with pytest.raises(native.ScpError):
            native.temper_grid(bad)
    assert native.temper_grid([1.0]) [1] == 0
    x = np.array([[0.1, -np.inf, 3.0]], np.float32)
    assert temper_ref.scale(x, 1.0).tobytes() == x.tobytes()
    y = temper_ref.scale(x, g[3])
    assert y.dtype == np.float32 and y[0, 1] == -np.inf and y[0, 0] == np.float32(g[3] * np.float32(0.1))
    bits, bad = temper_ref.row_bits(np.zeros((2, 255), np.float32), [3, 4], g)
    assert np.allclose(bits, np.log2(255.0), atol=1e-12) and not bad.any()               # a flat row costs log2(255) at every temperature


# ------------------------------------------------------------------------------------------------------------ the library's argument checks
def test_library_exports_the_temper_entry_points():
    L = _lib_or_skip()
    for name in ("scp_temper_workspace_bytes", "scp_temper_sweep", "scp_temper_choose", "scp_scale_rows"):
        assert hasattr(L, name), name
    assert L.scp_temper_workspace_bytes(0, 3, 25) == 0
    ws = L.scp_temper_workspace_bytes(1000, 3, 25)
    assert ws >= 1000 * (8 * 25 + 4) and ws % 8 == 0
    for bad in ((-1, 3, 25), (10, -1, 25), (10, 3, 0), (10, 3, 33)):
        assert L.scp_temper_workspace_bytes(*bad) == -1, bad


def _betas(vals):
    return (C.c_float * len(vals))(*vals)


def test_temper_sweep_rejects_bad_arguments_without_a_gpu():
    """The argument checks come before any HIP call: SCP_EINVAL (-1), nothing launched."""
    L = _lib_or_skip()
    z, one = None, 4096            # NULL and a fake (never dereferenced) non-NULL address
    good = _betas([0.5, 1.0, 2.0])
    ws = L.scp_temper_workspace_bytes(10, 2, 3)
    ok = dict(logits=one, ld=256, n=10, nsym=255, sym=one, seg_off=one, nseg=2, betas=good, nt=3, bits=one, bad=one, rows=z, ws=one, ws_bytes=ws,
              stream=z)

    def call(**kw):
        a = dict(ok, **kw)
        b = a["betas"]
        return L.scp_temper_sweep(a["logits"], a["ld"], a["n"], a["nsym"], a["sym"], a["seg_off"], a["nseg"],
                                  None if b is None else C.cast(b, C.c_void_p), a["nt"], a["bits"], a["bad"], a["rows"], a["ws"], a["ws_bytes"],
                                  a["stream"])
    for bad in (dict(logits=z), dict(sym=z), dict(seg_off=z), dict(bits=z), dict(bad=z), dict(ws=z), dict(nsym=1), dict(nsym=257), dict(ld=254),
                dict(ws_bytes=ws - 1), dict(ws_bytes=0), dict(nseg=-1), dict(n=-1), dict(ws=4097), dict(betas=None), dict(nt=0), dict(nt=33),
                dict(betas=_betas([0.5, 0.0, 2.0])), dict(betas=_betas([0.5, -1.0, 2.0])), dict(betas=_betas([0.5, float("inf"), 2.0])),
                dict(betas=_betas([0.5, float("nan"), 2.0]))):
        assert call(**bad) == -1, bad


def test_temper_choose_rejects_bad_arguments_without_a_gpu():
    L = _lib_or_skip()
    z, one = None, 4096
    good = _betas([0.5, 1.0, 2.0])
    ok = dict(bits=one, bad=one, seg_off=one, n=10, group=one, nseg=2, ngroup=2, betas=good, nt=3, unit=1, gain=8.0, choice=one, gbits=one,
              seg_beta=one, stream=z)

    def call(**kw):
        a = dict(ok, **kw)
        b = a["betas"]
        return L.scp_temper_choose(a["bits"], a["bad"], a["seg_off"], a["n"], a["group"], a["nseg"], a["ngroup"],
                                   None if b is None else C.cast(b, C.c_void_p), a["nt"], a["unit"], a["gain"], a["choice"], a["gbits"],
                                   a["seg_beta"], a["stream"])
    for bad in (dict(bits=z), dict(bad=z), dict(seg_off=z), dict(group=z), dict(choice=z), dict(gbits=z), dict(seg_beta=z), dict(n=-1),
                dict(nseg=-1), dict(ngroup=0), dict(betas=None), dict(nt=0), dict(nt=33), dict(unit=-1), dict(unit=3),
                dict(unit=0),                                    # the grid's value there is not 1
                dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(betas=_betas([0.5, 1.0, -2.0]))):
        assert call(**bad) == -1, bad


def test_scale_rows_rejects_bad_arguments_without_a_gpu():
    L = _lib_or_skip()
    z, one, two = None, 4096, 1 << 20
    ok = dict(src=one, ld_in=256, dst=two, ld_out=256, n=10, nsym=255, seg_off=one, seg_beta=one, nseg=2, stream=z)

    def call(**kw):
        a = dict(ok, **kw)
        return L.scp_scale_rows(a["src"], a["ld_in"], a["dst"], a["ld_out"], a["n"], a["nsym"], a["seg_off"], a["seg_beta"], a["nseg"], a["stream"])
    for bad in (dict(src=z), dict(dst=z), dict(seg_off=z), dict(seg_beta=z), dict(n=-1), dict(nseg=-1), dict(nsym=1), dict(nsym=257),
                dict(ld_in=254), dict(ld_out=254), dict(dst=one, ld_out=300)):     # (in place means the same rows: one stride)
        assert call(**bad) == -1, bad
    assert call(n=0, src=z, dst=z) == 0                                            # nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------------------ names and side information
class _Enc:
    """What write_sidecar and FrameEncoder.outfile read of an encoder."""
    data_type, lidar_level, mullevel, spher, cylin, profile = "kitti", 12, False, True, False, None

    def __init__(self, temper):
        self.temper = temper


def _res(n_levels=3, index=(12, 9, 12, 12, 14, 12)):
    from scp_amd import native
    g, unit = native.temper_grid()
    groups = [dict(level=i // 2, phase=i % 2 + 1, rows=5, index=k, bits_unit=10.0, bits_chosen=9.0) for i, k in enumerate(index)]
    return dict(n_points=100, n_nodes=30, bin_num=1025.0, z_offset=0.0, n_levels=n_levels,
                temper=dict(grid=[float(b) for b in g], grid_u32=[int(b) for b in g.view(np.uint32)], unit=unit, groups=groups))


def test_outfile_with_and_without_temper():
    from scp_amd.decoder import extract_info, is_tempered
    from scp_amd.encoder import FrameEncoder
    res = dict(n_levels=12, bin_num=1025.0, z_offset=0.0)
    for spher, cylin, token in ((True, False, "_spher"), (False, True, "_cylin"), (False, False, "")):
        names = {}
        for temper in (None, "report", "code"):
            enc = FrameEncoder.__new__(FrameEncoder)
            enc.spher, enc.cylin, enc.temper = spher, cylin, temper
            names[temper] = enc.outfile("out/000frame", res)
        assert names[None] == names["report"] == f"out/000frame{token}_12_1025_0.bin"
        assert names["code"] == f"out/000frame_temper{token}_12_1025_0.bin"
        assert is_tempered(names["code"]) and not is_tempered(names[None])
    assert not is_tempered("out/temperature_spher_12_1025_0.bin")                # a field of the name, not a substring
    # ... and only where the encoder puts it: a `temper` field of the original file's own name is not the token
    assert not is_tempered("out/scan_temper_01_spher_12_1025_0.bin") and not is_tempered("out/scan_temper_01_12_1025_0.bin")
    assert is_tempered("out/scan_temper_01_temper_cylin_12_1025_-3.bin") and is_tempered("out/scan_01_temper_12_1025_0.bin")
    assert not is_tempered("temper_1_2.bin") and not is_tempered("x.bin")


def test_extract_info_on_a_temper_name(tmp_path):
    import torch
    from scp_amd.decoder import extract_info
    name = str(tmp_path / "07000123_temper_spher_12_1025_-3.bin")
    torch.save(torch.zeros((12, 2)), name + ".dat")
    spher, cylin, pos_mm, n_levels, bin_num, z = extract_info(name)
    assert (spher, cylin, n_levels, bin_num, z) == (True, False, 12, 1025, -3) and pos_mm.shape == (12, 2)
    from scp_amd.cli import find_stream
    open(name, "wb").close()
    assert find_stream(str(tmp_path) + "/", "data/07/000123.bin") == (os.path.basename(name), "07000123")


def test_sidecar_carries_the_grid_and_the_indices_only_for_a_coded_choice(tmp_path):
    from scp_amd import native
    from scp_amd.decoder import read_sidecar, stream_temper, write_sidecar
    g, unit = native.temper_grid()
    name = str(tmp_path / "f_temper_spher_3_1025_0.bin")
    write_sidecar(name, _Enc("code"), _res(), "EHEM")
    side = read_sidecar(name)
    assert side["temper"] == dict(betas_u32=[int(b) for b in g.view(np.uint32)], index=[12, 9, 12, 12, 14, 12])
    betas = stream_temper(name, side, 3)
    assert betas.dtype == np.float32 and betas.tolist() == [1.0, g[9], 1.0, 1.0, g[14], 1.0]
    for temper in (None, "report"):
        plain = str(tmp_path / f"g{temper}_spher_3_1025_0.bin")
        write_sidecar(plain, _Enc(temper), _res(), "EHEM")
        assert "temper" not in read_sidecar(plain)
    # a stream without the token ignores any entry
    assert stream_temper(str(tmp_path / "f_spher_3_1025_0.bin"), dict(temper=dict(betas_u32=[1], index=[99])), 3) is None


def test_refusals_of_a_tempered_stream_name_the_reason(tmp_path):
    import torch
    from scp_amd import native
    from scp_amd.decoder import SIDECAR, _ehem_job, write_sidecar
    name = str(tmp_path / "f_temper_spher_3_1025_0.bin")
    with open(name, "wb") as f:
        f.write(b"\0" * 8)
    torch.save(torch.zeros((3, 2)), name + ".dat")
    with pytest.raises(native.ScpError, match="without its side-info file"):
        _ehem_job(name)
    side = write_sidecar(name, _Enc("code"), _res(), "EHEM")

    def rewrite(**temper):
        d = dict(side)
        if temper.get("drop"):
            d.pop("temper")
        else:
            d["temper"] = dict(side["temper"], **temper)
        with open(name + SIDECAR, "w") as f:
            json.dump(d, f)

    assert _ehem_job(name)["temper"].shape == (6,)
    rewrite(drop=True)
    with pytest.raises(native.ScpError, match="no `temper` entry"):
        _ehem_job(name)
    rewrite(index=[12, 12, 12, 12])
    with pytest.raises(native.ScpError, match="holds 4 indices, a stream of 3 levels has 6"):
        _ehem_job(name)
    rewrite(index=[12, 12, 12, 12, 12, 25])
    with pytest.raises(native.ScpError, match="temper index 25 out of range"):
        _ehem_job(name)
    rewrite(index=[12, 12, 12, 12, 12, -1])
    with pytest.raises(native.ScpError, match="temper index -1 out of range"):
        _ehem_job(name)
    for junk in (["a"] * 6, [12.5] * 6, "121212", [None] * 6, [True] * 6):           # not integers: the same kind of refusal, no ValueError
        rewrite(index=junk)
        with pytest.raises(native.ScpError, match="`index` is not a list of integers"):
            _ehem_job(name)
    rewrite(betas_u32=["1.0"] * 25)
    with pytest.raises(native.ScpError, match="`betas_u32` is not a list of integers"):
        _ehem_job(name)
    rewrite(betas_u32=[2 ** 70] + side["temper"]["betas_u32"][1:])
    with pytest.raises(native.ScpError, match="float32 bit patterns expected"):
        _ehem_job(name)
    rewrite(betas_u32=[0x7F800000] + side["temper"]["betas_u32"][1:])              # +inf
    with pytest.raises(native.ScpError, match="not finite and positive"):
        _ehem_job(name)


def test_cli_flags_and_the_octattention_refusal():
    from scp_amd import native
    from scp_amd.cli import get_args, refuse_unsupported, temper_request
    from scp_amd.encoder import OctAttnFrameEncoder
    base = ["--test_files", "x.bin", "--type", "kitti", "--lidar_level", "12", "--spher"]
    for mullevel in (False, True):
        off = get_args(base, mullevel)
        assert not hasattr(off, "temper") and not hasattr(off, "temper_report") and temper_request(off) == (None, False)
        assert temper_request(get_args(base + ["--temper"], mullevel)) == ("code", False)
        assert temper_request(get_args(base + ["--temper_report"], mullevel)) == ("report", True)
        both = get_args(base + ["--temper", "--temper_report", "--rate_report"], mullevel)
        assert temper_request(both) == ("code", True)
        refuse_unsupported(both, "EHEM", mullevel)
        refuse_unsupported(get_args(base + ["--temper_report", "--rate_report"], mullevel), "OctAttention", mullevel)
        with pytest.raises(native.ScpError, match="--temper is available for the EHEM encoders only"):
            refuse_unsupported(get_args(base + ["--temper"], mullevel), "OctAttention", mullevel)
    with pytest.raises(native.ScpError, match="one node per step"):
        OctAttnFrameEncoder(None, temper="code")


def test_temper_layout_groups_two_per_level_in_level_order():
    from scp_amd.encoder import _rate_layout, _temper_layout
    sizes = [1, 0, 3, 9000]
    off, group, meta = _temper_layout(sizes, 8192)
    assert off == _rate_layout(sizes, 8192)[0]
    assert [m[:2] for m in meta] == [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)]          # an empty level still has its groups
    assert [m[2] for m in meta] == [1, 0, 0, 0, 2, 1, 4096 + 404, 4096 + 404] and sum(m[2] for m in meta) == sum(sizes)
    assert group.tolist() == [0, 1, 4, 5, 6, 7, 6, 7]
    off, group, meta = _temper_layout(sizes, None)                                                             # OctAttention: a group per level
    assert group.tolist() == [0, 1, 2, 3] and [m for m in meta] == [(0, None, 1), (1, None, 0), (2, None, 3), (3, None, 9000)]
