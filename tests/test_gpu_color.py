"""Colour layer on the GPU ("Colour"): every entry of csrc/color.hip equals tests/color_ref.py bit for bit - leaf means, their
YCoCg-R image and counts, the coefficients of the three planes, contexts, histograms, level counts, the coder's pairs and the inverse -
on the hard trees of tests/color_cases.py; the Y plane of the shared launch equals the single-channel kernel's output.  Every comparison
is exact.  The reference of a case is computed once per process."""
import functools

import numpy as np
import pytest
import torch

import attr_ref
import color_ref
from color_cases import QS, cases
from test_gpu_ringrate import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    """The references are shared by the tests of this module only: afterwards they are dropped and the allocator's cached blocks go back
    to the device, so that the modules that follow start from the memory they always started from."""
    yield
    import gc
    reference.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def up(x, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev())               # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def reference(name, Q):
    c = cases()[name]
    f = color_ref.forward(c["leaves"], c["ycc"], c["D"], Q)
    f["back"] = color_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"])
    return f


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name", sorted(cases()))
def test_kernels_equal_the_reference(name, Q):
    from scp_amd import attr, native
    c, want = cases()[name], reference(name, Q)
    U, D = len(c["leaves"]), c["D"]
    lv = up(c["leaves"], np.int32).reshape(-1, 3)
    ycc = up(c["ycc"], np.int16).reshape(3, U)
    got = native.color_forward(lv, ycc, D, Q)
    assert got["k"].dtype == torch.int16 and got["ctx"].dtype == torch.uint8 and got["k"].shape == (3, U - 1) and got["ctx"].shape == (U - 1,)
    assert got["k"].cpu().tolist() == want["k"]
    assert got["ctx"].cpu().tolist() == want["ctx"]
    assert got["root"].cpu().tolist() == want["root"]
    assert got["hist"].shape == (3 * D, 1021) and got["hist"].cpu().tolist() == want["hist"]
    assert got["level_counts"].cpu().tolist() == want["level_counts"]
    assert native.attr_level_counts(lv, D).cpu().tolist() == want["level_counts"]
    # the shared launch has the single-channel kernel's bits on the Y plane
    one = native.attr_forward(lv, up(c["ycc"][0], np.uint8), D, Q)
    assert torch.equal(one["k"], got["k"][0]) and torch.equal(one["ctx"], got["ctx"]) and int(one["root"].item()) == int(got["root"][0].item())
    assert torch.equal(one["hist"], got["hist"][:D, :511]) and not got["hist"][:D, 511:].any()
    assert torch.equal(one["level_counts"], got["level_counts"])
    rng = np.random.default_rng(D * 1000 + Q)
    rows = color_ref.tables()[rng.integers(0, 16, size=3 * D)]
    rows[D] = color_ref.tables()[0 if Q == 1 else 15]
    lohi = native.color_pairs(got["k"], got["ctx"], up(rows.view(np.int16), np.int16))
    assert lohi.shape == (3 * (U - 1),) and lohi.cpu().numpy().view(np.uint32).tolist() == color_ref.pairs(want["k"], want["ctx"], rows, D)
    back = native.color_inverse(lv, D, Q, want["root"], up(want["k"], np.int16).reshape(3, U - 1))
    assert back.dtype == torch.uint8 and back.shape == (U, 3) and back.cpu().tolist() == want["back"]
    if Q == 1:
        assert want["back"] == c["rgb"].tolist()


def test_leaf_means_ycc_and_counts_equal_the_reference():
    from scp_amd import native
    c = cases()["random"]
    mean, ycc, cnt = native.color_leaf_values(up(c["q"], np.int32), up(c["rgb8"], np.uint8), up(c["leaves"], np.int32), c["D"])
    assert mean.dtype == torch.uint8 and ycc.dtype == torch.int16 and cnt.dtype == torch.int32 and ycc.shape == (3, len(c["leaves"]))
    assert cnt.cpu().tolist() == c["cnt"].tolist() and int(cnt.min()) >= 1
    assert mean.cpu().tolist() == c["rgb"].tolist()
    assert ycc.cpu().tolist() == c["ycc"]
    # a leaf nobody hits (mean 0, count 0), and no points at all
    lv = np.concatenate([c["leaves"][:1000], [[4095, 4095, 4095]]]).astype(np.int32)
    keep = np.ones(len(lv), bool)
    if (c["leaves"][1000:] == 4095).all(axis=1).any():
        keep[-1] = False
    lv = lv[keep]
    wm, wy, wc = color_ref.leaf_values(c["q"], c["rgb8"], lv, c["D"])
    mean, ycc, cnt = native.color_leaf_values(up(c["q"], np.int32), up(c["rgb8"], np.uint8), up(lv, np.int32), c["D"])
    assert mean.cpu().tolist() == wm and ycc.cpu().tolist() == wy and cnt.cpu().tolist() == wc and 0 in wc
    mean, ycc, cnt = native.color_leaf_values(up(c["q"][:0], np.int32).reshape(0, 3), up(c["rgb8"][:0], np.uint8).reshape(0, 3), up(lv, np.int32), c["D"])
    assert not mean.any() and not ycc.any() and not cnt.any()


def test_point_colours_round_half_up_and_clamp():
    from scp_amd import color
    vals = [np.nan, np.inf, -np.inf, -3.0, 0.49, 0.5, 1.5, 254.49, 254.5, 255.0, 300.0, 3e38]
    got = color.point_colors(up(vals, np.float32).reshape(-1, 3))
    assert got.dtype == torch.uint8 and got.reshape(-1).cpu().tolist() == [color_ref.point_color(v) for v in vals]


def test_empty_and_one_leaf_shells():
    from scp_amd import native
    empty = torch.zeros((0, 3), dtype=torch.int32, device=dev())
    f = native.color_forward(empty, torch.zeros((3, 0), dtype=torch.int16, device=dev()), 7, 1)
    assert f["k"].shape == (3, 0) and not f["hist"].any() and not f["level_counts"].any() and f["root"].cpu().tolist() == [0, 0, 0]
    assert native.color_inverse(empty, 7, 1, [0, 0, 0], f["k"]).shape == (0, 3)
    mean, ycc, cnt = native.color_leaf_values(up([[1, 2, 3]], np.int32), up([[9, 9, 9]], np.uint8), empty, 7)
    assert mean.shape == (0, 3) and ycc.shape == (3, 0) and cnt.shape == (0,)
    one = up([[3, 5, 1]], np.int32)
    ycc1 = list(color_ref.rgb_to_ycc(200, 30, 90))
    f = native.color_forward(one, up(ycc1, np.int16).reshape(3, 1), 4, 8)
    assert f["k"].shape == (3, 0) and f["root"].cpu().tolist() == ycc1 and f["level_counts"].cpu().tolist() == [1] * 5 and not f["hist"].any()
    assert native.color_inverse(one, 4, 8, ycc1, f["k"]).cpu().tolist() == [[200, 30, 90]]
    assert native.color_pairs(f["k"], f["ctx"], up(color_ref.tables()[:12].view(np.int16), np.int16)).shape == (0,)


def test_colour_stream_round_trips_through_the_host_coder():
    """encode_shells -> bytes -> decode_shells on two shells of different depth plus a one-leaf and an empty shell."""
    from scp_amd import color, native
    cs = cases()
    r, h, s = cs["random"], cs["heavy"], cs["single"]
    rgb8 = up(r["rgb8"], np.uint8)
    # every shell sees the same 6 000 points; only the first one's leaves are hit by them in full
    leaves = [up(r["leaves"], np.int32), up(s["leaves"], np.int32), torch.zeros((0, 3), dtype=torch.int32, device=dev()), up(h["leaves"], np.int32)]
    depths = [r["D"], s["D"], 7, h["D"]]
    qs = [up(r["q"], np.int32)] * 4
    for Q in QS:
        data, rep = color.encode_shells(leaves, depths, qs, rgb8, Q)
        assert rep["values"][0].cpu().tolist() == r["rgb"].tolist() and rep["bits"] == 8 * len(data)
        assert [len(sh["tables"]) for sh in rep["shells"]] == [3, 0, 0, 3] and len(rep["shells"][0]["level_bits"][2]) == r["D"]
        info = {}
        values = color.decode_shells(data, [lv.long() for lv in leaves], depths, info)
        assert info == dict(Q=Q) and [tuple(v.shape) for v in values] == [(2000, 3), (1, 3), (0, 3), (len(h["leaves"]), 3)]
        want = reference("random", Q)
        assert values[0].cpu().tolist() == want["back"]
        for v, d in zip(values, rep["decoded"]):
            assert torch.equal(v, d)
        if Q == 1:
            assert values[0].cpu().tolist() == r["rgb"].tolist() and torch.equal(values[3], rep["values"][3])
    with pytest.raises(native.ScpError, match="another stream"):
        color.decode_shells(data, [lv.long() for lv in leaves], [r["D"], s["D"], 7, h["D"] + 1])
    with pytest.raises(native.ScpError, match="another stream"):
        color.decode_shells(data, [leaves[0][:-1]] + leaves[1:], depths)
    with pytest.raises(native.ScpError, match="shells"):
        color.decode_shells(data, leaves[:3], depths[:3])


def test_argument_errors_return_einval_and_launch_nothing():
    """Every entry refuses on the host; outputs filled with a pattern beforehand still hold it afterwards."""
    import ctypes
    from scp_amd import native
    L = native.lib()
    c = cases()["heavy"]
    U, D = len(c["leaves"]), c["D"]
    lv, ycc = up(c["leaves"], np.int32), up(c["ycc"], np.int16).reshape(3, U)
    full = lambda shape, dtype: torch.full(shape, 77, dtype=dtype, device=dev())
    k, ctx, root, hist = full((3, U - 1), torch.int16), full((U - 1,), torch.uint8), full((3,), torch.int32), full((3 * D, 1021), torch.int32)
    counts, out, cnt, lohi = full((D + 1,), torch.int64), full((U, 3), torch.uint8), full((U,), torch.int32), full((3 * (U - 1),), torch.int32)
    mean, yout = full((U, 3), torch.uint8), full((3, U), torch.int16)
    tabs = up(color_ref.tables()[:3 * D].view(np.int16), np.int16)
    nb = L.scp_color_forward_workspace_bytes(U, D)
    assert nb > L.scp_attr_forward_workspace_bytes(U, D) and L.scp_color_inverse_workspace_bytes(U, D) == nb
    assert L.scp_color_leaf_values_workspace_bytes(U) >= 32 * U
    ws = torch.zeros(nb // 8 + 1, dtype=torch.int64, device=dev())
    st = native._stream()
    p = lambda t: t.data_ptr()
    E = -1
    for bad_U, bad_D in ((-1, D), (U, 0), (U, 22), ((1 << 31) + 2, D)):
        assert L.scp_color_forward_workspace_bytes(bad_U, bad_D) == E and L.scp_color_inverse_workspace_bytes(bad_U, bad_D) == E
    assert L.scp_color_leaf_values_workspace_bytes(-1) == E

    def fwd(U=U, D=D, Q=8, lvp=p(lv), yp=p(ycc), kp=p(k), wsp=p(ws), nb=nb):
        return L.scp_color_forward(lvp, yp, U, D, Q, kp, p(ctx), p(root), p(hist), p(counts), wsp, nb, st)

    for kw in (dict(U=-1), dict(U=(1 << 31) + 2), dict(D=0), dict(D=22), dict(Q=0), dict(Q=256), dict(lvp=None), dict(yp=None), dict(kp=None),
               dict(wsp=None), dict(wsp=p(ws) + 4), dict(nb=nb - 8), dict(nb=L.scp_attr_forward_workspace_bytes(U, D))):
        assert fwd(**kw) == E, kw

    def inv(U=U, D=D, Q=8, roots=(5, -5, 5), kp=p(k), wsp=p(ws), nb=nb, null_root=False):
        r = (ctypes.c_int32 * 3)(*roots)
        return L.scp_color_inverse(p(lv), U, D, Q, None if null_root else ctypes.cast(r, ctypes.c_void_p), kp, p(out), wsp, nb, st)

    for kw in (dict(U=-1), dict(D=0), dict(D=22), dict(Q=0), dict(Q=256), dict(roots=(-1, 0, 0)), dict(roots=(256, 0, 0)), dict(roots=(0, 256, 0)),
               dict(roots=(0, 0, -256)), dict(null_root=True), dict(kp=None), dict(wsp=None), dict(nb=nb - 8)):
        assert inv(**kw) == E, kw

    def val(P=3, D=D, nb=32 * U, qp=p(lv), cp=p(out)):
        return L.scp_color_leaf_values(qp, cp, P, p(lv), U, D, p(mean), p(yout), p(cnt), p(ws), nb, st)

    for kw in (dict(P=-1), dict(P=(1 << 31) + 1), dict(D=0), dict(D=22), dict(nb=32 * U - 8), dict(qp=None), dict(cp=None)):
        assert val(**kw) == E, kw
    for kw in (dict(n=-1), dict(D=0), dict(D=22), dict(tp=None), dict(kp=None)):
        args = dict(n=U - 1, D=D, tp=p(tabs), kp=p(k))
        args.update(kw)
        assert L.scp_color_pairs(args["kp"], p(ctx), args["n"], args["tp"], args["D"], p(lohi), st) == E, kw
    torch.cuda.synchronize()
    for t in (k, ctx, root, hist, counts, out, cnt, lohi, mean, yout):
        assert bool((t == 77).all())
    assert not ws.any()
    # the Python layer refuses the same and wrong shapes
    with pytest.raises(native.ScpError):
        native.color_forward(lv, ycc, D, 0)
    with pytest.raises(native.ScpError):
        native.color_forward(lv, ycc[:, :-1].contiguous(), D, 1)
    with pytest.raises(native.ScpError):
        native.color_inverse(lv, D, 1, [0, 0, 0], k[:, :-1].contiguous())
    with pytest.raises(native.ScpError):
        native.color_inverse(lv, D, 1, [0, 300, 0], k)
    with pytest.raises(native.ScpError):
        native.color_forward(lv.cpu(), ycc, D, 1)
    with pytest.raises(native.ScpError):
        native.color_pairs(k, ctx, tabs[:, :512].contiguous())
    with pytest.raises(native.ScpError):
        native.color_leaf_values(lv, out[:-1], lv, D)
