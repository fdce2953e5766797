"""Reflectance layer on the GPU ("Reflectance"): every entry of csrc/attr.hip equals tests/attr_ref.py bit for bit - leaf
values and counts, coefficients, contexts, histograms, level counts, the coder's pairs and the inverse - on the hard trees of
tests/attr_cases.py and on a multi-level frame, whose dropped last node's leaves must be absent on both sides.  Every comparison is
exact.  The reference of a case is computed once per process."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attr_ref
from attr_cases import QS, cases
from test_gpu_ringrate import dev, ehem_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    """The frame, its encoder and the references are shared by the tests of this module only: afterwards they are dropped and the
    allocator's cached blocks go back to the device, so that the modules that follow start from the memory they always started from."""
    yield
    import gc
    reference.cache_clear()
    multilevel_frame.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def up(x, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev())               # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def reference(name, Q):
    c = cases()[name]
    f = attr_ref.forward(c["leaves"], c["a"], c["D"], Q)
    f["back"] = attr_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"])
    return f


def check_against_reference(leaves, a, D, Q, want):
    """forward, level counts, pairs and inverse of one tree against the reference's dict."""
    from scp_amd import attr, native
    U = len(leaves)
    lv = up(leaves, np.int32).reshape(-1, 3)
    got = native.attr_forward(lv, up(a, np.uint8), D, Q)
    assert got["k"].dtype == torch.int16 and got["ctx"].dtype == torch.uint8 and got["k"].shape == (U - 1,)
    assert got["k"].cpu().tolist() == want["k"]
    assert got["ctx"].cpu().tolist() == want["ctx"]
    assert int(got["root"].item()) == want["root"]
    assert got["hist"].cpu().tolist() == want["hist"]
    assert got["level_counts"].cpu().tolist() == want["level_counts"]
    assert native.attr_level_counts(lv, D).cpu().tolist() == want["level_counts"]
    assert attr.level_contexts(want["level_counts"]).tolist() == want["ctx"]
    rng = np.random.default_rng(D * 1000 + Q)
    rows = attr_ref.tables()[rng.integers(0, 16, size=D)]
    rows[0] = attr_ref.tables()[0 if Q == 1 else 15]
    lohi = native.attr_pairs(got["k"], got["ctx"], up(rows.view(np.int16), np.int16))
    assert lohi.cpu().numpy().view(np.uint32).tolist() == attr_ref.pairs(want["k"], want["ctx"], rows)
    back = native.attr_inverse(lv, D, Q, want["root"], up(want["k"], np.int16).reshape(-1))
    assert back.dtype == torch.uint8 and back.cpu().tolist() == want["back"]
    if Q == 1:
        assert want["back"] == [int(v) for v in a]


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name", sorted(cases()))
def test_kernels_equal_the_reference(name, Q):
    c = cases()[name]
    check_against_reference(c["leaves"], c["a"], c["D"], Q, reference(name, Q))


def test_leaf_values_and_counts_equal_the_reference():
    from scp_amd import native
    c = cases()["random"]
    a, cnt = native.attr_leaf_values(up(c["q"], np.int32), up(c["r"], np.float32), up(c["leaves"], np.int32), c["D"], c["scale"])
    assert a.dtype == torch.uint8 and cnt.dtype == torch.int32
    assert cnt.cpu().tolist() == c["cnt"].tolist() and int(cnt.min()) >= 1
    assert a.cpu().tolist() == c["a"].tolist()
    # another scale, a leaf nobody hits (value 0, count 0), and no points at all
    lv = np.concatenate([c["leaves"][:1000], [[4095, 4095, 4095]]]).astype(np.int32)
    keep = np.ones(len(lv), bool)
    if (c["leaves"][1000:] == 4095).all(axis=1).any():
        keep[-1] = False
    lv = lv[keep]
    wa, wc = attr_ref.leaf_values(c["q"], c["r"], lv, c["D"], 100)
    a, cnt = native.attr_leaf_values(up(c["q"], np.int32), up(c["r"], np.float32), up(lv, np.int32), c["D"], 100)
    assert a.cpu().tolist() == wa and cnt.cpu().tolist() == wc and 0 in wc
    a, cnt = native.attr_leaf_values(up(c["q"][:0], np.int32).reshape(0, 3), up(c["r"][:0], np.float32), up(lv, np.int32), c["D"], 255)
    assert not a.any() and not cnt.any()


def test_attribute_stream_round_trips_through_the_host_coder():
    """encode_shells -> bytes -> decode_shells on two shells of different depth plus a one-leaf and an empty shell."""
    from scp_amd import attr
    cs = cases()
    r, h, s = cs["random"], cs["heavy"], cs["single"]
    refl = up(r["r"], np.float32)
    # every shell sees the same 6 000 points; only the first one's leaves are hit by them
    leaves = [up(r["leaves"], np.int32), up(s["leaves"], np.int32), torch.zeros((0, 3), dtype=torch.int32, device=dev()), up(h["leaves"], np.int32)]
    depths = [r["D"], s["D"], 7, h["D"]]
    qs = [up(r["q"], np.int32)] * 4
    for Q in QS:
        data, rep = attr.encode_shells(leaves, depths, qs, refl, Q, 255)
        assert rep["values"][0].cpu().tolist() == r["a"].tolist() and rep["bits"] == 8 * len(data)
        info = {}
        values = attr.decode_shells(data, [lv.long() for lv in leaves], depths, info)
        assert info == dict(Q=Q, scale=255) and [int(v.shape[0]) for v in values] == [2000, 1, 0, len(h["leaves"])]
        want = attr_ref.forward(r["leaves"], r["a"], r["D"], Q)
        assert values[0].cpu().tolist() == attr_ref.inverse(r["leaves"], r["D"], Q, want["root"], want["k"])
        for v, d in zip(values, rep["decoded"]):
            assert torch.equal(v, d)
        if Q == 1:
            assert values[0].cpu().tolist() == r["a"].tolist()
    from scp_amd import native
    with pytest.raises(native.ScpError, match="another stream"):
        attr.decode_shells(data, [lv.long() for lv in leaves], [r["D"], s["D"], 7, h["D"] + 1])
    with pytest.raises(native.ScpError, match="another stream"):
        attr.decode_shells(data, [leaves[0][:-1]] + leaves[1:], depths)
    with pytest.raises(native.ScpError, match="shells"):
        attr.decode_shells(data, leaves[:3], depths[:3])


@functools.lru_cache(maxsize=None)
def multilevel_frame():
    """synth_frame(0, beams=16, az=256) through the multi-level front end at L12: the encoder, its per-shell leaves with and without the
    children of the dropped last node, the quantised points and a reflectance."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame, synth_reflectance
    xyz = synth_frame(0, beams=16, az=256)
    refl = synth_reflectance(xyz, 0)
    enc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, mullevel=True, device=dev())
    res = enc.encode(xyz)
    x_dev, r_dev = torch.from_numpy(xyz).to(dev()), torch.from_numpy(refl).to(dev())
    kept = [lv.cpu().numpy() for lv in enc.attr_leaves()]
    full = [enc.geom.leaves(s).cpu().numpy() for s in range(3)]
    qs = [q.cpu().numpy() for q in enc.quantize(x_dev)[0]]
    return dict(enc=enc, res=res, xyz=xyz, refl=refl, x_dev=x_dev, r_dev=r_dev, kept=kept, full=full, qs=qs)


def test_multilevel_frame_drops_the_last_nodes_leaves_on_both_sides(tmp_path):
    from scp_amd import attr, decoder
    from test_gpu_ringlod import write_stream
    m = multilevel_frame()
    enc = m["enc"]
    occ = enc.geom.nodes(("occ",))["occ"].cpu().numpy()
    for s, info in enumerate(enc.geom.info):
        drop = bin(int(occ[int(info.node_base) + int(info.n_nodes) - 1])).count("1")
        assert drop >= 1 and len(m["kept"][s]) == len(m["full"][s]) - drop and np.array_equal(m["kept"][s], m["full"][s][:-drop])
        keys = [attr_ref.morton(p, int(info.depth)) for p in m["kept"][s]]
        assert keys == sorted(set(keys))                                     # the order of scp_geom_emit_leaves is the Morton order
    out = write_stream(enc, m["res"], str(tmp_path / "f"))
    dec = decoder.decode_file(out, ehem_model(), mullevel=True, device=dev())
    for s in range(3):                                                       # decode_file's leaf order is that order, without the dropped leaves
        assert np.array_equal(dec["leaves"][s].cpu().numpy(), m["kept"][s])
    depths = [int(i.depth) for i in enc.geom.info]
    for Q in (1, 8):
        data, rep = enc.encode_attr(m["x_dev"], m["r_dev"], Q)
        assert rep["scale"] == 255 and rep["n_points"] == len(m["xyz"]) and rep["bits"] == 8 * len(data)
        assert rep["bits_per_point"] == rep["bits"] / len(m["xyz"]) and rep["bits_per_leaf"] == rep["bits"] / sum(len(k) for k in m["kept"])
        for s in range(3):
            wa, wc = attr_ref.leaf_values(m["qs"][s], m["refl"], m["kept"][s], depths[s], 255)
            assert min(wc) >= 1                                              # every kept leaf holds a point
            assert rep["values"][s].cpu().tolist() == wa and rep["counts"][s].cpu().tolist() == wc
            if Q == 8 and s == 0:
                f = attr_ref.forward(m["kept"][s], wa, depths[s], Q)
                check_against_reference(m["kept"][s], wa, depths[s], Q, dict(f, back=attr_ref.inverse(m["kept"][s], depths[s], Q, f["root"], f["k"])))
        values = attr.decode_shells(data, dec["leaves"], depths)
        for s in range(3):
            assert torch.equal(values[s], rep["decoded"][s])
            if Q == 1:
                assert torch.equal(values[s], rep["values"][s])
        assert [sh["U"] for sh in rep["shells"]] == [len(k) for k in m["kept"]] and all(len(sh["tables"]) == sh["depth"] for sh in rep["shells"])


GUARD, PATTERN = 1 << 16, 0xA5


def unordered_leaves(name):
    """Leaf lists that are no Morton-ordered set -> (int32 [U,3], D)."""
    if name == "two_parents":                                                # level 1 counts 600 heads where 8 entries fit
        return np.array([[0, 0, 0], [2, 0, 0]] * 300, np.int32), 2
    if name == "heavy_reversed":
        c = cases()["heavy"]
        return np.ascontiguousarray(c["leaves"][::-1], dtype=np.int32), c["D"]
    return np.array([[3, 1, 6]] * 300, np.int32), 3                          # "one_leaf": 300 copies


@pytest.mark.parametrize("name", ["two_parents", "heavy_reversed", "one_leaf"])
def test_unordered_leaves_leave_every_buffer_intact(name):
    """The values of both layers are unspecified on such leaves; what is pinned is that no entry writes outside an output or outside the
    workspace of exactly the size its *_workspace_bytes function returns.  Every written buffer is followed, inside its own allocation, by
    64 KiB of pattern bytes, so that an index that left a buffer would show in the guard and stay in the test's memory.  (Inputs are only
    read and carry no guard.)  level_counts are the counts as scanned: the overflowing level stays visible to the host."""
    from scp_amd import native
    L = native.lib()
    leaves, D = unordered_leaves(name)
    U = len(leaves)
    lv = up(leaves, np.int32)
    a = up(np.arange(U) % 251, np.uint8)
    ycc = up(np.stack([np.arange(U) % 251, np.arange(U) % 509 - 254, np.arange(U) % 499 - 249]), np.int16)
    st = native._stream()
    guarded = []

    def buf(nbytes):
        t = torch.full((nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=dev())
        guarded.append((t, nbytes))
        return t.data_ptr()

    def counts_of(entry):
        t, nbytes = entry
        return t[:nbytes].cpu().numpy().view(np.int64).tolist()

    nb_a, nb_c = L.scp_attr_forward_workspace_bytes(U, D), L.scp_color_forward_workspace_bytes(U, D)
    assert nb_a > 0 and nb_c > nb_a and L.scp_attr_inverse_workspace_bytes(U, D) == nb_a and L.scp_color_inverse_workspace_bytes(U, D) == nb_c
    zeros = torch.zeros(3 * (U - 1), dtype=torch.int16, device=dev())
    roots = (ctypes.c_int32 * 3)(5, -5, 5)
    for Q in (1, 255):
        level_counts = []
        assert L.scp_attr_forward(lv.data_ptr(), a.data_ptr(), U, D, Q, buf(2 * (U - 1)), buf(U - 1), buf(4), buf(4 * D * 511), buf(8 * (D + 1)),
                                  buf(nb_a), nb_a, st) == 0
        level_counts.append(guarded[-2])
        assert L.scp_attr_level_counts(lv.data_ptr(), U, D, buf(8 * (D + 1)), buf(nb_a), nb_a, st) == 0
        level_counts.append(guarded[-2])
        assert L.scp_attr_inverse(lv.data_ptr(), U, D, Q, 5, zeros.data_ptr(), buf(U), buf(nb_a), nb_a, st) == 0
        assert L.scp_color_forward(lv.data_ptr(), ycc.data_ptr(), U, D, Q, buf(6 * (U - 1)), buf(U - 1), buf(12), buf(4 * 3 * D * 1021),
                                   buf(8 * (D + 1)), buf(nb_c), nb_c, st) == 0
        level_counts.append(guarded[-2])
        assert L.scp_color_inverse(lv.data_ptr(), U, D, Q, ctypes.cast(roots, ctypes.c_void_p), zeros.data_ptr(), buf(3 * U), buf(nb_c), nb_c, st) == 0
        torch.cuda.synchronize()
        for t, nbytes in guarded:
            assert bool((t[nbytes:] == PATTERN).all()), (name, Q, nbytes)
        if name == "two_parents":
            assert [counts_of(c)[:2] for c in level_counts] == [[600, 600]] * 3
        guarded.clear()


def test_argument_errors_return_einval_and_launch_nothing():
    """Every entry refuses on the host; outputs filled with a pattern beforehand still hold it afterwards."""
    from scp_amd import native
    L = native.lib()
    c = cases()["heavy"]
    U, D = len(c["leaves"]), c["D"]
    lv, a = up(c["leaves"], np.int32), up(c["a"], np.uint8)
    k = torch.full((U - 1,), 77, dtype=torch.int16, device=dev())
    ctx = torch.full((U - 1,), 77, dtype=torch.uint8, device=dev())
    root = torch.full((1,), 77, dtype=torch.int32, device=dev())
    hist = torch.full((D, 511), 77, dtype=torch.int32, device=dev())
    counts = torch.full((D + 1,), 77, dtype=torch.int64, device=dev())
    out = torch.full((U,), 77, dtype=torch.uint8, device=dev())
    cnt = torch.full((U,), 77, dtype=torch.int32, device=dev())
    lohi = torch.full((U - 1,), 77, dtype=torch.int32, device=dev())
    tabs = up(attr_ref.tables()[:D].view(np.int16), np.int16)
    nb = L.scp_attr_forward_workspace_bytes(U, D)
    assert nb > 0 and L.scp_attr_inverse_workspace_bytes(U, D) == nb and L.scp_attr_leaf_values_workspace_bytes(U) >= 16 * U
    ws = torch.zeros(nb // 8 + 1, dtype=torch.int64, device=dev())
    st = native._stream()
    p = lambda t: t.data_ptr()
    E = -1
    for bad_U, bad_D in ((-1, D), (U, 0), (U, 22), ((1 << 31) + 2, D)):
        assert L.scp_attr_forward_workspace_bytes(bad_U, bad_D) == E and L.scp_attr_inverse_workspace_bytes(bad_U, bad_D) == E
    assert L.scp_attr_leaf_values_workspace_bytes(-1) == E and L.scp_attr_forward_workspace_bytes((1 << 31) + 1, 21) > 0

    def fwd(U=U, D=D, Q=8, lvp=p(lv), ap=p(a), kp=p(k), wsp=p(ws), nb=nb):
        return L.scp_attr_forward(lvp, ap, U, D, Q, kp, p(ctx), p(root), p(hist), p(counts), wsp, nb, st)

    for kw in (dict(U=-1), dict(U=(1 << 31) + 2), dict(D=0), dict(D=22), dict(Q=0), dict(Q=256), dict(lvp=None), dict(ap=None), dict(kp=None),
               dict(wsp=None), dict(wsp=p(ws) + 4), dict(nb=nb - 8)):
        assert fwd(**kw) == E, kw

    def inv(U=U, D=D, Q=8, root=5, kp=p(k), wsp=p(ws), nb=nb):
        return L.scp_attr_inverse(p(lv), U, D, Q, root, kp, p(out), wsp, nb, st)

    for kw in (dict(U=-1), dict(D=0), dict(D=22), dict(Q=0), dict(Q=256), dict(root=-1), dict(root=256), dict(kp=None), dict(wsp=None), dict(nb=nb - 8)):
        assert inv(**kw) == E, kw
    assert L.scp_attr_level_counts(p(lv), U, 0, p(counts), p(ws), nb, st) == E and L.scp_attr_level_counts(p(lv), U, D, p(counts), p(ws), nb - 8, st) == E

    def val(P=3, D=D, scale=255, nb=16 * U, qp=p(lv), rp=p(torch.zeros(8, device=dev()))):
        return L.scp_attr_leaf_values(qp, rp, P, p(lv), U, D, scale, p(out), p(cnt), p(ws), nb, st)

    for kw in (dict(P=-1), dict(P=(1 << 31) + 1), dict(D=0), dict(D=22), dict(scale=0), dict(scale=(1 << 20) + 1), dict(nb=16 * U - 8), dict(qp=None), dict(rp=None)):
        assert val(**kw) == E, kw
    for kw in (dict(n=-1), dict(D=0), dict(D=22), dict(tp=None), dict(kp=None)):
        args = dict(n=U - 1, D=D, tp=p(tabs), kp=p(k))
        args.update(kw)
        assert L.scp_attr_pairs(args["kp"], p(ctx), args["n"], args["tp"], args["D"], p(lohi), st) == E, kw
    torch.cuda.synchronize()
    for t in (k, ctx, root, hist, counts, out, cnt, lohi):
        assert bool((t == 77).all())
    assert not ws.any()
    # the Python layer refuses the same and wrong shapes
    with pytest.raises(native.ScpError):
        native.attr_forward(lv, a, D, 0)
    with pytest.raises(native.ScpError):
        native.attr_forward(lv, a[:-1], D, 1)
    with pytest.raises(native.ScpError):
        native.attr_inverse(lv, D, 1, 0, k[:-1])
    with pytest.raises(native.ScpError):
        native.attr_forward(lv.cpu(), a, D, 1)
