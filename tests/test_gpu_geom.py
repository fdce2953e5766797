"""Stage G / C on the GPU through the C ABI, against the golden vectors and the CPU oracle (bit-exact)."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu


def names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scp_amd import native
    native.lib()
    return torch.device("cuda:0")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def build_one(dev, pts, path=None, drop=False):
    import torch
    from scp_amd import native
    g = native.Geom()
    q = torch.from_numpy(np.ascontiguousarray(pts, np.int32)).to(dev)
    g.build(q, [(0, len(pts), path, drop)])
    return g


# ----------------------------------------------------------------------------------------------- a2/a3
# The device quantiser against the correctly rounded reference of tests/quantiser_ref.py (vouched for on the CPU by
# tests/test_quantiser_ref.py): bit for bit, except values whose float64 angle lies next to a float32 rounding midpoint.
AMBIGUOUS_CAP = 2e-5          # at most 2 such values per 100 000 points; test_quantiser_ref.py counts 0 on every input used here


def assert_info_is_cr(info, ref):
    assert info.bin_num == ref.bin_num
    assert list(info.qs) == ref.qs and list(info.offset) == ref.offset
    assert info.max_coord == ref.max_coord and info.min_coord == ref.min_coord


def assert_quantised_is_cr(q, ref, tr=None):
    """q [n,3] (numpy) == the reference's integers on every row without an ambiguous value, tr (if given) bit-identical on every
    non-ambiguous value; -> number of values left out."""
    import quantiser_ref as R
    amb = R.ambiguous(ref.raw64)
    left_out = int(amb.sum())
    assert left_out <= AMBIGUOUS_CAP * len(ref.q), left_out
    if tr is not None:
        ok = (tr.view(np.int32) == ref.tr.view(np.int32)) | amb
        assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:8].tolist(), tr[~ok][:8].tolist(), ref.tr[~ok][:8].tolist())
    rows = ~amb.any(1)
    ok = (q == ref.q)[rows]
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:8].tolist())
    return left_out


def cr_inputs():
    import quantiser_ref as R
    from scp_amd.synth import ford_like, synth_frame
    kitti = [(400 / (2 ** L - 1), f"L{L}") for L in (12, 16, 18)]
    d = {"xform_s0": (lambda m: golden("xform_s0")["xyz"], kitti), "xform_s1": (lambda m: golden("xform_s1")["xyz"], kitti),
         "edge": (R.edge_points, kitti),
         "ford29": (lambda m: ford_like(synth_frame(0))[::29].copy(), [(2.0, "step2"), (0.5, "step0.5")])}
    for n in (1, 2, 63, 65, 257, 4001):
        d[f"synth7_{n}"] = (lambda m, n=n: synth_frame(7)[:n].copy(), kitti)
    return d


@pytest.mark.parametrize("name", ["xform_s0", "xform_s1", "edge", "synth7_1", "synth7_2", "synth7_63", "synth7_65", "synth7_257",
                                  "synth7_4001", "ford29"])
@pytest.mark.parametrize("mode", ["spher", "cylin"])
def test_transform_is_correctly_rounded(dev, mode, name):
    """scp_quantize (transform_kernel + quantize_kernel): the transformed float32 coordinates are the correctly rounded ones of
    DESIGN.md 2.1 bit for bit - axes, the +-pi seam, the poles and denormal coordinates included - the integers are the exact float64
    function of them, and scp_quant_info reports the reference's bin_num, steps, offsets and extreme integers."""
    import torch
    import quantiser_ref as R
    from conftest import parity_record
    from scp_amd import native
    make, steps = cr_inputs()[name]
    xyz = np.ascontiguousarray(make(mode), np.float32)
    x = torch.from_numpy(xyz).to(dev)
    mi = {"spher": native.SPHER, "cylin": native.CYLIN}[mode]
    for qs, tag in steps:
        ref = R.cr_quantise(xyz, qs, mode, -200.0)
        q, info, tr = native.quantize(x, mi, qs, -200.0, want_transformed=True)
        left_out = assert_quantised_is_cr(q.cpu().numpy(), ref, tr.cpu().numpy())
        assert_info_is_cr(info, ref)
        parity_record(f"quantiser-cr/{name}/{mode}/{tag}", points=len(xyz), values_left_out_as_ambiguous=left_out)


@pytest.mark.parametrize("mode", ["spher", "cylin"])
def test_fused_front_is_correctly_rounded(dev, mode):
    """scp_geom_build_xyz (front_transform_kernel + front_key_kernel) on three frames in one call - the crafted edge set, a frame that
    leaves the last tile ragged, a 7-point frame: the integers of every (frame, shell) segment and its scp_quant_info equal the
    correctly rounded reference's, and the depth derived from the extreme COORDINATES (the quantiser is monotone) is the depth of
    the largest INTEGER."""
    import torch
    import quantiser_ref as R
    from conftest import parity_record
    from scp_amd import native
    from scp_amd.synth import synth_frame
    frames = [R.edge_points(mode), synth_frame(3)[:4097].copy(), synth_frame(1)[:7].copy()]
    if mode == "spher":
        mi, off, levels, shells = native.SPHER, 0.0, (16, 17, 18), [([0, 0], True), ([0, 1], True), ([1], True)]
    else:
        mi, off, levels, shells = native.CYLIN, -200.0, (12,), [(None, False)]
    qs_list = [400 / (2 ** L - 1) for L in levels]
    g = native.Geom()
    infos, q = g.build_xyz([torch.from_numpy(f).to(dev) for f in frames], mi, qs_list, off, shells, want_q=True)
    q = q.cpu().numpy()
    assert len(infos) == len(frames) * len(shells) and q.shape == (sum(len(f) for f in frames) * len(shells), 3)
    row = left_out = 0
    for f, xyz in enumerate(frames):
        for s, qs in enumerate(qs_list):
            ref = R.cr_quantise(xyz, qs, mode, off)
            left_out += assert_quantised_is_cr(q[row:row + len(xyz)], ref)
            assert_info_is_cr(infos[f * len(shells) + s], ref)
            seg = g.info[f * len(shells) + s]
            assert seg.depth == R.depth_of(ref.max_coord) and seg.max_coord == ref.max_coord
            row += len(xyz)
    assert row == len(q)
    parity_record(f"quantiser-cr/fused/{mode}", points=row, values_left_out_as_ambiguous=left_out)


@pytest.mark.parametrize("seed", [0, 1])
def test_quantizer_vs_reference(dev, orc, seed):
    import torch
    import quantiser_ref as R
    from scp_amd import native
    z = golden(f"xform_s{seed}")
    xyz = torch.from_numpy(z["xyz"]).to(dev)
    report = {}
    for mi, mode in ((native.SPHER, "spher"), (native.CYLIN, "cylin"), (native.CART, "cart")):
        for L in (12, 14, 16, 18):
            q, info, tr = native.quantize(xyz, mi, 400 / (2 ** L - 1), -200.0, want_transformed=True)
            q = q.cpu().numpy()
            ref = R.cr_quantise(z["xyz"], 400 / (2 ** L - 1), mode, -200.0)
            assert_quantised_is_cr(q, ref, tr.cpu().numpy())
            assert_info_is_cr(info, ref)
            assert R.unexplained(mode, ref, z[f"{mode}_L{L}_q"])[2] == 0
            if mode != "cart":
                assert info.bin_num == float(z[f"{mode}_L{L}_bin"])
                ref = z[f"{mode}_tr"]
                ulp = np.abs(tr.cpu().numpy().view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
                # rho (sqrt) and z are exact; phi/theta within 2 ulp of numpy's SIMD float32 routines
                assert ulp[:, 0].max() == 0 and (mode == "cylin" or True)
                assert ulp.max() <= 2, (mode, ulp.max())
            if mode == "cylin":
                assert info.offset[2] == float(z[f"{mode}_L{L}_zoff"])
            bad = (q != z[f"{mode}_L{L}_q"]).any(1).sum()
            report[(mode, L)] = int(bad)
            if mode == "cart":
                assert bad == 0
            else:
                assert np.abs(q.astype(np.int64) - z[f"{mode}_L{L}_q"]).max() <= 1
                assert bad <= 40, (mode, L, bad)   # float->int boundary, see DESIGN.md
            assert info.max_coord == q.max() and info.min_coord == q.min()
    print("quantised points differing from the numpy reference (of 4096):", report)


# ----------------------------------------------------------------------------------------------- a4/a6
@pytest.mark.parametrize("name", names("oct_"))
def test_octree_vs_reference(dev, name):
    z = golden(name)
    g = build_one(dev, z["pts"])
    info = g.info[0]
    assert info.depth == int(z["depth"])
    nd = {k: v.cpu().numpy() for k, v in g.nodes().items()}
    assert np.array_equal(nd["occ"], z["occ"])            # the occupancy code stream
    assert np.array_equal(nd["occ"], z["codes"])
    assert np.array_equal(nd["level"], z["level"])
    assert np.array_equal(nd["octant"], z["octant"])
    assert np.array_equal(nd["parent"] + 1, z["parent"])  # reference ids are 1-based, root parent 0
    assert np.array_equal(nd["pos"], z["pos"])
    assert np.array_equal(g.krecords(0).cpu().numpy(), z["krec"])
    uq = np.unique(z["pts"], axis=0)
    assert info.n_leaves == len(uq)
    lv = g.leaves(0).cpu().numpy()
    assert np.array_equal(lv[np.lexsort((lv[:, 2], lv[:, 1], lv[:, 0]))], uq)


@pytest.mark.parametrize("name", names("octmul_"))
def test_mullevel_octree_vs_reference(dev, name):
    from scp_amd import native
    z = golden(name)
    for tag, path in (("00", [0, 0]), ("01", [0, 1]), ("1", [1])):
        if f"p{tag}_empty" in z:
            with pytest.raises(native.ScpError):
                build_one(dev, z["pts"], path, True)
            continue
        g = build_one(dev, z["pts"], path, True)
        nd = {k: v.cpu().numpy() for k, v in g.nodes().items()}
        assert g.info[0].depth == int(z[f"p{tag}_depth"])
        assert np.array_equal(nd["occ"], z[f"p{tag}_codes"])
        assert np.array_equal(nd["octant"], z[f"p{tag}_octant"])
        assert np.array_equal(nd["parent"] + 1, z[f"p{tag}_parent"])
        assert np.array_equal(nd["pos"], z[f"p{tag}_pos"])
        assert np.array_equal(g.krecords(0).cpu().numpy(), z[f"p{tag}_krec"])   # last node dropped
        assert np.array_equal(g.leaves(0).cpu().numpy(), z[f"p{tag}_deoct"])     # == DeOctree(codes)


def test_three_shells_in_one_build(dev):
    """The production layout: three quantisations concatenated, one scp_geom_build call with 3 segments."""
    import torch
    from scp_amd import native
    z = golden("octmul_frame5k_L14")
    pts = z["pts"]
    n = len(pts)
    q = torch.from_numpy(np.concatenate([pts, pts, pts]).astype(np.int32)).to(dev)
    g = native.Geom()
    g.build(q, [(0, n, [0, 0], True), (n, n, [0, 1], True), (2 * n, n, [1], True)])
    nd = {k: v.cpu().numpy() for k, v in g.nodes().items()}
    for s, tag in enumerate(("00", "01", "1")):
        i = g.info[s]
        sl = slice(i.node_base, i.node_base + i.n_nodes)
        assert np.array_equal(nd["occ"][sl], z[f"p{tag}_codes"])
        assert np.array_equal(nd["parent"][sl][1:] - i.node_base + 1, z[f"p{tag}_parent"][1:])
        assert np.array_equal(g.krecords(s).cpu().numpy(), z[f"p{tag}_krec"])


def test_octree_errors(dev):
    from scp_amd import native
    with pytest.raises(native.ScpError):
        build_one(dev, np.zeros((1, 3), np.int32))           # depth 0: the reference aborts
    with pytest.raises(native.ScpError):
        build_one(dev, np.array([[1, -2, 3]], np.int32))     # negative coordinate


def test_octree_random_vs_oracle(dev, orc):
    rng = np.random.default_rng(7)
    for n, hi in ((1, 5), (17, 3), (1000, 40), (30000, 5000), (200000, 9000)):
        pts = np.stack([rng.integers(0, hi, n), rng.integers(0, hi // 2 + 2, n), rng.integers(0, hi // 3 + 2, n)], 1)
        if pts.max() == 0:
            pts[0, 0] = 1
        g = build_one(dev, pts)
        t = orc.octree_build(pts)
        nd = {k: v.cpu().numpy() for k, v in g.nodes().items()}
        assert g.info[0].n_nodes == t.n
        assert np.array_equal(nd["occ"], t.occ) and np.array_equal(nd["octant"], t.octant)
        assert np.array_equal(nd["parent"] + 1, t.parent) and np.array_equal(nd["pos"], t.pos)
        assert np.array_equal(g.krecords(0).cpu().numpy(), t.krecords())


def test_full_frame_checksums(dev):
    """BASELINE-size frames (configs[1..4] geometry): the REFERENCE quantiser's integers in (tests/golden/frame_ints.npz, made by
    running data_preprocess.py:40-68 in the build container) -> node counts per level, sha256 of the occupancy stream and of the
    [N,4,6] K-records must equal what the reference's octree builders produced (frame_facts.json) - asserted unconditionally -
    and the device quantiser's own integers are exactly the correctly rounded ones (tests/quantiser_ref.py), which differ from the
    reference's in the pinned number of points (853 at L12 spherical, 6 at L18, 0 elsewhere), each a +-1 at a rounding boundary."""
    import torch
    import quantiser_ref as R
    from conftest import parity_record
    from scp_amd import native
    from scp_amd.synth import synth_frame
    facts = json.load(open(os.path.join(GOLDEN, "frame_facts.json")))
    ints = golden("frame_ints")
    xyz_np = synth_frame(0)
    xyz = torch.from_numpy(xyz_np).to(dev)
    n = xyz.shape[0]
    mode_name = {native.SPHER: "spher", native.CYLIN: "cylin", native.CART: "cart"}
    # measured on MI355X (profiles/parity_r2.json): points whose device-quantised integers differ from this fixture's
    max_diff_pts = {"L12-s": 900, "L16-s": 0, "C14": 0, "L12-c": 0, "L17": 0, "L18": 8}      # measured: 853, 0, 0, 0, 0, 6
    for key, mode, name, L in (("L12-s", native.SPHER, "q_spher_L12", 12), ("L16-s", native.SPHER, "q_spher_L16", 16),
                               ("C14", native.CYLIN, "q_cylin_L14", 14), ("L12-c", native.CART, "q_cart_L12", 12)):
        f = facts[key]
        q_dev, info, _ = native.quantize(xyz, mode, 400 / (2 ** L - 1), -200.0)
        assert info.bin_num == f["bin_num"]
        q_ref = np.ascontiguousarray(ints[name])
        ndiff = int((q_dev.cpu().numpy() != q_ref).any(1).sum())
        # the device's integers are the correctly rounded reference's, which differs from the fixture in exactly the pinned, explained points
        ref = R.cr_quantise(xyz_np, 400 / (2 ** L - 1), mode_name[mode], -200.0)
        assert_quantised_is_cr(q_dev.cpu().numpy(), ref)
        assert_info_is_cr(info, ref)
        cols, pts, bad = R.unexplained(mode_name[mode], ref, q_ref)
        parity_record(f"quantiser/{key}", points=n, points_differing_from_reference_ints=ndiff, coordinates_explained=sum(cols) - bad)
        assert ndiff <= max_diff_pts[key], (key, ndiff)
        assert bad == 0 and ndiff == pts == R.FRAME_DIFF_POINTS[name], (key, ndiff, pts, bad)
        g = native.Geom()
        g.build(torch.from_numpy(q_ref).to(dev), [(0, n, None, False)])
        i = g.info[0]
        assert i.depth == f["D"] and g.level_counts(0) == f["per_level"] and i.n_nodes == f["N"] and i.n_leaves == f["U"]
        assert sha(g.nodes(("occ",))["occ"].cpu().numpy()) == f["codes_sha"]
        if "krec_sha_i32" in f:
            assert sha(g.krecords(0).cpu().numpy().astype(np.int32)) == f["krec_sha_i32"]
    # mullevel L16 (BASELINE configs[2], the bench workload): three shells in one build
    shells = facts["L16-m"]
    qs_list = []
    for k in range(3):
        q_dev, info, _ = native.quantize(xyz, native.SPHER, 400 / (2 ** (16 + k) - 1), 0.0)
        assert info.bin_num == shells[k]["bin_num"]
        q_ref = np.ascontiguousarray(ints[f"q_spher_L{16 + k}"])
        ndiff = int((q_dev.cpu().numpy() != q_ref).any(1).sum())
        ref = R.cr_quantise(xyz_np, 400 / (2 ** (16 + k) - 1), "spher", 0.0)
        assert_quantised_is_cr(q_dev.cpu().numpy(), ref)
        assert_info_is_cr(info, ref)
        cols, pts, bad = R.unexplained("spher", ref, q_ref)
        parity_record(f"quantiser/L16-m shell {k}", points=n, points_differing_from_reference_ints=ndiff, coordinates_explained=sum(cols) - bad)
        assert ndiff <= max_diff_pts[("L16-s", "L17", "L18")[k]], (k, ndiff)
        assert bad == 0 and ndiff == pts == R.FRAME_DIFF_POINTS[f"q_spher_L{16 + k}"], (k, ndiff, pts, bad)
        qs_list.append(torch.from_numpy(q_ref).to(dev))
    g = native.Geom()
    g.build(torch.cat(qs_list), [(0, n, [0, 0], True), (n, n, [0, 1], True), (2 * n, n, [1], True)])
    for k in range(3):
        i = g.info[k]
        assert i.depth == shells[k]["D"] and i.n_leaves == shells[k]["leaves"] and g.rows(k) == shells[k]["records"], k
        assert g.level_counts(k) == shells[k]["per_level"], k
        occ = g.nodes(("occ",))["occ"][i.node_base:i.node_base + i.n_nodes].cpu().numpy()
        assert sha(occ) == shells[k]["codes_sha"], k
        assert sha(g.krecords(k).cpu().numpy().astype(np.int32)) == shells[k]["krec_sha_i32"], k


# ----------------------------------------------------------------------------------------------- a8/a9
@pytest.mark.parametrize("name,mode,L", [("ctx_ehem_spher_L12", "spher", 12), ("ctx_ehem_cylin_L12", "cylin", 12),
                                         ("ctx_ehem_cart_L10", "cart", 10)])
def test_ehem_context_vs_reference(dev, orc, name, mode, L):
    import torch
    from scp_amd import native
    z = golden(name)
    # integers from the oracle's numpy quantiser (identical integers in => bit-exact context out)
    r = orc.proc_pc(z["xyz"], 400 / (2 ** L - 1), mode)
    g = build_one(dev, r["pts"])
    pm = native.POS_POW2 if mode == "cart" else native.POS_MINMAX
    ctx, pos, sym, mm = [t.cpu().numpy() for t in g.context_ehem(0, pm, L)]
    counts = g.level_counts(0)
    assert len(counts) == int(z["n_levels"])
    a = 0
    for l, c in enumerate(counts):
        want = z[f"data{l}"]
        assert np.array_equal(ctx[a:a + c].reshape(c, 4, 3).astype(np.int16), want)
        assert np.array_equal(pos[a:a + c].T, z[f"pos{l}"])      # float32, bit-exact
        a += c
    assert np.array_equal(sym, z["oct_seq"][:, -1, 0].astype(np.uint8))
    if mode != "cart":
        assert np.array_equal(mm, z["pos_mm"])


def test_ehem_context_mullevel_vs_reference(dev, orc):
    import torch
    from scp_amd import native
    z = golden("ctx_ehem_mul_spher_L14")
    L = 14
    qs, n = [], len(z["xyz"])
    for k in range(3):
        _, _, _, _, pt = orc.quantise(z["xyz"], 400 / (2 ** (L + k) - 1), "spher")
        qs.append(np.ascontiguousarray(pt, np.int32))
    q = torch.from_numpy(np.concatenate(qs)).to(dev)
    g = native.Geom()
    g.build(q, [(0, n, [0, 0], True), (n, n, [0, 1], True), (2 * n, n, [1], True)])
    lvl = 0
    syms = []
    for s in range(3):
        ctx, pos, sym, mm = [t.cpu().numpy() for t in g.context_ehem(s, native.POS_MINMAX_MUL, L)]
        counts = g.level_counts(s)
        counts[-1] -= 1   # dropped last node
        a = 0
        for c in counts:
            assert np.array_equal(ctx[a:a + c].reshape(c, 4, 3).astype(np.int16), z[f"data{lvl}"])
            assert np.array_equal(pos[a:a + c].T, z[f"pos{lvl}"])
            assert tuple(mm[lvl - sum(len(g.level_counts(t)) for t in range(s))]) == tuple(z["pos_mm"][lvl])
            a += c
            lvl += 1
        syms.append(sym)
    assert lvl == int(z["n_levels"])
    assert np.array_equal(np.concatenate(syms), z["oct_seq"][:, -1, 0].astype(np.uint8))


def test_octattn_context_vs_reference(dev, orc):
    z = golden("ctx_octattn_spher_L12")
    r = orc.proc_pc(z["xyz"], 400 / (2 ** 12 - 1), "spher")
    g = build_one(dev, r["pts"])
    ctx, pos, sym = [t.cpu().numpy() for t in g.context_octattn(0)]
    assert np.array_equal(ctx.reshape(-1, 4, 3).astype(np.int16), z["data"][1023:])
    assert np.array_equal(pos, z["pos"][1023:])
    assert np.array_equal(sym, z["oct_seq"][:, -1, 0].astype(np.uint8))


# ----------------------------------------------------------------------------------------------- a15/a16
def test_cdf_kernel_vs_reference(dev, orc):
    import torch
    from scp_amd import native
    z = golden("cdf_mixed")
    pdf = torch.from_numpy(z["pdf"]).to(dev)
    n = len(z["pdf"])
    sym = torch.from_numpy((np.arange(n) * 37 % 255).astype(np.uint8)).to(dev)
    sym[0], sym[1] = 254, 0
    r = native.pmf_cdf(pdf, sym, want_cdf=True)
    cdf = r["cdf"].cpu().numpy().view(np.uint16)
    assert np.array_equal(cdf, z["cdf"])
    s = sym.cpu().numpy().astype(np.int64)
    lohi = r["lohi"].cpu().numpy().view(np.uint32)
    assert np.array_equal(lohi & 0xFFFF, z["cdf"][np.arange(n), s])
    hi = np.where(s == 254, 0, z["cdf"][np.arange(n), np.minimum(s + 1, 255)])
    assert np.array_equal(lohi >> 16, hi)


def test_cdf_kernel_large_random_vs_oracle(dev, orc):
    import torch
    from scp_amd import native
    rng = np.random.default_rng(11)
    n = 100_003
    logits = torch.from_numpy((rng.standard_normal((n, 255)) * rng.uniform(0.1, 8, (n, 1))).astype(np.float32)).to(dev)
    sym_np = rng.integers(0, 255, n).astype(np.uint8)
    sym_np[:5] = [254, 0, 254, 1, 253]
    sym = torch.from_numpy(sym_np).to(dev)
    r = native.softmax_cdf(logits, sym, want_pmf=True, want_cdf=True)
    pmf = r["pmf"].cpu().numpy()
    # the library's PMF agrees with a float64 softmax to float32 rounding ...
    ref = torch.softmax(logits.double().cpu(), 1).numpy()
    assert (np.abs(pmf - ref) <= 5e-6 * ref + 1e-30).all()   # x - max is rounded to float32 before exp
    # ... and the integer CDF is an exact function of that PMF (numpyAc semantics, checked by the oracle)
    want = orc.pmf_to_cdf(pmf)
    assert np.array_equal(r["cdf"].cpu().numpy().view(np.uint16), want)
    lohi = r["lohi"].cpu().numpy().view(np.uint32)
    s = sym_np.astype(np.int64)
    assert np.array_equal(lohi & 0xFFFF, want[np.arange(n), s])
    assert np.array_equal(lohi >> 16, np.where(s == 254, 0, want[np.arange(n), np.minimum(s + 1, 255)]))
    # device (lo,hi) pairs -> host range coder == oracle coder on the full table
    assert native.ac_encode_lohi(lohi) == orc.ac_encode(want, sym_np.astype(np.int16))
    # strided logits (a column slice of a wider buffer)
    wide = torch.zeros((1000, 300), device=dev)
    wide[:, :255] = logits[:1000]
    r2 = native.softmax_cdf(wide[:, :255], sym[:1000])
    assert torch.equal(r2["lohi"], r["lohi"][:1000])


def test_empty_and_ragged_cdf(dev):
    import torch
    from scp_amd import native
    for n in (0, 1, 63, 64, 65):
        logits = torch.randn((n, 255), device=dev)
        sym = torch.randint(0, 255, (n,), device=dev).to(torch.uint8)
        r = native.softmax_cdf(logits, sym, want_cdf=True)
        assert r["cdf"].shape == (n, 256)
        if n:
            c = r["cdf"].cpu().numpy().view(np.uint16).astype(np.int64)
            assert (np.diff(c[:, :255], axis=1) > 0).all() and (c[:, 0] == 0).all()   # entry 255 wraps to 0 (= 65536)


# ----------------------------------------------------------------------------------------------- B1: legacy octree ABI
def test_legacy_octree_abi_matches_reference_so(dev):
    """The ten symbols Octreewarpper.py:17-39 binds, driven exactly the way that wrapper drives them."""
    import ctypes as C
    from scp_amd import native

    class Node(C.Structure):     # Octreewarpper.py:6-14
        _fields_ = [("nodeid", C.c_uint), ("octant", C.c_uint), ("parent", C.c_uint), ("oct", C.c_uint8), ("pos", C.c_uint * 3)]

    lib = C.CDLL(native.LIB_PATH)
    lib.new_vector.restype = C.c_void_p
    lib.delete_vector.argtypes = [C.c_void_p]
    lib.vector_size.argtypes = [C.c_void_p]
    lib.vector_get.restype = C.c_void_p
    lib.vector_get.argtypes = [C.c_void_p, C.c_int]
    lib.genOctreeInterface.restype = C.c_void_p
    lib.genOctreeInterface.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    lib.Nodes_get.argtypes = [C.c_void_p, C.c_int]
    lib.Nodes_get.restype = C.POINTER(Node)
    lib.Nodes_size.argtypes = [C.c_void_p]
    lib.int_size.argtypes = [C.c_void_p]
    lib.int_get.argtypes = [C.c_void_p, C.c_int]
    assert C.sizeof(Node) == 28
    for name in ("oct_skew2000", "oct_frame5k_L12", "oct_single"):
        z = golden(name)
        data = np.ascontiguousarray(z["pts"]).astype(np.double)
        vec = lib.new_vector()
        codes = lib.genOctreeInterface(vec, data.ctypes.data_as(C.POINTER(C.c_double)), data.shape[0])
        assert codes
        assert lib.vector_size(vec) == int(z["depth"])
        got_codes = [lib.int_get(codes, i) for i in range(lib.int_size(codes))]
        assert got_codes == z["codes"].tolist()
        n = 0
        for L in range(lib.vector_size(vec)):
            lvl = lib.vector_get(vec, L)
            for i in range(lib.Nodes_size(lvl)):
                nd = lib.Nodes_get(lvl, i).contents
                assert nd.nodeid == n + 1 and nd.octant == z["octant"][n] and nd.oct == z["occ"][n]
                assert [nd.pos[0], nd.pos[1], nd.pos[2]] == z["pos"][n].tolist()
                if n:
                    assert nd.parent == z["parent"][n]
                n += 1
        assert n == len(z["occ"])
        lib.delete_vector(vec)
    assert lib.genOctreeInterface(lib.new_vector(), np.zeros(3).ctypes.data_as(C.POINTER(C.c_double)), 1) is None   # depth 0: NULL, no abort


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 255, 257, 4001, 119999])
def test_quantizer_any_point_count(dev, orc, n):
    """Point counts of every parity and size (a scratch pointer derived from an odd-sized allocation once made every odd-n frame
    fault on a misaligned atomic): same integers as the oracle up to the float -> int boundary points, all three modes."""
    import torch
    import quantiser_ref as R
    from conftest import parity_record
    from scp_amd import native
    from scp_amd.synth import synth_frame
    xyz = synth_frame(7)[:n].copy()
    for mode, name in ((native.SPHER, "spher"), (native.CYLIN, "cylin"), (native.CART, "cart")):
        q, info, _ = native.quantize(torch.from_numpy(xyz).to(dev), mode, 400 / (2 ** 12 - 1), -200.0)
        _, bin_num, _, _, pt = orc.quantise(xyz, 400 / (2 ** 12 - 1), name)
        got = q.cpu().numpy()
        assert got.shape == (n, 3) and info.bin_num == bin_num
        # (synthetic rings can sit on a rounding boundary of theta / qs as a whole: DESIGN.md 2.1)
        assert (got != pt.astype(np.int64)).any(1).sum() <= max(2, n // 40)
        ref = R.cr_quantise(xyz, 400 / (2 ** 12 - 1), name, -200.0)           # ... and exactly the correctly rounded integers
        assert_quantised_is_cr(got, ref)
        assert_info_is_cr(info, ref)
        cols, pts, bad = R.unexplained(name, ref, pt)
        assert bad == 0, (name, cols, bad)
        parity_record(f"quantiser-any-n/{n}/{name}", points=n, points_differing_from_oracle_ints=pts, coordinates_explained=sum(cols) - bad)
        g = native.Geom()
        g.build(q, [(0, n, None, False)])
        assert g.info[0].n_leaves == len(np.unique(got, axis=0))


@pytest.mark.parametrize("mode,level,mul,ford", [("spher", 16, True, False), ("spher", 12, False, False), ("cylin", 14, False, False),
                                                 ("cart", 12, False, False), ("spher", 17, True, True)])
@pytest.mark.parametrize("n", [120000, 4097, 1, 7])
def test_fused_front_equals_the_separate_launches(dev, mode, level, mul, ford, n):
    """scp_geom_build_xyz (transform once, one kernel for quantiser + shell filter + Morton keys + the sort's first histogram) against
    scp_quantize per shell + scp_geom_build: the same integers, quantiser reports, level counts and node tables, for every coordinate
    system, multi-level shells, Ford-like millimetre frames, and point counts that leave tiles ragged or nearly empty."""
    import torch
    from scp_amd import native
    from scp_amd.encoder import level_qs
    from scp_amd.synth import ford_like, synth_frame
    xyz = synth_frame(3)[:: max(1, 120000 // n)][:n].copy()
    if ford:
        xyz = ford_like(xyz)
    x = torch.from_numpy(xyz).to(dev)
    m = {"cart": native.CART, "spher": native.SPHER, "cylin": native.CYLIN}[mode]
    dt = "ford" if ford else "kitti"
    shells = [([0, 0], level), ([0, 1], level + 1), ([1], level + 2)] if mul else [(None, level)]
    off = 0.0 if mul else (-200.0 if not ford else -float(2 ** 17))
    qs_list = [level_qs(dt, lv) for _, lv in shells]
    ref_q, ref_info = [], []
    for q_ in qs_list:
        q, qi, _ = native.quantize(x, m, q_, off)
        ref_q.append(q); ref_info.append(qi)
    g0 = native.Geom()
    segs, o = [], 0
    for (path, _), q in zip(shells, ref_q):
        segs.append((o, q.shape[0], path, mul)); o += q.shape[0]
    try:
        g0.build(torch.cat(ref_q).contiguous(), segs)
    except native.ScpError:                       # e.g. a shell that keeps no point of a 1-point frame: both entry points refuse
        g1 = native.Geom()
        with pytest.raises(native.ScpError):
            g1.build_xyz([x], m, qs_list, off, [(p, mul) for p, _ in shells])
        return
    g1 = native.Geom()
    infos, q1 = g1.build_xyz([x], m, qs_list, off, [(p, mul) for p, _ in shells], want_q=True)
    assert torch.equal(q1, torch.cat(ref_q))
    for a, b in zip(infos, ref_info):
        assert a.bin_num == b.bin_num and list(a.qs) == list(b.qs) and list(a.offset) == list(b.offset)
        assert a.max_coord == b.max_coord and a.min_coord == b.min_coord
    # ... and both are the correctly rounded reference's (the two transform kernels are separate copies of one arithmetic)
    import quantiser_ref as R
    for s, q_ in enumerate(qs_list):
        ref = R.cr_quantise(xyz, q_, mode, off)
        assert_quantised_is_cr(ref_q[s].cpu().numpy(), ref)
        assert_info_is_cr(infos[s], ref)
        assert g1.info[s].depth == R.depth_of(ref.max_coord)
    for s in range(len(shells)):
        assert g0.level_counts(s) == g1.level_counts(s) and g0.info[s].depth == g1.info[s].depth and g0.info[s].n_leaves == g1.info[s].n_leaves
        assert torch.equal(g0.leaves(s), g1.leaves(s))
    n0, n1 = g0.nodes(), g1.nodes()
    for k in n0:
        assert torch.equal(n0[k], n1[k]), k
    # context tables of all segments in one launch + coded symbols in coding order == per-segment launches + a gather through the plan
    from scp_amd.encoder import EncodePlan
    pm = native.POS_MINMAX_MUL if mul else (native.POS_POW2 if m == native.CART else native.POS_MINMAX)
    cs = 8192
    ctx, pos, sym_coded, mm = g1.context_ehem_all(pm, level, cs)
    parts = [g0.context_ehem(s, pm, level) for s in range(len(shells))]
    assert torch.equal(ctx, torch.cat([p[0] for p in parts])) and torch.equal(pos, torch.cat([p[1] for p in parts]))
    assert torch.equal(mm, torch.cat([p[3] for p in parts]))
    sizes = []
    for s in range(len(shells)):
        c = g0.level_counts(s)
        if mul:
            c[-1] -= 1
        sizes += c
    order = torch.from_numpy(EncodePlan(sizes, cs).coding_order()).to(dev)
    assert torch.equal(sym_coded, torch.cat([p[2] for p in parts])[order])


def test_fused_front_batches_frames(dev):
    """Four frames in one scp_geom_build_xyz (FrameEncoder.preprocess_batch): every frame's trees and tables equal its own build."""
    import torch
    from scp_amd import native
    from scp_amd.encoder import level_qs
    from scp_amd.synth import synth_frame
    frames = [torch.from_numpy(synth_frame(s)[: 120000 - 1000 * s].copy()).to(dev) for s in range(4)]
    qs = [level_qs("kitti", 12)]
    g = native.Geom()
    infos = g.build_xyz(frames, native.SPHER, qs, -200.0, [(None, False)])
    ctx, pos, sym, mm = g.context_ehem_all(native.POS_MINMAX, 12, 8192)
    r0 = m0 = 0
    for f, x in enumerate(frames):
        g1 = native.Geom()
        i1 = g1.build_xyz([x], native.SPHER, qs, -200.0, [(None, False)])
        assert infos[f].bin_num == i1[0].bin_num and g.level_counts(f) == g1.level_counts(0)
        c1, p1, s1, m1 = g1.context_ehem_all(native.POS_MINMAX, 12, 8192)
        n, d = c1.shape[0], m1.shape[0]
        assert torch.equal(ctx[r0:r0 + n], c1) and torch.equal(pos[r0:r0 + n], p1) and torch.equal(sym[r0:r0 + n], s1) and torch.equal(mm[m0:m0 + d], m1)
        r0 += n; m0 += d
    assert r0 == ctx.shape[0]
