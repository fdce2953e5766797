"""D2 (point-to-plane) PSNR without a GPU: the numpy reference (tests/d2_ref.py) against the MPEG pc_error tool's recorded numbers, its
behaviour on degenerate clouds, the argument checks of the new entry points, the PLY with normals, and the --normals flag."""
import json
import os

import numpy as np
import pytest

import d2_cases
import d2_ref
from conftest import GOLDEN, golden


def fixture(name):
    z = golden("d2_" + name)
    return z["a"], z["n_a"], z["b"], json.load(open(os.path.join(GOLDEN, "d2_metrics.json")))[name]


@pytest.mark.parametrize("name", ["sphere", "lattice"])
def test_reference_reproduces_the_pc_error_tool(name):
    """mse within 1e-5 relative (the tool prints six significant digits: 5e-6 of rounding, times two), PSNR within 1e-3 dB.  The
    sphere pair has no distance tie, the lattice pair up to 8 equal nearest neighbours per point."""
    a, n_a, b, e = fixture(name)
    assert (e["max_ties_ab"], e["max_ties_ba"]) == ((1, 1) if name == "sphere" else (8, 8))
    got = d2_ref.d2_psnr(a, n_a, b, e["peak"])
    for k in ("mse_ab", "mse_ba"):
        assert abs(got[k] - e[k]) <= 1e-5 * e[k], (k, got, e)
    assert abs(got["psnr_d2"] - e["psnr_d2"]) <= 1e-3, (got, e)
    # the same run's p2point lines pin the nearest-neighbour half
    assert abs(d2_ref.nn_sqdist(a, b).mean() - e["d1_mse_ab"]) <= 1e-5 * e["d1_mse_ab"]
    assert abs(d2_ref.nn_sqdist(b, a).mean() - e["d1_mse_ba"]) <= 1e-5 * e["d1_mse_ba"]


def test_reference_merges_duplicates_with_the_mean_normal():
    a = np.array([[0.0, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0]])
    n = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0]])
    u, m = d2_ref.merge_duplicates(a, n)
    assert u.tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0]] and m.tolist() == [[0.5, 0, 0.5], [0, 1, 0], [0, 1, 0]]
    same = d2_ref.merge_duplicates(a[1:], n[1:])
    assert same[0] is not u and np.array_equal(same[0], a[1:]) and np.array_equal(same[1], n[1:])


def test_reference_normals_on_degenerate_clouds():
    """One point, two points: fewer than 3 neighbours, the default normal turned towards the sensor.  Three collinear points: a rank-one
    covariance whose null space is a plane - any unit vector of it will do, but it must be finite, unit length and perpendicular."""
    one = d2_ref.estimate_normals(np.array([[1.0, 2.0, 3.0]]))
    assert one.count.tolist() == [1] and one.idx[0, 0] == 0 and (one.idx[0, 1:] == -1).all() and one.normals.tolist() == [[0.0, 0.0, -1.0]]
    two = d2_ref.estimate_normals(np.array([[1.0, 2.0, 3.0], [1.0, 2.0, -3.5]]), radius=10.0)
    assert two.count.tolist() == [2, 2] and two.idx[:, :2].tolist() == [[0, 1], [1, 0]]
    assert two.normals.tolist() == [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]
    line = np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [4.0, 4.0, 4.0]])
    three = d2_ref.estimate_normals(line, radius=10.0)
    assert three.count.tolist() == [3, 3, 3] and three.idx[:, :3].tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0]]
    assert np.isfinite(three.normals).all()
    assert np.allclose((three.normals ** 2).sum(1), 1.0, atol=1e-14) and np.allclose(three.normals @ np.ones(3), 0.0, atol=1e-12)
    assert not d2_ref.comparable(three, line).any()            # and such points are what the device comparison leaves out
    far = d2_ref.estimate_normals(line, radius=0.5)
    assert far.count.tolist() == [1, 1, 1] and far.normals.tolist() == [[0.0, 0.0, -1.0]] * 3


def test_reference_neighbour_ties_go_to_the_lower_index():
    xyz = d2_cases.tie_lattice()
    idx, count = d2_ref.neighbours(xyz, 3.0, 30)
    full = d2_ref._sqdist_rows(xyz, xyz)
    interior = [i for i in range(len(xyz)) if (np.sort(full[i])[:31] == [0] + [1] * 4 + [2] * 4 + [4] * 6 + [5] * 16).all()]
    assert len(interior) >= 30 and (count[interior] == 30).all()
    for i in interior:
        at5 = np.nonzero(full[i] == 5.0)[0]
        assert idx[i, 15:].tolist() == at5[:15].tolist()        # 16 candidates at the same distance, the 15 lowest indices are kept


def test_test_clouds_stay_inside_the_exclusion_cap():
    """The GPU comparison may leave out points whose normal is ill-determined ((lam1 - lam0) / lam2 < 1e-3, or an orientation product at
    its threshold); the reference alone must keep that share below each case's cap - none at all on near4096."""
    for cid, xyz, radius, max_nn, cap in d2_cases.normal_cases():
        ref = d2_ref.estimate_normals(xyz, radius, max_nn, d2_cases.VIEW)
        out = ~d2_ref.comparable(ref, xyz, d2_cases.VIEW) & (ref.count >= 3)
        assert out.sum() <= cap * len(xyz), (cid, int(out.sum()))
    ref = d2_ref.estimate_normals(d2_cases.near4096(), 1.0, 31)
    d31 = d2_ref._sqdist_rows(d2_cases.near4096()[:1], d2_cases.near4096())      # spot check of the fixture's description on point 0
    assert (ref.count >= 3).all() and np.sort(d31[0])[29] < np.sort(d31[0])[30]
    few = d2_ref.estimate_normals(d2_cases.gauss(1025), 0.06, 30)
    assert 0 < (few.count < 3).sum() < 1025


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    """NULL pointers, n <= 0, max_nn outside 1 .. 32, radius <= 0, an unknown mode: SCP_EINVAL before any HIP call."""
    import ctypes as C
    from scp_amd import native
    L = native.lib()
    z, one = None, 4096                      # NULL and a fake (never dereferenced) non-NULL address
    view = (C.c_double * 3)(0.0, 0.0, 0.0)
    v = C.cast(view, C.c_void_p)
    assert L.scp_estimate_normals_f64(z, 10, 1.0, 30, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, 1.0, 30, z, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, 1.0, 30, v, z, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, 1.0, 30, v, one, z, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 0, 1.0, 30, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, -5, 1.0, 30, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, 1.0, 0, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, 1.0, 33, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, 0.0, 30, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, -1.0, 30, v, one, one, z, z) == -1
    assert L.scp_estimate_normals_f64(one, 10, float("nan"), 30, v, one, one, z, z) == -1
    for mode in (native.TIE_MEAN_NORMAL, native.TIE_PLANE_ERROR):
        for bad in range(5):
            ptrs = [one] * 5
            ptrs[bad] = z
            q, p, dmin, nrm, out = ptrs
            assert L.scp_nn_tieset_f64(mode, q, 10, p, 10, dmin, nrm, out, z) == -1
        assert L.scp_nn_tieset_f64(mode, one, 0, one, 10, one, one, one, z) == -1
        assert L.scp_nn_tieset_f64(mode, one, 10, one, -1, one, one, one, z) == -1
    assert L.scp_nn_tieset_f64(2, one, 10, one, 10, one, one, one, z) == -1
    with pytest.raises(native.ScpError):
        native.estimate_normals(__import__("torch").zeros((4, 3)))            # and no CPU path behind the binding


def test_ply_with_normals_reads_back_as_float32(tmp_path):
    from scp_amd.data_preproc import pt
    rng = np.random.default_rng(3)
    xyz = (rng.standard_normal((500, 3)) * np.array([1e-5, 1.0, 1e4])).astype(np.float32)
    nrm = d2_cases.unit_rows(rng, 500)                                          # float64 in, float32 on file
    f = str(tmp_path / "n.ply")
    pt.write_ply_normals(f, xyz, nrm)
    head = open(f).read().split("end_header")[0].split("\n")
    assert head[:3] == ["ply", "format ascii 1.0", "element vertex 500"] and head[3:9] == ["property float32 " + c for c in ("x", "y", "z", "nx", "ny", "nz")]
    p, n = pt.load_ply_normals(f)
    assert p.dtype == n.dtype == np.float32 and np.array_equal(p, xyz) and np.array_equal(n, nrm.astype(np.float32))
    assert np.array_equal(pt.ptread(f), xyz)                                     # the plain reader still sees the points
    with pytest.raises(ValueError):
        pt.write_ply_normals(f, xyz, nrm[:10])


def test_normals_flag_is_refused_outside_ehem_metrics():
    from scp_amd import native
    from scp_amd.cli import get_args, normals_file, refuse_unsupported
    base = ["--test_files", "x.bin", "--type", "kitti", "--lidar_level", "12", "--spher"]
    for mullevel in (False, True):
        plain, with_n = get_args(base + ["--metrics"], mullevel), get_args(base + ["--metrics", "--normals", "estimate"], mullevel)
        assert plain.normals is None and with_n.normals == "estimate"
        d = dict(vars(with_n))
        d["normals"] = None
        assert d == vars(plain)                                                  # nothing else in the namespace moves
        today = dict(vars(plain))
        del today["normals"]
        assert sorted(today) == sorted(["ckpt_path", "test_files", "sequential", "type", "lidar_level", "level_wise", "cylin", "spher", "preproc_path",
                                        "gpus", "model", "random_weights", "out_dir", "metrics", "decodable", "host_transform"]
                                       + ([] if mullevel else ["spher_circle"]))
        refuse_unsupported(with_n, "EHEM", mullevel)                             # accepted
        refuse_unsupported(plain, "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--normals"):
            refuse_unsupported(get_args(base + ["--normals", "estimate"], mullevel), "EHEM", mullevel)          # without --metrics
        with pytest.raises(native.ScpError, match="--normals"):
            refuse_unsupported(get_args(base + ["--normals", "nrm/"], mullevel), "EHEM", mullevel)
        with pytest.raises(native.ScpError):
            refuse_unsupported(with_n, "OctAttention", mullevel)                 # OctAttention has no --metrics, hence no --normals
        with pytest.raises(native.ScpError, match="--normals"):
            refuse_unsupported(get_args(base + ["--normals", "estimate"], mullevel), "OctAttention", mullevel)
        with pytest.raises(native.ScpError, match="--metrics is available"):
            refuse_unsupported(plain, "OctAttention", mullevel)                  # the existing refusal keeps its words
    assert normals_file("nrm", "data/kitti/07/velodyne/000012.bin") == os.path.join("nrm", "07", "000012.ply")


def test_summary_gains_psnr_d2_only_with_normals():
    from scp_amd import distributed as D
    five = D.summary_means(D.reduce_summary([2.0, 80.0, 0.5, 4.0, 2.0]))
    assert five == dict(bpp=1.0, psnr=40.0, chamfer=0.25, time=2.0, count=2)
    six = D.summary_means(D.reduce_summary([2.0, 80.0, 0.5, 4.0, 2.0, 90.0]))
    assert six == dict(five, psnr_d2=45.0)
