"""Distortion report without a GPU: the numpy statement of its definitions (tests/distortion_ref.py) on cases whose answer is known,
the host side of the report (scp_amd/metrics.py: records -> dict) and the CLI's flag."""
import json
import math

import numpy as np
import pytest

import distortion_ref as ref
from conftest import golden


def raw_of(records):
    """Reference records -> the int64 [n_bins, 72] image of scp_dist_seg records, as the device writes them."""
    from scp_amd import native
    raw = np.zeros((len(records), len(native.DIST_FIELDS) + native.DIST_HIST), np.int64)
    for k, r in enumerate(records):
        for c, name in enumerate(native.DIST_FIELDS):
            if name in ("rows", "axis_rows"):
                raw[k, c] = r[name]
            else:
                raw[k:k + 1, c].view(np.float64)[0] = r[name]
        raw[k, len(native.DIST_FIELDS):] = r["hist"]
    return raw


def report_of(a, b, edges, group=None, n_groups=1):
    """metrics.distortion_dict over the reference's records of both directions."""
    from scp_amd import metrics
    ab = ref.direction(a, b, edges)
    ba = ref.direction(b, a, edges, group, n_groups)
    return metrics.distortion_dict(edges, raw_of(ab["records"]), raw_of(ba["records"]), n_groups), ab, ba


def _cloud(n=500, seed=11):
    rng = np.random.default_rng(seed)
    rho = rng.uniform(2.0, 100.0, n)
    phi = rng.uniform(-np.pi, np.pi, n)
    theta = rng.uniform(0.3, 2.8, n)
    return rho, phi, theta


def _cart(rho, phi, theta):
    return np.stack((rho * np.sin(theta) * np.cos(phi), rho * np.sin(theta) * np.sin(phi), rho * np.cos(theta)), 1)


@pytest.mark.parametrize("axis", ["r", "phi", "theta"])
def test_pure_perturbations_land_in_their_own_component(axis):
    """B = A moved along exactly one spherical axis (rho rounded up to a 0.01 grid, or phi + 1e-6, or theta + 1e-6): every neighbour is
    the point's own copy, and the two other components' sums stay below 1e-9 of sum_sq - the chord of an arc of angle D leaves the
    tangent by D / 2, a share of (D / 2)^2 = 2.5e-13."""
    rho, phi, theta = _cloud()
    a = _cart(rho, phi, theta)
    if axis == "r":
        b = _cart(np.ceil(rho / 0.01) * 0.01, phi, theta)
    elif axis == "phi":
        b = _cart(rho, phi + 1e-6, theta)
    else:
        b = _cart(rho, phi, theta + 1e-6)
    rep, ab, _ = report_of(a, b, [0.0, 20.0, 50.0])
    assert np.array_equal(ab["idx"], np.arange(len(a))) and not ab["axis"].any()
    t = rep["a_to_b"]["total"]
    assert t["rows"] == 500 and t["axis_rows"] == 0 and t["sum_sq"] > 0
    own = {"r": "sum_r2", "phi": "sum_phi2", "theta": "sum_theta2"}[axis]
    others = [t[k] for k in ("sum_r2", "sum_phi2", "sum_theta2") if k != own]
    print(axis, t["sum_sq"], [o / t["sum_sq"] for o in others])
    assert all(o <= 1e-9 * t["sum_sq"] for o in others)
    assert abs(t[own] - t["sum_sq"]) <= 1e-9 * t["sum_sq"]
    if axis == "r":
        assert t["sum_r"] > 0 and t["bias_r"] > 0 and t["bias_r"] == t["sum_r"] / 500
    assert sum(e["rows"] for e in rep["a_to_b"]["rings"]) == 500


def test_components_add_up_to_the_distance_on_the_sphere_fixture():
    """e_r^2 + e_phi^2 + e_theta^2 = d2 per point to 1e-12 relative: the frame is orthonormal."""
    z = golden("d2_sphere")
    a, b = z["a"].astype(np.float64), z["b"].astype(np.float64)
    rep, ab, ba = report_of(a, b, [0.0, 10.0])
    for d in (ab, ba):
        assert not d["axis"].any() and (d["d2"] > 0).all()
        err = np.abs((d["comp"] ** 2).sum(1) - d["d2"]) / d["d2"]
        print(err.max())
        assert err.max() <= 1e-12
    for t in (rep["a_to_b"]["total"], rep["b_to_a"]["total"]):
        assert abs(t["mse_r"] + t["mse_phi"] + t["mse_theta"] - t["mse"]) <= 1e-12 * t["mse"]
    assert rep["a_to_b"]["total"]["rows"] == 2000 and rep["b_to_a"]["total"]["rows"] == 1902


def test_axis_points_and_ties_on_the_lattice_fixture():
    """The 6 points of `a` on the sensor's axis count in rows, sum_sq, max_sq and hist, are counted in axis_rows and add nothing to the
    component sums; among equal neighbours the lowest index wins."""
    z = golden("d2_lattice")
    a, b = z["a"].astype(np.float64), z["b"].astype(np.float64)
    rep, ab, _ = report_of(a, b, [0.0, 4.0, 8.0])
    on_axis = (a[:, 0] == 0) & (a[:, 1] == 0)
    assert on_axis.sum() == 6 and np.array_equal(ab["axis"], on_axis)
    assert (ab["comp"][on_axis] == 0).all() and (ab["d2"][on_axis] > 0).all()
    t = rep["a_to_b"]["total"]
    assert t["rows"] == 120 and t["axis_rows"] == 6 and sum(t["hist"]) == 120
    assert t["sum_sq"] == math.fsum(ab["d2"]) and t["max_sq"] == ab["d2"].max()
    framed = ab["d2"][~on_axis]
    assert abs((t["sum_r2"] + t["sum_phi2"] + t["sum_theta2"]) - math.fsum(framed)) <= 1e-12 * math.fsum(framed)
    assert t["bias_r"] == t["sum_r"] / 114
    d = ref.sqdist_rows(a, b)
    ties = (d == d.min(1, keepdims=True)).sum(1)
    assert ties.max() >= 2 and ties.max() <= 8
    first = np.array([np.flatnonzero(row == row.min())[0] for row in d])
    assert np.array_equal(ab["idx"], first)
    many = np.flatnonzero(ties > 1)
    assert all(ab["idx"][i] < np.flatnonzero(d[i] == d[i].min())[1] for i in many)


def test_ring_rule_puts_an_edge_point_into_the_upper_ring():
    from scp_amd import native
    edges = native.dist_edges([0, 5, 10, 20])
    a = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 6.0, 8.0], [4.999999, 0.0, 0.0], [0.0, 0.0, 20.0], [1e3, 0.0, 0.0], [np.nextafter(10.0, 0), 0, 0]])
    rho2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    assert ref.ring(rho2, edges).tolist() == [0, 1, 2, 0, 3, 3, 1]
    d = ref.direction(a, a + 0.125, edges, group=[0, 1, 2, 0, 1, 2, 0], n_groups=3)
    assert d["bin"].tolist() == [0, 4 + 1, 8 + 2, 0, 4 + 3, 8 + 3, 1]
    assert [r["rows"] for r in d["records"]] == [2, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1]
    for bad in ([], [1, 2], [0, 2, 2], [0, 3, 2], [0, -1], [0, float("inf")], [0, float("nan")], list(range(65)), "x"):
        with pytest.raises(native.ScpError, match="ring edges"):
            native.dist_edges(bad)


def test_histogram_buckets_at_their_edges():
    from scp_amd import metrics
    d2 = np.array([0.0, 2.0 ** -41, 2.0 ** -40, 1.0, 2.0 ** 22, 2.0 ** 30, 5e-324, np.nextafter(2.0 ** -39, 0), 2.0 ** -39])
    assert ref.bucket(d2).tolist() == [0, 1, 1, 41, 63, 63, 1, 1, 2]
    rec = ref.record(d2, np.zeros((len(d2), 3)), np.zeros(len(d2), bool))
    e = metrics.dist_entries(raw_of([rec]))[0]
    want = [0] * 64
    for k in (0, 1, 1, 41, 63, 63, 1, 1, 2):
        want[k] += 1
    assert e["hist"] == want and e["rows"] == len(d2) and e["max_sq"] == 2.0 ** 30 and e["max"] == 2.0 ** 15


def test_cli_accepts_distortion_report_and_refuses_where_it_cannot_run():
    from scp_amd import metrics, native
    from scp_amd.cli import distortion_request, get_args, refuse_unsupported
    base = ["--test_files", "x.bin", "--type", "kitti", "--lidar_level", "12", "--spher"]
    for mullevel in (False, True):
        off = get_args(base, mullevel)
        assert not hasattr(off, "distortion_report") and distortion_request(off) == (False, None)
        for name in ("EHEM", "OctAttention"):
            refuse_unsupported(off, name, mullevel)                                   # as today
        on = get_args(base + ["--distortion_report"], mullevel)
        assert distortion_request(on) == (True, None)
        refuse_unsupported(on, "EHEM", mullevel)
        given = get_args(base + ["--distortion_report", "0,2.5,10", "--rate_report", "--metrics"], mullevel)
        assert distortion_request(given) == (True, (0.0, 2.5, 10.0)) and given.rate_report is True
        refuse_unsupported(given, "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--distortion_report is available for the EHEM encoders only"):
            refuse_unsupported(on, "OctAttention", mullevel)
        with pytest.raises(native.ScpError, match="--distortion_report with --preproc_path: no geometry of the frame is built"):
            refuse_unsupported(get_args(base + ["--distortion_report", "--preproc_path", "pp/"], mullevel), "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--type obj has none"):
            refuse_unsupported(get_args(["--test_files", "x.ply", "--type", "obj", "--distortion_report", "0,1"], mullevel), "EHEM", False)
        for bad in ("1,2", "0,3,3", "0,a", ""):
            with pytest.raises(native.ScpError, match="ring edges"):
                get_args(base + ["--distortion_report", bad], mullevel)
    assert metrics.default_edges("kitti") == (0.0, 5.0, 10.0, 15.0, 20.0, 30.0, 40.0, 60.0, 80.0)
    assert metrics.default_edges("ford") == tuple(1000.0 * e for e in metrics.default_edges("kitti"))
    with pytest.raises(native.ScpError, match="give edges"):
        metrics.default_edges("obj")


def test_report_layout_is_plain_python_and_adds_up():
    """metrics.distortion_dict: edges, a_to_b.rings[r], b_to_a.groups[g][r], both totals; totals are math.fsum over the bins."""
    rng = np.random.default_rng(5)
    a = rng.uniform(-30, 30, (400, 3))
    a[:3, :2] = 0.0                                                     # three axis points
    b = a[rng.permutation(400)[:300]] + rng.normal(0, 0.01, (300, 3))
    group = (np.arange(300) % 3).astype(np.int32)
    edges = [0.0, 10.0, 20.0, 40.0]
    rep, ab, ba = report_of(a, b, edges, group, 3)
    json.loads(json.dumps(rep))
    assert sorted(rep) == ["a_to_b", "b_to_a", "edges"] and rep["edges"] == edges
    assert sorted(rep["a_to_b"]) == ["rings", "total"] and sorted(rep["b_to_a"]) == ["groups", "total"]
    assert len(rep["a_to_b"]["rings"]) == 4 and [len(g) for g in rep["b_to_a"]["groups"]] == [4, 4, 4]
    keys = sorted(["rows", "axis_rows", "sum_sq", "sum_r2", "sum_phi2", "sum_theta2", "sum_r", "max_sq", "hist",
                   "mse", "mse_r", "mse_phi", "mse_theta", "bias_r", "max"])
    flat_ba = [e for g in rep["b_to_a"]["groups"] for e in g]
    for e in rep["a_to_b"]["rings"] + flat_ba + [rep["a_to_b"]["total"], rep["b_to_a"]["total"]]:
        assert sorted(e) == keys and len(e["hist"]) == 64 and sum(e["hist"]) == e["rows"]
        if e["rows"]:
            assert e["mse"] == e["sum_sq"] / e["rows"] and e["max"] == math.sqrt(e["max_sq"]) and e["mse_r"] == e["sum_r2"] / e["rows"]
        else:
            assert e["mse"] == 0.0 and e["max"] == 0.0 and e["bias_r"] == 0.0
    for entries, total, n in ((rep["a_to_b"]["rings"], rep["a_to_b"]["total"], 400), (flat_ba, rep["b_to_a"]["total"], 300)):
        assert total["rows"] == n == sum(e["rows"] for e in entries)
        for k in ("sum_sq", "sum_r2", "sum_phi2", "sum_theta2", "sum_r"):
            assert total[k] == math.fsum(e[k] for e in entries)
        assert total["max_sq"] == max(e["max_sq"] for e in entries)
        assert total["hist"] == [sum(e["hist"][k] for e in entries) for k in range(64)]
    assert rep["a_to_b"]["total"]["axis_rows"] == 3 and rep["a_to_b"]["rings"][0]["axis_rows"] >= 0
    assert rep["a_to_b"]["total"]["sum_sq"] == pytest.approx(math.fsum(ab["d2"]), rel=1e-15)
    for g in range(3):
        assert sum(e["rows"] for e in rep["b_to_a"]["groups"][g]) == int((group == g).sum())
    from scp_amd import metrics, native
    with pytest.raises(native.ScpError, match="records for"):
        metrics.distortion_dict(edges, raw_of(ab["records"])[:3], raw_of(ba["records"]), 3)


def test_library_rejects_bad_distortion_arguments_without_a_gpu():
    """The argument checks come before any HIP call: SCP_EINVAL (-1), nothing launched."""
    import ctypes as C
    from scp_amd import native
    L = native.lib()
    z, one = None, 4096                         # NULL and a fake (never dereferenced) non-NULL address
    view = (C.c_double * 3)(0.0, 0.0, 0.0)
    esq = (C.c_double * 3)(0.0, 25.0, 100.0)
    ok = dict(a=one, na=10, b=one, nb=10, view=C.cast(view, C.c_void_p), esq=C.cast(esq, C.c_void_p), R=3, group=z, G=1, idx=one, d2=one, comp=one,
              bin=one, flag=one)

    def call(**kw):
        k = dict(ok, **kw)
        return L.scp_nn_error_split_f64(k["a"], k["na"], k["b"], k["nb"], k["view"], k["esq"], k["R"], k["group"], k["G"], k["idx"], k["d2"], k["comp"],
                                        k["bin"], k["flag"], None)
    unsorted = (C.c_double * 3)(0.0, 25.0, 25.0)
    negative = (C.c_double * 3)(-1.0, 25.0, 100.0)
    nanview = (C.c_double * 3)(0.0, float("nan"), 0.0)
    wide = (C.c_double * 65)(*[float(i) for i in range(65)])
    for bad in (dict(a=z), dict(b=z), dict(view=z), dict(esq=z), dict(idx=z), dict(d2=z), dict(comp=z), dict(bin=z), dict(flag=z), dict(na=0), dict(nb=0),
                dict(na=-1), dict(na=(1 << 30) + 1), dict(R=0), dict(G=0), dict(G=1366), dict(esq=C.cast(unsorted, C.c_void_p)),
                dict(esq=C.cast(negative, C.c_void_p)), dict(view=C.cast(nanview, C.c_void_p)), dict(esq=C.cast(wide, C.c_void_p), R=65)):
        assert call(**bad) == -1, bad
    assert L.scp_dist_segments_f64(z, one, one, z, 10, one, 3, one, None) == -1
    assert L.scp_dist_segments_f64(one, one, one, z, 0, one, 3, one, None) == -1
    assert L.scp_dist_segments_f64(one, one, one, z, 10, z, 3, one, None) == -1
    assert L.scp_dist_segments_f64(one, one, one, z, 10, one, 0, one, None) == -1
    assert L.scp_dist_segments_f64(one, one, one, z, 10, one, 4097, one, None) == -1
    assert L.scp_dist_segments_f64(one, one, one, z, 10, one, 3, z, None) == -1
