"""The correctly rounded quantiser reference (tests/quantiser_ref.py) against everything numpy-made that the repository records: the
reference differs from numpy's integers only where numpy's documented float32 error (phi / theta within 2 ulp) can flip
a rounding boundary of t / qs, and the counts of such coordinates are pinned - both sides are fixed data.  No GPU: this file vouches
for the helper that tests/test_gpu_geom.py holds the device kernels to."""
import numpy as np
import pytest

import quantiser_ref as R
from conftest import golden

AMBIGUOUS_CAP = 2e-5          # at most 2 ambiguous values per 100 000 points: a condition on the inputs, not a tolerance
ANY_COUNT_NS = [1, 2, 3, 5, 63, 64, 65, 255, 257, 4001, 119999]       # test_gpu_geom.py: test_quantizer_any_point_count


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def within_cap(ref):
    return R.n_ambiguous(ref) <= AMBIGUOUS_CAP * len(ref.q)


@pytest.fixture(scope="module")
def frame0():
    from scp_amd.synth import synth_frame
    return synth_frame(0)


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_vs_numpy_transform_fixtures(seed):
    z = golden(f"xform_s{seed}")
    for mode in ("spher", "cylin"):
        tr = R.cr_transform(z["xyz"], mode)
        u = ulps(tr, z[f"{mode}_tr"])
        assert u[:, 0].max() == 0 and u[:, 2].max() == 0          # rho, theta / z: bit-identical
        assert u[:, 1].max() <= 2                                 # numpy's SIMD float32 arctan2
        print(f"xform_s{seed} {mode}: phi differs from numpy at {int((u[:, 1] > 0).sum())} of {len(u)} points, max {u[:, 1].max()} ulp")
        for L in (12, 14, 16, 18):
            ref = R.cr_quantise(z["xyz"], 400 / (2 ** L - 1), mode, -200.0)
            assert np.array_equal(ref.tr, tr)
            assert ref.bin_num == float(z[f"{mode}_L{L}_bin"])
            if mode == "cylin":
                assert ref.offset[2] == float(z[f"{mode}_L{L}_zoff"])
            cols, pts, bad = R.unexplained(mode, ref, z[f"{mode}_L{L}_q"])
            assert bad == 0 and cols[0] == 0, (mode, L, cols, bad)
            assert within_cap(ref)
    for L in (12, 14, 16, 18):
        ref = R.cr_quantise(z["xyz"], 400 / (2 ** L - 1), "cart", -200.0)
        assert np.array_equal(ref.q, z[f"cart_L{L}_q"])


FRAME, FORD = R.FRAME_INTS_CASES[:6], R.FRAME_INTS_CASES[6:]


@pytest.mark.parametrize("name,mode,qs,off,want_cols,want_pts", FRAME + FORD, ids=[c[0] for c in FRAME + FORD])
def test_reference_vs_full_frame_ints(frame0, name, mode, qs, off, want_cols, want_pts):
    from scp_amd.synth import ford_like
    xyz = ford_like(frame0) if "ford" in name else frame0
    ref = R.cr_quantise(xyz, qs, mode, off)
    cols, pts, bad = R.unexplained(mode, ref, golden("frame_ints")[name])
    print(f"{name}: differing coordinates {cols}, points {pts}, unexplained {bad}, ambiguous {R.n_ambiguous(ref)}")
    assert bad == 0
    assert cols == want_cols and pts == want_pts
    assert within_cap(ref)
    assert not np.isnan(ref.tr).any() and ref.min_coord >= 0


@pytest.mark.parametrize("mode", ["spher", "cylin", "cart"])
def test_reference_vs_oracle_quantiser(orc, mode):
    """numpy's own arithmetic on this machine (oracle.quantise): every differing coordinate is explained; bin_num and offsets agree."""
    from scp_amd.synth import synth_frame
    xyz7 = synth_frame(7)
    cases = [(f"synth7[:{n}]", xyz7[:n].copy(), 12) for n in ANY_COUNT_NS]
    if mode != "cart":
        cases += [("edge", R.edge_points(mode), L) for L in (12, 16, 18)]
    seen = {}
    for tag, xyz, L in cases:
        qs = 400 / (2 ** L - 1)
        ref = R.cr_quantise(xyz, qs, mode, -200.0)
        with np.errstate(all="ignore"):
            _, bin_num, _, offset, pt = orc.quantise(xyz, qs, mode)
        if mode != "cart":
            assert ref.bin_num == bin_num
        if mode == "cylin":
            assert ref.offset[2] == float(offset[0, 2])
        cols, pts, bad = R.unexplained(mode, ref, pt)
        assert bad == 0 and cols[0] == 0, (tag, L, cols, bad)
        if mode != "spher":
            assert cols[2] == 0
        assert within_cap(ref), (tag, L)
        if pts:
            seen[(tag, L)] = cols
    print(f"{mode}: cases with coordinates differing from this machine's numpy: {seen}")


@pytest.mark.parametrize("mode", ["spher", "cylin"])
def test_edge_points_are_well_defined(mode):
    """The crafted set does what it is there for: no NaN, no negative integer, no ambiguous value, the seam reaches the top phi bin,
    denormals survive into the transformed coordinates, and the frame is ragged for 256-thread workgroups."""
    xyz = R.edge_points(mode)
    assert xyz.dtype == np.float32 and len(xyz) == 4050 + (mode == "cylin") and len(xyz) % 256
    tiny = np.abs(xyz[(xyz != 0) & (np.abs(xyz) < np.finfo(np.float32).tiny)])
    assert len(tiny) == 8                                             # the 1e-40 coordinates are float32 denormals
    for L in (12, 16, 18):
        ref = R.cr_quantise(xyz, 400 / (2 ** L - 1), mode, -200.0)
        assert not np.isnan(ref.tr).any() and ref.min_coord == 0
        assert R.n_ambiguous(ref) == 0
        assert ref.q[:, 1].max() == ref.bin_num - 1                   # -1e-30 -> + 2 pi
        assert ref.q[:, 1].min() == 0
    phi = ref.tr[:, 1]
    assert ((phi > 0) & (phi < np.finfo(np.float32).tiny)).sum() == 2      # atan2(1e-40, r): a denormal float32 angle
    assert (phi == R.TWO_PI_F).sum() >= 4                              # -1e-30 and -1e-40 wrap to 2 pi itself
    assert (phi == R.PI_F).sum() >= 10                                 # the seam from both sides
    if mode == "spher":
        th = ref.tr[:, 2]
        assert (th == 0).sum() >= 2 and (th == R.PI_F).sum() >= 2      # the poles (z / rho rounds to +-1 next to them too)


@pytest.mark.parametrize("mode", ["spher", "cylin"])
def test_ambiguity_census_of_the_gpu_inputs(frame0, mode):
    """The inputs that only the GPU tests use keep to the cap as well (the ambiguity of a value does not depend on the step)."""
    from scp_amd.synth import ford_like, synth_frame
    for tag, xyz in (("synth3[:4097]", synth_frame(3)[:4097]), ("synth1[:7]", synth_frame(1)[:7]), ("ford[::29]", ford_like(frame0)[::29]),
                     ("synth7", synth_frame(7))):
        ref = R.cr_quantise(xyz, 1.0, mode, 0.0)
        assert within_cap(ref), (tag, R.n_ambiguous(ref))
        assert not np.isnan(ref.tr).any()


def test_ambiguous_window():
    """Midpoints of float32 neighbours are ambiguous, values a float32 ulp / 1000 away are not, and the window holds ~2^-21 of all values."""
    f = np.array([1.0, 3.1415927, 6.2831855, 1e-3, 1.5e-40], np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    ulp = np.spacing(f).astype(np.float64)
    assert R.ambiguous(mid).all() and R.ambiguous(-mid).all()
    assert R.ambiguous(mid[:4] * (1 + 2.0 ** -46)).all()
    assert not R.ambiguous(mid + ulp / 1000).any() and not R.ambiguous(f.astype(np.float64)).any()
    assert not R.ambiguous(np.array([0.0, np.nan, np.pi, np.pi / 2])).any()
    v = np.random.default_rng(0).uniform(0.5, 6.3, 4_000_000)
    assert 0.5 * 2.0 ** -21 < R.ambiguous(v).mean() < 2 * 2.0 ** -21


def test_explained_refuses_everything_else():
    one = np.ones(1)
    # a +-1 flip right at the boundary of an angular column is explained ...
    assert R.explained("spher", 1, [10], [11], 10.5 * one, np.float32(10.5) * one, 0.0, 1.0).all()
    assert R.explained("cylin", 1, [10], [9], 9.5 * one, np.float32(9.5) * one, 0.0, 1.0).all()
    # ... not in rho, z or a Cartesian axis, not a difference of 2, not 3 ulp away from the boundary
    assert not R.explained("spher", 0, [10], [11], 10.5 * one, np.float32(10.5) * one, 0.0, 1.0).any()
    assert not R.explained("cylin", 2, [10], [11], 10.5 * one, np.float32(10.5) * one, 0.0, 1.0).any()
    assert not R.explained("cart", 1, [10], [11], 10.5 * one, np.float32(10.5) * one, 0.0, 1.0).any()
    assert not R.explained("spher", 2, [10], [12], 11.0 * one, np.float32(11.0) * one, 0.0, 1.0).any()
    u = float(np.spacing(np.float32(10.5)))
    assert R.explained("spher", 2, [10], [11], (10.5 - 2.4 * u) * one, np.float32(10.5) * one, 0.0, 1.0).all()
    assert not R.explained("spher", 2, [10], [11], (10.5 - 3 * u) * one, np.float32(10.5) * one, 0.0, 1.0).any()
