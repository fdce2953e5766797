"""The windows of tests/knn_cases.py and the checkers of tests/knn_ref.py, on the CPU: every case still has the edge it is named for, and
the checkers reject deliberately wrong lists, so that tests/test_gpu_knn.py cannot pass for want of a hard input or of teeth."""
import functools

import numpy as np
import pytest

import knn_cases as KC
import knn_ref as KR

K = KC.K
EXACT = [c.name for c in KC.cases() if c.exact]
INEXACT = [c.name for c in KC.cases() if not c.exact]


@functools.lru_cache(maxsize=None)
def top(name, k):
    c = KC.by_name(name)
    return KR.topk_f64(c.x, min(k, len(c.x)))


def tie_share(name):
    """Share of the queries whose 20th and 21st neighbour are at exactly the same distance."""
    _, val = top(name, K + 1)
    return float((val[:, K - 1] == val[:, K]).mean())


def test_the_list_covers_what_it_promises():
    names = {c.name for c in KC.cases()}
    assert len(names) == len(KC.cases())
    assert {"morton-lattice", "morton-lattice-raw", "lattice-8192", "all-equal", "two-clusters-of-duplicates", "line"} <= names
    assert {f"lattice-{n}" for n in (1, 7, 19, 20, 21, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 2049)} <= names
    for C in (144, 192):
        assert {f"scaled-int-c{C}-{n}" for n in (21, 300, 513, 2049)} <= names
        assert {f"{f}-c{C}-{n}" for f in ("siblings", "mixed-magnitude", "offset") for n in (300, 2049)} <= names
    assert "siblings-c144-8192" in names and "generic-misaligned-c144" in names
    for C in (5, 8, 64, 145, 200):
        assert {f"generic-scaled-int-c{C}", f"generic-siblings-c{C}"} <= names
        assert all(KC.by_name(n).x.shape == (300, C) for n in (f"generic-scaled-int-c{C}", f"generic-siblings-c{C}"))
    assert KC.dense_batch().shape == (3, 1000, 3) and 1000 % 32 != 0
    for c in KC.cases():
        assert c.x.dtype == np.float32 and np.isfinite(c.x).all()
        assert c.x.shape[1] == {"pos": 3, "f144": 144, "f192": 192}.get(c.group, c.x.shape[1])
    assert np.array_equal(KC.by_name("morton-lattice").x * 1024, KC.by_name("morton-lattice-raw").x)
    assert len(np.unique(KC.lattice_cloud(), axis=0)) == len(KC.lattice_cloud())


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_are_exact_in_the_kernels_fp32_arithmetic(name):
    c = KC.by_name(name)
    assert KR.is_exact_in_fp32(c.x)
    if c.x.shape[1] in KC.FEATURE_C:                       # the f16x3 split is exact as well: 11 bits hold every scaled entry
        m = np.abs(c.x).max(1, keepdims=True).astype(np.float64)
        t = c.x / np.where(m > 0, 2.0 ** np.floor(np.log2(np.where(m > 0, m, 1.0))), 1.0) * 2.0 ** 13
        assert np.array_equal(t.astype(np.float16).astype(np.float64), t)
    k = min(K, len(c.x))
    idx, _ = top(name, K + 1)
    assert np.array_equal(KR.exact_topk(c.x, k), idx[:, :k])           # the integer and the float64 reference agree


def test_dense_batch_is_exact():
    for item in KC.dense_batch():
        assert KR.is_exact_in_fp32(item)


def test_is_exact_in_fp32_sees_a_rounding():
    x = np.array(KC.by_name("lattice-33").x)
    assert KR.is_exact_in_fp32(x)
    x[5, 1] += np.float32(2.0 ** -13) + np.float32(2.0 ** -24)
    assert not KR.is_exact_in_fp32(x)
    assert not KR.is_exact_in_fp32(KC.by_name("siblings-c144-300").x[:40])
    assert not KR.is_exact_in_fp32(np.full((3, 2), 0.1))               # not float32 values at all


@pytest.mark.parametrize("name", KC.names(family="morton"))
def test_morton_lattice_has_ties_skippable_tiles_and_touching_boxes(name):
    """The box test of knn_mfma_kernel<2, 16, true> on the final bound: a (query group, 32-candidate tile) pair is skippable when the
    squared gap of the two boxes exceeds the farthest 20th-best distance of the group's queries."""
    x = KC.by_name(name).x.astype(np.float64)
    _, val = top(name, K + 1)
    assert tie_share(name) >= 0.25
    g = len(x) // 32
    xb = x.reshape(g, 32, 3)
    lo, hi = xb.min(1), xb.max(1)
    gap = np.maximum(np.maximum(lo[None, :, :] - hi[:, None, :], lo[:, None, :] - hi[None, :, :]), 0.0)
    lb2 = (gap * gap).sum(2)                               # [query group, tile], exact on the lattice
    far2 = val[:, K - 1].reshape(g, 32).max(1)[:, None]
    n2 = (xb * xb).sum(2).max(1)
    margin = 2.0 ** -14 * (n2[:, None] + n2[None, :])      # the kernel's guard on top of far2
    assert (lb2 > far2).mean() >= 0.30 and (lb2 > far2 + margin).mean() >= 0.30
    assert (lb2 == far2).sum() >= 1


@pytest.mark.parametrize("name", KC.names(family="scaled-int"))
def test_scaled_integer_cases_tie_and_mix_scales(name):
    x = KC.by_name(name).x.astype(np.float64)
    m = np.abs(x).max(1)
    assert len(np.unique(np.floor(np.log2(m[m > 0])))) >= 3
    assert (m == 0).sum() == 1
    if len(x) > K:
        _, val = top(name, K + 1)
        assert 10 * int((val[:, K - 1] == val[:, K]).sum()) >= len(x)
        assert np.array_equal(x[5], x[2]) and np.array_equal(x[9], 2 * x[4])


@pytest.mark.parametrize("name", KC.names(family="mixed-magnitude"))
def test_mixed_magnitude_spans_twenty_octaves(name):
    x = KC.by_name(name).x.astype(np.float64)
    nr = np.sqrt((x * x).sum(1))
    assert (nr == 0).sum() == 1 and nr.max() / nr[nr > 0].min() >= 2.0 ** 20
    a = np.sort(np.abs(x[3]))
    assert a[-1] >= 2.0 ** 20 * a[-2] * 0.25 and a[-2] > 0              # one feature about 2^20 times the others


@pytest.mark.parametrize("name", KC.names(family="siblings"))
def test_siblings_share_their_first_columns(name):
    x = KC.by_name(name).x
    sh = min(128, x.shape[1] - 1) if x.shape[1] in KC.FEATURE_C else (x.shape[1] * 2) // 3
    same = (x[1:, :sh] == x[:-1, :sh]).all(1)
    assert 0.5 < same.mean() < 0.95 and not (x[1:] == x[:-1]).all(1).any()
    run = np.diff(np.flatnonzero(np.concatenate([[True], ~same, [True]])))
    assert run.max() <= 8


@pytest.mark.parametrize("name", KC.names(family="offset"))
def test_offset_is_ten_spreads(name):
    x = KC.by_name(name).x.astype(np.float64)
    assert (np.abs(x.mean(0)) > 8 * x.std(0)).all()


@pytest.mark.parametrize("name", INEXACT)
def test_inexact_cases_keep_a_clearly_farther_neighbour_outside_the_bound(name):
    c = KC.by_name(name)
    idx, val = top(name, 2 * K)
    for mode in sorted({KC.device_mode(c, True), KC.device_mode(c, False)}):
        tol = KR.row_tolerance(c.x, idx[:, :K], mode)
        assert ((val[:, 2 * K - 1] - val[:, K - 1]) > tol).mean() >= 0.90, mode


# ----------------------------------------------------------------------------------------------------------- the checkers have teeth
TEETH_EXACT = ["morton-lattice", "lattice-257", "line", "two-clusters-of-duplicates", "scaled-int-c144-300", "generic-scaled-int-c5"]
TEETH_INEXACT = ["siblings-c144-300", "mixed-magnitude-c192-300", "offset-c144-300", "generic-siblings-c5"]


def structural_damage(want, n):
    dup = want.copy()
    dup[n // 2, 5] = dup[n // 2, 4]
    nb = want.copy()
    nb[n - 1, 3] = n                                       # first row of the sequence behind this one
    neg = want.copy()
    neg[0, 0] = -1                                         # last row of the sequence in front of it
    return {"duplicated index": dup, "index of the next sequence": nb, "index of the previous sequence": neg}


@pytest.mark.parametrize("name", TEETH_EXACT)
def test_exact_checker_accepts_the_reference_and_rejects_wrong_lists(name):
    c = KC.by_name(name)
    n = len(c.x)
    idx, val = top(name, K + 1)
    want = idx[:, :K]
    assert KR.check_exact(c.x, want, K) is None
    assert KR.check_valid(c.x, want, K, "f32")[0] is None
    r, t = [int(v[0]) for v in np.nonzero(val[:, :K - 1] == val[:, 1:K])]
    swapped = want.copy()
    swapped[r, [t, t + 1]] = swapped[r, [t + 1, t]]
    assert KR.check_exact(c.x, swapped, K) is not None                  # a tie pair in the wrong order
    clear = np.flatnonzero(val[:, K] > val[:, K - 1])
    if name != "two-clusters-of-duplicates":                            # (every row of that one ties at the 20th)
        late = want.copy()
        late[clear[0], K - 1] = idx[clear[0], K]
        assert KR.check_exact(c.x, late, K) is not None                 # the 21st instead of the 20th on a row without a tie
    for what, bad in structural_damage(want, n).items():
        assert KR.check_exact(c.x, bad, K) is not None, what
        assert KR.check_valid(c.x, bad, K, "f32")[0] is not None, what


@pytest.mark.parametrize("name", TEETH_INEXACT)
def test_validity_checker_accepts_the_reference_and_rejects_wrong_lists(name):
    c = KC.by_name(name)
    n = len(c.x)
    idx, val = top(name, K + 1)
    want = idx[:, :K]
    for mode in sorted({KC.device_mode(c, True), KC.device_mode(c, False)}):
        msg, worst = KR.check_valid(c.x, want, K, mode, truth=(want, val[:, :K]))
        assert msg is None and worst < 1e-6                            # (float64 noise of two ways to form D)
        tol = KR.row_tolerance(c.x, idx, mode)                          # over the 21 nearest: covers every list built below
        r, t = [int(v[0]) for v in np.nonzero(np.diff(val[:, :K], axis=1) > tol[:, None])]
        swapped = want.copy()
        swapped[r, [t, t + 1]] = swapped[r, [t + 1, t]]
        assert KR.check_valid(c.x, swapped, K, mode)[0] is not None     # two clearly different neighbours in the wrong order
        r = int(np.flatnonzero(val[:, K] - val[:, K - 1] > tol)[0])
        late = want.copy()
        late[r, K - 1] = idx[r, K]
        assert KR.check_valid(c.x, late, K, mode)[0] is not None        # the 21st instead of the 20th where they clearly differ
        near = int(np.argmin(np.where(val[:, K] > val[:, K - 1], val[:, K] - val[:, K - 1], np.inf) / tol))
        if val[near, K] - val[near, K - 1] < 0.5 * tol[near]:           # ... and accepted where the bound cannot tell them apart
            ok = want.copy()
            ok[near, K - 1] = idx[near, K]
            assert KR.check_valid(c.x, ok, K, mode)[0] is None
        for what, bad in structural_damage(want, n).items():
            assert KR.check_valid(c.x, bad, K, mode)[0] is not None, what


def test_bound_is_per_pair_and_scales_with_the_pair():
    """E(i, j) is built from the pair's own sums: scaling both rows by s scales it by s^2, and a small pair inside a window of large
    rows keeps a small bound (a window-wide maximum would not)."""
    c = KC.by_name("mixed-magnitude-c144-300")
    x = c.x.astype(np.float64)
    nr = (x * x).sum(1)
    small = np.argsort(nr)[1:3]                            # the two smallest non-zero rows
    for mode in KR.MODES:
        e = float(KR.bound(x, small[0], small[1], mode))
        assert 0 < e <= 2e-4 * (nr[small[0]] + nr[small[1]]) * 2 and e < 1e-9 * nr.max()
        assert np.isclose(float(KR.bound(4.0 * x, small[0], small[1], mode)), 16.0 * e, rtol=1e-12)
        assert float(KR.bound(x, 1, 1, mode)) == 0.0       # the zero row against itself
    assert float(KR.bound(x, 5, 6, "f16x3")) > float(KR.bound(x, 5, 6, "f32"))
    i = np.arange(10)[:, None]
    assert KR.bound(x, i, np.arange(7)[None, :], "f32").shape == (10, 7)


def test_pack_lays_sequences_out_in_512_row_chunks():
    x, tab, bases = KC.pack([KC.by_name("lattice-7").x, KC.by_name("lattice-513").x, KC.by_name("lattice-512").x])
    assert x.shape == (512 + 1024 + 512, 3) and bases == [0, 512, 1536]
    assert tab.tolist() == [[0, 7], [512, 513], [512, 513], [1536, 512]]
    assert np.array_equal(x[512:512 + 513], KC.by_name("lattice-513").x) and not x[7:512].any()
