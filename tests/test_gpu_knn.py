"""The kNN searches of scp_amd/csrc/knn.hip on the windows of tests/knn_cases.py against tests/knn_ref.py: THE list, entry for entry,
wherever the distances are exact (lattice positions through the box-skipping kernel, scaled-integer features through the per-row
scales of the f16x3 path), validity under the derived per-pair bound elsewhere, and one list per window whatever the launch it sits
in.  The only tolerances here are equality and knn_ref.bound."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import knn_cases as KC
import knn_ref as KR
from conftest import parity_record

pytestmark = pytest.mark.gpu
K = KC.K
KNN_MODES = (True, False)                                  # f16x3 (default), exact fp32 chain
SHAPES = (128, 256, 257, 258, 272)                         # workgroup shapes of the packed f16x3 search; 256 alone splits short launches
PACKED = [c.name for c in KC.cases() if c.group != "generic"]
GROUPS = ("pos", "f144", "f192")
ORDERS = (0, 1, 2)                                         # arrangements of a group's windows in one packed launch, see `among`


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from scp_amd import native
    native.lib()
    return torch.device("cuda:0")


@contextlib.contextmanager
def knn_setting(f16x3, shape=256):
    from scp_amd import native
    try:
        native.set_knn_mode(f16x3)
        native.set_knn_workgroup(shape)
        yield
    finally:
        native.set_knn_mode(True)
        native.set_knn_workgroup(256)


@functools.lru_cache(maxsize=None)
def truth(name):
    """(idx, D) of the case's k = min(20, n) nearest in float64; for exact cases idx is exact_topk's list."""
    c = KC.by_name(name)
    k = min(K, len(c.x))
    idx, val = KR.topk_f64(c.x, k)
    if c.exact:
        assert np.array_equal(idx, KR.exact_topk(c.x, k))
    return idx, val


_CACHE = {}


def dense(dev, name, f16x3):
    """The case through scp_knn_topk as one item: int64 [n, k]."""
    key = ("dense", name, f16x3)
    if key not in _CACHE:
        from scp_amd import native
        c = KC.by_name(name)
        n, C = c.x.shape
        if c.misaligned:                                   # same values, one float behind a 16-byte boundary
            buf = torch.zeros(n * C + 4, dtype=torch.float32, device=dev)
            buf[1:1 + n * C] = torch.from_numpy(np.array(c.x)).reshape(-1).to(dev)
            x = buf[1:1 + n * C].view(1, n, C)
            assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        else:
            x = torch.from_numpy(np.array(c.x))[None].to(dev)
        with knn_setting(f16x3):
            _CACHE[key] = native.knn_topk(x, min(K, n)).cpu().numpy().astype(np.int64)[0]
    return _CACHE[key]


def launch_packed(dev, windows, f16x3, shape):
    from scp_amd import native
    x, tab, bases = KC.pack(windows)
    with knn_setting(f16x3, shape):
        out = native.knn_topk_packed(torch.from_numpy(x).to(dev), torch.from_numpy(tab).to(dev)).cpu().numpy().astype(np.int64)
    return out, bases


def alone(dev, name, f16x3, shape=256):
    """The case as the only sequence of a packed launch: the whole output [T, 20], global indices (its base is 0)."""
    key = ("alone", name, f16x3, shape)
    if key not in _CACHE:
        _CACHE[key] = launch_packed(dev, [KC.by_name(name).x], f16x3, shape)[0]
    return _CACHE[key]


def among(dev, group, order, f16x3, shape=256):
    """Every case of a group in ONE packed launch: in list order (order 0), rotated by half the list (order 1: every case starts at
    another row) or reversed (order 2: every case has other neighbours): (output [T, 20], {name: base})."""
    key = ("among", group, order, f16x3, shape)
    if key not in _CACHE:
        names = KC.names(group=group)
        names = [names, names[len(names) // 2:] + names[:len(names) // 2], names[::-1]][order]
        out, bases = launch_packed(dev, [KC.by_name(n).x for n in names], f16x3, shape)
        _CACHE[key] = (out, dict(zip(names, bases)))
    return _CACHE[key]


def shapes_of(name, f16x3):
    """The workgroup shapes that reach different kernels for the case: only the f16x3 feature search has more than one."""
    return SHAPES if f16x3 and KC.by_name(name).group != "pos" else (256,)


# ------------------------------------------------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("name", [n for n in PACKED if KC.by_name(n).exact])
def test_exact_windows_give_the_exact_list(dev, name):
    """Distances without a rounding, ties by the thousand: dense and packed, both arithmetic modes, must return exact_topk's list -
    on positions through the tile skipping (a tile at exactly the bound must not be skipped, an equal distance with a lower index
    must displace), on features through unequal row scales, a zero row, a repeated row and a doubled row."""
    c = KC.by_name(name)
    want, _ = truth(name)
    k = want.shape[1]
    for f16x3 in KNN_MODES:
        assert KR.check_exact(c.x, dense(dev, name, f16x3), k, want) is None, ("dense", f16x3)
        assert KR.check_exact(c.x, alone(dev, name, f16x3)[:len(c.x), :k], k, want) is None, ("packed", f16x3)


def test_dense_batch_gives_the_exact_lists_of_its_items(dev):
    from scp_amd import native
    xb = KC.dense_batch()
    for f16x3 in KNN_MODES:
        with knn_setting(f16x3):
            got = native.knn_topk(torch.from_numpy(np.array(xb)).to(dev), K).cpu().numpy().astype(np.int64)
            one = native.knn_topk(torch.from_numpy(np.array(xb[1:2])).to(dev), K).cpu().numpy().astype(np.int64)
        for b in range(len(xb)):
            assert KR.check_exact(xb[b], got[b], K) is None, (b, f16x3)
        assert np.array_equal(one[0], got[1])


# ------------------------------------------------------------------------------------------------------------ 2. inexact cases
@pytest.mark.parametrize("name", [n for n in PACKED if not KC.by_name(n).exact])
def test_inexact_windows_give_valid_lists_under_the_derived_bound(dev, name):
    """Real-valued feature windows (shared sibling columns, rows of unequal magnitude, a common offset): every row of every list is
    valid under the bound of ITS pairs.  The largest observed excess over D_k, as a share of the row's tolerance, is recorded."""
    c = KC.by_name(name)
    t = truth(name)
    rec = {}
    for f16x3 in KNN_MODES:
        mode = KC.device_mode(c, f16x3)
        for how, got in (("dense", dense(dev, name, f16x3)), ("packed", alone(dev, name, f16x3)[:len(c.x)])):
            msg, worst = KR.check_valid(c.x, got, K, mode, truth=t)
            print(f"{name} {mode} {how}: worst excess / tol = {worst:.3e}")
            rec[f"{mode}_worst_excess_over_tol"] = max(worst, rec.get(f"{mode}_worst_excess_over_tol", 0.0))
            assert msg is None, (how, mode, msg)
        rec[f"{mode}_lists_equal_float64_lists"] = float((dense(dev, name, f16x3) == t[0]).all(1).mean())
    parity_record(f"knn_cases/{name}", **rec)


# ------------------------------------------------------------------------------------------------------------ 3. shape invariance
@pytest.mark.parametrize("name", PACKED)
def test_a_list_is_a_function_of_its_window(dev, name):
    """Encoder and decoder reach the same window through different launches.  The list of a window must be the same through the dense
    entry point, alone in a packed launch (short: its sweeps are split), among all other cases of its width at two different places
    of one packed launch, and - for the f16x3 feature search - under every workgroup shape (257 never splits a sweep)."""
    c = KC.by_name(name)
    n = len(c.x)
    k = min(K, n)
    for f16x3 in KNN_MODES:
        want = dense(dev, name, f16x3)
        for shape in shapes_of(name, f16x3):
            got = alone(dev, name, f16x3, shape)[:n, :k]
            assert np.array_equal(got, want), ("alone", f16x3, shape, int((got != want).any(1).sum()))
            for order in ORDERS:
                out, bases = among(dev, c.group, order, f16x3, shape)
                got = out[bases[name]:bases[name] + n, :k] - bases[name]
                assert np.array_equal(got, want), ("among", order, f16x3, shape, int((got != want).any(1).sum()))
    assert among(dev, c.group, 0, True)[1][name] != among(dev, c.group, 1, True)[1][name]


# ------------------------------------------------------------------------------------------------------------ 4. packed layout
@pytest.mark.parametrize("group", GROUPS)
def test_packed_rows_behind_a_sequence_stay_zero_and_short_sequences_repeat_their_first(dev, group):
    for f16x3 in KNN_MODES:
        for shape in (SHAPES if f16x3 and group != "pos" else (256,)):
            for order in ORDERS:
                out, bases = among(dev, group, order, f16x3, shape)
                for name, base in bases.items():
                    n = len(KC.by_name(name).x)
                    pad = -(-n // 512) * 512
                    assert not out[base + n:base + pad].any(), (name, f16x3, shape)
                    rows = out[base:base + n]
                    assert (rows >= base).all() and (rows < base + n).all(), (name, f16x3, shape)
                    if n < K:
                        assert (rows[:, n:] == rows[:, :1]).all(), (name, f16x3, shape)
    short = [n for n in KC.names(group="pos") if len(KC.by_name(n).x) < K]
    assert group != "pos" or len(short) >= 3
    for name in short if group == "pos" else ():
        n = len(KC.by_name(name).x)
        out = alone(dev, name, True)
        assert (out[:n, n:] == out[:n, :1]).all() and not out[n:].any()
        assert np.array_equal(out[:n, 0], np.arange(n))                # a point's nearest is itself (no duplicates in the lattice)


# ------------------------------------------------------------------------------------------------------------ 5. generic kernel
@pytest.mark.parametrize("name", KC.names(group="generic"))
def test_generic_kernel(dev, name):
    """Any other feature count, and 144 features on a base that is not 16-byte aligned, go through knn_generic_kernel: exact windows
    give THE list, real-valued ones a valid list under the fp32 bound; the arithmetic mode has no say."""
    c = KC.by_name(name)
    t = truth(name)
    for f16x3 in KNN_MODES:
        got = dense(dev, name, f16x3)
        if c.exact:
            assert KR.check_exact(c.x, got, K, t[0]) is None, f16x3
        else:
            msg, worst = KR.check_valid(c.x, got, K, "f32", truth=t)
            parity_record(f"knn_cases/{name}", f32_worst_excess_over_tol=worst, f32_lists_equal_float64_lists=float((got == t[0]).all(1).mean()))
            assert msg is None, msg
    assert np.array_equal(dense(dev, name, True), dense(dev, name, False))


def test_misaligned_base_gives_the_aligned_list(dev):
    """The same 144-feature window on an aligned base runs the MFMA kernels; both must agree with each other entry for entry."""
    from scp_amd import native
    c = KC.by_name("generic-misaligned-c144")
    with knn_setting(False):
        aligned = native.knn_topk(torch.from_numpy(np.array(c.x))[None].to(dev), K).cpu().numpy().astype(np.int64)[0]
    assert np.array_equal(aligned, dense(dev, c.name, False))


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_entry_points_refuse_what_they_cannot_serve(dev):
    from scp_amd import native
    with pytest.raises(native.ScpError):
        native.knn_topk(torch.zeros((1, 30, 3), device=dev), 21)                               # k > 20
    with pytest.raises(native.ScpError):
        native.knn_topk(torch.zeros((1, 5, 3), device=dev), 6)                                 # k > n
    tab = torch.tensor([[0, 300]], dtype=torch.int32, device=dev)
    buf = torch.zeros(512 * 144 + 4, device=dev)
    off = buf[1:1 + 512 * 144].view(512, 144)
    assert off.data_ptr() % 16 == 4
    for thr in (None, torch.full((512,), float("-inf"), device=dev)):                          # plain and bounded packed entry points
        with pytest.raises(native.ScpError):
            native.knn_topk_packed(torch.zeros((512, 100), device=dev), tab, thr)              # a width without a packed kernel
        with pytest.raises(native.ScpError):
            native.knn_topk_packed(off, tab, thr)                                              # 144 features off a 16-byte boundary
        with pytest.raises(native.ScpError):
            native.knn_topk_packed(torch.zeros((500, 144), device=dev), tab, None if thr is None else thr[:500])   # rows not x512
    assert native.knn_topk_packed(buf[:512 * 144].view(512, 144), tab).shape == (512, 20)      # the aligned view is served
