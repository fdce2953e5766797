"""Step sweep of the attribute layers, host side ("Step sweep"): the choice of a step from a sweep table, the grid's rules,
the CLI request helpers' refusals and the argument checks of the two C entries, which run before any HIP call.  No GPU."""
import argparse
import math

import numpy as np
import pytest


def table(rows, points=1000):
    """A hand-made sweep table: rows of (Q, est_bits, psnr, linf)."""
    return dict(points=points, rows=[dict(Q=q, est_bits=b, psnr=p, linf=e) for q, b, p, e in rows])


MONOTONE = [(1, 9000, math.inf, 0), (2, 7000, 50.0, 1), (4, 5000, 44.0, 2), (8, 3000, 38.0, 5), (16, 2000, 31.0, 11)]


def test_choose_step_for_each_kind():
    from scp_amd import attr, color
    assert color.choose_step is attr.choose_step
    t = table(MONOTONE)
    assert attr.choose_step(t, "psnr", 40.0) == dict(kind="psnr", value=40.0, Q=4, index=2, met=True)
    assert attr.choose_step(t, "psnr", 1000.0) == dict(kind="psnr", value=1000.0, Q=1, index=0, met=True)     # inf >= anything finite
    assert attr.choose_step(t, "linf", 5) == dict(kind="linf", value=5.0, Q=8, index=3, met=True)
    assert attr.choose_step(t, "linf", 0) == dict(kind="linf", value=0.0, Q=1, index=0, met=True)
    assert attr.choose_step(t, "bpp", 4.0) == dict(kind="bpp", value=4.0, Q=8, index=3, met=True)             # 3000 <= 4000 < 5000
    assert attr.choose_step(t, "bpp", 100.0)["Q"] == 1                                                        # the smallest step that fits


def test_choose_step_takes_the_largest_qualifying_step_of_a_non_monotone_table():
    """The error need not grow with the step: Q = 4 misses the target, Q = 8 meets it again - the largest qualifying step wins, not the
    step before the first failure."""
    from scp_amd import attr
    t = table([(1, 9000, math.inf, 0), (2, 7000, 50.0, 1), (4, 5000, 39.0, 7), (8, 3000, 41.0, 4), (16, 2000, 31.0, 11)])
    assert attr.choose_step(t, "psnr", 40.0) == dict(kind="psnr", value=40.0, Q=8, index=3, met=True)
    assert attr.choose_step(t, "linf", 4) == dict(kind="linf", value=4.0, Q=8, index=3, met=True)
    # a non-monotone rate: the smallest qualifying step, though a smaller step's neighbour fails
    t = table([(1, 9000, math.inf, 0), (2, 3900, 50.0, 1), (4, 5000, 44.0, 2), (8, 3000, 38.0, 5)])
    assert attr.choose_step(t, "bpp", 4.0) == dict(kind="bpp", value=4.0, Q=2, index=1, met=True)


def test_choose_step_reports_a_target_nothing_meets():
    from scp_amd import attr
    t = table(MONOTONE[1:])
    assert attr.choose_step(t, "psnr", 60.0) == dict(kind="psnr", value=60.0, Q=2, index=0, met=False)
    assert attr.choose_step(t, "linf", 0) == dict(kind="linf", value=0.0, Q=2, index=0, met=False)
    assert attr.choose_step(t, "bpp", 1.0) == dict(kind="bpp", value=1.0, Q=16, index=3, met=False)


def test_choose_step_on_ties():
    from scp_amd import attr
    t = table([(1, 9000, 45.0, 2), (2, 5000, 45.0, 2), (4, 5000, 45.0, 2), (8, 3000, 38.0, 5)])
    assert attr.choose_step(t, "psnr", 45.0)["Q"] == 4           # equal to the target qualifies; of equal rows the largest step
    assert attr.choose_step(t, "linf", 2)["Q"] == 4
    assert attr.choose_step(t, "bpp", 5.0)["Q"] == 2             # est_bits == value x points qualifies; of equal rows the smallest step
    assert attr.choose_step(t, "bpp", 3.0)["Q"] == 8


def test_choose_step_refuses_bad_targets():
    from scp_amd import attr, native
    t = table(MONOTONE)
    for kind, value in (("mse", 1.0), ("psnr", math.nan), ("psnr", math.inf), ("bpp", -0.5), ("linf", -1), ("psnr", "forty")):
        with pytest.raises(native.ScpError):
            attr.choose_step(t, kind, value)
    with pytest.raises(native.ScpError, match="empty"):
        attr.choose_step(dict(points=1, rows=[]), "psnr", 40.0)


def test_sweep_rows_sum_shells_and_price_the_file():
    """table_bits through choose_tables per context and shell, est_bits with the frame's header and record bytes and a rounded-up
    payload per coded shell, PSNR over leaf values."""
    from scp_amd import attr
    h = np.zeros((2, 3, attr.ALPHABET), np.int64)
    h[0, :, 0] = 100                                             # step 0: 300 zeros; step 1: 30 symbols 2
    h[1, 0, 2] = 30
    shells = [(101, h, np.array([[0], [640]]), np.array([[0], [9]])), (1, None, None, None), (31, h, np.array([[0], [60]]), np.array([[0], [3]]))]
    rows = attr.sweep_rows([1, 8], 1, 50, shells)
    per = [float(attr.choose_tables(h[g])[1].sum()) for g in range(2)]
    for g, r in enumerate(rows):
        assert r["Q"] == (1, 8)[g] and r["table_bits"] == 2 * per[g] and r["leaves"] == 133
        assert r["est_bits"] == 8 * (50 + 2 * math.ceil(per[g] / 8))
    assert rows[0]["sse"] == 0 and rows[0]["linf"] == 0 and rows[0]["psnr"] == math.inf
    assert rows[1]["sse"] == 700 and rows[1]["linf"] == 9 and rows[1]["psnr"] == 10 * math.log10(255 ** 2 * 133 / 700)
    assert attr.record_bytes(12, 0) == 5 and attr.record_bytes(12, 1) == 6 and attr.record_bytes(12, 2) == 22
    from scp_amd import color
    assert color.record_bytes(12, 0) == 5 and color.record_bytes(12, 1) == 10 and color.record_bytes(12, 2) == 50
    # the record sizes are the ones `pack` writes
    assert len(attr.pack(1, 255, [dict(D=12, U=0), dict(D=12, U=1, root=7), dict(D=12, U=2, root=7, tables=[0] * 12, payload=b"abc")])) == 11 + 5 + 6 + 22 + 3
    assert len(color.pack(1, [dict(D=12, U=0), dict(D=12, U=1, root=(7, 0, 0)), dict(D=12, U=2, root=(7, 0, 0), tables=[0] * 36, payload=b"abc")])) == 8 + 5 + 10 + 50 + 3


def test_sweep_steps_accepts_the_default_grid_and_refuses_malformed_ones():
    from scp_amd import native
    assert native.SWEEP_MAX_STEPS == 16
    g = native.sweep_steps()
    assert g.dtype == np.int32 and g.tolist() == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 255]
    assert native.sweep_steps(g).tolist() == g.tolist() and native.sweep_steps((1,)).tolist() == [1]
    assert native.sweep_steps([3, 200, 255]).tolist() == [3, 200, 255]
    for bad in ([], list(range(1, 18)), [1, 1], [2, 1], [1, 8, 8], [0, 1], [1, 256], [-3], [1.5], [True, 2], ["a"]):
        with pytest.raises(native.ScpError, match="sweep steps"):
            native.sweep_steps(bad)


def ns(**kw):
    return argparse.Namespace(**kw)


def test_request_helpers_accept_well_formed_options():
    from scp_amd import cli
    assert cli.sweep_request(ns(), "attr") == (None, None) and cli.sweep_request(ns(attr=4), "attr") == (None, None)
    steps, target = cli.sweep_request(ns(attr=1, attr_sweep=""), "attr")
    assert steps.tolist() == list(cli.native.SWEEP_STEPS) and target is None
    steps, target = cli.sweep_request(ns(color=1, color_sweep="1,8,255", color_target="linf=4"), "color")
    assert steps.tolist() == [1, 8, 255] and target == ("linf", 4.0)
    assert cli.sweep_request(ns(attr=1, attr_target="psnr=40.5"), "attr") == (None, ("psnr", 40.5))
    assert cli.sweep_request(ns(attr=1, attr_target="bpp=0"), "attr") == (None, ("bpp", 0.0))
    assert cli.sweep_request(ns(attr=7, attr_sweep="2,4"), "attr")[0].tolist() == [2, 4]          # a sweep alone goes with any Q


@pytest.mark.parametrize("layer", ["attr", "color"])
def test_request_helpers_refuse_with_the_reason(layer):
    from scp_amd import cli, native

    def refused(match, **kw):
        with pytest.raises(native.ScpError, match=match):
            cli.sweep_request(ns(**{k.replace("L", layer): v for k, v in kw.items()}), layer)

    refused(f"give --{layer} as well", L_sweep="")                           # without the layer flag
    refused(f"give --{layer} as well", L_target="psnr=40")
    refused("chooses the step", L=4, L_target="psnr=40")                     # a Q other than 1 together with a target
    refused("unknown kind", L=1, L_target="mse=3")
    refused("KIND=VALUE", L=1, L_target="psnr")
    refused("KIND=VALUE", L=1, L_target="psnr=high")
    refused("finite value >= 0", L=1, L_target="psnr=nan")
    refused("finite value >= 0", L=1, L_target="bpp=inf")
    refused("finite value >= 0", L=1, L_target="linf=-1")
    refused("sweep steps", L=1, L_sweep=",".join(str(v) for v in range(1, 18)))     # longer than 16
    refused("strictly ascending", L=1, L_sweep="1,4,4")
    refused("strictly ascending", L=1, L_sweep="8,4")
    refused("1 .. 255", L=1, L_sweep="0,4")
    refused("1 .. 255", L=1, L_sweep="4,256")
    refused("comma-separated", L=1, L_sweep="1,,4")
    refused("comma-separated", L=1, L_sweep="a,b")
    refused("comma-separated", L=1, L_sweep=",")


def test_sweep_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks come before any HIP call: SCP_EINVAL (-1) on a machine without a GPU, nothing launched."""
    from scp_amd import native
    L = native.lib()
    z, one = None, 4096                 # NULL and a fake (never dereferenced) non-NULL address
    big = 1 << 40

    def grid(*v):
        return np.array(v, np.int32)

    def attr(steps=grid(1, 8, 255), G=None, U=100, D=10, hist=one, sse=one, linf=one, root=one, counts=one, ws=one, nb=big, a=one, leaves=one):
        sp = z if steps is None else steps.ctypes.data
        return L.scp_attr_sweep(leaves, a, U, D, sp, len(steps) if G is None else G, hist, sse, linf, root, counts, ws, nb, z)

    def color(steps=grid(1, 8, 255), G=None, U=100, D=10, hist=one, sse=one, linf=one, root=one, counts=one, ws=one, nb=big, ycc=one, mean=one,
              leaves=one):
        sp = z if steps is None else steps.ctypes.data
        return L.scp_color_sweep(leaves, ycc, mean, U, D, sp, len(steps) if G is None else G, hist, sse, linf, root, counts, ws, nb, z)

    for fn in (attr, color):
        assert fn(G=0) == -1 and fn(grid(*range(1, 18))) == -1 and fn(steps=None, G=3) == -1               # G = 0, G = 17, no grid
        assert fn(grid(8, 4)) == -1 and fn(grid(4, 4)) == -1 and fn(grid(1, 8, 8)) == -1                   # descending, repeated
        assert fn(grid(0, 4)) == -1 and fn(grid(4, 256)) == -1 and fn(grid(-1)) == -1                      # a step of 0, 256, below 0
        assert fn(D=0) == -1 and fn(D=native.MAX_DEPTH + 1) == -1 and fn(U=-1) == -1                       # a bad D, a bad U
        for out in ("hist", "sse", "linf", "root", "counts"):
            assert fn(**{out: z}) == -1, out                                                               # a NULL output
        assert fn(leaves=z) == -1 and fn(ws=z) == -1 and fn(ws=4097) == -1 and fn(nb=64) == -1
    assert attr(a=z) == -1 and color(ycc=z) == -1 and color(mean=z) == -1
    for name, per_leaf in (("scp_attr_sweep_workspace_bytes", 4), ("scp_color_sweep_workspace_bytes", 12)):
        f = getattr(L, name)
        assert f(100, 10, 0) == -1 and f(100, 10, 17) == -1 and f(100, 0, 4) == -1 and f(-1, 10, 4) == -1
        assert f(100, 10, 16) - f(100, 10, 15) == 2 * per_leaf * 100                                       # two buffers of step planes
        assert f(0, 10, 1) > 0 and f(1, 10, 16) > 0
