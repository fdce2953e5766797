"""The context kernels of scp_amd/csrc/geom.hip (ctx_ehem_kernel, ctx_ehem_all_kernel, ctx_octattn_kernel, krecords_kernel) against the
CPU oracle on the hard trees of tests/ctx_cases.py (tests/test_ctx_cases.py vouches on the CPU that every case has its edge).  The
device gets the same integers as the oracle; everything is compared for equality - level bytes, positions as uint32 bit patterns
(a NaN of the reference's own arithmetic must be a NaN on the device, with any payload), (min, max) rows, symbols."""
import numpy as np
import pytest

import ctx_cases as CC
from conftest import parity_record

pytestmark = pytest.mark.gpu

ALL = [c.name for c in CC.cases()]
EMPTY_MM_ROW = (2 ** 31 - 1, -2 ** 31)      # the (min, max) row of a level without coded rows: the build's initial words


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scp_amd import native
    native.lib()
    return torch.device("cuda:0")


def pos_mode(c):
    from scp_amd import native
    return {CC.MINMAX: native.POS_MINMAX, CC.MUL: native.POS_MINMAX_MUL, CC.POW2: native.POS_POW2}[c.mode]


def build_case(dev, c):
    import torch
    from scp_amd import native
    q = torch.from_numpy(np.concatenate([s.pts for s in c.segs]).astype(np.int32)).to(dev)
    segs, a = [], 0
    for s in c.segs:
        segs.append((a, len(s.pts), s.path, s.drop))
        a += len(s.pts)
    g = native.Geom()
    g.build(q, segs)
    return g


def bits(a):
    """float32 -> uint32 bit patterns, every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_rows_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want).reshape(len(got), -1).any(1) if len(got) else np.zeros(0, bool)
    idx = np.flatnonzero(bad)
    assert len(idx) == 0, (what, f"{len(idx)} of {len(got)} rows differ", idx[:8].tolist(), got[idx[:4]].tolist(), want[idx[:4]].tolist())


def want_ehem(o):
    """(ctx [R,12] u8, position bits [R,3], symbols [R]) of one oracle segment, chunk after chunk."""
    ctx = np.concatenate(o.data).reshape(-1, 12)
    assert ctx.min() >= 0 and ctx.max() <= 255
    return ctx.astype(np.uint8), bits(np.concatenate([p.T for p in o.pos])), o.sym


def want_mm(o):
    """(min, max) per tree level: the oracle's pair on every level with coded rows (same-level Cartesian chunks carry none: the extremes of
    the oracle's node origins there), the pinned initial words on a last level the drop emptied."""
    rows, k = [], 0
    for l, n in enumerate(o.sizes):
        if n == 0:
            rows.append(EMPTY_MM_ROW)
            continue
        p = o.tree.pos[o.tree.level_off[l]:o.tree.level_off[l] + n]
        if o.pos_mm:
            assert o.pos_mm[k] == (p.min(), p.max())
        rows.append((int(p.min()), int(p.max())))
        k += 1
    return np.array(rows, np.int64).reshape(-1, 2)


def check_ehem_tables(name, g, c, os_, context_sizes):
    """Geom.context_ehem per segment and Geom.context_ehem_all against the oracle; sym_coded of context_ehem_all == sym[order] with the
    order of orc.ehem_coding_plan(..., mullevel=True) - the decodable one, which the kernel writes in BOTH modes (encode.py:122 leaves
    coded_cnt out for a single-node level of a same-level frame and so names a row twice; tests/test_ctx_cases.py pins the difference)."""
    from oracle import scp_oracle as orc
    pm = pos_mode(c)
    want = [want_ehem(o) for o in os_]
    mms = [want_mm(o) for o in os_]
    for s, o in enumerate(os_):
        assert g.info[s].depth == o.depth and g.level_counts(s) == o.level_nodes and g.rows(s) == len(o.records)
        ctx, pos, sym, mm = [t.cpu().numpy() for t in g.context_ehem(s, pm, c.lidar_level)]
        assert_rows_equal(ctx, want[s][0], f"{name}: ctx, segment {s}")
        assert_rows_equal(bits(pos), want[s][1], f"{name}: position bits, segment {s}")
        assert_rows_equal(sym, want[s][2], f"{name}: symbols, segment {s}")
        assert_rows_equal(mm, mms[s], f"{name}: pos_mm, segment {s}")
    w_ctx, w_pos, w_sym = (np.concatenate([w[k] for w in want]) for k in range(3))
    w_mm = np.concatenate(mms)
    sizes = [n for o in os_ for n in o.sizes if n]
    for cs in context_sizes:
        ctx, pos, sym_coded, mm = [t.cpu().numpy() for t in g.context_ehem_all(pm, c.lidar_level, cs)]
        assert_rows_equal(ctx, w_ctx, f"{name}: ctx, all segments, cs {cs}")
        assert_rows_equal(bits(pos), w_pos, f"{name}: position bits, all segments, cs {cs}")
        assert_rows_equal(mm, w_mm, f"{name}: pos_mm, all segments, cs {cs}")
        _, order = orc.ehem_coding_plan(sizes, cs, mullevel=True)
        assert_rows_equal(sym_coded, w_sym[order], f"{name}: sym_coded, cs {cs}")
    return len(w_ctx)


def check_octattn(name, g, c, os_):
    from oracle import scp_oracle as orc
    got = [[t.cpu().numpy() for t in g.context_octattn(s)] for s in range(len(os_))]
    for s, o in enumerate(os_):
        _, pos, data, seq = orc.octattn_context(o.records, 1)
        ctx, p, sym = got[s]
        assert_rows_equal(ctx.reshape(-1, 4, 3).astype(np.int64), data, f"{name}: octattn ctx, segment {s}")
        assert_rows_equal(bits(p), bits(pos), f"{name}: octattn position bits, segment {s}")
        assert_rows_equal(sym.astype(np.int64), seq[:, -1, 0], f"{name}: octattn symbols, segment {s}")
    if c.mode == CC.MUL:
        for level_wise in (False, True):
            ids, pos, data, seq = orc.octattn_mullevel_context([o.records for o in os_], 1, level_wise)
            assert len(ids) == (sum(len([n for n in o.sizes if n]) for o in os_) if level_wise else len(os_))
            assert_rows_equal(np.concatenate([x[0] for x in got]).reshape(-1, 4, 3).astype(np.int64), np.concatenate(data),
                              f"{name}: octattn multi-level ctx, level_wise {level_wise}")
            assert_rows_equal(bits(np.concatenate([x[1] for x in got])), bits(np.concatenate(pos)),
                              f"{name}: octattn multi-level position bits, level_wise {level_wise}")
            assert_rows_equal(np.concatenate([x[2] for x in got]).astype(np.int64), seq[:, -1, 0], f"{name}: octattn multi-level symbols")


def check_krecords(name, g, os_):
    for s, o in enumerate(os_):
        assert_rows_equal(g.krecords(s).cpu().numpy(), o.records, f"{name}: K-records, segment {s}")


@pytest.mark.parametrize("name", ALL)
def test_ehem_context_vs_oracle(dev, name):
    """ctx bytes, position bit patterns, (min, max) rows and symbols of context_ehem (every segment) and context_ehem_all, and the coded
    symbols of context_ehem_all in coding order at context sizes 2, 3, 5, 256 and 8192 (the small ones cut every level into many windows
    of odd and even length with a ragged tail)."""
    c = CC.by_name(name)
    os_ = CC.oracle_case(name)
    rows = check_ehem_tables(name, build_case(dev, c), c, os_, CC.CONTEXT_SIZES)
    parity_record(f"context-ehem/{name}", rows=rows, rows_differing_from_oracle=0)


@pytest.mark.parametrize("name", ALL)
def test_octattn_context_vs_oracle(dev, name):
    """ctx, all four position rows bit for bit and the symbols of context_octattn: per segment against octattn_context, the multi-level
    cases also against octattn_mullevel_context, level-wise and not (positions over 2^(deepest level of the shell's records))."""
    c = CC.by_name(name)
    check_octattn(name, build_case(dev, c), c, CC.oracle_case(name))


@pytest.mark.parametrize("name", ALL)
def test_krecords_vs_oracle(dev, name):
    c = CC.by_name(name)
    check_krecords(name, build_case(dev, c), CC.oracle_case(name))


def test_large_segment_takes_the_grid_stride_loop_round_again(dev):
    """One same-level segment of 1.2 M rows (more than 2048 workgroups x 256 threads): every table of the four kernels."""
    c = CC.large_case()
    os_ = CC.oracle_case(c.name)
    g = build_case(dev, c)
    assert g.rows(0) > CC.GRID_ROWS
    rows = check_ehem_tables(c.name, g, c, os_, (8192, 256))
    check_octattn(c.name, g, c, os_)
    check_krecords(c.name, g, os_)
    parity_record(f"context-ehem/{c.name}", rows=rows, rows_differing_from_oracle=0)


def test_deep_builds_hold_fewer_trees(dev):
    """Trees of 20 / 21 levels take 60 / 63 Morton bits of the 64-bit sort key: one build holds at most 15 / 1 of them and refuses more
    (19 levels and fewer: SCP_MAX_SEGMENTS), and 22 levels are refused outright."""
    import torch
    from oracle import scp_oracle as orc
    from scp_amd import native
    for d, most in ((21, 1), (20, 15)):
        pts = np.array([[(1 << d) - 1, 3, 4], [9, 1 << (d - 1), 2]], np.int32)
        q = torch.from_numpy(np.tile(pts, (most + 1, 1))).to(dev)
        g = native.Geom()
        g.build(q, [(2 * k, 2, None, False) for k in range(most)])
        want = CC.oracle_segment(orc, CC.Seg(pts.astype(np.int64), None, False), CC.MINMAX, 12).records
        for k in (0, most - 1):
            assert_rows_equal(g.krecords(k).cpu().numpy(), want, f"depth {d}, tree {k}")
        with pytest.raises(native.ScpError):
            native.Geom().build(q, [(2 * k, 2, None, False) for k in range(most + 1)])
    with pytest.raises(native.ScpError):
        native.Geom().build(torch.tensor([[1 << 21, 0, 0]], dtype=torch.int32, device=dev), [(0, 1, None, False)])


@pytest.fixture(scope="module")
def ehem_model(dev):
    from cfgs import ehem_cfg
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    return fill_weights(EHEM(ehem_cfg()), 0).to(dev)


@pytest.mark.parametrize("name", CC.names("three"))
def test_preprocess_records_equals_the_octree_path(dev, ehem_model, name):
    """FrameEncoder.preprocess_records on the oracle's record files (the --preproc_path flow) == the tables of the octree path on the same
    integers, on frames with one-leaf shells (clip cases included): ctx, position bits, symbols; its level sizes are the octree path's
    without the levels the drop emptied."""
    import torch
    from oracle import scp_oracle as orc
    from scp_amd.encoder import FrameEncoder
    c = CC.by_name(name)
    os_ = CC.oracle_case(name)
    enc = FrameEncoder(ehem_model, "kitti", c.lidar_level, spher=True, mullevel=True, device=dev)
    assert [p for p, _ in enc.shells()] == [s.path for s in c.segs]
    qs = [torch.from_numpy(s.pts.astype(np.int32)).to(dev) for s in c.segs]
    tree = enc.preprocess_ints(qs, 0.0, 0.0, len(c.segs[0].pts))
    rec = enc.preprocess_records([o.records for o in os_], 0.0, 0.0, len(c.segs[0].pts))
    assert tree["level_sizes"] == [n for o in os_ for n in o.sizes]
    assert rec["level_sizes"] == [n for n in tree["level_sizes"] if n]
    assert_rows_equal(rec["ctx"].cpu().numpy(), tree["ctx"].cpu().numpy(), f"{name}: ctx")
    assert_rows_equal(bits(rec["pos"].cpu().numpy()), bits(tree["pos"].cpu().numpy()), f"{name}: position bits")
    _, order = orc.ehem_coding_plan(rec["level_sizes"], enc.context_size, mullevel=True)
    assert_rows_equal(rec["sym"].cpu().numpy()[order], tree["sym_coded"].cpu().numpy(), f"{name}: symbols")
    # ... and both are the oracle's
    assert_rows_equal(rec["ctx"].cpu().numpy(), np.concatenate([want_ehem(o)[0] for o in os_]), f"{name}: ctx against the oracle")
    assert_rows_equal(bits(rec["pos"].cpu().numpy()), np.concatenate([want_ehem(o)[1] for o in os_]), f"{name}: position bits against the oracle")
