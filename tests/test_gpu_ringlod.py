"""Ring LOD on the GPU ("Ring LOD"): the two kernels of csrc/ringlod.hip against tests/ringlod_ref.py and the oracle's table
rule, a uniform table against the plain encode of the same frame, a general table against the reference snap of the plain integers
through encode -> files -> decode, the paths that must not change, every refusal, and the command lines.

Frames are the depth tests' own: synth_frame(4)[::30] at L12 --spher and L14 multi-level, random weights.  A multi-level stream does
not code the last BFS node of a shell (the reference's record files drop it), so a decoder never regenerates the leaves below it: where a
test compares decoded leaves of such a stream with a full set, the children of the shell's last level-D node are taken out, and the test says so."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ringlod_ref as ref
from conftest import ROOT
from test_gpu_ringrate import SHELLS, dev, ehem_model

pytestmark = pytest.mark.gpu

FRAMES = {"L12-spher": (12, False), "L14-multi-level": (14, True)}
GENERAL = ((0.0, 10.0, 25.0), (2, 0, 1))
UNIFORM_K = 2


def frame(i=4):
    from scp_amd.synth import synth_frame
    return synth_frame(i)[::30].copy()


def encoder(tag, **kw):
    from scp_amd.encoder import FrameEncoder
    level, mullevel = FRAMES[tag]
    return FrameEncoder(ehem_model(), "kitti", level, spher=True, mullevel=mullevel, device=dev(), **kw)


def write_stream(enc, res, stem):
    from scp_amd.decoder import write_sidecar
    out = enc.outfile(stem, res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), out + ".dat")
    write_sidecar(out, enc, res, "EHEM")
    return out


def cells(origins, thr, drops, **kw):
    from scp_amd import native
    return native.ringlod_cells(torch.from_numpy(np.ascontiguousarray(origins, np.int32)).to(dev()), thr, drops, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. scp_ringlod_cells
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_cells_equal_the_reference_on_random_rows_for_every_kmax(n):
    rng = np.random.default_rng(n)
    q = rng.integers(0, 4096, (n, 3)).astype(np.int32)
    for kmax in range(1, 9):
        drops = [int(v) for v in rng.integers(0, kmax + 1, 4)]
        drops[int(rng.integers(0, 4))] = kmax
        thr = sorted(int(v) for v in rng.integers(0, 4096, 3))
        for start in (0, 1, kmax, kmax + 1):
            got = cells(q, thr, drops, start=start).cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, ref.J(q[:, 0], start, thr, drops)), (kmax, start)
            assert start <= kmax or not got.any()                           # a start size above kmax gives 0
        j, snapped = cells(q, thr, drops, snapped=True)
        want, wj = ref.snap(q, thr, drops)
        assert np.array_equal(snapped.cpu().numpy(), want) and np.array_equal(j.cpu().numpy(), wj)
    # non-monotone drops, one ring, and the snap in place
    from scp_amd import native
    for thr, drops in (([100, 900, 2000], [0, 3, 1, 2]), ([], [5]), ([4095], [0, 8])):
        qd = torch.from_numpy(q).to(dev())
        want, wj = ref.snap(q, thr, drops)
        j2, out = native.ringlod_cells(qd, thr, drops, snapped=qd)
        assert out is qd and np.array_equal(qd.cpu().numpy(), want) and np.array_equal(j2.cpu().numpy(), wj)


def test_cells_on_hand_made_rows_at_the_thresholds():
    thr, drops = [100, 900, 2000], [0, 3, 1, 2]
    rows = []
    for t in thr:
        rows += [t, t - 1]
        for j in (1, 2, 3):
            # cells of size 2^j whose doubled centre is exactly 2 t and 2 t - 1: origin = t - (2^j - 1) / 2 is no integer for c2 = 2 t
            # (c2 is odd), so c2 = 2 t + 1 and 2 t - 1 are the nearest a cell gets
            for c2 in (2 * t + 1, 2 * t - 1):
                o = (c2 - 2 ** j + 1) // 2
                rows += [o, o + 2 ** j - 1]
    x = np.array(rows, np.int64)
    q = np.stack((x, np.arange(len(x)) * 7 % 4096, np.arange(len(x)) * 13 % 4096), 1)
    for start in (0, 1, 2, 3):
        assert np.array_equal(cells(q, thr, drops, start=start).cpu().numpy(), ref.J(x, start, thr, drops)), start
    # an even threshold sum: c2 == 2 t exactly cannot happen (c2 is odd), so the comparison c2 >= 2 t is strict in effect: pinned by hand
    assert cells(np.array([[100, 0, 0], [99, 0, 0], [96, 0, 0], [104, 0, 0]]), thr, drops).cpu().tolist() == [2, 0, 0, 3]


def test_cells_with_per_node_start_sizes_over_two_segments_of_different_depth_and_table():
    rng = np.random.default_rng(5)
    n0, n1 = 300, 500
    q = rng.integers(0, 4096, (n0 + n1 + 17, 3)).astype(np.int32)
    tabs = [([50, 1000], [3, 0, 2]), ([700, 701], [1, 4, 4])]
    depth = [12, 9]
    level = np.concatenate((rng.integers(1, 14, n0), rng.integers(1, 11, n1), rng.integers(1, 5, 17))).astype(np.uint8)
    size = np.concatenate((depth[0] - level[:n0].astype(np.int64) + 1, depth[1] - level[n0:n0 + n1].astype(np.int64) + 1))
    # node origins are multiples of their size
    q[:n0 + n1] = (q[:n0 + n1].astype(np.int64) >> size[:, None] << size[:, None]).astype(np.int32)
    segs = [(0, n0, depth[0], 1), (n0, n1, depth[1], 0)]                       # (the tables crossed over on purpose)
    got = cells(q, [t for t, _ in tabs], [d for _, d in tabs], level=torch.from_numpy(level).to(dev()), segs=segs).cpu().numpy()
    want = np.concatenate((ref.J(q[:n0, 0], size[:n0], *tabs[1]), ref.J(q[n0:n0 + n1, 0], size[n0:], *tabs[0]), np.zeros(17, np.int64)))
    assert np.array_equal(got, want) and got[:n0 + n1].any()                    # rows in no segment: 0
    # the same segments with one start size for the call
    got = cells(q, [t for t, _ in tabs], [d for _, d in tabs], start=1, segs=segs).cpu().numpy()
    assert np.array_equal(got[:n0], ref.J(q[:n0, 0], 1, *tabs[1])) and np.array_equal(got[n0:n0 + n1], ref.J(q[n0:n0 + n1, 0], 1, *tabs[0]))


def test_malformed_cell_calls_are_refused_and_write_nothing():
    from scp_amd import native
    L = native.lib()
    n = 64
    q = torch.arange(3 * n, dtype=torch.int32, device=dev()).reshape(n, 3).contiguous()
    j = torch.full((n,), 77, dtype=torch.uint8, device=dev())
    out = torch.full((n, 3), -5, dtype=torch.int32, device=dev())
    ws = torch.zeros(8192, dtype=torch.int64, device=dev())
    thr, drops = np.array([10, 20], np.int64), np.array([1, 2, 3], np.uint8)
    seg = np.zeros(1, native.RINGLOD_SEG)
    seg[0] = (0, n, 12, 0)

    def call(origins=q.data_ptr(), rows=n, start=0, level=None, segs=None, nseg=0, t=thr, d=drops, ntab=1, nring=3, jp=j.data_ptr(),
             sp=out.data_ptr(), w=ws.data_ptr(), wb=8 * 8192):
        return L.scp_ringlod_cells(origins, rows, start, level, segs, nseg, None if t is None else t.ctypes.data, None if d is None else d.ctypes.data,
                                   ntab, nring, jp, sp, w, wb, native._stream())

    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(j.cpu().numpy(), ref.J(q[:, 0].cpu().numpy(), 0, [10, 20], [1, 2, 3]))
    j.fill_(77); out.fill_(-5)
    big_thr, big_drops = np.arange(32, dtype=np.int64), np.ones(33, np.uint8)
    lv = torch.ones(n, dtype=torch.uint8, device=dev())
    bad_seg = np.zeros(2, native.RINGLOD_SEG)
    bad_seg[0], bad_seg[1] = (0, 40, 12, 0), (30, 20, 12, 0)
    seg_tab1, seg_beyond = np.array([(0, n, 12, 1)], native.RINGLOD_SEG), np.array([(1, n, 12, 0)], native.RINGLOD_SEG)
    for what, rc in (("null origins", call(origins=None)), ("null j", call(jp=None)), ("null drops", call(d=None)), ("null thresholds", call(t=None)),
                     ("null workspace", call(w=None)), ("n < 0", call(rows=-1)), ("33 rings", call(t=big_thr, d=big_drops, nring=33)),
                     ("0 rings", call(nring=0)), ("descending", call(t=np.array([20, 10], np.int64))), ("negative", call(t=np.array([-1, 10], np.int64))),
                     ("beyond 2^31 - 1", call(t=np.array([1, 2 ** 31], np.int64))), ("kmax 9", call(d=np.array([1, 9, 0], np.uint8))),
                     ("short workspace", call(wb=64)), ("level without segments", call(level=lv.data_ptr())),
                     ("segment table index", call(segs=seg_tab1.ctypes.data, nseg=1)),
                     ("segment beyond n", call(segs=seg_beyond.ctypes.data, nseg=1)),
                     ("overlapping segments", call(segs=bad_seg.ctypes.data, nseg=2)), ("null segments", call(nseg=1)),
                     ("65 tables", call(ntab=65)), ("negative start", call(start=-1))):
        assert rc == -1, what
    torch.cuda.synchronize()
    assert (j == 77).all() and (out == -5).all()
    assert call(segs=seg.ctypes.data, nseg=1, level=lv.data_ptr()) == 0
    for bad, why in ((dict(thresholds=[20, 10], drops=[1, 2, 3]), "SCP_EINVAL"), (dict(thresholds=[10, 20], drops=[1, 2, 9]), "SCP_EINVAL"),
                     (dict(thresholds=[10, 20], drops=[1, 2]), "one more drop"), (dict(thresholds=list(range(32)), drops=[1] * 33), "SCP_EINVAL"),
                     (dict(thresholds=[10, 20], drops=[1, 2, 300]), "0 .. 8")):
        with pytest.raises(native.ScpError, match=why):
            native.ringlod_cells(q, bad["thresholds"], bad["drops"])


# ------------------------------------------------------------------------------------------------------------------ 2. scp_force_rows
MASKS = {"none": lambda n: np.zeros(n, np.uint8), "all": lambda n: np.ones(n, np.uint8), "every third": lambda n: (np.arange(n) % 3 == 0).astype(np.uint8),
         "last row only": lambda n: (np.arange(n) == n - 1).astype(np.uint8)}


@pytest.mark.parametrize("ld", [255, 256])
@pytest.mark.parametrize("mask_name", list(MASKS))
def test_forced_rows_are_one_hot_under_the_coder_and_nothing_else_is_touched(ld, mask_name, orc):
    from scp_amd import native
    n, nsym = 1027, 255
    rng = np.random.default_rng(ld)
    host = rng.normal(0, 4, (n, ld)).astype(np.float32)
    mask = MASKS[mask_name](n)
    sym = rng.integers(0, 255, n).astype(np.uint8)
    planted = np.zeros(n, bool)
    planted[rng.choice(n, 40, replace=False)] = True
    sym[planted] = np.maximum(sym[planted], 1)
    sym[~planted & (mask != 0)] = 0                                             # masked rows carry 0, except the planted ones
    full = torch.from_numpy(host.copy()).to(dev())
    table = full[:, :nsym]
    counter = torch.zeros(1, dtype=torch.int64, device=dev())
    m_d, s_d = torch.from_numpy(mask).to(dev()), torch.from_numpy(sym).to(dev())
    assert native.force_rows(table, m_d, s_d, counter) is table
    got = full.cpu().numpy()
    forced = np.full(nsym, -1000.0, np.float32)
    forced[0] = 0.0
    on = mask != 0
    assert np.array_equal(got[~on].view(np.uint32), host[~on].view(np.uint32))                 # unmasked rows keep their bits
    if ld == 256:
        assert np.array_equal(got[:, 255].view(np.uint32), host[:, 255].view(np.uint32))        # ... and so does the 256th column
    assert (got[on][:, :nsym] == forced).all() and not np.signbit(got[on][:, 0]).any()
    assert int(counter.item()) == int((planted & on).sum())                                     # exactly the planted rows
    # the counter adds up over calls; without symbols nothing is counted
    native.force_rows(table, m_d, s_d, counter)
    assert int(counter.item()) == 2 * int((planted & on).sum())
    native.force_rows(table, m_d)
    assert np.array_equal(full.cpu().numpy().view(np.uint32), got.view(np.uint32))              # idempotent
    # under the coder: (c_low, c_high) = (0, 65282) for symbol 0, and the CDF row of a one-hot PMF, plain and after scaling
    onehot = np.zeros((1, nsym), np.float32)
    onehot[0, 0] = 1.0
    want_row = np.asarray(orc.pmf_to_cdf(onehot)).view(np.uint16).reshape(-1)
    assert int(want_row[0]) == 0 and int(want_row[1]) == 65282
    zero = torch.zeros(n, dtype=torch.uint8, device=dev())
    for beta in (None, 0.354, 2.83):
        t = full.clone()[:, :nsym]
        if beta is not None:
            native.scale_rows(t, [0, n], [beta])
        r = native.softmax_cdf(t, zero, want_cdf=True)
        lohi = r["lohi"].cpu().numpy().view(np.uint32).astype(np.int64)[on]
        assert (lohi & 0xFFFF == 0).all() and (lohi >> 16 == 65282).all(), beta
        cdf = r["cdf"].cpu().numpy().view(np.uint16)[on]
        assert cdf.shape[0] == on.sum() and (cdf[:, :want_row.shape[0]] == want_row).all(), beta


def test_malformed_force_calls_are_refused_and_write_nothing():
    from scp_amd import native
    L = native.lib()
    n = 16
    t = torch.ones((n, 256), dtype=torch.float32, device=dev())
    mask = torch.ones(n, dtype=torch.uint8, device=dev())
    sym = torch.ones(n, dtype=torch.uint8, device=dev())
    cnt = torch.zeros(1, dtype=torch.int64, device=dev())
    st = native._stream()
    for what, rc in (("null table", L.scp_force_rows(None, 256, n, 255, mask.data_ptr(), None, None, st)),
                     ("null mask", L.scp_force_rows(t.data_ptr(), 256, n, 255, None, None, None, st)),
                     ("n < 0", L.scp_force_rows(t.data_ptr(), 256, -1, 255, mask.data_ptr(), None, None, st)),
                     ("stride below nsym", L.scp_force_rows(t.data_ptr(), 200, n, 255, mask.data_ptr(), None, None, st)),
                     ("nsym 1", L.scp_force_rows(t.data_ptr(), 256, n, 1, mask.data_ptr(), None, None, st)),
                     ("nsym 257", L.scp_force_rows(t.data_ptr(), 300, n, 257, mask.data_ptr(), None, None, st)),
                     ("symbols without a counter", L.scp_force_rows(t.data_ptr(), 256, n, 255, mask.data_ptr(), sym.data_ptr(), None, st)),
                     ("a counter without symbols", L.scp_force_rows(t.data_ptr(), 256, n, 255, mask.data_ptr(), None, cnt.data_ptr(), st))):
        assert rc == -1, what
    torch.cuda.synchronize()
    assert (t == 1).all() and int(cnt.item()) == 0
    assert L.scp_force_rows(None, 256, 0, 255, None, None, None, st) == 0       # no rows: nothing to do
    with pytest.raises(native.ScpError, match="go together"):
        native.force_rows(t[:, :255], mask, sym)
    with pytest.raises(native.ScpError, match="one mask byte per row"):
        native.force_rows(t[:, :255], mask[:3])


# ------------------------------------------------------------------------------------------------------------------ shared encodes
@functools.lru_cache(maxsize=None)
def plain(tag):
    """The frame encoded once WITHOUT the option, rate report on: (encoder, frame, result, per shell the plain quantised integers as host
    int64, the quantiser infos, LOD-2 cells per shell, all leaves per shell).  Shared, read-only; the encoder is not used again."""
    enc = encoder(tag, rate=True)
    xyz = frame()
    res = enc.encode(xyz)
    lod = [c.cpu().numpy().astype(np.int64) for c in enc.lod_cells(UNIFORM_K)]
    leaves = [enc.geom.leaves(s).cpu().numpy().astype(np.int64) for s in range(len(enc.geom.info))]
    depths = [int(i.depth) for i in enc.geom.info]
    qs, _, _ = enc.quantize(torch.from_numpy(xyz).to(dev()))
    q = [t.cpu().numpy().astype(np.int64) for t in qs]
    if FRAMES[tag][1]:
        # a multi-level cloud is the whole frame at the shell's step; the shell's tree holds the points whose top bits on the radial
        # axis are the shell's path (Octree.py:188)
        for s, path in enumerate(SHELLS):
            bits = int("".join(str(b) for b in path), 2)
            q[s] = q[s][(q[s][:, 0] >> (depths[s] - len(path))) == bits]
    infos = [(float(i.qs[0]), float(i.offset[0])) for i in enc._infos]
    for s in range(len(q)):                                                     # the device quantiser's integers are the build's
        assert np.array_equal(ref.unique_rows(q[s]), ref.unique_rows(leaves[s]))
    return dict(enc=enc, xyz=xyz, res=res, q=q, infos=infos, lod=lod, leaves=leaves, depths=depths)


@functools.lru_cache(maxsize=None)
def coded(tag, table, temper=None):
    """The frame encoded WITH a table, written to files and decoded once -> everything the tests compare.  Shared, read-only."""
    import tempfile
    from scp_amd.decoder import _ehem_job, decode_file
    enc = encoder(tag, rate=True, ring_lod=table, temper=temper)
    res = enc.encode(frame())
    recon = [p.cpu().numpy() for p in enc._reconstructed()]
    enc_leaves = [enc.geom.leaves(s).cpu().numpy().astype(np.int64) for s in range(len(enc.geom.info))]
    enc_centres = [enc.ring_centres(enc.geom.leaves(s), s)[0].cpu().numpy() for s in range(len(enc.geom.info))]
    d = tempfile.mkdtemp(prefix="ringlod_")
    out = write_stream(enc, res, os.path.join(d, "f"))
    got = decode_file(out, ehem_model(), mullevel=FRAMES[tag][1], device=dev())
    return dict(enc=enc, res=res, out=out, got=got, job=_ehem_job(out, mullevel=FRAMES[tag][1]), recon=recon, enc_leaves=enc_leaves,
                enc_centres=enc_centres)


def coded_part(rows, mullevel):
    """The rows (Morton order, as the geometry holds cells or leaves) a decoder regenerates: all of them, or - multi-level - all but the
    children of the shell's last level-D node, which is never coded."""
    if not mullevel:
        return rows
    return rows[~((rows >> 1) == (rows[-1] >> 1)).all(1)]


def level_slices(res):
    off = np.concatenate(([0], np.cumsum(res["level_sizes"])))
    return [slice(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


# ------------------------------------------------------------------------------------------------------------------ 3. uniform table
@pytest.mark.parametrize("tag", list(FRAMES))
def test_a_uniform_table_codes_the_plain_trees_upper_levels_and_nothing_below(tag):
    from scp_amd import metrics
    from scp_amd.decoder import dequantise_leaves
    K, mullevel = UNIFORM_K, FRAMES[tag][1]
    p, c = plain(tag), coded(tag, ((0.0,), (K,)))
    res, pres, depths = c["res"], p["res"], p["depths"]
    assert res["n_levels"] == pres["n_levels"] == sum(depths) and res["ring_lod"]["thresholds"] == [[]] * len(depths)
    sl, psl = level_slices(res), level_slices(pres)
    sym, psym, implied = res["_debug"]["sym_coded"].cpu().numpy(), pres["_debug"]["sym_coded"].cpu().numpy(), res["_debug"]["implied"].cpu().numpy()
    off, n_implied = 0, 0
    for d in depths:
        for L in range(1, d + 1):
            i = off + L - 1
            lv, plv = res["rate"]["levels"][i], pres["rate"]["levels"][i]
            if L <= d - K:
                assert res["level_sizes"][i] == pres["level_sizes"][i] and np.array_equal(sym[sl[i]], psym[psl[i]]), (tag, L)
                assert lv["ideal_bits"] == plv["ideal_bits"] and lv["nodes"] == plv["nodes"], (tag, L)        # bit-identical
                assert not implied[sl[i]].any()
            else:
                rows = res["level_sizes"][i]
                assert rows > 0 and implied[sl[i]].all() and not sym[sl[i]].any(), (tag, L)
                assert lv["nodes"] == rows and lv["ideal_bits"] == 0.0, (tag, L, lv["ideal_bits"])
                want = rows * ref.ROW_TABLE_BITS
                print(tag, "level", L, "rows", rows, "table bits", lv["table_bits"], "want", want)
                assert abs(lv["table_bits"] - want) <= 1e-9 * want
                n_implied += rows
        off += d
    assert res["ring_lod"]["implied_rows"] == n_implied == int(implied.sum())
    assert res["ring_lod"]["snapped"] == [0] * K + [sum(len(q) for q in p["q"])]
    assert res["bits"] < pres["bits"]
    print(tag, "bits plain", pres["bits"], "uniform drop", K, res["bits"])
    # the decoder: the plain encoder's LOD-K cells, each of size 2^K, and their centres
    got, job = c["got"], c["job"]
    assert len(got["leaves"]) == len(depths) and got["ring_lod"]["drops"] == (K,)
    for s in range(len(depths)):
        want = coded_part(p["lod"][s], mullevel)
        assert got["leaves"][s].dtype == torch.int64 and np.array_equal(got["leaves"][s].cpu().numpy(), want), (tag, s)
        assert (got["cell_j"][s] == K).all() and got["cell_j"][s].shape[0] == want.shape[0]
        assert res["ring_lod"]["leaves"][s] == p["lod"][s].shape[0]
    want_pts = torch.cat([dequantise_leaves(metrics.lod_centres(lv, K), q, b, job["z_offset"], job["spher"], job["cylin"], job["data_type"])
                          for lv, q, b in zip(got["leaves"], job["qs"], job["bins"])])
    assert got["points"].dtype == torch.float64 and torch.equal(got["points"], want_pts)


# ------------------------------------------------------------------------------------------------------------------ 4. general table
def reference_tree(p, tag, table):
    """From the plain integers alone: per shell thresholds, snapped unique leaves, their j, the implied rows, the points per j."""
    edges, drops = table
    mullevel = FRAMES[tag][1]
    out = dict(thr=[], leaves=[], j=[], implied=0, snapped=np.zeros(max(drops) + 1, np.int64))
    for s, q in enumerate(p["q"]):
        thr = ref.thresholds(edges, *p["infos"][s])
        snapped, j = ref.snap(q, thr, drops)
        out["snapped"] += np.bincount(j, minlength=max(drops) + 1)
        leaves = ref.unique_rows(snapped)
        d = p["depths"][s]
        for L in range(1, d + 1):
            e = d - L + 1
            nodes = ref.unique_rows((leaves >> e) << e)
            out["implied"] += int(ref.implied(nodes, e, thr, drops).sum())
        out["thr"].append(thr); out["leaves"].append(leaves); out["j"].append(ref.J(leaves[:, 0], 0, thr, drops))
    return out


@pytest.mark.parametrize("temper", [None, "code"])
@pytest.mark.parametrize("tag", list(FRAMES))
def test_a_general_table_round_trips_to_the_reference_snap_of_the_plain_integers(tag, temper):
    from scp_amd.decoder import dequantise_leaves, is_ringlod, is_tempered
    mullevel = FRAMES[tag][1]
    p, c = plain(tag), coded(tag, GENERAL, temper)
    want = reference_tree(p, tag, GENERAL)
    res, got, job = c["res"], c["got"], c["job"]
    assert is_ringlod(c["out"]) and is_tempered(c["out"]) == (temper == "code")
    assert os.path.basename(c["out"]).startswith("f_ringlod_temper_spher_" if temper else "f_ringlod_spher_")
    rl = res["ring_lod"]
    assert rl["edges"] == list(GENERAL[0]) and rl["drops"] == list(GENERAL[1]) and rl["thresholds"] == want["thr"]
    assert json.load(open(c["out"] + ".scp.json"))["ring_lod"] == dict(drops=list(GENERAL[1]), thresholds=want["thr"])
    assert rl["snapped"] == want["snapped"].tolist() and all(v > 0 for v in rl["snapped"])          # every drop of the table is exercised
    assert rl["leaves"] == [len(lv) for lv in want["leaves"]]
    dropped_implied = 0
    pts = []
    for s, lv in enumerate(want["leaves"]):
        # the encoder's tree holds exactly the reference's leaves
        assert np.array_equal(ref.unique_rows(c["enc_leaves"][s]), lv), (tag, s)
        dec = got["leaves"][s].cpu().numpy()
        part = coded_part(c["enc_leaves"][s], mullevel)
        assert np.array_equal(ref.unique_rows(dec), ref.unique_rows(part)) and len(dec) == len(part), (tag, s)
        if not mullevel:
            assert np.array_equal(ref.unique_rows(dec), lv)
        else:
            last = (c["enc_leaves"][s][-1:] >> 1) << 1                                              # the node without a row
            dropped_implied += int(ref.implied(last, 1, want["thr"][s], GENERAL[1])[0])
            assert 1 <= len(lv) - len(dec) <= 8
        j = got["cell_j"][s].cpu().numpy().astype(np.int64)
        assert np.array_equal(j, ref.J(dec[:, 0], 0, want["thr"][s], GENERAL[1])), (tag, s)
        assert np.array_equal(dec, (dec >> j[:, None]) << j[:, None])                               # every leaf is its cell's origin
        centres = ref.centres(dec, j)
        pts.append(dequantise_leaves(torch.from_numpy(centres).to(dev()), job["qs"][s], job["bins"][s], job["z_offset"], job["spher"], job["cylin"],
                                     job["data_type"]))
        # the encoder's centres are the decoder's, integer for integer; its points go through its own dequantiser
        keep = np.ones(len(c["enc_leaves"][s]), bool) if not mullevel else ~((c["enc_leaves"][s] >> 1) == (c["enc_leaves"][s][-1] >> 1)).all(1)
        assert np.array_equal(c["enc_centres"][s][keep], centres), (tag, s)
        mine = got["points"].cpu().numpy()[sum(len(x) for x in pts[:-1]):sum(len(x) for x in pts)]
        diff = np.abs(c["recon"][s][keep] - mine).max(1)
        # two float paths for the same centres, so the points agree to rounding only, and the bound is worked out per point
        # of range r.  Both paths: the encoder's steps are the quantiser's float32-rounded ones, the decoder's the float64 formula - 2e-7
        # relative apart (tests/test_gpu_e2e.py pins that figure) on rho (<= r), phi (<= 2 pi) and theta (<= pi): r * 2e-7 * (1 + 3 pi).
        # Same-level only: the encoder rounds (rho, phi, theta) to float32 - another r * 2^-24 * (1 + 3 pi) - and evaluates the inverse
        # transform in float32, three products and two function values each within an ulp of a number <= r: 5 r 2^-24.
        r = np.linalg.norm(mine, axis=1)
        bound = r * 2e-7 * (1 + 3 * np.pi) + (0.0 if mullevel else r * 2.0 ** -24 * (6 + 3 * np.pi)) + 1e-12
        print(tag, temper, "shell", s, "max |encoder point - decoder point|", diff.max(), "largest share of its bound", (diff / bound).max())
        assert (diff <= bound).all()
    assert torch.equal(got["points"], torch.cat(pts))
    assert rl["implied_rows"] == want["implied"] - dropped_implied
    assert rl["implied_rows"] == int(res["_debug"]["implied"].sum()) and not res["_debug"]["sym_coded"][res["_debug"]["implied"].bool()].any()
    if temper:
        assert res["temper"]["mode"] == "code"
        print(tag, "groups moved", res["temper"]["moved"], "bits untempered", coded(tag, GENERAL)["res"]["bits"])
        for a, b in zip(got["leaves"], coded(tag, GENERAL)["got"]["leaves"]):
            assert torch.equal(a, b)
    print(tag, temper, "bits plain", p["res"]["bits"], "ring LOD", res["bits"], "implied rows", rl["implied_rows"], "snapped", rl["snapped"])


# ------------------------------------------------------------------------------------------------------------------ 5. invariance
@pytest.mark.parametrize("tag", list(FRAMES))
def test_all_drops_zero_is_the_encoder_without_the_option(tag, tmp_path):
    p = plain(tag)
    enc = encoder(tag, rate=True, ring_lod=((0.0, 10.0, 25.0), (0, 0, 0)))
    assert enc.ring_lod is None
    res = enc.encode(frame())
    assert res["bytes"] == p["res"]["bytes"] and "ring_lod" not in res
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    a, b = write_stream(enc, res, str(tmp_path / "a" / "f")), write_stream(p["enc"], p["res"], str(tmp_path / "b" / "f"))
    assert os.path.basename(a) == os.path.basename(b) and "ringlod" not in a
    for sfx in ("", ".scp.json"):
        assert open(a + sfx, "rb").read() == open(b + sfx, "rb").read()
    asy = enc.finish(enc.encode_async(frame()))
    assert asy["bytes"] == res["bytes"] and "ring_lod" not in asy


@pytest.mark.parametrize("tag", list(FRAMES))
def test_every_entry_point_writes_the_same_stream(tag):
    c = coded(tag, GENERAL)
    enc = encoder(tag, ring_lod=GENERAL)
    a, b = frame(4), frame(5)
    one = enc.encode(a)
    assert one["bytes"] == c["res"]["bytes"] and one["ring_lod"] == c["res"]["ring_lod"]
    two = enc.encode(b)
    assert two["bytes"] != one["bytes"]
    asy = enc.finish(enc.encode_async(a))
    assert asy["bytes"] == one["bytes"] and asy["ring_lod"] == one["ring_lod"]
    qs, bin_num, z_off = enc.quantize(torch.from_numpy(a).to(dev()))
    before = [q.clone() for q in qs]
    ints = enc.encode_ints(qs, bin_num, z_off, len(a))
    assert ints["bytes"] == one["bytes"] and ints["ring_lod"] == one["ring_lod"]
    assert all(torch.equal(x, y) for x, y in zip(qs, before))                   # the caller's integers are not snapped in place
    host = encoder(tag, ring_lod=GENERAL, host_transform=True)
    h = host.encode(a)
    assert host.finish(host.encode_async(a))["bytes"] == h["bytes"] and "ring_lod" in h
    batch = enc.finish_batch(enc.encode_batch_async([a, b]))
    assert [r["bytes"] for r in batch] == [one["bytes"], two["bytes"]]
    assert [r["ring_lod"] for r in batch] == [one["ring_lod"], two["ring_lod"]]
    assert enc.outfile("x", one).startswith("x_ringlod_spher_")


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_encoder_refusals_raise_with_their_reason():
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder, OctAttnFrameEncoder
    kw = dict(device=dev())
    with pytest.raises(native.ScpError, match="no radial axis"):
        FrameEncoder(ehem_model(), "kitti", 12, spher=False, cylin=False, ring_lod=GENERAL, **kw)
    with pytest.raises(native.ScpError, match="--type obj"):
        FrameEncoder(ehem_model(), "obj", 12, spher=True, ring_lod=GENERAL, **kw)
    with pytest.raises(native.ScpError, match="OctAttention: ring_lod is not available"):
        OctAttnFrameEncoder(None, "kitti", 12, spher=True, ring_lod=GENERAL, **kw)
    with pytest.raises(native.ScpError, match="one drop per ring"):
        FrameEncoder(ehem_model(), "kitti", 12, spher=True, ring_lod=((0.0, 10.0), (1,)), **kw)
    with pytest.raises(native.ScpError, match="not ascending from 0"):
        FrameEncoder(ehem_model(), "kitti", 12, spher=True, ring_lod=((0.0, 10.0, 5.0), (1, 1, 1)), **kw)
    with pytest.raises(native.ScpError, match="0 .. 8"):
        FrameEncoder(ehem_model(), "kitti", 12, spher=True, ring_lod=((0.0, 10.0), (1, 9)), **kw)
    enc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, ring_lod=GENERAL, **kw)
    with pytest.raises(native.ScpError, match="record files"):
        enc.encode_records([np.zeros((1, 4, 6), np.int64)], 4097.0, 0.0, 1)
    # a drop above the shallowest shell's depth - 1: a shallow tree (level 5) under a drop of 8, for every entry point
    shallow = FrameEncoder(ehem_model(), "kitti", 5, spher=True, ring_lod=((0.0,), (8,)), **kw)
    with pytest.raises(native.ScpError, match=r"a drop of 8 levels, but the shells of this frame are \[\d\] levels deep"):
        shallow.encode(frame())
    with pytest.raises(native.ScpError, match="a drop of 8 levels"):
        shallow.encode_async(frame())
    # integers without the quantiser's steps and offsets
    fresh = FrameEncoder(ehem_model(), "kitti", 12, spher=True, ring_lod=GENERAL, **kw)
    with pytest.raises(native.ScpError, match="quantiser infos"):
        fresh.encode_ints([torch.zeros((4, 3), dtype=torch.int32, device=dev())], 4097.0, 0.0, 4)


def test_decoder_refusals_and_the_modes_that_stay_for_plain_files(tmp_path, monkeypatch):
    import shutil
    from scp_amd import decoder, native
    from scp_amd.cli import decode_main
    c, p = coded("L12-spher", GENERAL), plain("L12-spher")
    p_out = write_stream(p["enc"], p["res"], str(tmp_path / "p"))
    # --lod / --streams: refused on the ring-LOD file, served on the plain one
    with pytest.raises(native.ScpError, match="ring-LOD stream with --lod 2"):
        decoder.decode_file(c["out"], ehem_model(), device=dev(), lod=2)
    with pytest.raises(native.ScpError, match="ring-LOD stream with --streams"):
        decoder.decode_files([p_out, c["out"]], ehem_model(), streams=2, device=dev())
    assert decoder.decode_file(p_out, ehem_model(), device=dev(), lod=2)["lod"] == 2
    both = decoder.decode_files([p_out, p_out], ehem_model(), streams=2, device=dev())
    assert torch.equal(both[0]["points"], both[1]["points"]) and np.array_equal(both[0]["leaves"][0].cpu().numpy(), p["leaves"][0])
    # a ring-LOD name without a well-formed table: refused before anything is decoded
    name = str(tmp_path / os.path.basename(c["out"]))
    for sfx in ("", ".dat", decoder.SIDECAR):
        shutil.copy(c["out"] + sfx, name + sfx)
    side = json.load(open(name + decoder.SIDECAR))

    def boom(*a, **k):
        raise AssertionError("a decoder was started")
    monkeypatch.setattr(decoder.FrameDecoder, "decode", boom)
    monkeypatch.setattr(decoder.EhemBatchDecoder, "decode", boom)
    entry = side["ring_lod"]
    for bad, why in ((dict(entry, drops=entry["drops"][:-1]), "one more drop than thresholds"), (dict(entry, drops=[2, 0, 12]), "out of range"),
                     (dict(entry, thresholds=[entry["thresholds"][0][::-1]]), "descending"), (dict(entry, thresholds=entry["thresholds"] * 3), "shells"),
                     (dict(entry, drops=[2, 0, 1.0]), "not a list of integers"), (None, "no `ring_lod` entry")):
        s = dict(side)
        if bad is None:
            s.pop("ring_lod")
        else:
            s["ring_lod"] = bad
        json.dump(s, open(name + decoder.SIDECAR, "w"))
        with pytest.raises(native.ScpError, match=why):
            decoder.decode_file(name, ehem_model(), device=dev())
        with pytest.raises(native.ScpError, match=why):
            decoder.decode_files([name], ehem_model(), streams=1, device=dev())
    os.remove(name + decoder.SIDECAR)
    with pytest.raises(native.ScpError, match="without its side-info file"):
        decoder.decode_file(name, ehem_model(), device=dev())


# ------------------------------------------------------------------------------------------------------------------ 7. command lines
LINE = "ring LOD snapped per drop, implied rows, leaves :"


def two_frames(tmp_path):
    from scp_amd.synth import synth_frame, write_kitti_bin
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    return seq


@pytest.mark.parametrize("script,decoder_script,mullevel", [("encode.py", "decode_ehem.py", False), ("encode_mullevel.py", "decode_ehem_mullevel.py", True)])
def test_cli_ring_lod_writes_streams_the_decoder_turns_into_the_apis_clouds(script, decoder_script, mullevel, tmp_path):
    from scp_amd import native
    from scp_amd.cli import decode_main
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.decoder import SIDECAR, decode_file
    from scp_amd.encoder import FrameEncoder
    seq = two_frames(tmp_path)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, script), "--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", "12", "--spher",
           "--random_weights", "0", "--out_dir", str(out), "--ring_lod", "0,10,25:2,0,1"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count(LINE) == 2
    bins = sorted(f.name for f in out.iterdir() if f.name.endswith(".bin"))
    assert len(bins) == 2 and all("_ringlod_spher_" in b for b in bins)
    enc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, mullevel=mullevel, device=dev(), ring_lod=GENERAL)
    api = []
    for i, b in enumerate(bins):
        res = enc.encode(pointCloud.ptread(str(seq / f"{i:06d}.bin")))
        assert res["bytes"] == (out / b).read_bytes() and os.path.basename(enc.outfile(str(out / b).split("_ringlod_")[0], res)) == b
        assert json.load(open(out / (b + SIDECAR)))["ring_lod"] == dict(drops=res["ring_lod"]["drops"], thresholds=res["ring_lod"]["thresholds"])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(LINE)][i]
        assert line.split(":")[1].strip() == f"{res['ring_lod']['snapped']} {res['ring_lod']['implied_rows']} {sum(res['ring_lod']['leaves'])}"
        api.append(decode_file(str(out / b), ehem_model(), mullevel=mullevel, device=dev()))
    dec = ["--test_files", str(seq), "--random_weights", "0", "--out_dir", str(out)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, decoder_script)] + dec, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    plys = sorted(f for f in out.iterdir() if f.name.endswith(".ply"))
    assert len(plys) == 2
    for ply, want in zip(plys, api):
        ref_ply = str(tmp_path / ("want_" + ply.name))
        pointCloud.write_ply_data(ref_ply, want["points"].cpu().numpy())
        assert ply.read_bytes() == open(ref_ply, "rb").read()
    if not mullevel:                                                            # (refused before anything is decoded: no process needed)
        with pytest.raises(native.ScpError, match="ring-LOD stream with --lod 1"):
            decode_main(dec + ["--lod", "1"])
        with pytest.raises(native.ScpError, match="ring-LOD stream with --streams"):
            decode_main(dec + ["--streams", "2"])
