"""D2 (point-to-plane) PSNR on the device (csrc/normals.hip, scp_amd/metrics.py) against the numpy reference tests/d2_ref.py and the
MPEG pc_error tool's recorded numbers (tests/golden/d2_metrics.json)."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import d2_cases
import d2_ref
from conftest import GOLDEN, ROOT, golden

pytestmark = pytest.mark.gpu

NORMAL_CASES = d2_cases.normal_cases()


def dev():
    return torch.device("cuda:0")


def up(x):
    return torch.from_numpy(np.array(x, np.float64)).to(dev())            # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def reference_normals(k):
    _, xyz, radius, max_nn, _ = NORMAL_CASES[k]
    return d2_ref.estimate_normals(xyz, radius, max_nn, d2_cases.VIEW)


@pytest.mark.parametrize("k", range(len(NORMAL_CASES)), ids=[c[0] for c in NORMAL_CASES])
def test_normals_match_the_reference(k):
    """Neighbour lists and counts exactly; normals within 1e-9 per component wherever the neighbourhood determines them
    ((lam1 - lam0) / lam2 >= 1e-3 and |n . (view - p)| > 1e-9 |p|).  1e-9: an eigenvector moves by at most |dC| / gap, dC is about
    30 * 2^-53 |C| between two summation orders, i.e. 3e-12 at the gap floor - a 300-fold margin.  The rest must still be finite unit
    vectors, and points below 3 neighbours exactly (0, 0, +-1)."""
    from scp_amd import native
    cid, xyz, radius, max_nn, cap = NORMAL_CASES[k]
    ref = reference_normals(k)
    normals, count, idx = native.estimate_normals(up(xyz), radius, max_nn, d2_cases.VIEW, want_idx=True)
    normals, count, idx = normals.cpu().numpy(), count.cpu().numpy(), idx.cpu().numpy()
    assert count.dtype == np.int32 and idx.dtype == np.int32 and idx.shape == (len(xyz), max_nn)
    assert np.array_equal(count, ref.count) and np.array_equal(idx, ref.idx)
    ok = d2_ref.comparable(ref, xyz, d2_cases.VIEW)
    few = ref.count < 3
    left_out = int((~ok & ~few).sum())
    err = float(np.abs(normals - ref.normals)[ok].max()) if ok.any() else 0.0
    print(f"{cid}: n {len(xyz)}  below 3 neighbours {int(few.sum())}  left out {left_out}  max |dn| {err:.3e}")
    assert left_out <= cap * len(xyz)
    assert err <= 1e-9
    assert np.isfinite(normals).all() and np.abs((normals * normals).sum(1) - 1.0).max() <= 1e-14
    assert np.array_equal(normals[few], ref.normals[few]) and (np.abs(normals[few]) == [0.0, 0.0, 1.0]).all()
    if cid == "tie-lattice":
        assert (count == 30).sum() >= 30           # the interior points, whose 30th and 31st neighbours tie (test_d2_ref.py)
    # the list is optional; the normals do not depend on asking for it
    again = native.estimate_normals(up(xyz), radius, max_nn, d2_cases.VIEW)
    assert again[2] is None and torch.equal(again[0].cpu(), torch.from_numpy(normals)) and np.array_equal(again[1].cpu().numpy(), count)


def test_normals_public_function_and_view_point():
    """metrics.estimate_normals: gene_normals.py's parameters by default, float32 input welcome; another view point turns normals over."""
    from scp_amd import metrics
    xyz = d2_cases.near4096()[:1025]
    ref = d2_ref.estimate_normals(xyz)
    got = metrics.estimate_normals(torch.from_numpy(xyz.astype(np.float32)).to(dev()))
    assert got.dtype == torch.float64 and np.abs(got.cpu().numpy() - ref.normals).max() <= 1e-9
    view = (0.0, 0.0, -50.0)
    ref_up = d2_ref.estimate_normals(xyz, view=view)
    got_up = metrics.estimate_normals(up(xyz), view=view).cpu().numpy()
    ok = d2_ref.comparable(ref_up, xyz, view)
    assert ok.mean() >= 0.98 and np.abs(got_up - ref_up.normals)[ok].max() <= 1e-9
    assert (d2_ref.orientation(got_up, xyz, view) >= 0.0).all()


# ------------------------------------------------------------------------------------------------------------------ tie sets
def _fixture(name):
    z = golden("d2_" + name)
    return z["a"].astype(np.float64), z["n_a"].astype(np.float64), z["b"].astype(np.float64), json.load(open(os.path.join(GOLDEN, "d2_metrics.json")))[name]


TIE_CASES = d2_cases.tie_pairs() + [(name,) + _fixture(name)[:3] for name in ("sphere", "lattice")]


@pytest.mark.parametrize("k", range(len(TIE_CASES)), ids=[c[0] for c in TIE_CASES])
def test_tie_set_terms_equal_the_reference_bit_for_bit(k):
    """n_B, e_AB and e_BA per point under torch.equal; their means within 1e-12 relative (the mean is a tree sum on the device)."""
    from scp_amd import metrics, native
    cid, a, n_a, b = TIE_CASES[k]
    want = d2_ref.d2_terms(a, n_a, b)
    A, NA, B = up(a), up(n_a), up(b)
    got = metrics.d2_terms(A, NA, B)
    for name, g, w in zip(("n_B", "e_AB", "e_BA"), got, want):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (cid, name, float(np.abs(g.cpu().numpy() - w).max()))
    for g, w in zip(got[1:], want[1:]):
        assert abs(float(g.mean().item()) - w.mean()) <= 1e-12 * w.mean()
    # NaN guard: the normal of a b_j that is nobody's nearest neighbour never enters a sum
    dab = native.nn_sqdist(A, B)
    assert np.array_equal(dab.cpu().numpy(), d2_ref.nn_sqdist(a, b))
    referenced = (d2_ref._sqdist_rows(a, b) == d2_ref.nn_sqdist(a, b)[:, None]).any(0)
    poisoned = got[0].clone()
    poisoned[torch.from_numpy(~referenced).to(dev())] = float("nan")
    assert torch.equal(native.nn_tieset(native.TIE_PLANE_ERROR, A, B, dab, poisoned), got[1])


@pytest.mark.parametrize("name", ["sphere", "lattice"])
def test_d2_psnr_against_the_pc_error_tool(name):
    """Same tolerances as the reference's own comparison: mse 1e-5 relative (six printed digits), PSNR 1e-3 dB."""
    from scp_amd import metrics
    a, n_a, b, e = _fixture(name)
    got = metrics.d2_psnr(up(a), up(n_a), up(b), e["peak"])
    print(name, got, e)
    assert sorted(got) == ["mse_ab", "mse_ba", "psnr_d2"]
    for key in ("mse_ab", "mse_ba"):
        assert abs(got[key] - e[key]) <= 1e-5 * e[key], (key, got, e)
    assert abs(got["psnr_d2"] - e["psnr_d2"]) <= 1e-3
    # float32 inputs are compared in float64, like chamfer_psnr's
    f32 = metrics.d2_psnr(torch.from_numpy(a.astype(np.float32)).to(dev()), torch.from_numpy(n_a.astype(np.float32)).to(dev()),
                          torch.from_numpy(b.astype(np.float32)).to(dev()), e["peak"])
    assert f32 == got
    # the D1 path on the same pair: chamfer_psnr keeps its results
    d1 = metrics.chamfer_psnr(up(a), up(b), e["peak"])
    assert abs(d1["psnr"] - e["d1_psnr"]) <= 1e-3 and sorted(d1) == ["chamfer", "mse_ab", "mse_ba", "psnr"]


def test_d2_psnr_merges_duplicates_with_the_mean_normal():
    """Duplicates in the cloud that carries the normals are merged as for D1 and take the mean normal (the tool's own rule for
    duplicates with different normals was not identified; no fixture holds any): equal to the reference's statement of that rule, and
    to the device's own result on the merged cloud."""
    from scp_amd import metrics
    rng = np.random.default_rng(9)
    a = rng.integers(0, 6, (700, 3)).astype(np.float64)           # 216 distinct positions at most
    n_a = d2_cases.unit_rows(rng, 700)
    b = rng.integers(0, 6, (300, 3)) + 0.5
    want = d2_ref.d2_psnr(a, n_a, b, 59.70)
    got = metrics.d2_psnr(up(a), up(n_a), up(b), 59.70)
    for key in want:
        assert abs(got[key] - want[key]) <= 1e-12 * abs(want[key]), (key, got, want)
    ua, un = d2_ref.merge_duplicates(a, n_a)
    assert len(ua) < len(a)
    assert metrics.d2_psnr(up(ua), up(un), up(np.unique(b, axis=0)), 59.70, dropdups=False) == got


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_encoder_distortion_with_normals():
    """FrameEncoder.distortion(normals=...) on one small frame at level 10 --spher against the reference on the same leaves and
    normals: means within 1e-12 relative; without normals the dict is today's."""
    from cfgs import ehem_cfg
    from scp_amd import metrics
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame
    xyz = synth_frame(3)[::40].copy()
    enc = FrameEncoder(EHEM(ehem_cfg()).to(dev()), "kitti", 10, spher=True, device=dev())
    x = torch.from_numpy(xyz).to(dev())
    enc.preprocess(x)
    plain = enc.distortion(x)
    normals = metrics.estimate_normals(x)
    full = enc.distortion(x, normals=normals)
    assert sorted(plain) == ["chamfer", "mse_ab", "mse_ba", "psnr"]
    assert sorted(full) == sorted(list(plain) + ["psnr_d2", "mse_ab_d2", "mse_ba_d2"]) and {k: full[k] for k in plain} == plain
    info = enc._infos[0]
    quant = metrics.dequantize(enc.geom.leaves(0), info.qs, info.offset, spher=True, f32=True).double()
    assert plain == metrics.chamfer_psnr(x, quant, 59.70)
    want = d2_ref.d2_psnr(xyz.astype(np.float64), normals.cpu().numpy(), quant.cpu().numpy(), 59.70)
    print(full, want)
    assert abs(full["mse_ab_d2"] - want["mse_ab"]) <= 1e-12 * want["mse_ab"] and abs(full["mse_ba_d2"] - want["mse_ba"]) <= 1e-12 * want["mse_ba"]
    assert abs(full["psnr_d2"] - want["psnr_d2"]) <= 1e-11       # 10 / ln 10 * 1e-12 dB, and the rounding of a logarithm near 60
    assert full["psnr_d2"] > full["psnr"]                       # the plane error is a projection of the point error


def test_cli_gene_normals_then_encode_with_normals(tmp_path):
    """gene_normals.py on two tiny KITTI files, then encode.py --metrics --normals DIR and --normals estimate: the same PSNR (D2) lines,
    a PSNR_D2 summary, and files that read back to the estimator's normals as float32."""
    from scp_amd import metrics
    from scp_amd.data_preproc import pt
    from scp_amd.synth import synth_frame, write_kitti_bin
    vel = tmp_path / "data" / "07" / "velodyne"
    vel.mkdir(parents=True)
    frames = [synth_frame(i)[::150].copy() for i in range(2)]
    for i, f in enumerate(frames):
        write_kitti_bin(str(vel / f"{i:06d}.bin"), f)
    nrm = tmp_path / "nrm"
    run = lambda script, args: subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True,
                                              cwd=str(tmp_path), timeout=600)
    r = run("gene_normals.py", ["--ori_dir", str(vel / "*.bin"), "--out_dir", str(nrm)])
    assert r.returncode == 0, r.stderr[-2000:]
    for i, f in enumerate(frames):
        p, n = pt.load_ply_normals(str(nrm / "07" / f"{i:06d}.ply"))
        want = metrics.estimate_normals(torch.from_numpy(f[:, :3].copy()).to(dev())).float().cpu().numpy()
        assert np.array_equal(p, f[:, :3]) and np.array_equal(n, want)
    base = ["--test_files", str(vel / "*.bin"), "--type", "kitti", "--lidar_level", "10", "--spher", "--random_weights", "0", "--metrics"]
    lines = {}
    for tag, src in (("dir", str(nrm)), ("estimate", "estimate")):
        r = run("encode.py", base + ["--out_dir", str(tmp_path / ("o_" + tag)), "--normals", src])
        assert r.returncode == 0, r.stderr[-2000:]
        lines[tag] = re.findall(r"^PSNR \(D2\) +: (\S+)$", r.stdout, re.M)
        assert len(lines[tag]) == 2 and len(re.findall(r"^PSNR \(D1\) +: ", r.stdout, re.M)) == 2
        mean = float(re.search(r"^PSNR_D2: (\S+)$", r.stdout, re.M).group(1))
        assert abs(mean - sum(float(v) for v in lines[tag]) / 2) <= 1e-9
        assert f"PSNR_D2: {mean}" in open(tmp_path / "test_results_same_kitti_10.txt").read()
    assert lines["dir"] == lines["estimate"]
    # without the flag nothing of it shows; without --metrics it is refused
    r = run("encode.py", base + ["--out_dir", str(tmp_path / "o_plain")])
    assert r.returncode == 0 and "D2" not in r.stdout and "PSNR (D1)" in r.stdout
    r = run("encode.py", base[:-1] + ["--out_dir", str(tmp_path / "o_bad"), "--normals", "estimate"])
    assert r.returncode != 0 and "ScpError" in r.stderr and "--normals" in r.stderr
