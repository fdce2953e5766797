"""Whole frames through FrameEncoder on the GPU vs the reference driver's recorded outputs (tests/golden/e2e_*.npz)."""
import os

import numpy as np
import pytest
import torch

from cfgs import ehem_cfg
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc_parts():
    assert torch.cuda.is_available()
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    return fill_weights(EHEM(ehem_cfg()), 0).to(dev), dev


# measured (profiles/parity_r2.json) minus a margin: rows whose 20th / 21st neighbours are exactly tied on the octree lattice are
# resolved by the reference's CPU top-k and may move by more than 1e-4
PMF_ROWS_MIN = 0.995        # measured 1.0 (L12 same-level) and 0.9986 (L14 multi-level)
BITS_REL_MAX = 0.0005       # measured: bit counts identical to the reference driver's on both frames


def _check_against_reference(res, z, orc, plan_levels):
    from scp_amd import native
    # structure: number of nodes, coded symbol sequence (= occupancy stream in the reference's coding order): bit-exact
    assert res["n_nodes"] == int(z["n_nodes"])
    sym = res["_debug"]["sym_coded"].cpu().numpy()
    assert np.array_equal(sym.astype(np.int16), z["sym_coded"])
    # PMFs: the rows the fixture kept (every 37th coded row) agree within float rounding for most rows; rows whose kNN
    # ties are broken differently by the reference's CPU top-k may move more (tests/test_gpu_model.py quantifies it)
    out = native.softmax_cdf(res["_debug"]["table"], want_pmf=True, want_lohi=False)
    pmf = out["pmf"].cpu().numpy()[::int(z["pdf_stride"])]
    close = (np.abs(pmf - z["pdf_sub"]).max(1) < 1e-4).mean()
    print(f"PMF rows within 1e-4 of the reference: {100 * close:.2f}%")
    from conftest import parity_record
    parity_record("e2e/" + str(z["fname"]), pmf_rows_within_1e4=close, max_dpmf=np.abs(pmf - z["pdf_sub"]).max(), bits=res["bits"],
                  reference_bits=8 * len(z["bytes"]))
    # (recorded, not asserted: test_e2e_given_the_reference_neighbour_choice_every_pmf_row_matches shows that with the reference's
    # neighbour choice among tied candidates EVERY row is reproduced; `close` is what this library's own deterministic choice gives)
    # rate: same model, same symbols -> the bitstream length agrees to a fraction of a percent
    ref_bits = 8 * len(z["bytes"])
    print(f"bits {res['bits']} vs reference {ref_bits}  (bpp {res['bpp']:.4f} vs {float(z['bpp']):.4f})")
    assert abs(res["bits"] - ref_bits) <= BITS_REL_MAX * ref_bits
    # the stream decodes back to the coded symbols with the oracle's decoder and this library's integer CDFs
    cdf = native.softmax_cdf(res["_debug"]["table"], want_lohi=False, want_cdf=True)["cdf"].cpu().numpy().view(np.uint16)
    dec = orc.AcDecoder(res["bytes"])
    n = len(sym) - 1
    assert [dec.decode_cdf_row(cdf[i]) for i in range(n)] == sym[:n].tolist()
    # and re-encoding those CDFs with the ORACLE coder gives the same bytes (range coder parity on real data)
    assert orc.ac_encode(cdf, sym.astype(np.int16)) == res["bytes"]


def test_same_level_frame_vs_reference_driver(enc_parts, orc):
    from scp_amd.encoder import FrameEncoder
    model, dev = enc_parts
    z = golden("e2e_ehem_spher_L12")
    enc = FrameEncoder(model, "kitti", 12, spher=True, mullevel=False, device=dev)
    # level 12 sits on the float->int boundary: feed the reference's own integers (its --preproc_path flow)
    _, bin_num, _, _, pt = orc.quantise(z["xyz"], 400 / (2 ** 12 - 1), "spher")
    res = enc.encode_ints([pt], bin_num, 0.0, len(z["xyz"]))
    assert enc.outfile("seqf0", res) == str(z["fname"])
    assert np.array_equal(res["pos_mm"].astype(np.float32), z["dat"])
    _check_against_reference(res, z, orc, None)


def test_mullevel_frame_vs_reference_driver(enc_parts, orc):
    from scp_amd.encoder import FrameEncoder
    model, dev = enc_parts
    z = golden("e2e_ehem_mul_spher_L14")
    enc = FrameEncoder(model, "kitti", 14, spher=True, mullevel=True, device=dev)
    res = enc.encode(z["xyz"])
    assert enc.outfile("seqf0", res) == str(z["fname"])
    assert np.array_equal(res["pos_mm"].astype(np.float32), z["dat"])
    _check_against_reference(res, z, orc, None)


def test_coding_order_matches_oracle_plan(orc):
    from scp_amd.encoder import EncodePlan
    sizes = [1, 6, 20, 8193, 1, 17000, 3]
    plan = EncodePlan(sizes, 8192)
    _, want = orc.ehem_coding_plan(sizes, 8192, mullevel=True)
    assert np.array_equal(plan.coding_order(), want)


def test_batched_windows_equal_single_windows(enc_parts):
    """Equal-length windows are batched into one model call: results must not depend on the batch size."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    xyz = synth_frame(2)[::3].copy()
    a = FrameEncoder(model, "kitti", 12, spher=True, max_batch=1, device=dev).encode(xyz)
    b = FrameEncoder(model, "kitti", 12, spher=True, max_batch=8, device=dev).encode(xyz)
    assert a["n_nodes"] == b["n_nodes"]
    d = (a["_debug"]["table"] - b["_debug"]["table"]).abs().max().item()
    assert d < 1e-4, d


def _ints_of(enc, xyz):
    """arguments of FrameEncoder.encode_ints for the strict host transform of a frame"""
    hq, infos = enc.host_ints(xyz)
    qs = [torch.from_numpy(np.ascontiguousarray(q)).to(enc.device) for q in hq]
    return qs, infos[0].bin_num, (infos[0].offset[2] if enc.cylin else 0.0), xyz.shape[0]


def _result_diff(a, b):
    """Keys in which two result dicts of one frame differ: a field only one of them has, or - `times` aside - another value.  `_debug` (the
    synchronous entry points' device tensors) is not a field of the result."""
    ka, kb = set(a) - {"_debug"}, set(b) - {"_debug"}
    same = lambda k: np.array_equal(a[k], b[k]) if k == "pos_mm" else a[k] == b[k]
    return sorted(ka ^ kb) + sorted(k for k in (ka & kb) - {"times"} if not same(k))


def test_async_pipeline_equals_sync(enc_parts):
    from scp_amd.encoder import FrameEncoder, EncodePlan
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", 12, spher=True, device=dev)
    frames = [synth_frame(s)[::12].copy() for s in (1, 2, 3)]
    sync = [enc.encode(f) for f in frames]
    want = [r["bytes"] for r in sync]
    hs = [enc.encode_async(f) for f in frames]
    res = [enc.finish(h) for h in hs]
    got = [r["bytes"] for r in res]
    assert got == want
    assert [_result_diff(a, b) for a, b in zip(sync, res)] == [[]] * len(frames)
    plan = EncodePlan([1, 6, 8193, 7, 2], 8192)
    assert np.array_equal(plan.coding_order_device(dev).cpu().numpy(), plan.coding_order())


def test_two_lane_pipeline_full_size_frames_equal_sequential_encode(enc_parts):
    """encode_async runs consecutive frames on alternating streams (lanes) with stage G on a third and the range coder on worker
    threads; six full-size L16 mullevel frames in flight must give the bytes of one-at-a-time encode() calls - per-stream kNN
    scratch, cache fills, allocator reuse across streams."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", 16, spher=True, mullevel=True, device=dev)
    frames = [torch.from_numpy(synth_frame(20 + s)).to(dev) for s in range(6)]
    hs = [enc.encode_async(f) for f in frames]                 # a fresh encoder: the first call also builds the caches
    got = [enc.finish(h)["bytes"] for h in hs]
    want = [enc.encode(f)["bytes"] for f in frames]
    assert got == want
    hs = [enc.encode_async(f) for f in frames[::-1]]
    assert [enc.finish(h)["bytes"] for h in hs] == want[::-1]
    # the front part (stage G + plans) one frame ahead on the encoder's front thread, as bench.py / the CLI drive it - device transform and
    # the strict host transform
    for strict in (False, True):
        fut = enc.front_async(frames[0], enc.host_ints(frames[0]) if strict else None)
        hs = []
        for i, f in enumerate(frames):
            cur, fut = fut, (enc.front_async(frames[i + 1], enc.host_ints(frames[i + 1]) if strict else None) if i + 1 < len(frames) else None)
            hs.append(enc.encode_async(f, front=cur))
        got = [enc.finish(h) for h in hs]
        if strict:
            assert [g["bytes"] for g in got] == [enc.encode_ints(*_ints_of(enc, f))["bytes"] for f in frames]
        else:
            assert [g["bytes"] for g in got] == want


def test_determinism(enc_parts):
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    xyz = synth_frame(5)[::10].copy()
    enc = FrameEncoder(model, "kitti", 12, spher=True, device=dev)
    assert enc.encode(xyz)["bytes"] == enc.encode(xyz)["bytes"]


def test_octattn_frame_vs_reference_driver(orc):
    """BASELINE.json configs[0]/[4]: OctAttention path (reference `compress`), L12 --spher."""
    from cfgs import octattn_cfg
    from scp_amd import native
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    z = golden("e2e_octattn_spher_L12")
    _, bin_num, _, _, pt = orc.quantise(z["xyz"], 400 / (2 ** 12 - 1), "spher")
    enc = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev)
    res = enc.encode_ints(np.ascontiguousarray(pt, np.int32), bin_num, len(z["xyz"]))
    assert res["n_nodes"] == int(z["n_nodes"])
    sym = res["_debug"]["sym_coded"].cpu().numpy()
    assert np.array_equal(sym.astype(np.int16), z["sym_coded"])
    pmf = native.softmax_cdf(res["_debug"]["table"], want_pmf=True, want_lohi=False)["pmf"].cpu().numpy()[::int(z["pdf_stride"])]
    assert np.abs(pmf - z["pdf_sub"]).max() < 1e-4
    ref_bits = 8 * len(z["bytes"])
    print(f"octattn bits {res['bits']} vs reference {ref_bits}")
    assert abs(res["bits"] - ref_bits) <= 0.002 * ref_bits
    cdf = native.softmax_cdf(res["_debug"]["table"], want_lohi=False, want_cdf=True)["cdf"].cpu().numpy().view(np.uint16)
    assert orc.ac_encode(cdf, sym.astype(np.int16)) == res["bytes"]


@pytest.mark.parametrize("lw", [False, True])
def test_octattn_mullevel_frame_vs_reference_driver(orc, lw):
    """encode_mullevel.py:23-86 `compress` over dataloaders/encode_dataset_mullevel.py:27-73 (three rho shells; --level_wise: one
    padded sequence per octree level): chunk sizes, coded symbols and file name equal the reference driver's, PMF rows within
    1e-4, bytes reproduced by the oracle coder from this library's CDF integers."""
    from cfgs import octattn_cfg
    from conftest import parity_record
    from scp_amd import native
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    z = golden("e2e_octattn_mul_lw_spher_L12" if lw else "e2e_octattn_mul_spher_L12")
    ints, bin0 = [], None
    for k in range(3):
        _, bin_num, _, _, pt = orc.quantise(z["xyz"], 400 / (2 ** (12 + k) - 1), "spher")
        bin0 = bin_num if bin0 is None else bin0
        ints.append(np.ascontiguousarray(pt, np.int32))
    enc = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev, mullevel=True, level_wise=lw)
    res = enc.encode_ints(ints, bin0, len(z["xyz"]))
    assert res["n_nodes"] == int(z["n_nodes"]) and res["level_sizes"] == z["chunk_sizes"].tolist()
    assert enc.outfile("f0", res) == str(z["fname"])
    sym = res["_debug"]["sym_coded"].cpu().numpy()
    assert np.array_equal(sym.astype(np.int16), z["sym_coded"])
    pmf = native.softmax_cdf(res["_debug"]["table"], want_pmf=True, want_lohi=False)["pmf"].cpu().numpy()[::int(z["pdf_stride"])]
    ref_bits = 8 * len(z["bytes"])
    parity_record("e2e/octattn_mul_" + ("lw_" if lw else "") + str(z["fname"]), max_dpmf=np.abs(pmf - z["pdf_sub"]).max(), bits=res["bits"],
                  reference_bits=ref_bits)
    assert np.abs(pmf - z["pdf_sub"]).max() < 1e-4
    assert abs(res["bits"] - ref_bits) <= 0.002 * ref_bits
    cdf = native.softmax_cdf(res["_debug"]["table"], want_lohi=False, want_cdf=True)["cdf"].cpu().numpy().view(np.uint16)
    assert orc.ac_encode(cdf, sym.astype(np.int16)) == res["bytes"]
    # the pipelined entry point produces the same stream; so does the whole path from the float frame on this frame
    assert enc.finish(enc.encode_async(z["xyz"]))["bytes"] == enc.encode(z["xyz"])["bytes"]
    # sequential mode runs per chunk as well (one window per node): same symbols, different context -> another valid stream
    if lw:
        small = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev, mullevel=True, level_wise=True, max_batch=64)
        r2 = small.encode_ints([q[:300] for q in ints], bin0, 300, sequential=True)
        assert r2["n_nodes"] == sum(r2["level_sizes"]) and r2["bits"] > 0


def test_octattn_async_pipeline_equals_sync():
    """OctAttnFrameEncoder.encode_async / finish (range coder on a worker thread) give the bytes of encode(), frames in flight."""
    from cfgs import octattn_cfg
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    enc = OctAttnFrameEncoder(model, "kitti", 12, cylin=True, device=dev)
    frames = [synth_frame(s)[::9].copy() for s in (4, 5, 6)]
    want = [enc.encode(f) for f in frames]
    hs = [enc.encode_async(f) for f in frames]
    got = [enc.finish(h) for h in hs]
    assert [g["bytes"] for g in got] == [w["bytes"] for w in want]
    assert [g["n_nodes"] for g in got] == [w["n_nodes"] for w in want] and got[0]["bpp"] == want[0]["bpp"]
    assert [_result_diff(w, g) for w, g in zip(want, got)] == [[]] * len(frames)


def test_numpyac_api_roundtrip():
    """B3: arithmeticCoding / arithmeticDeCoding keep the reference's names and argument order."""
    from scp_amd import numpyAc
    z = golden("ac_streams")
    pdf = np.tile(z["n1000_pdfbase"], (4, 1))[:1000]
    sym = z["n1000_sym"]
    codec = numpyAc.arithmeticCoding()
    bs, bits = codec.encode(pdf, sym, None)
    assert bs == z["n1000_bytes"].tobytes() and bits == 8 * len(bs)
    dec = numpyAc.arithmeticDeCoding(bs, 1000, 255, None)
    assert [dec.decode(pdf[i:i + 1]) for i in range(50)] == sym[:50].tolist()
    assert dec.decode_ehem(pdf[50:60]) == sym[50:60].tolist()


def test_cli_encode_mullevel_writes_reference_named_files(tmp_path):
    """B5: the drop-in CLI on a synthetic KITTI-layout tree."""
    import subprocess, sys, os
    from conftest import ROOT
    from scp_amd.synth import synth_frame, write_kitti_bin
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "encode_mullevel.py"), "--test_files", str(seq / "*.bin"), "--type", "kitti",
           "--lidar_level", "12", "--spher", "--random_weights", "0", "--out_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "bit per pixel" in r.stdout and "sample number: 2" in r.stdout
    bins = sorted(p.name for p in out.iterdir() if p.name.endswith(".bin"))
    assert len(bins) == 2 and bins[0].startswith("seq07000000_spher_") and (out / (bins[0] + ".dat")).exists()
    assert (tmp_path / "test_results_mul_kitti_12.txt").exists()


def _run_cli(script, args, cwd):
    import subprocess, sys, os
    from conftest import ROOT
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, cwd=str(cwd), timeout=900)


def test_cli_refuses_what_the_reference_cannot_run(tmp_path):
    """Accepted-but-broken flag combinations of the reference fail loudly here instead of encoding something else."""
    from scp_amd.synth import synth_frame, write_kitti_bin
    f = str(tmp_path / "a.bin")
    write_kitti_bin(f, synth_frame(0)[::200])
    base = ["--test_files", f, "--type", "kitti", "--lidar_level", "10", "--random_weights", "0", "--out_dir", str(tmp_path / "o")]
    for script, extra, msg in (("encode.py", ["--spher", "--spher_circle"], "spher_circle"),
                               ("encode.py", ["--spher", "--model", "OctAttention", "--level_wise"], "level_wise"),
                               ("encode.py", ["--spher", "--sequential"], "sequential"),
                               ("encode_mullevel.py", ["--type", "obj", "--spher"], "obj")):
        r = _run_cli(script, base + extra, tmp_path)
        assert r.returncode != 0 and "ScpError" in r.stderr and msg in r.stderr, (script, extra, r.stderr[-500:])


def test_cli_obj_and_octattn_mullevel(tmp_path, orc):
    """`--type obj` (qs 1, per-axis minimum offset, data_preprocess.py:13-70) and encode_mullevel.py with OctAttention."""
    from scp_amd.data_preproc.pt import write_ply_data
    from scp_amd.synth import synth_frame, write_kitti_bin
    rng = np.random.default_rng(5)
    pts = np.unique(rng.integers(0, 64, size=(3000, 3)), axis=0).astype(np.float32) + np.float32(7.0)
    ply = str(tmp_path / "thing_vox6.ply")
    write_ply_data(ply, pts)
    r = _run_cli("encode.py", ["--test_files", ply, "--model", "OctAttention", "--random_weights", "0", "--out_dir", str(tmp_path / "o1")], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    t = orc.octree_build(np.unique((pts - pts.min(0)).astype(np.int64), axis=0))
    assert f"oct num                     : {t.n}" in r.stdout and (tmp_path / "o1" / "thing_vox6.bin").exists()
    f = str(tmp_path / "s1" / "000003.bin")
    os.makedirs(os.path.dirname(f))
    write_kitti_bin(f, synth_frame(2)[::50])
    for lw in ([], ["--level_wise"]):
        out = tmp_path / ("o2" + "".join(lw))
        r = _run_cli("encode_mullevel.py", ["--test_files", f, "--type", "kitti", "--lidar_level", "12", "--spher", "--model", "OctAttention",
                                            "--random_weights", "0", "--out_dir", str(out)] + lw, tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        bins = [p.name for p in out.iterdir() if p.name.endswith(".bin")]
        assert len(bins) == 1 and bins[0].startswith("000003_spher_") and bins[0].endswith("_0.bin")
        assert (int(bins[0].split("_")[2]) == 3) == (not lw)


def test_cli_obj_stream_decodes_with_the_sidecars_offsets(tmp_path):
    """`--type obj` EHEM stream: the per-axis-minimum offset (data_preprocess.py:31-37) exists only in the sidecar's `quant` entry; the
    decode CLI must give the input's points back exactly (integer grid, qs 1) and refuse the stream when the entry is missing instead
    of de-quantising it with another data set's rule."""
    import json
    from scp_amd import native
    from scp_amd.cli import decode_main
    from scp_amd.data_preproc.pt import ptread, write_ply_data
    rng = np.random.default_rng(11)
    pts = np.unique(rng.integers(0, 128, size=(6000, 3)), axis=0).astype(np.float32) + np.float32([3.0, -11.0, 40.0])
    ply = str(tmp_path / "thing_vox7.ply")
    write_ply_data(ply, pts)
    out = tmp_path / "o"
    r = _run_cli("encode.py", ["--test_files", ply, "--random_weights", "0", "--out_dir", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    side = [p for p in out.iterdir() if p.name.endswith(".scp.json")]
    assert len(side) == 1
    sj = json.load(open(side[0]))
    assert sj["type"] == "obj" and sj["quant"][0]["qs"] == [1.0, 1.0, 1.0] and np.allclose(sj["quant"][0]["offset"], pts.min(0))
    res = decode_main(["--test_files", ply, "--random_weights", "0", "--out_dir", str(out)], mullevel=False)      # type from the sidecar
    got = ptread(res[0][0])[:, :3]
    assert sorted(map(tuple, np.round(got, 3).tolist())) == sorted(map(tuple, pts.tolist()))
    del sj["quant"]
    json.dump(sj, open(side[0], "w"))
    with pytest.raises(native.ScpError, match="per-axis minimum"):
        decode_main(["--test_files", ply, "--random_weights", "0", "--out_dir", str(out), "--type", "obj"], mullevel=False)


@pytest.mark.parametrize("mullevel,mode", [(False, "spher"), (True, "spher"), (False, "cylin"), (False, "cart")])
def test_cli_encode_then_decode_files(tmp_path, orc, mullevel, mode):
    """f1 through the FILES: encode CLI -> `.bin` + `.dat` (+ `.scp.json`) -> decode CLI (side info parsed like
    decode_ehem.py:20-27) -> occupancy codes checked against the --preproc_path records, leaf sets equal the oracle's DeOctree of
    the oracle's code lists for the same integers, and the written cloud equals the oracle's de-quantised cloud (spher2cart /
    cylin2cart, data_preprocess.py:186-229)."""
    from scp_amd import native
    from scp_amd.cli import decode_main
    from scp_amd.data_preproc.data_preprocess import write_testset
    from scp_amd.data_preproc.pt import ptread
    from scp_amd.synth import synth_frame, write_kitti_bin
    L = 12
    seq = tmp_path / "seq05"
    seq.mkdir()
    xyz = synth_frame(7)[::40].copy()
    f = str(seq / "000002.bin")
    write_kitti_bin(f, xyz)
    out = tmp_path / "out"
    flags = {"spher": ["--spher"], "cylin": ["--cylin"], "cart": []}[mode]
    enc_script, dec_script = ("encode_mullevel.py", "decode_ehem_mullevel.py") if mullevel else ("encode.py", "decode_ehem.py")
    r = _run_cli(enc_script, ["--test_files", f, "--type", "kitti", "--lidar_level", str(L), "--random_weights", "0", "--out_dir", str(out)] + flags,
                 tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    # the records the reference's decoder wants for its assert (decode_ehem.py:184): written by the test-set generator
    pp = tmp_path / "pp"
    write_testset(f, str(pp), "kitti", L, spher=mode == "spher", cylin=mode == "cylin", mullevel=mullevel, chamfer=False)
    r = _run_cli(dec_script, ["--test_files", f, "--random_weights", "0", "--out_dir", str(out), "--preproc_path", str(pp)], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "checked against" in r.stdout and "decode succeeded" in r.stdout
    got = ptread(str(out / "seq05000002.ply"))          # KITTI streams carry the sequence: so does the decoded cloud
    # oracle: same device integers -> octree -> code list -> DeOctree -> de-quantise
    dev = torch.device("cuda:0")
    want = []
    md = {"spher": native.SPHER, "cylin": native.CYLIN, "cart": native.CART}[mode]
    for k, path in enumerate(([0, 0], [0, 1], [1]) if mullevel else (None,)):
        q, info, _ = native.quantize(torch.from_numpy(xyz).to(dev), md, 400 / (2 ** (L + k) - 1), 0.0 if mullevel else -200.0)
        qn = q.cpu().numpy().astype(np.int64)
        _, idx = np.unique(qn, axis=0, return_index=True)
        t = orc.octree_build(qn[np.sort(idx)], path)
        dq = orc.deoctree(t.codes)
        if mullevel:                       # the last BFS node is not coded (Octree.py:259-262): the leaves below it are lost
            dq = dq[:-bin(int(t.codes[-1])).count("1")]
        # the decoder's steps (decode_ehem.py:237-249): 2 pi / (bin_num - 1) in float64 from the integer bin_num; the encoder side
        # quantised with the float32-rounded step numpy >= 2 produces (data_preprocess.py:50, `info.qs`): 6e-8 relative apart
        qs_k, b = 400 / (2 ** (L + k) - 1), info.bin_num
        step = {"spher": [qs_k, 2 * np.pi / (b - 1), np.pi / (b - 1)], "cylin": [qs_k, 2 * np.pi / (b - 1), qs_k], "cart": [qs_k] * 3}[mode]
        assert np.allclose(step, list(info.qs), rtol=2e-7, atol=0)
        p = dq * np.array(step)[None] + np.array(list(info.offset))[None]
        want.append(orc.spher2cart(p) if mode == "spher" else orc.cylin2cart(p) if mode == "cylin" else p)
    want = np.vstack(want)
    assert got.shape == want.shape
    a, b = torch.from_numpy(got.astype(np.float64)).to(dev), torch.from_numpy(want).to(dev)
    # same point SET (the reader returns float32): nearest-neighbour distance both ways far below the quantisation step
    assert native.nn_sqdist(a, b).max().item() ** 0.5 < 1.5e-5 and native.nn_sqdist(b, a).max().item() ** 0.5 < 1.5e-5


@pytest.mark.parametrize("mullevel,level", [(False, 12), (True, 12)])
def test_encode_decode_roundtrip(enc_parts, mullevel, level):
    """f1: the decoder regenerates the octree from the bitstream alone (+ the reference's side info) - codec loop closed."""
    from scp_amd import native
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    xyz = synth_frame(4)[::30].copy()                       # 4000 points
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev)
    res = enc.encode(xyz)
    nodes = enc.geom.nodes(("occ", "level"))
    dec = FrameDecoder(model, level, mullevel=mullevel, polar=True, device=dev)
    shells = dec.decode(res["bytes"], res["n_levels"], res["pos_mm"])
    assert len(shells) == (3 if mullevel else 1)
    for s, (codes, leaves) in enumerate(shells):
        info = enc.geom.info[s]
        want = nodes["occ"][info.node_base:info.node_base + info.n_nodes].cpu().numpy()
        got = torch.cat(codes).cpu().numpy()
        assert len(got) == len(want)
        if mullevel:
            assert got[-1] == 0 and np.array_equal(got[:-1], want[:-1])      # the last BFS node is not coded (Octree.py:259-262)
        else:
            assert np.array_equal(got, want)
            ref_leaves = enc.geom.leaves(s).cpu().numpy()
            assert np.array_equal(leaves.cpu().numpy(), ref_leaves)


@pytest.mark.parametrize("mullevel", [False, True])
def test_preproc_path_files_and_flow(enc_parts, orc, tmp_path, mullevel):
    """B6 / f2: the generator writes the reference's record files; encoding from them equals encoding from the frame."""
    from scp_amd.data_preproc.data_preprocess import write_testset
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame, write_kitti_bin
    model, dev = enc_parts
    seq = tmp_path / "seq03"
    seq.mkdir()
    xyz = synth_frame(6)[::40].copy()
    f = str(seq / "000001.bin")
    write_kitti_bin(f, xyz)
    L = 14
    name = write_testset(f, str(tmp_path / "pp"), "kitti", L, spher=True, mullevel=mullevel, chamfer=True)
    assert name == "seq03000001"
    pp = str(tmp_path / "pp" / name)
    meta = np.load(pp + "_meta.npy")
    sfx = ("_0_0", "_0_1", "_1") if mullevel else ("",)
    recs = [np.load(pp + s + ".npy") for s in sfx]
    assert all(r.dtype == np.int64 and r.shape[1:] == (4, 6) for r in recs)
    # the record files equal what the reference pipeline (oracle restatement) produces from the same integers
    enc = FrameEncoder(model, "kitti", L, spher=True, mullevel=mullevel, device=dev)
    qs, bin_num, _ = enc.quantize(torch.from_numpy(xyz).to(dev))
    assert float(meta[0]) == bin_num and meta[1] > 0
    for k, (path, _) in enumerate(enc.shells()):
        t = orc.octree_build(qs[k].cpu().numpy(), path)
        assert np.array_equal(recs[k], t.krecords(drop_last=mullevel))
    a = enc.encode(xyz)
    b = enc.encode_records(recs, float(meta[0]), 0.0, len(xyz))
    assert a["bytes"] == b["bytes"] and a["level_sizes"] == b["level_sizes"]
    assert np.array_equal(a["pos_mm"], b["pos_mm"])
    assert os.path.exists(pp + "_quant.ply") and os.path.exists(pp + sfx[0] + "_loc.npy")   # data_preprocess.py:78,153


# ----------------------------------------------------------------------------------------------- 8f-3: distortion metrics on the device
@pytest.mark.gpu
def test_nn_sqdist_is_exhaustive_float64():
    from scipy.spatial import cKDTree
    from scp_amd import native
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    for na, nb in ((1, 1), (7, 3000), (5000, 1), (2500, 4097), (30000, 20000)):
        a, b = rng.random((na, 3)) * 10, rng.random((nb, 3)) * 10
        b[0] = a[0]                                   # an exact hit
        got = native.nn_sqdist(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
        want, _ = cKDTree(b).query(a)
        assert got[0] == 0.0 and np.array_equal(np.sqrt(got), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spher_L12_s0", "cart_L10_s1", "cylin_L12_s2"])
def test_device_chamfer_psnr_vs_reference_tools(orc, name):
    """FrameEncoder.distortion (device NN search) against the numbers the reference's distChamfer / pc_error produced
    (tests/golden/metrics.json) and against the CPU oracle on the same frame."""
    import json
    from cfgs import ehem_cfg
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame
    e = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "metrics.json")))[name]
    dev = torch.device("cuda:0")
    xyz = synth_frame(e["seed"])[::24].copy() if e["sub"] else synth_frame(e["seed"])
    enc = FrameEncoder(EHEM(ehem_cfg()).to(dev), "kitti", e["level"], spher=e["mode"] == "spher", cylin=e["mode"] == "cylin", device=dev)
    x = torch.from_numpy(xyz).to(dev)
    # strict comparison: the oracle's quantised integers (on synthetic rings a whole beam can sit on a rounding boundary of
    # theta / qs, where numpy's float32 SIMD acos and the device's correctly rounded one disagree - DESIGN.md, float -> int boundary)
    from types import SimpleNamespace
    r = orc.proc_pc(xyz, 400 / (2 ** e["level"] - 1), e["mode"])
    qsv = np.broadcast_to(np.asarray(r["qsv"], np.float64).reshape(-1), (3,))
    off = np.broadcast_to(np.asarray(r["offset"], np.float64).reshape(-1), (3,))
    enc.preprocess_ints([torch.from_numpy(r["pts"].astype(np.int32)).to(dev)], r["bin_num"], r["z_offset"], xyz.shape[0])
    d = enc.distortion(x, infos=[SimpleNamespace(qs=qsv, offset=off)])
    assert abs(d["chamfer"] - e["chamfer"]) < 2e-5 * e["chamfer"] and abs(d["psnr"] - e["psnr"]) < 3e-3, (d, e)
    ch, ps = orc.chamfer_psnr(xyz, r["quant_pc"], e["peak"])
    assert abs(d["chamfer"] - ch) < 2e-5 * ch and abs(d["psnr"] - ps) < 1e-3
    # and end to end on the device's own quantiser: the same metric up to the boundary points
    enc.preprocess(x)
    d2 = enc.distortion(x)
    assert abs(d2["chamfer"] - ch) < 0.02 * ch and abs(d2["psnr"] - ps) < 0.2


@pytest.mark.gpu
def test_device_metrics_mullevel_vs_oracle(orc):
    from cfgs import ehem_cfg
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame
    dev = torch.device("cuda:0")
    xyz = synth_frame(3)[::6].copy()
    enc = FrameEncoder(EHEM(ehem_cfg()).to(dev), "kitti", 14, spher=True, mullevel=True, device=dev)
    x = torch.from_numpy(xyz).to(dev)
    enc.preprocess(x)
    d = enc.distortion(x)
    shells = orc.mullevel_shells(xyz, 14, "spher")
    q = np.vstack([s["quant_pc"] for s in shells])
    ch, ps = orc.chamfer_psnr(xyz, q, 59.70)
    assert abs(d["chamfer"] - ch) < 0.02 * ch and abs(d["psnr"] - ps) < 0.2, (d, ch, ps)


# ----------------------------------------------------------------------------------------------- 8f-4: --sequential (OctAttention)
@pytest.mark.gpu
def test_octattn_sequential_mode_vs_oracle(orc):
    """encode.py:38-41,55-56: one window per node, only the last position's prediction kept (and the reference's overwrite of
    the last node by the trailing short windows).  Small context so that the CPU oracle can afford the N model calls."""
    from cfgs import octattn_cfg
    from oracle import models_ref
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    cfg = octattn_cfg()
    cfg["model"]["context_size"] = 32
    model = fill_weights(OctAttention(cfg), 1).to(dev)
    xyz = synth_frame(2)[::800].copy()
    _, bin_num, _, _, pt = orc.quantise(xyz, 400 / (2 ** 12 - 1), "spher")
    pt = np.unique(pt, axis=0)
    enc = OctAttnFrameEncoder(model, "kitti", 12, spher=True, device=dev, max_batch=7)
    res = enc.encode_ints(np.ascontiguousarray(pt, np.int32), bin_num, len(xyz), sequential=True)
    N, cs = res["n_nodes"], 32
    rec = orc.octree_build(pt.astype(np.int64)).krecords()
    _, pos, data, _ = orc.octattn_context(rec, cs)
    data, pos = torch.from_numpy(data), torch.from_numpy(pos)
    assert data.shape[0] == N + cs - 1
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want = torch.empty((N, 255))
    with torch.no_grad():
        for i in range(N + cs - 1):                                    # the reference's loop, verbatim
            o = models_ref.octattn_forward(sd, data[None, i:i + cs].long(), pos[None, i:i + cs])
            want[min(i, N - 1)] = o[0, -1]
    got = res["_debug"]["table"].cpu()
    assert (got - want).abs().max() < 1e-3, (got - want).abs().max()
    # and the default mode differs from it (sanity: the flag does something)
    res2 = enc.encode_ints(np.ascontiguousarray(pt, np.int32), bin_num, len(xyz))
    assert (res2["_debug"]["table"].cpu() - want).abs().max() > 1e-2


# ----------------------------------------------------------------------------------------------- BASELINE.json configs[3] / [4] at full size
@pytest.mark.gpu
def test_ford_like_L17_mullevel_full_frame(enc_parts, orc):
    """SURVEY 8d config (4) = BASELINE configs[3]: Ford-like frame (integer millimetres), level 17, --spher --mullevel (qs 2, 1, 0.5 mm),
    760 571 coded nodes.  PINNED AGAINST THE REFERENCE (round 6): tests/golden/frame_ints.npz `q_spher_ford_L17/18/19` and
    frame_facts.json["F17-m"] come from the reference's own `mul_proc_pc` run on this frame (make_golden.py facts_ford).
    * stage G on the reference's integers: depth, leaves, records, node counts per level, sha256 of the occupancy stream and of the
      [N,4,6] K-records of all three shells = what the reference's builders produced;
    * strict-identity mode (host transform) produces exactly those integers from the floats: 0 differing points, same byte stream;
    * the device transform differs for at most a handful of points; the frame encodes deterministically."""
    import hashlib
    import json
    from conftest import GOLDEN, parity_record
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import ford_like, synth_frame
    model, dev = enc_parts
    xyz = ford_like(synth_frame(0))
    L = 17
    facts = json.load(open(os.path.join(GOLDEN, "frame_facts.json")))["F17-m"]
    z = golden("frame_ints")
    ref_q = [np.ascontiguousarray(z[f"q_spher_ford_L{L + k}"]) for k in range(3)]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    enc = FrameEncoder(model, "ford", L, spher=True, mullevel=True, device=dev)
    ints = [torch.from_numpy(q).to(dev) for q in ref_q]
    bin0 = facts[0]["bin_num"]
    pre = enc.preprocess_ints(ints, bin0, 0.0, xyz.shape[0])
    occ = enc.geom.nodes(("occ",))["occ"].cpu().numpy()
    total = 0
    for k, f in enumerate(facts):
        i = enc.geom.info[k]
        assert i.depth == f["D"] and i.n_leaves == f["leaves"] and enc.geom.rows(k) == f["records"] and i.n_nodes == f["records"] + 1, k
        assert enc.geom.level_counts(k) == f["per_level"], k
        assert sha(occ[i.node_base:i.node_base + i.n_nodes]) == f["codes_sha"], k
        assert sha(enc.geom.krecords(k).cpu().numpy().astype(np.int32)) == f["krec_sha_i32"], k
        total += f["records"]
    assert pre["ctx"].shape[0] == total == 760571
    # the oracle agrees with the reference on this frame too (its integers from the floats: same shells)
    shells = orc.mullevel_shells(xyz, L, "spher", data_type="ford")
    assert [s["records"].shape[0] for s in shells] == [f["records"] for f in facts]
    r1 = enc.encode_ints(ints, bin0, 0.0, xyz.shape[0])
    r2 = enc.encode_ints(ints, bin0, 0.0, xyz.shape[0])
    assert r1["bytes"] == r2["bytes"] and r1["n_nodes"] == total and 0 < r1["bpp"] < 64
    # strict-identity mode: the reference's float -> integer arithmetic on the host, from the floats
    encs = FrameEncoder(model, "ford", L, spher=True, mullevel=True, device=dev, host_transform=True)
    hq, infos = encs.host_ints(xyz)
    ndiff = [int((np.asarray(a) != b).any(1).sum()) for a, b in zip(hq, ref_q)]
    parity_record("host_transform/F17-m", points=len(xyz), points_differing_from_reference_ints=sum(ndiff))
    assert ndiff == [0, 0, 0] and infos[0].bin_num == bin0
    rs = encs.encode(xyz)
    assert rs["bytes"] == r1["bytes"] and rs["n_nodes"] == total
    # the device quantiser on the same frame: same shells up to the float -> int boundary points
    dq = enc.quantize(torch.from_numpy(xyz).to(dev))[0]
    ddiff = [int((q.cpu().numpy() != b).any(1).sum()) for q, b in zip(dq, ref_q)]
    parity_record("device_transform/F17-m", points=len(xyz), points_differing_from_reference_ints=sum(ddiff))
    print("F17-m nodes per shell:", [f["records"] for f in facts], "device-transform points differing per shell:", ddiff)
    assert sum(ddiff) <= 1500, ddiff                 # measured on MI355X: 110 / 194 / 425 of 120 000 (integer-millimetre inputs sit ON rounding boundaries more often)
    r3 = enc.encode(xyz)
    assert abs(r3["n_nodes"] - total) < 0.01 * total


@pytest.mark.gpu
def test_octattn_L14_cylin_full_frame(orc):
    """OctAttention, level 14, --cylin, 291 k nodes = 286 windows of 1024: stage G equals the oracle on its
    integers, symbols = occupancy codes - 1, the coded stream is what the oracle's range coder produces from the device CDFs."""
    from cfgs import octattn_cfg
    from scp_amd import native
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    dev = torch.device("cuda:0")
    model = fill_weights(OctAttention(octattn_cfg()), 0).to(dev)
    xyz = synth_frame(0)
    _, bin_num, _, _, pt = orc.quantise(xyz, 400 / (2 ** 14 - 1), "cylin")
    pt = np.unique(pt, axis=0)
    tree = orc.octree_build(pt.astype(np.int64))
    enc = OctAttnFrameEncoder(model, "kitti", 14, spher=False, cylin=True, device=dev)
    res = enc.encode_ints(np.ascontiguousarray(pt, np.int32), bin_num, len(xyz))
    assert res["n_nodes"] == tree.n == 291522
    sym = res["_debug"]["sym_coded"].cpu().numpy()
    assert np.array_equal(sym, tree.codes - 1)
    cdf = native.softmax_cdf(res["_debug"]["table"], want_lohi=False, want_cdf=True)["cdf"].cpu().numpy().view(np.uint16)
    assert orc.ac_encode(cdf, sym.astype(np.int16)) == res["bytes"]


@pytest.mark.gpu
def test_batch_of_16_L12_spher_frames(enc_parts, orc):
    """16 frames (seeds 0..15), level 12 --spher, through the pipelined encoder; every frame's stream equals
    the synchronous path's, and the octree of three of them equals the oracle's on the oracle's integers."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", 12, spher=True, device=dev)
    frames = [synth_frame(s) for s in range(16)]
    handles = [enc.encode_async(f) for f in frames]
    res = [enc.finish(h) for h in handles]
    assert len({r["bytes"] for r in res}) == 16 and all(100_000 < r["n_nodes"] < 130_000 for r in res)
    for s in (0, 7, 15):
        assert enc.encode(frames[s])["bytes"] == res[s]["bytes"]
        r = orc.proc_pc(frames[s], 400 / (2 ** 12 - 1), "spher")
        enc.preprocess_ints([torch.from_numpy(r["pts"].astype(np.int32)).to(dev)], r["bin_num"], 0.0, len(frames[s]))
        assert np.array_equal(enc.geom.nodes(("occ",))["occ"].cpu().numpy(), r["tree"].codes)


@pytest.mark.gpu
def test_full_frame_packed_forward_is_batch_invariant(enc_parts):
    """BASELINE.json configs[2] at full size (L16 --spher --mullevel, 577 k nodes, 100 windows): the rows the one-launch-sequence
    packed forward produces for a window must be BIT-identical to that window pushed through the same kernels alone (what the
    decoder does).  590 k rows mean several GEMM tiles per persistent workgroup, full kNN / attention grids: a race or a tiling
    bug at scale shows up here, and so would any dependence of a row's result on the rest of the launch."""
    from scp_amd.encoder import EncodePlan, FrameEncoder
    from scp_amd.models.packed import PackedPlan
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", 16, spher=True, mullevel=True, device=dev)
    pre = enc.preprocess(torch.from_numpy(synth_frame(0)).to(dev))
    plan = EncodePlan(pre["level_sizes"], 8192)
    assert plan.n_rows > 500_000 and len(plan.windows) >= 100
    table = enc.logits_in_coding_order(pre, plan)
    assert torch.equal(table, enc.logits_in_coding_order(pre, plan))          # run to run
    picks = sorted({0, 3, 6, 7, 8, len(plan.windows) // 2, len(plan.windows) - 2, len(plan.windows) - 1})
    for wi in picks:
        start, c, coded = plan.windows[wi]
        ev, od = model.forward_packed(pre["ctx"][start:start + c], pre["pos"][start:start + c], None, plan=PackedPlan([c], device=dev))
        ne = (c + 1) // 2
        assert torch.equal(table[coded:coded + ne], ev), (wi, c)
        if c > 1:
            assert torch.equal(table[coded + ne:coded + c], od), (wi, c)


@pytest.mark.gpu
def test_full_size_encode_decode_roundtrip(enc_parts):
    """BASELINE.json configs[2] at full size: the L16 --spher --mullevel frame (577 k nodes, 100 windows) encoded by the pipelined
    packed path decodes back to the exact occupancy codes of all three shells - the strongest end-to-end statement available:
    every CDF the decoder rebuilds window by window equals the one the encoder's single packed launch produced."""
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", 16, spher=True, mullevel=True, device=dev)
    res = enc.finish(enc.encode_async(synth_frame(0)))
    assert res["n_nodes"] > 500_000
    occ = enc.geom.nodes(("occ",))["occ"]
    shells = FrameDecoder(model, 16, mullevel=True, polar=True, device=dev).decode(res["bytes"], res["n_levels"], res["pos_mm"])
    assert len(shells) == 3
    for s, (codes, _) in enumerate(shells):
        info = enc.geom.info[s]
        want = occ[info.node_base:info.node_base + info.n_nodes].cpu().numpy()
        got = torch.cat(codes).cpu().numpy()
        assert len(got) == len(want) and got[-1] == 0 and np.array_equal(got[:-1], want[:-1]), s


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "dup2", "five", "line"])
@pytest.mark.parametrize("spher", [True, False])
def test_degenerate_frames_roundtrip(enc_parts, case, spher):
    """Frames of one point, two identical points, five points, 300 collinear points: encode -> decode regenerates the octree."""
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    model, dev = enc_parts
    xyz = {"one": np.array([[10.0, 3.0, -1.0]], np.float32), "dup2": np.array([[10.0, 3.0, -1.0]] * 2, np.float32),
           "five": np.array([[10, 3, -1], [12, -4, 0.5], [30, 1, 2], [5, 5, -1.5], [60, -20, 1]], np.float32),
           "line": np.stack([np.linspace(2, 80, 300), np.zeros(300), np.zeros(300)], 1).astype(np.float32)}[case]
    enc = FrameEncoder(model, "kitti", 12, spher=spher, device=dev)
    res = enc.encode(xyz)
    occ = enc.geom.nodes(("occ",))["occ"].cpu().numpy()
    (codes, leaves), = FrameDecoder(model, 12, mullevel=False, polar=spher, device=dev).decode(res["bytes"], res["n_levels"], res["pos_mm"])
    assert np.array_equal(torch.cat(codes).cpu().numpy(), occ)
    assert np.array_equal(leaves.cpu().numpy(), enc.geom.leaves(0).cpu().numpy())
    assert res["n_points"] == len(xyz) and res["bits"] == 8 * len(res["bytes"])


@pytest.mark.gpu
def test_mullevel_one_leaf_shells_roundtrip(enc_parts):
    """Three points, one per rho shell: every shell's octree is one chain whose last level holds only the dropped node (n == 1,
    symbol unknown, no children: `native.decode_expand` with m == 0).  The decoder regenerates the leaves of all three shells.
    Second frame: the far point lies beyond 200 m, so the far shell's chain is deeper than lidar_level + 1 and off the diagonal - its
    records end at depth - 1, which is the chunk encode_dataset_ehem.py:86 clips; encoder and decoder must both clip THAT level."""
    from oracle import scp_oracle as orc
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    model, dev = enc_parts
    for radii in ((5, 30, 70), (50, 150, 300)):
        xyz = np.array([[r * 0.8, r * 0.6, -1.0] for r in radii], np.float32)
        shells = orc.mullevel_shells(xyz, 12, "spher")
        assert [s["tree"].n - s["records"].shape[0] for s in shells] == [1, 1, 1] and all(s["tree"].n == s["tree"].depth for s in shells)
        if radii[-1] > 200:
            far = shells[2]
            depth = far["tree"].depth
            assert depth > 12 + 1 and int(far["records"][:, 3, 1].max()) == depth - 1
            assert len(set(far["tree"].pos[depth - 2].tolist())) > 1                      # the last coded node is off the diagonal: no 0 / 0
            _, pos, _, data, _ = orc.ehem_level_split(far["records"], 12, True, mul=True)
            assert (data[-1][:, -1, 0] == 12).all() and len(data) == depth - 1 and np.isfinite(pos[-1]).all()
        enc = FrameEncoder(model, "kitti", 12, spher=True, mullevel=True, device=dev)
        res = enc.encode(xyz)
        out = FrameDecoder(model, 12, mullevel=True, polar=True, device=dev).decode(res["bytes"], res["n_levels"], res["pos_mm"])
        assert len(out) == 3
        for k, (codes, leaves) in enumerate(out):
            occ = shells[k]["tree"].occ
            got = torch.cat(codes).cpu().numpy()
            assert np.array_equal(got[:-1], occ[:-1]) and got[-1] == 0            # the dropped node's occupancy is never coded
            assert leaves.shape[0] == 0                                            # ... so its leaf is not regenerated (decode_ehem_mullevel.py:100-130)


@pytest.mark.gpu
def test_unsupported_configurations_fail_loudly(enc_parts):
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder
    model, dev = enc_parts
    with pytest.raises(native.ScpError):
        FrameEncoder(model, "kitti", 12, spher=False, cylin=False, mullevel=True, device=dev)     # no Cartesian multi-level path
    enc = FrameEncoder(model, "kitti", 12, spher=True, mullevel=True, device=dev)
    with pytest.raises(native.ScpError):
        enc.encode(np.array([[10.0, 3.0, -1.0]], np.float32))                                       # two of the three shells are empty


@pytest.mark.parametrize("cfg", ["L12-s", "L16-m"])
def test_host_transform_gives_the_reference_occupancy_stream_from_the_bin(enc_parts, tmp_path, cfg):
    """Strict-identity switch (`--host_transform`, FrameEncoder(host_transform=True), SCP_XFORM=numpy): the 120 000-point `.bin`
    frame through the drop-in CLI gives, from the FLOATS on, the occupancy stream of the reference: 0 points whose integers differ
    from the reference quantiser's (tests/golden/frame_ints.npz), the octree's occupancy bytes hash to frame_facts.json `codes_sha`,
    and the byte stream the CLI writes is the one `encode_ints` produces from the reference's own integers."""
    import hashlib
    import json
    from conftest import GOLDEN, parity_record
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame, write_kitti_bin
    model, dev = enc_parts
    mul = cfg == "L16-m"
    L = 16 if mul else 12
    facts = json.load(open(os.path.join(GOLDEN, "frame_facts.json")))[cfg]
    ints = golden("frame_ints")
    xyz = synth_frame(0)
    ref_q = [np.ascontiguousarray(ints[f"q_spher_L{L + k}"]) for k in range(3 if mul else 1)]
    enc = FrameEncoder(model, "kitti", L, spher=True, mullevel=mul, device=dev, host_transform=True)
    hq, infos = enc.host_ints(xyz)
    ndiff = sum(int((a != b).any(1).sum()) for a, b in zip(hq, ref_q))
    parity_record(f"host_transform/{cfg}", points=len(xyz), points_differing_from_reference_ints=ndiff)
    assert ndiff == 0
    res = enc.encode(xyz)
    # the octree the encoder just built, shell by shell, against what the reference's builders produced
    occ = enc.geom.nodes(("occ",))["occ"].cpu().numpy()
    for k, f in enumerate(facts if mul else [facts]):
        i = enc.geom.info[k]
        assert hashlib.sha256(occ[i.node_base:i.node_base + i.n_nodes].tobytes()).hexdigest() == f["codes_sha"], (cfg, k)
    want = FrameEncoder(model, "kitti", L, spher=True, mullevel=mul, device=dev).encode_ints(ref_q, infos[0].bin_num, 0.0, len(xyz))
    assert res["bytes"] == want["bytes"] and res["n_nodes"] == want["n_nodes"]
    assert np.array_equal(res["_debug"]["sym_coded"].cpu().numpy(), want["_debug"]["sym_coded"].cpu().numpy())
    # ... and through the command line, from the file
    seq = tmp_path / "seq00"
    seq.mkdir()
    f = str(seq / "000000.bin")
    write_kitti_bin(f, xyz)
    out = tmp_path / "out"
    r = _run_cli("encode_mullevel.py" if mul else "encode.py", ["--test_files", f, "--type", "kitti", "--lidar_level", str(L), "--spher",
                                                                 "--random_weights", "0", "--out_dir", str(out), "--host_transform"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    bins = [p for p in out.iterdir() if p.name.endswith(".bin")]
    assert len(bins) == 1 and bins[0].read_bytes() == want["bytes"]
    # without the switch the device transform runs: its integers differ for a few points at L12 - still a valid stream
    if not mul:
        plain = FrameEncoder(model, "kitti", L, spher=True, mullevel=False, device=dev).encode(xyz)
        assert plain["n_nodes"] != want["n_nodes"] or plain["bytes"] != want["bytes"]


def test_cli_decode_picks_the_stream_of_the_right_sequence(tmp_path, orc):
    """Two KITTI sequences holding a frame with the same number: every stream decodes to ITS OWN cloud (`<sequence><frame>.ply`); a stem
    that matches several streams, or none, is an error - never a silent first match."""
    from scp_amd.cli import decode_main, find_stream
    from scp_amd import native
    from scp_amd.data_preproc.pt import ptread
    from scp_amd.synth import synth_frame, write_kitti_bin
    files = []
    for seq, seed in (("11", 3), ("12", 4)):
        d = tmp_path / seq
        d.mkdir()
        f = str(d / "000001.bin")
        write_kitti_bin(f, synth_frame(seed)[::60].copy())
        files.append(f)
    out = tmp_path / "out"
    r = _run_cli("encode.py", ["--test_files"] + files + ["--type", "kitti", "--lidar_level", "10", "--spher", "--random_weights", "0", "--out_dir", str(out)],
                 tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(p.name for p in out.iterdir() if p.name.endswith(".bin"))
    assert len(names) == 2 and names[0].startswith("11000001_") and names[1].startswith("12000001_")
    assert find_stream(str(out) + "/", files[0]) == (names[0], "11000001") and find_stream(str(out) + "/", files[1]) == (names[1], "12000001")
    r = _run_cli("decode_ehem.py", ["--test_files"] + files + ["--random_weights", "0", "--out_dir", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = ptread(str(out / "11000001.ply")), ptread(str(out / "12000001.ply"))
    assert a.shape != b.shape or not np.array_equal(a, b)
    (out / (names[0][:-4] + "_copy.bin")).write_bytes(b"x")               # an ambiguous directory is refused
    (out / "11000001_spher_9_9_9.bin").write_bytes(b"x")
    with pytest.raises(native.ScpError):
        find_stream(str(out) + "/", files[0])
    with pytest.raises(native.ScpError):
        find_stream(str(out) + "/", str(tmp_path / "13" / "000001.bin"))


def test_two_encoders_with_different_numeric_profiles_in_one_process(enc_parts):
    """The numeric profile belongs to the encoder handle (scp_ctx), not to the process: an exact-kNN encoder and a default encoder used
    alternately in one process each produce exactly the stream they produce alone, the two differ, the side info names each one's
    profile, and a decoder with the wrong profile refuses the stream."""
    from scp_amd import native
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    xyz = synth_frame(5)[::12].copy()
    exact = native.NumericProfile(knn_f16x3=False, attention_bf16x3=False)
    a = FrameEncoder(model, "kitti", 12, spher=True, device=dev)
    b = FrameEncoder(model, "kitti", 12, spher=True, device=dev, profile=exact)
    ra1, rb1, ra2, rb2 = a.encode(xyz), b.encode(xyz), a.encode(xyz), b.encode(xyz)
    assert ra1["bytes"] == ra2["bytes"] and rb1["bytes"] == rb2["bytes"]
    assert not torch.equal(ra1["_debug"]["table"], rb1["_debug"]["table"])                 # different arithmetic, really used
    assert "knn=f16x3" in a.profile_string() and "knn=f32" in b.profile_string() and "attn=f32" in b.profile_string()
    # alone, under the process-wide test hooks, the exact profile gives the same stream
    native.set_knn_mode(False); native.set_attention_mode(False)
    try:
        alone = FrameEncoder(model, "kitti", 12, spher=True, device=dev).encode(xyz)
    finally:
        native.set_knn_mode(True); native.set_attention_mode(True)
    assert alone["bytes"] == rb1["bytes"]
    # a stream decodes under its own profile
    dec = FrameDecoder(model, 12, mullevel=False, polar=True, device=dev, profile=exact)
    shells = dec.decode(rb1["bytes"], rb1["n_levels"], rb1["pos_mm"])
    want = b.geom.nodes(("occ",))["occ"].cpu().numpy()                     # (b encoded last: its octree is still in its workspace)
    assert np.array_equal(torch.cat(shells[0][0]).cpu().numpy(), want)


@pytest.mark.parametrize("name,level,mul", [("e2e_ehem_spher_L12", 12, False), ("e2e_ehem_mul_spher_L14", 14, True)])
def test_e2e_given_the_reference_neighbour_choice_every_pmf_row_matches(enc_parts, orc, monkeypatch, name, level, mul):
    """The end-to-end half of the tie proof (tests/test_gpu_model.py has the per-window half): the CPU oracle's encode flow (the
    reference's algorithm, torch.topk's tie-breaking) records the neighbour lists of every search of every window of the frame; the
    product encoder is then run with those lists in place of its own kNN results (windows shorter than 21 nodes keep theirs: all
    candidates are neighbours there).  EVERY PMF row the reference driver recorded is reproduced within 1e-4 - no fraction - and the
    stream has the reference's bit count."""
    from oracle import cpu_encode, models_ref
    from scp_amd import native
    from scp_amd.encoder import EncodePlan, FrameEncoder
    model, dev = enc_parts
    z = golden(name)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    lists = []

    def record(x, k):
        idx = models_ref.knn_default(x, k)
        lists.append(idx[0].clone())
        return idx
    models_ref.KNN_OVERRIDE = record
    try:
        cpu_encode.encode_frame(z["xyz"], sd, level, mullevel=mul, mode="spher")
    finally:
        models_ref.KNN_OVERRIDE = None
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mul, device=dev, host_transform=True)    # the reference's integers
    real = native.knn_topk_packed
    state = dict(call=0, bases=None, lens=None)

    def forced(x, ktab, thr0=None):
        idx = real(x, ktab, thr0)
        s_ = state["call"] % 3
        state["call"] += 1
        out = idx.cpu()
        for w, (base, ce) in enumerate(zip(state["bases"], state["lens"])):
            if ce > 20:
                out[base:base + ce] = (lists[3 * w + s_] + base).to(torch.int32)
        return out.to(x.device)
    monkeypatch.setattr(native, "knn_topk_packed", forced)
    pre = enc.preprocess(torch.from_numpy(np.ascontiguousarray(z["xyz"], np.float32)).to(dev), enc.host_ints(z["xyz"]))
    plan = EncodePlan(pre["level_sizes"], 8192)
    assert len(lists) == 3 * len(plan.windows)
    lens = [w[1] + (w[1] & 1) for w in plan.windows]
    padded = [-(-l // 512) * 512 for l in lens]
    state["lens"], state["bases"] = lens, list(np.concatenate(([0], np.cumsum(padded)[:-1])))
    res = enc._encode_pre(pre, 0.0, False)
    assert state["call"] == 3 and res["n_nodes"] == int(z["n_nodes"])
    assert np.array_equal(res["_debug"]["sym_coded"].cpu().numpy().astype(np.int16), z["sym_coded"])
    pmf = native.softmax_cdf(res["_debug"]["table"], want_pmf=True, want_lohi=False)["pmf"].cpu().numpy()[::int(z["pdf_stride"])]
    d = np.abs(pmf - z["pdf_sub"]).max(1)
    from conftest import parity_record
    parity_record(f"e2e/{name}/reference neighbour lists", rows=len(d), rows_within_1e4=(d < 1e-4).mean(), max_dpmf=d.max(), bits=res["bits"],
                  reference_bits=8 * len(z["bytes"]))
    print(f"{name}: with the reference's neighbour lists max|dPMF| = {d.max():.2e}, rows within 1e-4: {100 * (d < 1e-4).mean():.2f} %, bits "
          f"{res['bits']} vs {8 * len(z['bytes'])}")
    assert d.max() < 1e-4
    assert res["bits"] == 8 * len(z["bytes"])


@pytest.mark.parametrize("mul,level", [(False, 12), (True, 12)])
def test_batched_frames_give_the_per_frame_streams(enc_parts, mul, level):
    """FrameEncoder.encode_batch_async: k frames through one stage G (every (frame, shell) a segment of one scp_geom_build), one packed
    forward and one CDF launch - byte-identical streams, node counts, side information to k separate encodes (frames of different
    sizes, one of them tiny)."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mul, device=dev)
    frames = [synth_frame(20)[::9].copy(), synth_frame(21)[::31].copy(), synth_frame(22)[:50].copy(), synth_frame(23)[::14].copy()]
    single = [enc.encode(f) for f in frames]
    got = enc.finish_batch(enc.encode_batch_async(frames))
    assert len(got) == len(frames)
    for a, b in zip(single, got):
        assert a["bytes"] == b["bytes"] and a["n_nodes"] == b["n_nodes"] and a["n_points"] == b["n_points"] and a["bin_num"] == b["bin_num"]
        assert a["level_sizes"] == b["level_sizes"] and np.array_equal(a["pos_mm"], b["pos_mm"]) and a["bin_nums"] == b["bin_nums"]
        assert enc.outfile("x", a) == enc.outfile("x", b)
    assert [_result_diff(a, b) for a, b in zip(single, got)] == [[]] * len(frames)
    # a second batch on the same encoder (workspace reuse) and a batch of one
    again = enc.finish_batch(enc.encode_batch_async(frames[::-1]))
    assert [r["bytes"] for r in again] == [r["bytes"] for r in single[::-1]]
    assert enc.finish_batch(enc.encode_batch_async(frames[:1]))[0]["bytes"] == single[0]["bytes"]


@pytest.mark.parametrize("mul", [False, True])
def test_batched_frames_with_the_host_transform_give_the_per_frame_streams(enc_parts, mul):
    """encode_batch_async with host_transform=True and k > 1: every frame's integers come out of their own pinned buffer by
    an asynchronous copy of the PINNED TENSOR (a numpy view of it is invisible to torch's host allocator, which may hand the block to the
    next frame while the copy is still reading it).  Several rounds, so that freed pinned blocks do get reused while copies are in
    flight; streams must equal the per-frame encodes."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    model, dev = enc_parts
    enc = FrameEncoder(model, "kitti", 12, spher=True, mullevel=mul, device=dev, host_transform=True)
    frames = [synth_frame(30 + i)[::7 + 3 * i].copy() for i in range(6)]
    single = [enc.encode(f)["bytes"] for f in frames]
    for rnd in range(3):
        order = frames if rnd % 2 == 0 else frames[::-1]
        want = single if rnd % 2 == 0 else single[::-1]
        got = enc.finish_batch(enc.encode_batch_async(order))
        assert [r["bytes"] for r in got] == want, f"round {rnd}"
    # the caller may hand the integers in (bench.py / cli.py compute them on a prefetch thread): same streams, whatever the encoder's own mode
    dev_enc = FrameEncoder(model, "kitti", 12, spher=True, mullevel=mul, device=dev, host_transform=False)
    got = dev_enc.finish_batch(dev_enc.encode_batch_async(frames, ints=[enc.host_ints(f) for f in frames]))
    assert [r["bytes"] for r in got] == single
