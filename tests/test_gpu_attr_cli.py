"""`--attr` through the command lines ("Reflectance"): encode*.py --attr [Q] writes `<stream>.attr`, decode_ehem*.py --attr turns
it into `<stem>.attr.bin`; the geometry files keep their bytes; every refusal names the flag; without the flag no entry of the attribute
layer is called.  Two frames of 4 096 points (synth_frame(i, beams=16, az=256) with synth_reflectance), random weights, at L10 --spher and
at L12 multi-level --spher.  The command lines run in this process, once per configuration, and the tests share what they wrote."""
import contextlib
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

import attr_ref
import distortion_ref
from test_gpu_ringrate import dev, ehem_model

pytestmark = pytest.mark.gpu

CONFIGS = {"L10-spher": (10, False), "L12-multi-level": (12, True)}
LINE = "attr bits, bits per point"
CALLS = [0]


@functools.lru_cache(maxsize=None)
def frames():
    from scp_amd.synth import synth_frame, synth_reflectance
    out = []
    for i in range(2):
        xyz = synth_frame(i, beams=16, az=256)
        out.append((xyz, synth_reflectance(xyz, i)))
    return out


@contextlib.contextmanager
def counted_attr_entries():
    """Every native.attr_* function behind a counting wrapper."""
    from scp_amd import native
    names = [n for n in dir(native) if n.startswith("attr_") and callable(getattr(native, n))]
    assert len(names) >= 5
    saved = {n: getattr(native, n) for n in names}

    def wrap(f):
        def g(*a, **k):
            CALLS[0] += 1
            return f(*a, **k)
        return g

    for n, f in saved.items():
        setattr(native, n, wrap(f))
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(native, n, f)


def run(fn, argv, mullevel):
    """One command line in this process -> (its return value, its stdout, the attr entries it called)."""
    buf, before = io.StringIO(), CALLS[0]
    with contextlib.redirect_stdout(buf):
        ret = fn(argv, mullevel=mullevel)
    torch.cuda.synchronize()
    return ret, buf.getvalue(), CALLS[0] - before


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def world(request, tmp_path_factory):
    from scp_amd import cli
    from scp_amd.synth import write_kitti_bin4
    level, mullevel = CONFIGS[request.param]
    tmp = tmp_path_factory.mktemp(request.param)
    seq = tmp / "seq07"
    seq.mkdir()
    for i, (xyz, refl) in enumerate(frames()):
        write_kitti_bin4(str(seq / f"{i:06d}.bin"), xyz, refl)
    enc_args = ["--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", str(level), "--spher", "--random_weights", "0"]
    dec_args = ["--test_files", str(seq), "--random_weights", "0"]
    w = dict(tmp=tmp, seq=seq, level=level, mullevel=mullevel, enc_args=enc_args, dec_args=dec_args)
    cwd = os.getcwd()
    os.chdir(tmp)                                                      # (a run over several KITTI files appends its summary to a file in the cwd)
    try:
        with counted_attr_entries():
            for tag, extra in (("plain", []), ("q1", ["--attr", "--metrics"]), ("q8", ["--attr", "8", "--attr_scale", "255", "--metrics"])):
                out = tmp / tag
                w[tag] = dict(out=out)
                _, w[tag]["enc_stdout"], w[tag]["enc_calls"] = run(cli.main, enc_args + ["--out_dir", str(out)] + extra, mullevel)
                res, _, w[tag]["dec_calls"] = run(cli.decode_main, dec_args + ["--out_dir", str(out)] + (["--attr"] if extra else []), mullevel)
                w[tag]["dec"] = res
            shutil.copytree(tmp / "q1", tmp / "q1s", ignore=shutil.ignore_patterns("*.ply", "*.attr.bin"))
            w["q1s"] = dict(out=tmp / "q1s")
            w["q1s"]["dec"], _, _ = run(cli.decode_main, dec_args + ["--out_dir", str(tmp / "q1s"), "--attr", "--streams", "2"], mullevel)
    finally:
        os.chdir(cwd)
    yield w
    # what the command lines and the library calls of this configuration left behind (models, encoders with their worker threads and
    # streams, decoded clouds) is dropped here, and the allocator's cached blocks go back to the device: the modules that follow start
    # from the memory they always started from
    import gc
    w.clear()
    api.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def api(tag):
    """The library calls behind the command lines, per frame: the stream, the attribute files at Q = 1 and 8 with their reports, the kept
    leaves and the depths."""
    from scp_amd.encoder import FrameEncoder
    level, mullevel = CONFIGS[tag]
    enc = FrameEncoder(ehem_model(), "kitti", level, spher=True, mullevel=mullevel, device=dev())
    out = []
    for xyz, refl in frames():
        res = enc.encode(xyz)
        x, r = torch.from_numpy(xyz).to(dev()), torch.from_numpy(refl).to(dev())
        d1, r1 = enc.encode_attr(x, r)
        d8, r8 = enc.encode_attr(x, r, 8, 255)
        out.append(dict(res=res, d1=d1, r1=r1, d8=d8, r8=r8, kept=[lv.cpu().numpy() for lv in enc.attr_leaves()],
                        depths=[int(i.depth) for i in enc.geom.info]))
    return out


def tag_of(w):
    return [t for t, (lv, m) in CONFIGS.items() if (lv, m) == (w["level"], w["mullevel"])][0]


def streams(out):
    return sorted(f for f in out.iterdir() if f.name.endswith(".bin") and not f.name.endswith(".attr.bin"))


def test_lossless_values_come_back_and_the_frame_file_holds_them(world):
    from scp_amd.data_preproc import pt as pointCloud
    a = api(tag_of(world))
    bins = streams(world["q1"]["out"])
    assert len(bins) == 2 and world["q1"]["enc_stdout"].count(LINE) == 2
    for i, (b, (ply, out)) in enumerate(zip(bins, world["q1"]["dec"])):
        assert b.read_bytes() == a[i]["res"]["bytes"]
        assert (b.parent / (b.name + ".attr")).read_bytes() == a[i]["d1"]
        assert len(out["attr_values"]) == len(a[i]["kept"]) == (3 if world["mullevel"] else 1)
        for s, v in enumerate(out["attr_values"]):
            assert np.array_equal(out["leaves"][s].cpu().numpy(), a[i]["kept"][s])
            assert int(a[i]["r1"]["counts"][s].min()) >= 1                                   # every kept leaf holds a point
            assert v.dtype == torch.uint8 and torch.equal(v, a[i]["r1"]["values"][s])
        U = sum(len(k) for k in a[i]["kept"])
        rows = np.fromfile(ply[:-len(".ply")] + ".attr.bin", np.float32).reshape(-1, 4)
        assert rows.shape == (U, 4) and out["reflectance"].dtype == torch.float32 and out["reflectance"].shape == (U,)
        assert np.array_equal(rows[:, :3], pointCloud.loadply(ply)[0]) and np.array_equal(rows[:, :3], out["points"].cpu().numpy().astype(np.float32))
        values = torch.cat(out["attr_values"]).cpu().numpy()
        assert np.array_equal(rows[:, 3], (values.astype(np.float64) / 255.0).astype(np.float32))
        assert (out["attr_Q"], out["attr_scale"]) == (1, 255)


def numpy_psnr(xyz, refl, points, values, scale):
    v = np.array([attr_ref.point_value(r, scale) for r in refl], np.int64)
    w = values.astype(np.int64)
    ab, _ = distortion_ref.nearest(xyz, points)
    ba, _ = distortion_ref.nearest(points, xyz)
    worst = max(float(np.sum((v - w[ab]) ** 2)) / len(v), float(np.sum((w - v[ba]) ** 2)) / len(w))
    return float("inf") if worst == 0 else 10.0 * float(np.log10(255.0 ** 2 / worst))


@pytest.mark.parametrize("run_tag,Q", [("q1", 1), ("q8", 8)])
def test_decoded_values_are_the_references_inverse_and_the_printed_psnr_is_the_metric(world, run_tag, Q):
    a = api(tag_of(world))
    lines = [ln for ln in world[run_tag]["enc_stdout"].splitlines() if ln.startswith(LINE)]
    assert len(lines) == 2 and all("PSNR (refl)" in ln for ln in lines)
    for i, (ply, out) in enumerate(world[run_tag]["dec"]):
        rep = a[i]["r1" if Q == 1 else "r8"]
        b = streams(world[run_tag]["out"])[i]
        assert (b.parent / (b.name + ".attr")).read_bytes() == a[i]["d1" if Q == 1 else "d8"]
        for s, v in enumerate(out["attr_values"]):
            leaves, vals, D = a[i]["kept"][s], rep["values"][s].cpu().tolist(), a[i]["depths"][s]
            f = attr_ref.forward(leaves, vals, D, Q)
            assert v.cpu().tolist() == attr_ref.inverse(leaves, D, Q, f["root"], f["k"])
        bits, bpp, psnr = (float(t) for t in lines[i].split(":")[1].split())
        assert bits == rep["bits"] == 8 * len(a[i]["d1" if Q == 1 else "d8"]) and bpp == rep["bits"] / 4096
        xyz, refl = frames()[i]
        want = numpy_psnr(xyz.astype(np.float64), refl, out["points"].cpu().numpy(), torch.cat(out["attr_values"]).cpu().numpy(), 255)
        assert psnr == want and (Q == 1 or psnr < 60.0)


def test_geometry_files_keep_their_bytes(world):
    plain = sorted(f.name for f in world["plain"]["out"].iterdir())
    assert len(plain) == 2 * 4 and len([n for n in plain if n.endswith(".ply")]) == 2        # stream, .dat, .scp.json, .ply per frame
    for tag in ("q1", "q8"):
        names = sorted(f.name for f in world[tag]["out"].iterdir())
        assert sorted(n for n in names if not n.endswith((".attr", ".attr.bin"))) == plain
        assert len([n for n in names if n.endswith(".bin.attr")]) == 2 and len([n for n in names if n.endswith(".attr.bin")]) == 2
        for n in plain:
            assert (world[tag]["out"] / n).read_bytes() == (world["plain"]["out"] / n).read_bytes(), (tag, n)
    assert LINE not in world["plain"]["enc_stdout"]


def test_lockstep_decoding_writes_the_same_frame_files(world):
    one = sorted(f for f in world["q1"]["out"].iterdir() if f.name.endswith((".attr.bin", ".ply")))
    assert len(one) == 4
    for f in one:
        assert (world["q1s"]["out"] / f.name).read_bytes() == f.read_bytes(), f.name
    for (_, a), (_, b) in zip(world["q1"]["dec"], world["q1s"]["dec"]):
        assert torch.equal(a["reflectance"], b["reflectance"]) and all(torch.equal(x, y) for x, y in zip(a["attr_values"], b["attr_values"]))


def test_without_the_flag_no_attribute_entry_is_called(world):
    assert world["plain"]["enc_calls"] == 0 and world["plain"]["dec_calls"] == 0
    assert all("attr_values" not in out and "reflectance" not in out for _, out in world["plain"]["dec"])
    assert world["q1"]["enc_calls"] >= 2 * 3 and world["q1"]["dec_calls"] >= 2 * 2


def test_refusals_name_the_flag(world, tmp_path, monkeypatch):
    from scp_amd import cli, native
    monkeypatch.chdir(tmp_path)
    base = world["enc_args"] + ["--out_dir", str(tmp_path / "o")]
    m = world["mullevel"]
    for extra, why in ((["--attr", "--model", "OctAttention"], "EHEM encoders only"), (["--attr", "--preproc_path", str(tmp_path) + "/"], "--preproc_path"),
                       (["--attr", "--ring_lod", "0,10,25:2,0,1"], "--ring_lod"), (["--attr", "0"], "1 .. 255|1 \\(lossless\\)"),
                       (["--attr", "256"], "255"), (["--attr_scale", "255"], "give --attr"), (["--attr", "--attr_scale", "0"], "--attr_scale")):
        with pytest.raises(native.ScpError, match="--attr") as e:
            cli.main(base + extra, mullevel=m)
        assert __import__("re").search(why, str(e.value)), (extra, str(e.value))
    obj = [a if a != "kitti" else "obj" for a in base if a != "--spher"]
    if not m:
        with pytest.raises(native.ScpError, match="--attr.*--type obj"):
            cli.main(obj + ["--attr"], mullevel=False)
    with pytest.raises(native.ScpError, match="--attr with --lod 1"):
        cli.decode_main(world["dec_args"] + ["--out_dir", str(world["q1"]["out"]), "--attr", "--lod", "1"], mullevel=m)
    assert not (tmp_path / "o").exists() or not any((tmp_path / "o").iterdir())              # refused before anything was written


def test_missing_and_foreign_attribute_files_are_refused(world, tmp_path):
    from scp_amd import decoder, native
    model, m = ehem_model(), world["mullevel"]
    with pytest.raises(native.ScpError, match="--attr.*lod"):
        decoder.decode_file(str(streams(world["q1"]["out"])[0]), model, mullevel=m, device=dev(), lod=1, attr=True)
    b = streams(world["plain"]["out"])[0]
    with pytest.raises(native.ScpError, match="--attr: .*\\.attr is missing"):
        decoder.decode_file(str(b), model, mullevel=m, device=dev(), attr=True)
    for f in world["plain"]["out"].iterdir():
        if f.name.startswith(b.name):
            shutil.copy(f, tmp_path / f.name)
    local = tmp_path / b.name
    other = streams(world["q1"]["out"])[1]
    shutil.copy(str(other) + ".attr", str(local) + ".attr")                                  # the other frame's layer
    with pytest.raises(native.ScpError, match="--attr: .*another stream"):
        decoder.decode_file(str(local), model, mullevel=m, device=dev(), attr=True)
    good = (streams(world["q1"]["out"])[0].parent / (b.name + ".attr")).read_bytes()
    for data, why in ((b"RIFF" + good[4:], "magic"), (good[:-3], "truncated"), (good + b"\0", "behind"), (good[:4] + b"\x07" + good[5:], "version")):
        (tmp_path / (b.name + ".attr")).write_bytes(data)
        with pytest.raises(native.ScpError, match="--attr: .*" + why):
            decoder.decode_file(str(local), model, mullevel=m, device=dev(), attr=True)
    (tmp_path / (b.name + ".attr")).write_bytes(good)
    out = decoder.decode_file(str(local), model, mullevel=m, device=dev(), attr=True)
    assert torch.equal(out["reflectance"], world["q1"]["dec"][0][1]["reflectance"])
