"""`--color` through the command lines ("Colour"): encode.py --type obj --color [Q] writes `<stream>.color`, decode_ehem.py
--color turns it into `<stem>.color.ply`; the geometry files keep their bytes; every refusal names the flag; without the flag no entry
of the colour layer is called.  Two object clouds of 4 096 points (synth_object with synth_colors), random weights, and a third cloud
of 3 600 cells of which 496 hold two points, so that its leaf means are means.  The command lines run in this process, once per
configuration, and the tests share what they wrote."""
import contextlib
import functools
import io
import shutil

import numpy as np
import pytest
import torch

import color_ref
import distortion_ref
from test_gpu_ringrate import dev, ehem_model

pytestmark = pytest.mark.gpu

LINE = "color bits, bits per point"
CALLS = [0]
SHIFT = np.float32([3.0, -11.0, 40.0])
Y4 = np.array([2126, 7152, 722], np.int64)


@functools.lru_cache(maxsize=None)
def frames():
    from scp_amd.synth import synth_colors, synth_object
    out = []
    for i in range(2):
        xyz = synth_object(i, 4096).astype(np.float32) + SHIFT
        out.append((xyz, synth_colors(xyz, i)))
    return out


@functools.lru_cache(maxsize=None)
def doubled():
    """3 600 cells, the first 496 of them with a second point of another colour."""
    from scp_amd.synth import synth_colors, synth_object
    cells = synth_object(7, 3600)
    xyz = np.concatenate([cells, cells[:496]]).astype(np.float32) + SHIFT
    return xyz, synth_colors(xyz, 7)


@contextlib.contextmanager
def counted_color_entries():
    """Every native.color_* function behind a counting wrapper."""
    from scp_amd import native
    names = [n for n in dir(native) if n.startswith("color_") and callable(getattr(native, n))]
    assert len(names) >= 4
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


def run(fn, argv):
    """One command line in this process -> (its return value, its stdout, the colour entries it called)."""
    buf, before = io.StringIO(), CALLS[0]
    with contextlib.redirect_stdout(buf):
        ret = fn(argv, mullevel=False)
    torch.cuda.synchronize()
    return ret, buf.getvalue(), CALLS[0] - before


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from scp_amd import cli
    from scp_amd.data_preproc.pt import write_ply_colors
    tmp = tmp_path_factory.mktemp("color")
    src = tmp / "clouds"
    src.mkdir()
    for i, (xyz, rgb) in enumerate(frames()):
        write_ply_colors(str(src / f"thing{i}_vox10.ply"), xyz, rgb)
    enc_args = ["--test_files", str(src / "*.ply"), "--type", "obj", "--random_weights", "0"]
    dec_args = ["--test_files", str(src), "--random_weights", "0"]
    w = dict(tmp=tmp, src=src, enc_args=enc_args, dec_args=dec_args)
    with counted_color_entries():
        for tag, extra in (("plain", []), ("q1", ["--color", "--metrics"]), ("q8", ["--color", "8", "--metrics"])):
            out = tmp / tag
            w[tag] = dict(out=out)
            _, w[tag]["enc_stdout"], w[tag]["enc_calls"] = run(cli.main, enc_args + ["--out_dir", str(out)] + extra)
            w[tag]["dec"], _, w[tag]["dec_calls"] = run(cli.decode_main, dec_args + ["--out_dir", str(out)] + (["--color"] if extra else []))
        dup = tmp / "dup_src"
        dup.mkdir()
        write_ply_colors(str(dup / "pair_vox10.ply"), *doubled())
        w["dup"] = dict(out=tmp / "dup")
        _, w["dup"]["enc_stdout"], _ = run(cli.main, ["--test_files", str(dup / "pair_vox10.ply"), "--type", "obj", "--random_weights", "0",
                                                     "--out_dir", str(tmp / "dup"), "--color", "--metrics"])
        w["dup"]["dec"], _, _ = run(cli.decode_main, ["--test_files", str(dup), "--random_weights", "0", "--out_dir", str(tmp / "dup"), "--color"])
        shutil.copytree(tmp / "q1", tmp / "q1s", ignore=shutil.ignore_patterns("*.ply"))
        w["q1s"] = dict(out=tmp / "q1s")
        w["q1s"]["dec"], _, _ = run(cli.decode_main, dec_args + ["--out_dir", str(tmp / "q1s"), "--color", "--streams", "2"])
    yield w
    # what the command lines and the library calls left behind is dropped here, and the allocator's cached blocks go back to the device
    import gc
    w.clear()
    api.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def api():
    """The library calls behind the command lines, per frame: the stream, the colour files at Q = 1 and 8 with their reports, the leaves,
    the depth, the integers and the reference's leaf means."""
    from scp_amd import cli, color
    from scp_amd.encoder import FrameEncoder
    enc = FrameEncoder(ehem_model(), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev())
    out = []
    for i, (xyz, rgb) in enumerate(frames() + [doubled()]):
        q, off = cli.obj_ints(xyz, f"thing{i}_vox10.ply", dev())
        res = enc.encode_ints([q], 0, 0.0, len(xyz))
        c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev()))
        assert np.array_equal(c.cpu().numpy(), rgb)
        d1, r1 = enc.encode_color(q, c)
        d8, r8 = enc.encode_color(q, c, 8)
        leaves, D = enc.attr_leaves()[0].cpu().numpy(), int(enc.geom.info[0].depth)
        mean, ycc, cnt = color_ref.leaf_values(q.cpu().numpy(), rgb, leaves, D)
        out.append(dict(res=res, d1=d1, r1=r1, d8=d8, r8=r8, leaves=leaves, D=D, off=off, mean=mean, ycc=ycc, cnt=cnt))
    return out


def streams(out):
    return sorted(f for f in out.iterdir() if f.name.endswith(".bin"))


def test_lossless_colours_come_back_and_the_cloud_file_holds_them(world):
    from scp_amd.data_preproc import pt
    a = api()
    bins = streams(world["q1"]["out"])
    assert len(bins) == 2 and world["q1"]["enc_stdout"].count(LINE) == 2
    for i, (b, (ply, out)) in enumerate(zip(bins, world["q1"]["dec"])):
        assert b.read_bytes() == a[i]["res"]["bytes"]
        assert (b.parent / (b.name + ".color")).read_bytes() == a[i]["d1"]
        U = len(a[i]["leaves"])
        assert U == 4096 and a[i]["cnt"] == [1] * U
        assert np.array_equal(out["leaves"][0].cpu().numpy(), a[i]["leaves"])
        assert a[i]["r1"]["values"][0].cpu().tolist() == a[i]["mean"] and a[i]["r1"]["counts"][0].cpu().tolist() == a[i]["cnt"]
        assert out["colors"].dtype == torch.uint8 and out["colors"].shape == (U, 3) and out["color_Q"] == 1
        assert out["colors"].cpu().tolist() == a[i]["mean"]
        p, c = pt.loadply(ply[:-len(".ply")] + ".color.ply", "rgb")
        assert np.array_equal(p, pt.loadply(ply)[0]) and np.array_equal(p, out["points"].cpu().numpy().astype(np.float32))
        assert c.tolist() == a[i]["mean"]
        assert np.array_equal(p, (a[i]["leaves"].astype(np.float64) + np.array(a[i]["off"])).astype(np.float32))
        rep = a[i]["r1"]
        assert rep["n_points"] == 4096 and rep["bits"] == 8 * len(a[i]["d1"]) and rep["bits_per_leaf"] == rep["bits"] / U
        sh = rep["shells"][0]
        assert sh["U"] == U and sh["depth"] == a[i]["D"] and [len(t) for t in sh["tables"]] == [a[i]["D"]] * 3 and len(sh["roots"]) == 3


def numpy_psnr(xyz, rgb, points, decoded):
    v, w = rgb.astype(np.int64), decoded.astype(np.int64)
    ab, _ = distortion_ref.nearest(xyz, points)
    ba, _ = distortion_ref.nearest(points, xyz)
    out = []
    for d, n in ((v - w[ab], len(v)), (w - v[ba], len(w))):
        sse = [int(s) for s in (d * d).sum(0)]
        y = int(((d @ Y4) ** 2).sum())
        out.append((y / n / 1e8, sum(sse) / 3 / n))
    worst_y, worst_rgb = max(out[0][0], out[1][0]), max(out[0][1], out[1][1])
    f = lambda m: float("inf") if m == 0 else 10.0 * float(np.log10(255.0 ** 2 / m))
    return f(worst_y), f(worst_rgb)


@pytest.mark.parametrize("run_tag,Q", [("q1", 1), ("q8", 8)])
def test_decoded_colours_are_the_references_inverse_and_the_printed_psnr_is_the_metric(world, run_tag, Q):
    a = api()
    lines = [ln for ln in world[run_tag]["enc_stdout"].splitlines() if ln.startswith(LINE)]
    assert len(lines) == 2 and all("PSNR (Y), PSNR (RGB)" in ln for ln in lines)
    for i, (ply, out) in enumerate(world[run_tag]["dec"]):
        rep, data = a[i]["r1" if Q == 1 else "r8"], a[i]["d1" if Q == 1 else "d8"]
        b = streams(world[run_tag]["out"])[i]
        assert (b.parent / (b.name + ".color")).read_bytes() == data
        f = color_ref.forward(a[i]["leaves"], a[i]["ycc"], a[i]["D"], Q)
        assert out["colors"].cpu().tolist() == color_ref.inverse(a[i]["leaves"], a[i]["D"], Q, f["root"], f["k"]) and out["color_Q"] == Q
        assert torch.equal(out["colors"], rep["decoded"][0])
        bits, bpp, psnr_y, psnr_rgb = (float(t) for t in lines[i].split(":")[1].split())
        assert bits == rep["bits"] == 8 * len(data) and bpp == rep["bits"] / 4096
        xyz, rgb = frames()[i]
        want = numpy_psnr(xyz.astype(np.float64), rgb, out["points"].cpu().numpy(), out["colors"].cpu().numpy())
        assert (psnr_y, psnr_rgb) == want
        if Q == 1:
            assert out["colors"].cpu().tolist() == a[i]["mean"] and (psnr_y, psnr_rgb) == (float("inf"), float("inf"))
            assert lines[i].split(":")[1].split()[2:] == ["inf", "inf"]
        else:
            assert np.isfinite(psnr_y) and np.isfinite(psnr_rgb) and 20.0 < psnr_rgb < 60.0


def test_cells_with_two_points_code_their_mean(world):
    """The third cloud: 496 leaves average two colours (halves round up), so Q = 1 is exact on the means and not on the points."""
    a = api()[2]
    (ply, out), = world["dup"]["dec"]
    assert len(a["leaves"]) == 3600 and sorted(set(a["cnt"])) == [1, 2] and a["cnt"].count(2) == 496
    assert out["colors"].cpu().tolist() == a["mean"] and a["r1"]["values"][0].cpu().tolist() == a["mean"]
    assert streams(world["dup"]["out"])[0].with_name(streams(world["dup"]["out"])[0].name + ".color").read_bytes() == a["d1"]
    line, = [ln for ln in world["dup"]["enc_stdout"].splitlines() if ln.startswith(LINE)]
    bits, bpp, psnr_y, psnr_rgb = (float(t) for t in line.split(":")[1].split())
    xyz, rgb = doubled()
    assert (psnr_y, psnr_rgb) == numpy_psnr(xyz.astype(np.float64), rgb, out["points"].cpu().numpy(), out["colors"].cpu().numpy())
    assert np.isfinite(psnr_y) and np.isfinite(psnr_rgb) and bits == a["r1"]["bits"] and bpp == bits / 4096


def test_geometry_files_keep_their_bytes(world):
    plain = sorted(f.name for f in world["plain"]["out"].iterdir())
    assert len(plain) == 2 * 4 and len([n for n in plain if n.endswith(".ply")]) == 2        # stream, .dat, .scp.json, .ply per frame
    for tag in ("q1", "q8"):
        names = sorted(f.name for f in world[tag]["out"].iterdir())
        assert sorted(n for n in names if not n.endswith((".color", ".color.ply"))) == plain
        assert len([n for n in names if n.endswith(".bin.color")]) == 2 and len([n for n in names if n.endswith(".color.ply")]) == 2
        for n in plain:
            assert (world[tag]["out"] / n).read_bytes() == (world["plain"]["out"] / n).read_bytes(), (tag, n)
    assert LINE not in world["plain"]["enc_stdout"]


def test_lockstep_decoding_writes_the_same_cloud_files(world):
    one = sorted(f for f in world["q1"]["out"].iterdir() if f.name.endswith(".ply"))
    assert len(one) == 4
    for f in one:
        assert (world["q1s"]["out"] / f.name).read_bytes() == f.read_bytes(), f.name
    for (_, a), (_, b) in zip(world["q1"]["dec"], world["q1s"]["dec"]):
        assert torch.equal(a["colors"], b["colors"]) and a["color_Q"] == b["color_Q"]


def test_without_the_flag_no_colour_entry_is_called(world):
    assert world["plain"]["enc_calls"] == 0 and world["plain"]["dec_calls"] == 0
    assert all("colors" not in out and "color_Q" not in out for _, out in world["plain"]["dec"])
    assert world["q1"]["enc_calls"] >= 2 * 3 and world["q1"]["dec_calls"] >= 2


def test_refusals_name_the_flag(world, tmp_path, monkeypatch):
    from scp_amd import cli, native
    from scp_amd.data_preproc.pt import write_ply_data
    monkeypatch.chdir(tmp_path)
    base = world["enc_args"] + ["--out_dir", str(tmp_path / "o")]
    bare = tmp_path / "bare_vox10.ply"
    write_ply_data(str(bare), frames()[0][0])
    for extra, why in ((["--color", "--model", "OctAttention"], "EHEM encoders only"), (["--color", "--preproc_path", str(tmp_path) + "/"], "--preproc_path"),
                       (["--color", "0"], "1 .*\\.\\. 255"), (["--color", "256"], "255"), (["--color", "--test_files", str(bare)], "no colour columns")):
        with pytest.raises(native.ScpError, match="--color") as e:
            cli.main(base + extra, mullevel=False)
        assert __import__("re").search(why, str(e.value)), (extra, str(e.value))
    for t in ("kitti", "ford"):
        with pytest.raises(native.ScpError, match=f"--color.*--type {t}.*--attr"):
            cli.main([a if a != "obj" else t for a in base] + ["--color"], mullevel=False)
    with pytest.raises(native.ScpError, match="--attr.*--type obj"):
        cli.main(base + ["--attr"], mullevel=False)
    with pytest.raises(native.ScpError, match="--color with --lod 1"):
        cli.decode_main(world["dec_args"] + ["--out_dir", str(world["q1"]["out"]), "--color", "--lod", "1"], mullevel=False)
    assert not (tmp_path / "o").exists() or not any((tmp_path / "o").iterdir())              # refused before anything was written


def test_missing_and_foreign_colour_files_are_refused(world, tmp_path):
    from scp_amd import decoder, native
    from scp_amd.encoder import FrameEncoder
    model = ehem_model()
    with pytest.raises(native.ScpError, match="--color.*lod"):
        decoder.decode_file(str(streams(world["q1"]["out"])[0]), model, device=dev(), lod=1, color=True)
    b = streams(world["plain"]["out"])[0]
    with pytest.raises(native.ScpError, match="--color: .*\\.color is missing"):
        decoder.decode_file(str(b), model, device=dev(), color=True)
    for f in world["plain"]["out"].iterdir():
        if f.name.startswith(b.name):
            shutil.copy(f, tmp_path / f.name)
    local = tmp_path / b.name
    other = streams(world["dup"]["out"])[0]
    shutil.copy(str(other) + ".color", str(local) + ".color")                                # another cloud's layer
    with pytest.raises(native.ScpError, match="--color: .*another stream"):
        decoder.decode_file(str(local), model, device=dev(), color=True)
    good = (streams(world["q1"]["out"])[0].parent / (b.name + ".color")).read_bytes()
    for data, why in ((b"RIFF" + good[4:], "magic"), (good[:-3], "truncated"), (good + b"\0", "behind"), (good[:4] + b"\x07" + good[5:], "version"),
                      (good[:6] + b"\x09" + good[7:], "transform")):
        (tmp_path / (b.name + ".color")).write_bytes(data)
        with pytest.raises(native.ScpError, match="--color: .*" + why):
            decoder.decode_file(str(local), model, device=dev(), color=True)
    (tmp_path / (b.name + ".color")).write_bytes(good)
    out = decoder.decode_file(str(local), model, device=dev(), color=True)
    assert torch.equal(out["colors"], world["q1"]["dec"][0][1]["colors"])
    with pytest.raises(native.ScpError, match="encode_color with ring_lod"):
        FrameEncoder(model, "kitti", 10, spher=True, device=dev(), ring_lod=((0.0, 10.0), (1, 0))).encode_color(
            torch.zeros((1, 3), dtype=torch.int32, device=dev()), torch.zeros((1, 3), dtype=torch.uint8, device=dev()))
