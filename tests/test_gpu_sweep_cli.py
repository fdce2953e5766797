"""`--attr_sweep` / `--attr_target` and `--color_sweep` / `--color_target` through the command lines ("Step sweep"): the layer
file's header holds the step the target chose, the decoders read it unchanged, the geometry files keep their bytes, a sweep alone leaves
the layer file as it was and writes the table of FrameEncoder.attr_sweep.  One frame of 4 096 points per configuration (synth_frame with
synth_reflectance at L10 --spher and at L12 multi-level --spher; synth_object with synth_colors), random weights.  The command lines run
in this process, once per configuration, and the tests share what they wrote."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_ringrate import dev, ehem_model

pytestmark = pytest.mark.gpu

CONFIGS = {"L10-spher": (10, False), "L12-multi-level": (12, True)}
ATTR_TARGET, COLOR_TARGET, SHORT = "psnr=38", "linf=12", "1,4,16,64"


def run(fn, argv, mullevel):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ret = fn(argv, mullevel=mullevel)
    torch.cuda.synchronize()
    return ret, buf.getvalue()


def leave_as_found(w):
    import gc
    w.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def lidar(request, tmp_path_factory):
    from scp_amd import cli
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame, synth_reflectance, write_kitti_bin4
    level, mullevel = CONFIGS[request.param]
    tmp = tmp_path_factory.mktemp(request.param)
    seq = tmp / "seq07"
    seq.mkdir()
    xyz = synth_frame(0, beams=16, az=256)
    refl = synth_reflectance(xyz, 0)
    write_kitti_bin4(str(seq / "000000.bin"), xyz, refl)
    enc_args = ["--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", str(level), "--spher", "--random_weights", "0"]
    w = dict(mullevel=mullevel, enc_args=enc_args)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for tag, extra in (("plain", []), ("attr", ["--attr"]), ("sweep", ["--attr", "--attr_sweep"]), ("target", ["--attr", "--attr_target", ATTR_TARGET]),
                           ("both", ["--attr", "--attr_target", ATTR_TARGET, "--attr_sweep", SHORT])):
            w[tag] = dict(out=tmp / tag)
            w[tag]["stdout"] = run(cli.main, enc_args + ["--out_dir", str(tmp / tag)] + extra, mullevel)[1]
        w["dec"] = run(cli.decode_main, ["--test_files", str(seq), "--random_weights", "0", "--out_dir", str(tmp / "target"), "--attr"], mullevel)[0]
    finally:
        os.chdir(cwd)
    enc = FrameEncoder(ehem_model(), "kitti", level, spher=True, mullevel=mullevel, device=dev())
    enc.encode(xyz)
    x, r = torch.from_numpy(xyz).to(dev()), torch.from_numpy(refl).to(dev())
    kind, value = ATTR_TARGET.split("=")
    w["api"] = dict(sweep=enc.attr_sweep(x, r), target=enc.encode_attr(x, r, target=(kind, float(value))),
                    short=enc.encode_attr(x, r, target=(kind, float(value)), steps=[int(t) for t in SHORT.split(",")]))
    yield w
    leave_as_found(w)


def files(out):
    return {f.name: f.read_bytes() for f in out.iterdir()}


def stream_of(out, suffix):
    names = [n for n in files(out) if n.endswith(".bin" + suffix)]
    assert len(names) == 1, names
    return out / names[0]


def test_attr_target_writes_the_chosen_step_and_the_decoder_reads_it(lidar):
    from scp_amd import attr
    data, rep = lidar["api"]["target"]
    assert rep["met"] and 1 < rep["chosen_Q"] < 255                          # the target sits inside the grid on this frame
    got = stream_of(lidar["target"]["out"], ".attr").read_bytes()
    assert got == data and attr.unpack(got)[0] == rep["chosen_Q"] and got[5] == rep["chosen_Q"]       # magic, version, then Q
    (ply, out), = lidar["dec"]
    assert out["attr_Q"] == rep["chosen_Q"] and len(out["attr_values"]) == len(rep["decoded"])
    for v, d in zip(out["attr_values"], rep["decoded"]):
        assert torch.equal(v, d)
    line, = [ln for ln in lidar["target"]["stdout"].splitlines() if ln.startswith("attr target, chosen Q, met")]
    row = rep["sweep"]["rows"][[r["Q"] for r in rep["sweep"]["rows"]].index(rep["chosen_Q"])]
    assert line.split(":")[1].split() == [ATTR_TARGET, str(rep["chosen_Q"]), "True", str(row["est_bits"]), str(rep["bits"])]
    assert "attr sweep Q:est bpp" not in lidar["target"]["stdout"] and not [n for n in files(lidar["target"]["out"]) if n.endswith(".sweep.json")]
    # --attr_sweep STEPS alongside: the target chooses on that grid, and the table is written
    data2, rep2 = lidar["api"]["short"]
    assert stream_of(lidar["both"]["out"], ".attr").read_bytes() == data2 and rep2["chosen_Q"] in (1, 4, 16, 64)
    doc = json.loads(stream_of(lidar["both"]["out"], ".attr.sweep.json").read_text())
    assert doc["rows"] == rep2["sweep"]["rows"] and doc["steps"] == [1, 4, 16, 64] and doc["chosen_Q"] == rep2["chosen_Q"] and doc["met"] is True
    assert doc["target"] == ["psnr", 38.0] and doc["psnr_over"] == "leaf values"


def test_attr_sweep_alone_leaves_the_layer_file_and_writes_the_table(lidar):
    base, swept = files(lidar["attr"]["out"]), files(lidar["sweep"]["out"])
    extra = sorted(set(swept) - set(base))
    assert len(extra) == 1 and extra[0].endswith(".bin.attr.sweep.json") and {n: swept[n] for n in base} == base
    doc = json.loads(swept[extra[0]])
    want = lidar["api"]["sweep"]
    assert doc["rows"] == want["rows"] and doc["steps"] == want["steps"] and doc["points"] == 4096 and doc["leaves"] == want["leaves"]
    assert "chosen_Q" not in doc and doc["layer"] == "attr"
    line, = [ln for ln in lidar["sweep"]["stdout"].splitlines() if ln.startswith("attr sweep Q:est bpp:leaf PSNR")]
    assert "over leaf values" in line
    cells = line.split(":", 3)[3].split()
    assert cells == ["%d:%.4f:%.2f" % (r["Q"], r["est_bits"] / 4096, r["psnr"]) for r in want["rows"]]
    assert "attr sweep" not in lidar["attr"]["stdout"] and "attr target" not in lidar["sweep"]["stdout"]


def test_geometry_files_keep_their_bytes_under_the_attr_options(lidar):
    plain = files(lidar["plain"]["out"])
    assert len(plain) == 3                                                   # stream, .dat, side info
    for tag in ("attr", "sweep", "target", "both"):
        got = files(lidar[tag]["out"])
        assert {n: got[n] for n in plain} == plain, tag
        assert sorted(n for n in got if n not in plain and not n.endswith((".attr", ".attr.sweep.json", ".ply", ".attr.bin"))) == []


def test_attr_refusals_through_the_command_line(lidar, tmp_path, monkeypatch):
    from scp_amd import cli, native
    monkeypatch.chdir(tmp_path)
    base = lidar["enc_args"] + ["--out_dir", str(tmp_path / "o")]
    for extra, why in ((["--attr_sweep"], "give --attr as well"), (["--attr_target", "psnr=40"], "give --attr as well"),
                       (["--attr", "4", "--attr_target", "psnr=40"], "chooses the step"), (["--attr", "--attr_target", "mse=1"], "unknown kind"),
                       (["--attr", "--attr_target", "psnr=-1"], "finite value >= 0"), (["--attr", "--attr_sweep", "4,2"], "strictly ascending"),
                       (["--attr", "--attr_sweep", "0,2"], "1 .. 255")):
        with pytest.raises(native.ScpError, match=why):
            cli.main(base + extra, mullevel=lidar["mullevel"])
    assert not (tmp_path / "o").exists() or not any((tmp_path / "o").iterdir())              # refused before anything was written


@pytest.fixture(scope="module")
def thing(tmp_path_factory):
    from scp_amd import cli, color
    from scp_amd.data_preproc.pt import write_ply_colors
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_colors, synth_object
    tmp = tmp_path_factory.mktemp("color_sweep")
    src = tmp / "clouds"
    src.mkdir()
    xyz = synth_object(0, 4096).astype(np.float32)
    rgb = synth_colors(xyz, 0)
    write_ply_colors(str(src / "thing0_vox10.ply"), xyz, rgb)
    enc_args = ["--test_files", str(src / "*.ply"), "--type", "obj", "--random_weights", "0"]
    w = dict(enc_args=enc_args)
    for tag, extra in (("plain", []), ("color", ["--color"]), ("target", ["--color", "--color_target", COLOR_TARGET, "--color_sweep"])):
        w[tag] = dict(out=tmp / tag)
        w[tag]["stdout"] = run(cli.main, enc_args + ["--out_dir", str(tmp / tag)] + extra, False)[1]
    w["dec"] = run(cli.decode_main, ["--test_files", str(src), "--random_weights", "0", "--out_dir", str(tmp / "target"), "--color"], False)[0]
    enc = FrameEncoder(ehem_model(), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev())
    q, _ = cli.obj_ints(xyz, "thing0_vox10.ply", dev())
    enc.encode_ints([q], 0, 0.0, len(xyz))
    c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev()))
    kind, value = COLOR_TARGET.split("=")
    w["api"] = enc.encode_color(q, c, target=(kind, float(value)))
    yield w
    leave_as_found(w)


def test_color_target_writes_the_chosen_step_and_the_decoder_reads_it(thing):
    from scp_amd import color
    data, rep = thing["api"]
    assert rep["met"] and 1 < rep["chosen_Q"] < 255
    got = stream_of(thing["target"]["out"], ".color").read_bytes()
    assert got == data and color.unpack(got)[0] == rep["chosen_Q"] and got[5] == rep["chosen_Q"]
    (ply, out), = thing["dec"]
    assert out["color_Q"] == rep["chosen_Q"] and torch.equal(out["colors"], torch.cat(rep["decoded"]))
    d = (torch.cat(rep["values"]).long() - out["colors"].long()).abs()
    assert int(d.max()) <= 12
    line, = [ln for ln in thing["target"]["stdout"].splitlines() if ln.startswith("color target, chosen Q, met")]
    assert line.split(":")[1].split()[:3] == [COLOR_TARGET, str(rep["chosen_Q"]), "True"]
    doc = json.loads(stream_of(thing["target"]["out"], ".color.sweep.json").read_text())
    assert doc["rows"] == rep["sweep"]["rows"] and doc["chosen_Q"] == rep["chosen_Q"] and doc["layer"] == "color"
    plain = files(thing["plain"]["out"])
    assert len(plain) == 3
    for tag in ("color", "target"):
        got = files(thing[tag]["out"])
        assert {n: got[n] for n in plain} == plain, tag


def test_color_refusals_through_the_command_line(thing, tmp_path):
    from scp_amd import cli, native
    base = thing["enc_args"] + ["--out_dir", str(tmp_path / "o")]
    for extra, why in ((["--color_sweep"], "give --color as well"), (["--color_target", "linf=4"], "give --color as well"),
                       (["--color", "8", "--color_target", "linf=4"], "chooses the step"), (["--color", "--color_target", "linf"], "KIND=VALUE"),
                       (["--color", "--color_sweep", ",".join(str(v) for v in range(1, 18))], "sweep steps")):
        with pytest.raises(native.ScpError, match=why):
            cli.main(base + extra, mullevel=False)
    assert not (tmp_path / "o").exists() or not any((tmp_path / "o").iterdir())
