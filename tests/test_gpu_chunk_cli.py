"""`--chunk [N]` through the command lines ("Chunked payloads"): encode*.py --attr --chunk 256 and encode.py --color --chunk 256
write version-2 files; decode_ehem*.py --attr / --color take the version from the file and write the frame files they write from the
version-1 files, also in lockstep (--streams 2) over a version-1 and a version-2 file; every other file keeps its bytes; without the flag
no native.ac_chunks_* entry is called; the flag alone is refused.  The frames and clouds are those of test_gpu_attr_cli.py and
test_gpu_color_cli.py; the command lines run in this process, once per configuration."""
import contextlib
import io
import os
import shutil

import pytest
import torch

import test_gpu_attr_cli as A
import test_gpu_color_cli as K

pytestmark = pytest.mark.gpu

CALLS = [0]


@contextlib.contextmanager
def counted_chunk_entries():
    """Every native.ac_chunks_* function behind a counting wrapper."""
    from scp_amd import native
    names = [n for n in dir(native) if n.startswith("ac_chunks_") and callable(getattr(native, n))]
    assert sorted(names) == ["ac_chunks_decode", "ac_chunks_encode"]
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
    buf, before = io.StringIO(), CALLS[0]
    with contextlib.redirect_stdout(buf):
        ret = fn(argv, mullevel=mullevel)
    torch.cuda.synchronize()
    return ret, buf.getvalue(), CALLS[0] - before


def drop(w):
    import gc
    w.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def layer_runs(w, tmp, flag, enc_args, dec_args, mullevel, made):
    """v1: the flag alone; v2: with --chunk 256; mix: the version-2 directory with the second frame's layer file replaced by the
    version-1 one, decoded in lockstep."""
    from scp_amd import cli
    with counted_chunk_entries():
        for tag, extra in (("v1", [flag]), ("v2", [flag, "--chunk", "256"])):
            out = tmp / tag
            w[tag] = dict(out=out)
            _, w[tag]["enc_stdout"], w[tag]["enc_calls"] = run(cli.main, enc_args + ["--out_dir", str(out)] + extra, mullevel)
            w[tag]["dec"], _, w[tag]["dec_calls"] = run(cli.decode_main, dec_args + ["--out_dir", str(out), flag], mullevel)
        shutil.copytree(tmp / "v2", tmp / "mix", ignore=shutil.ignore_patterns(*made))
        suffix = "." + flag.strip("-")
        layer = sorted(f for f in (tmp / "mix").iterdir() if f.name.endswith(suffix))
        assert len(layer) == 2
        shutil.copy(tmp / "v1" / layer[1].name, layer[1])
        w["mix"] = dict(out=tmp / "mix", layer=layer)
        w["mix"]["dec"], _, w["mix"]["dec_calls"] = run(cli.decode_main, dec_args + ["--out_dir", str(tmp / "mix"), flag, "--streams", "2"], mullevel)


@pytest.fixture(scope="module", params=sorted(A.CONFIGS))
def attr_world(request, tmp_path_factory):
    from scp_amd.synth import write_kitti_bin4
    level, mullevel = A.CONFIGS[request.param]
    tmp = tmp_path_factory.mktemp("chunk-" + request.param)
    seq = tmp / "seq07"
    seq.mkdir()
    for i, (xyz, refl) in enumerate(A.frames()):
        write_kitti_bin4(str(seq / f"{i:06d}.bin"), xyz, refl)
    enc_args = ["--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", str(level), "--spher", "--random_weights", "0"]
    dec_args = ["--test_files", str(seq), "--random_weights", "0"]
    w = dict(mullevel=mullevel, enc_args=enc_args, suffix=".attr", made=(".attr.bin", ".ply"), line=A.LINE)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        layer_runs(w, tmp, "--attr", enc_args, dec_args, mullevel, ("*.ply", "*.attr.bin"))
    finally:
        os.chdir(cwd)
    yield w
    drop(w)


@pytest.fixture(scope="module")
def color_world(tmp_path_factory):
    from scp_amd.data_preproc.pt import write_ply_colors
    tmp = tmp_path_factory.mktemp("chunk-color")
    src = tmp / "clouds"
    src.mkdir()
    for i, (xyz, rgb) in enumerate(K.frames()):
        write_ply_colors(str(src / f"thing{i}_vox10.ply"), xyz, rgb)
    enc_args = ["--test_files", str(src / "*.ply"), "--type", "obj", "--random_weights", "0"]
    w = dict(mullevel=False, enc_args=enc_args, suffix=".color", made=(".color.ply", ".ply"), line=K.LINE)
    layer_runs(w, tmp, "--color", enc_args, ["--test_files", str(src), "--random_weights", "0"], False, ("*.ply",))
    yield w
    drop(w)


def check_world(w, key):
    names = sorted(f.name for f in w["v1"]["out"].iterdir())
    assert names == sorted(f.name for f in w["v2"]["out"].iterdir()) and len([n for n in names if n.endswith(w["suffix"])]) == 2
    frame_files = [n for n in names if n.endswith(w["made"])]
    assert len(frame_files) == 2 * len(w["made"])
    for n in names:
        a, b = (w["v1"]["out"] / n).read_bytes(), (w["v2"]["out"] / n).read_bytes()
        if n.endswith(w["suffix"]):
            # version 1 and version 2 of the same layer: the header fields agree, the chunk size follows the fixed header
            assert a[4] == 1 and b[4] == 2 and a[:4] == b[:4] and a[5:8] == b[5:8] and a != b
            head = 11 if w["suffix"] == ".attr" else 8
            assert a[5:head] == b[5:head] and int.from_bytes(b[head:head + 4], "little") == 256
        else:
            assert a == b, n                                                 # streams, .dat, side info, .ply and the decoded frame files
    for n in frame_files:
        assert (w["mix"]["out"] / n).read_bytes() == (w["v1"]["out"] / n).read_bytes(), n
    assert [f.read_bytes()[4] for f in w["mix"]["layer"]] == [2, 1]
    for (_, x), (_, y), (_, z) in zip(w["v1"]["dec"], w["v2"]["dec"], w["mix"]["dec"]):
        assert torch.equal(x[key], y[key]) and torch.equal(x[key], z[key])
    assert w["v1"]["enc_stdout"].count(w["line"]) == w["v2"]["enc_stdout"].count(w["line"]) == 2           # the per-frame line is still there, once per frame
    assert len(w["v1"]["enc_stdout"].splitlines()) == len(w["v2"]["enc_stdout"].splitlines())
    # without --chunk no entry of the chunk coder is called; with it one per coded shell and side
    assert w["v1"]["enc_calls"] == 0 and w["v1"]["dec_calls"] == 0
    assert w["v2"]["enc_calls"] >= 2 and w["v2"]["dec_calls"] >= 2 and 1 <= w["mix"]["dec_calls"] < w["v2"]["dec_calls"]


def test_attr_chunk_writes_version_2_and_the_decoders_write_the_same_frame_files(attr_world):
    check_world(attr_world, "reflectance")


def test_color_chunk_writes_version_2_and_the_decoders_write_the_same_cloud_files(color_world):
    check_world(color_world, "colors")


def test_chunk_alone_and_out_of_range_sizes_are_refused(attr_world, tmp_path, monkeypatch):
    from scp_amd import cli, native
    monkeypatch.chdir(tmp_path)
    base = attr_world["enc_args"] + ["--out_dir", str(tmp_path / "o")]
    m = attr_world["mullevel"]
    for extra, why in ((["--chunk"], "give --attr or --color"), (["--chunk", "256"], "give --attr or --color"), (["--attr", "--chunk", "63"], "64 .. 2\\^20"),
                       (["--attr", "--chunk", str((1 << 20) + 1)], "64 .. 2\\^20")):
        with pytest.raises(native.ScpError, match="--chunk") as e:
            cli.main(base + extra, mullevel=m)
        assert __import__("re").search(why, str(e.value)), (extra, str(e.value))
    assert not (tmp_path / "o").exists() or not any((tmp_path / "o").iterdir())              # refused before anything was written
