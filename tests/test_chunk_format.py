"""Version 2 of `<stream>.attr` / `<stream>.color` (include/scp.h, "Chunk-parallel range coder"; DESIGN.md 6, "Chunked payloads") without a
GPU: pack / unpack round trips, version 1 keeps its bytes, every refusal names its reason, `--chunk` needs its layer, and csrc/ac_chunk.h -
the coder and decoder step every device lane runs - equals rangecoder.cpp chunk by chunk in a stand-alone host program built with
-fsanitize=address,undefined."""
import argparse
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

N = 64


def chunked(n, seed):
    """A well-formed chunked payload of n symbols: (lengths, the chunks back to back); the bytes are arbitrary, the format does not look."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 40, size=-(-n // N)).astype(np.uint32)
    return lengths, rng.integers(0, 256, size=int(lengths.sum()), dtype=np.uint8).tobytes()


def attr_shells():
    """Several shells: 0, 1 and 2 leaves, n = U - 1 a multiple of N (193 leaves: 3 chunks) and not (5000 leaves: 79 chunks)."""
    out = [dict(D=12, U=5000, root=93, tables=[3] * 6 + [9] * 6), dict(D=13, U=1, root=255), dict(D=14, U=0),
           dict(D=3, U=2, root=0, tables=[0, 15, 7]), dict(D=9, U=3 * N + 1, root=17, tables=list(range(9)))]
    for i, s in enumerate(out):
        if s["U"] >= 2:
            s["lengths"], s["payload"] = chunked(s["U"] - 1, i)
    return out


def color_shells():
    out = [dict(D=4, U=5000, root=(93, -255, 255), tables=[3] * 4 + [9] * 4 + [15] * 4), dict(D=13, U=1, root=(255, 0, -1)), dict(D=14, U=0),
           dict(D=1, U=2, root=(0, 7, -7), tables=[0, 15, 7]), dict(D=2, U=N + 1, root=(1, 2, 3), tables=[1, 2, 3, 4, 5, 6])]
    for i, s in enumerate(out):
        if s["U"] >= 2:
            s["lengths"], s["payload"] = chunked(3 * (s["U"] - 1), 10 + i)
    return out


def same_shells(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["D"] == w["D"] and g["U"] == w["U"] and (g["root"] == w.get("root") or tuple(g["root"]) == tuple(w["root"]))
        assert g["tables"] == w.get("tables", []) and g["payload"] == w.get("payload", b"")
        assert ("lengths" in g) == ("lengths" in w) and (("lengths" not in w) or g["lengths"].tolist() == w["lengths"].tolist())


def test_attribute_files_round_trip_in_version_2():
    from scp_amd import attr
    data = attr.pack(8, 255, attr_shells(), chunk=N)
    assert data[:4] == b"SCPA" and data[4] == 2 and struct.unpack("<I", data[11:15])[0] == N
    info = {}
    Q, scale, shells = attr.unpack(data, info)
    assert (Q, scale, info) == (8, 255, dict(version=2, chunk=N))
    same_shells(shells, attr_shells())
    assert [len(s["lengths"]) for s in shells if s["U"] >= 2] == [79, 1, 3]
    assert attr.pack(Q, scale, shells, chunk=N) == data
    assert attr.unpack(attr.pack(1, 1, [], chunk=4096))[2] == []


def test_colour_files_round_trip_in_version_2():
    from scp_amd import color
    data = color.pack(8, color_shells(), chunk=N)
    assert data[:4] == b"SCPC" and tuple(data[4:8]) == (2, 8, 1, 5) and struct.unpack("<I", data[8:12])[0] == N
    info = {}
    Q, shells = color.unpack(data, info)
    assert (Q, info) == (8, dict(version=2, chunk=N))
    same_shells(shells, color_shells())
    assert [len(s["lengths"]) for s in shells if s["U"] >= 2] == [-(-3 * 4999 // N), 1, 3]
    assert color.pack(Q, shells, chunk=N) == data


def test_without_a_chunk_size_both_layers_write_version_1_byte_for_byte():
    """The version-1 bytes built field by field here, as DESIGN.md 6 lists them."""
    from scp_amd import attr, color
    payload = bytes(range(200)) * 3
    shells = [dict(D=12, U=5000, root=93, tables=[3] * 6 + [9] * 6, payload=payload), dict(D=13, U=1, root=255), dict(D=14, U=0)]
    want = (b"SCPA" + struct.pack("<BBIB", 1, 8, 255, 3) + struct.pack("<BI", 12, 5000) + bytes([93]) + bytes([3] * 6 + [9] * 6) + struct.pack("<I", 600)
            + struct.pack("<BI", 13, 1) + bytes([255]) + struct.pack("<BI", 14, 0) + payload)
    assert attr.pack(8, 255, shells) == attr.pack(8, 255, shells, chunk=None) == want
    info = {}
    assert attr.unpack(want, info)[0] == 8 and info == dict(version=1, chunk=None) and "lengths" not in attr.unpack(want)[2][0]
    shells = [dict(D=4, U=5000, root=(93, -255, 255), tables=[3] * 4 + [9] * 4 + [15] * 4, payload=payload), dict(D=13, U=1, root=(255, 0, -1)), dict(D=14, U=0)]
    want = (b"SCPC" + struct.pack("<BBBB", 1, 8, 1, 3) + struct.pack("<BI", 4, 5000) + struct.pack("<Bhh", 93, -255, 255) + bytes([3] * 4 + [9] * 4 + [15] * 4)
            + struct.pack("<I", 600) + struct.pack("<BI", 13, 1) + struct.pack("<Bhh", 255, 0, -1) + struct.pack("<BI", 14, 0) + payload)
    assert color.pack(8, shells) == color.pack(8, shells, chunk=None) == want
    info = {}
    assert color.unpack(want, info)[0] == 8 and info == dict(version=1, chunk=None)


def test_version_2_is_version_1_plus_the_chunk_size_and_the_length_tables():
    from scp_amd import attr
    lengths, body = chunked(4999, 3)
    v2 = attr.pack(8, 255, [dict(D=12, U=5000, root=93, tables=[3] * 12, lengths=lengths, payload=body)], chunk=N)
    v1 = attr.pack(8, 255, [dict(D=12, U=5000, root=93, tables=[3] * 12, payload=lengths.astype("<u4").tobytes() + body)])
    assert v2 == v1[:4] + b"\x02" + v1[5:11] + struct.pack("<I", N) + v1[11:]


@pytest.mark.parametrize("layer", ["attr", "color"])
def test_every_refusal_names_its_reason(layer):
    from scp_amd import attr, color, native
    if layer == "attr":
        mod, make, head, ch = attr, lambda sh, **k: attr.pack(8, 255, sh, **k), 11, 1
        shell = dict(D=3, U=2 * N + 2, root=0, tables=[0, 15, 7])
    else:
        mod, make, head, ch = color, lambda sh, **k: color.pack(8, sh, **k), 8, 3
        shell = dict(D=1, U=2 * N + 2, root=(0, 7, -7), tables=[0, 15, 7])
    n = ch * (shell["U"] - 1)
    C = -(-n // N)
    lengths, body = chunked(n, 5)
    good = make([dict(shell, lengths=lengths, payload=body)], chunk=N)
    assert mod.unpack(good)[-1][0]["lengths"].tolist() == lengths.tolist()
    with pytest.raises(native.ScpError, match="version 3, this library reads versions 1 and 2"):
        mod.unpack(good[:4] + b"\x03" + good[5:])
    for bad in (63, 0, (1 << 20) + 1, 0xFFFFFFFF):
        with pytest.raises(native.ScpError, match=f"chunk size of {bad} symbols, outside 64 .. 2\\^20"):
            mod.unpack(good[:head] + struct.pack("<I", bad) + good[head + 4:])
    assert mod.unpack(make([], chunk=64))[-1] == [] and mod.unpack(make([], chunk=1 << 20))[-1] == []
    for cut in range(head, head + 4):
        with pytest.raises(native.ScpError, match="truncated in the chunk size"):
            mod.unpack(good[:cut])
    # a payload too short for its length table: the count of lengths is not ceil(n / N)
    at = len(good) - (4 * C + len(body)) - 4                              # the shell's payload length field
    assert struct.unpack("<I", good[at:at + 4])[0] == 4 * C + len(body)
    short = good[:at] + struct.pack("<I", 4 * C - 1) + good[at + 4:at + 4 + 4 * C - 1]
    with pytest.raises(native.ScpError, match=f"cannot hold the {C} chunk lengths of {n} symbols in chunks of {N}"):
        mod.unpack(short)
    # a length table whose sum is not the payload length minus 4 C
    wrong = lengths.copy()
    wrong[1] += 1
    with pytest.raises(native.ScpError, match=f"{C} chunk lengths add up to {int(lengths.sum()) + 1}, its payload holds {len(body)} bytes"):
        mod.unpack(good[:at + 4] + wrong.astype("<u4").tobytes() + body)
    with pytest.raises(native.ScpError, match="add up"):
        mod.unpack(good[:at] + struct.pack("<I", 4 * C + len(body) - 1) + good[at + 4:-1])
    # the same N read with another chunk size: another count
    other = good[:head] + struct.pack("<I", 4 * N) + good[head + 4:]
    with pytest.raises(native.ScpError, match="add up|cannot hold"):
        mod.unpack(other)
    # pack refuses what unpack would
    with pytest.raises(native.ScpError, match=f"{C - 1} chunk lengths for {n} symbols in chunks of {N}, {C} expected"):
        make([dict(shell, lengths=lengths[:-1], payload=body)], chunk=N)
    with pytest.raises(native.ScpError, match="add up"):
        make([dict(shell, lengths=lengths, payload=body + b"\0")], chunk=N)
    for bad in (63, (1 << 20) + 1):
        with pytest.raises(native.ScpError, match="64 .. 2\\^20"):
            make([], chunk=bad)


def test_chunk_flag_needs_its_layer_and_a_size_in_range():
    from scp_amd import cli, native
    ns = argparse.Namespace
    assert cli.chunk_request(ns()) is None and cli.chunk_request(ns(attr=1)) is None
    assert cli.chunk_request(ns(attr=1, chunk=4096)) == 4096 and cli.chunk_request(ns(color=8, chunk=64)) == 64
    assert native.CHUNK_DEFAULT == 4096
    with pytest.raises(native.ScpError, match="--chunk.*give --attr or --color"):
        cli.chunk_request(ns(chunk=4096))
    for bad in (63, 0, -4096, (1 << 20) + 1):
        with pytest.raises(native.ScpError, match="--chunk.*64 .. 2\\^20"):
            cli.chunk_request(ns(attr=1, chunk=bad))
    for mod in ("attr", "color"):
        with pytest.raises(native.ScpError, match="64 .. 2\\^20"):
            getattr(__import__("scp_amd." + mod), mod).encode_shells([], [], [], None, chunk=63)


def test_workspace_size_refuses_bad_arguments():
    from scp_amd import native
    L = native.lib()
    assert L.scp_ac_chunks_workspace_bytes(-1, 4096) == L.scp_ac_chunks_workspace_bytes(1, -1) == L.scp_ac_chunks_workspace_bytes(1, 63) == -1
    assert L.scp_ac_chunks_workspace_bytes(1, (1 << 20) + 1) == L.scp_ac_chunks_workspace_bytes((1 << 31) + 1, 64) == -1
    slot = 4 * ((18 * 4096 + 2 + 31) // 32)
    assert L.scp_ac_chunks_workspace_bytes(0, 4096) == 8 and L.scp_ac_chunks_workspace_bytes(4097, 4096) == 3 * 8 + 2 * slot


def test_pair_sets_of_the_gpu_tests_do_what_they_are_for():
    """Input checks of tests/chunk_cases.py through the host coder alone (they say nothing about the device coder, which
    tests/test_gpu_ac_chunks.py holds to these chunks): a whole chunk of midpoint pairs leaves as pending runs of thousands of bits -
    what the word bursts are for; width-1 pairs expand to 14 bits per symbol and more, the largest expansion the sets hold, and stay
    inside the slot (the slot's bound of 18 bits per symbol is derived in csrc/ac_chunk.h; random pairs do not reach it); full-width
    pairs write nothing but the flush."""
    from chunk_cases import CHUNKS, host_chunks
    for N in (256, 4096):
        (c,) = host_chunks("mid", N, N)
        bits = np.unpackbits(np.frombuffer(c, np.uint8))
        edges = np.nonzero(np.diff(bits))[0]
        assert len(c) >= 15 * N // 8 and np.diff(np.concatenate([[-1], edges, [len(bits) - 1]])).max() >= 1000
    for N in CHUNKS:
        slot = 4 * ((18 * N + 2 + 31) // 32)
        whole = host_chunks("width1", 64 * N + 1, N)[:-1]
        assert min(len(c) for c in whole) >= 14 * N // 8 and max(len(c) for c in whole) <= slot
        assert set(host_chunks("full", 2 * N, N)) == {b"\x40"}


def test_chunk_header_equals_the_host_coder_under_address_and_ub_sanitizers(tmp_path):
    """csrc/ac_chunk.h against csrc/rangecoder.cpp in tests/src/ac_chunk_host.cpp (its own main, nothing loaded into Python): 200 random
    cases on both alphabets and the adversarial pair sets - width-1 pairs, midpoint straddles whole and broken, full-width pairs, the sets
    interleaved: the header's encoder equals scp_ac_encode_lohi on every chunk, its decoder scp_ac_dec_run_ctx on whole and cut chunks - the adversarial sets' chunks included, as bytes under random tables;
    slots and chunks are heap buffers of their exact size."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "ac_chunk_host"
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "scp_amd", "csrc"), os.path.join(ROOT, "tests", "src", "ac_chunk_host.cpp"),
           os.path.join(ROOT, "scp_amd", "csrc", "rangecoder.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "sanitize" in b.stdout:
        pytest.skip("this g++ has no sanitizer runtime")
    assert b.returncode == 0, b.stdout[-2000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "254 chunk cases ok" in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
