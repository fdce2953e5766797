"""Version-2 (chunked) attribute and colour files on the GPU ("Chunked payloads"): on the hard trees of tests/attr_cases.py and
tests/color_cases.py - all of them as the shells of one file - and on a multi-level frame, at Q = 1, 8 and 255: every chunk of the version-2
file is what the host coder (native.ac_encode_lohi) writes for the same pairs, and decode_shells returns from it what it returns from the
version-1 file of the same input.  The pairs come from the version-1 file alone: its payload through the host decoder
(AcDecoder.run_ctx), the symbols through the tables the file names - nothing from the code under test."""
import functools

import numpy as np
import pytest
import torch

import attr_cases
import color_cases
from test_gpu_attr import multilevel_frame
from test_gpu_ringrate import dev

pytestmark = pytest.mark.gpu

QS = attr_cases.QS
N_CASES, N_FRAME = 64, 256


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    yield
    import gc
    world.cache_clear()
    multilevel_frame.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def up(x, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev())


@functools.lru_cache(maxsize=None)
def world(layer):
    """All cases of a layer as the shells of one frame: one point per leaf carrying the leaf's value; a shell's point list holds -1 where
    the point belongs to another shell (such a point hits no leaf)."""
    cs = attr_cases.cases() if layer == "attr" else color_cases.cases()
    names = sorted(cs)
    total = sum(len(cs[n]["leaves"]) for n in names)
    leaves, depths, qs, vals, at = [], [], [], [], 0
    for n in names:
        lv = cs[n]["leaves"]
        q = np.full((total, 3), -1, np.int32)
        q[at:at + len(lv)] = lv
        at += len(lv)
        leaves.append(up(lv, np.int32).reshape(-1, 3))
        depths.append(cs[n]["D"])
        qs.append(up(q, np.int32))
        vals.append(cs[n]["a"].astype(np.float32) / np.float32(255.0) if layer == "attr" else cs[n]["rgb"])
    values = up(np.concatenate(vals), np.float32 if layer == "attr" else np.uint8)
    return dict(names=names, leaves=leaves, depths=depths, qs=qs, values=values)


def encode(layer, w, Q, **k):
    from scp_amd import attr, color
    if layer == "attr":
        return attr.encode_shells(w["leaves"], w["depths"], w["qs"], w["values"], Q, 255, **k)
    return color.encode_shells(w["leaves"], w["depths"], w["qs"], w["values"], Q, **k)


def host_pairs(layer, shell, lv, D):
    """uint32 pairs of a version-1 shell from its bytes alone: host decoder, then the rows of the tables the file names."""
    from scp_amd import attr, color, native
    channels = 1 if layer == "attr" else 3
    alphabet = attr.ALPHABET if layer == "attr" else color.ALPHABET
    if layer == "attr":
        table_of = [shell["tables"][D - 1 - c] for c in range(D)]
    else:
        by_ctx = dict(zip(color._file_order(D), shell["tables"]))
        table_of = [by_ctx[c] for c in range(3 * D)]
    level = attr.level_contexts(native.attr_level_counts(lv, D).cpu().numpy())
    ctx = np.concatenate([level + np.uint8(c * D) for c in range(channels)])
    rows = attr.tables(alphabet)[table_of]
    z = native.AcDecoder(shell["payload"], Lp=alphabet + 1).run_ctx(rows, ctx).astype(np.int64)
    i = ctx.astype(np.int64)
    return rows[i, z].astype(np.uint32) | (rows[i, z + 1].astype(np.uint32) << 16)


def check_files(layer, data1, rep1, data2, rep2, leaves, depths, N):
    from scp_amd import attr, color, native
    mod = attr if layer == "attr" else color
    info = {}
    s1, s2 = mod.unpack(data1)[-1], mod.unpack(data2, info)[-1]
    assert info == dict(version=2, chunk=N) and data1[4] == 1 and rep2["chunk"] == N and "chunk" not in rep1
    assert rep2["bits"] == 8 * len(data2)
    coded = 0
    for k, (a, b, lv, D) in enumerate(zip(s1, s2, leaves, depths)):
        assert (a["D"], a["U"], a["root"], a["tables"]) == (b["D"], b["U"], b["root"], b["tables"])
        r1, r2 = rep1["shells"][k], rep2["shells"][k]
        if a["U"] < 2:
            assert "lengths" not in b and b["payload"] == b"" and "chunk" not in r2
            continue
        coded += 1
        lohi = host_pairs(layer, a, lv, D)
        want = [native.ac_encode_lohi(lohi[i:i + N]) for i in range(0, len(lohi), N)]
        assert native.ac_encode_lohi(lohi) == a["payload"]                   # the pairs are the ones the version-1 file was coded from
        assert b["lengths"].tolist() == [len(c) for c in want], (k, a["U"])
        assert b["payload"] == b"".join(want), (k, a["U"])
        C = len(want)
        assert (r2["chunk"], r2["chunks"]) == (N, C) and r2["bits"] == 8 * (4 * C + len(b["payload"])) and r1["bits"] == 8 * len(a["payload"])
        assert r2["chunk_overhead_bits"] == 8 * (4 * C + len(b["payload"]) - len(a["payload"])) and "chunk_overhead_bits" not in r1
        assert {kk: v for kk, v in r2.items() if not kk.startswith("chunk") and kk != "bits"} == {kk: v for kk, v in r1.items() if kk != "bits"}
    assert coded >= 3
    i1, i2 = {}, {}
    v1 = mod.decode_shells(data1, leaves, depths, i1)
    v2 = mod.decode_shells(data2, [lv.long() for lv in leaves], depths, i2)
    assert i1 == i2 and len(v1) == len(v2) == len(leaves)
    for x, y, d1, d2 in zip(v1, v2, rep1["decoded"], rep2["decoded"]):
        assert x.dtype == y.dtype == torch.uint8 and torch.equal(x, y) and torch.equal(d1, d2) and torch.equal(y, d2)
    return s2


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("layer", ["attr", "color"])
def test_hard_trees_code_to_the_host_coders_chunks_and_decode_to_the_version_1_values(layer, Q):
    from scp_amd import attr, color, native
    w = world(layer)
    data1, rep1 = encode(layer, w, Q)
    data2, rep2 = encode(layer, w, Q, chunk=N_CASES, want_overhead=True)
    s2 = check_files(layer, data1, rep1, data2, rep2, w["leaves"], w["depths"], N_CASES)
    assert max(len(s.get("lengths", ())) for s in s2) >= (60 if layer == "attr" else 190)      # more than one wave of chunks per shell
    data3, rep3 = encode(layer, w, Q, chunk=N_CASES)
    assert data3 == data2 and all("chunk_overhead_bits" not in r for r in rep3["shells"])      # the overhead costs a host coder run: only when asked
    mod = attr if layer == "attr" else color
    i, j = w["names"].index("heavy"), w["names"].index("random")
    swapped = list(w["leaves"])
    swapped[i], swapped[j] = swapped[j], swapped[i]
    with pytest.raises(native.ScpError, match="another stream"):
        mod.decode_shells(data2, swapped, w["depths"])
    with pytest.raises(native.ScpError, match="shells"):
        mod.decode_shells(data2, w["leaves"][:3], w["depths"][:3])


@pytest.mark.parametrize("Q", QS)
def test_multilevel_frame_through_the_frame_encoder(Q):
    m = multilevel_frame()
    enc = m["enc"]
    depths = [int(i.depth) for i in enc.geom.info]
    leaves = [up(k, np.int32).reshape(-1, 3) for k in m["kept"]]
    data1, rep1 = enc.encode_attr(m["x_dev"], m["r_dev"], Q)
    data2, rep2 = enc.encode_attr(m["x_dev"], m["r_dev"], Q, chunk=N_FRAME, want_overhead=True)
    check_files("attr", data1, rep1, data2, rep2, leaves, depths, N_FRAME)
    assert rep2["n_points"] == rep1["n_points"] and rep2["bits_per_point"] == rep2["bits"] / len(m["xyz"])


def test_colour_through_the_frame_encoder_and_bad_chunk_sizes():
    from scp_amd import cli, color, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_colors, synth_object
    from test_gpu_ringrate import ehem_model
    xyz = synth_object(3, 4096).astype(np.float32)
    rgb = synth_colors(xyz, 3)
    enc = FrameEncoder(ehem_model(), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev())
    q, _ = cli.obj_ints(xyz, "thing_vox10.ply", dev())
    enc.encode_ints([q], 0, 0.0, len(xyz))
    c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev()))
    leaves, depths = enc.attr_leaves(), [int(i.depth) for i in enc.geom.info]
    for Q in (1, 8):
        data1, rep1 = enc.encode_color(q, c, Q)
        data2, rep2 = enc.encode_color(q, c, Q, chunk=4096, want_overhead=True)
        # one shell here: check_files wants three coded shells, so the same checks by hand
        s1, s2 = color.unpack(data1)[1][0], color.unpack(data2)[1][0]
        lohi = host_pairs("color", s1, leaves[0], depths[0])
        want = [native.ac_encode_lohi(lohi[i:i + 4096]) for i in range(0, len(lohi), 4096)]
        assert len(want) == 3 and s2["lengths"].tolist() == [len(x) for x in want] and s2["payload"] == b"".join(want)
        assert torch.equal(color.decode_shells(data2, leaves, depths)[0], color.decode_shells(data1, leaves, depths)[0])
        assert torch.equal(rep2["decoded"][0], rep1["decoded"][0]) and rep2["shells"][0]["chunks"] == 3
        assert rep2["shells"][0]["chunk_overhead_bits"] == 8 * (12 + len(s2["payload"]) - len(s1["payload"])) > 0
    for bad in (63, (1 << 20) + 1):
        with pytest.raises(native.ScpError, match="64 .. 2\\^20"):
            enc.encode_color(q, c, 1, chunk=bad)
