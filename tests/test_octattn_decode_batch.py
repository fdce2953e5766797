"""The lockstep OctAttention decoder's host side (no device): the slot bookkeeping against the one-stream window rule, `--streams`
parsing, and the refusal of a batch before any decoding."""
import json

import pytest

from cfgs import octattn_cfg


def _alone(levels, cs, level_wise):
    """One stream decoded alone (OctAttnFrameDecoder.decode's loop): per node (level, index in the level, window, position, reset, pad)."""
    from scp_amd.decoder import octattn_window_of
    seq, r = [], 0
    for L, n in enumerate(levels, 1):
        if L == 1 or level_wise:
            r = 0
        for i in range(n):
            w, p = octattn_window_of(r, cs)
            reset = r == 0 or p == 0
            seq.append((L, i, w, p, reset, reset and w == 0))
            r += 1
    return seq


def _drive(files, slots, cs):
    """Drive OctAttnLockstep the way OctAttnBatchDecoder.decode does, with made-up level sizes -> (per file the nodes it visited, the
    (slot, file) assignments in the order they were made, the number of rows of every step)."""
    from scp_amd.decoder import OctAttnLockstep
    sched = OctAttnLockstep(len(files), slots, cs, [lw for _, lw in files])
    seen = [[] for _ in files]
    started = list(sched.refill())
    widths = []
    while sched.active():
        act = sched.active()
        rows = sched.step()
        assert tuple(r[0] for r in rows) == act
        widths.append(len(rows))
        for s, f, i, w, p, reset, pad in rows:
            seen[f].append((sched.L[s], i, w, p, reset, pad))
        ends = sched.level_ends()
        for s in ends:
            levels = files[sched.file[s]][0]
            assert sched.n[s] == levels[sched.L[s] - 1]
            if sched.L[s] == len(levels):
                sched.finish(s)
            else:
                sched.next_level(s, levels[sched.L[s]])
        if ends:
            started += sched.refill()
    return seen, started, widths


_TREES = [([1], False), ([1, 3, 9, 20, 11], False), ([1, 8, 40], True), ([1, 2, 4, 8, 16, 27, 30, 5], False), ([1, 5, 23, 7], True),
          ([1, 1, 1, 1], False), ([1, 6], True)]


@pytest.mark.parametrize("slots", [1, 2, 3, 7, 10])
@pytest.mark.parametrize("cs", [1, 4, 8, 1024])
def test_lockstep_visits_every_node_as_the_one_stream_decoder_does(slots, cs):
    """A one-node tree, levels larger than two windows (cs = 4, 8), level_wise on and off, more files than slots and more slots than
    files: per file the (level, node, window, position, reset, pad) sequence is the stream's own, every node exactly once."""
    seen, started, widths = _drive(_TREES, slots, cs)
    for f, (levels, lw) in enumerate(_TREES):
        assert seen[f] == _alone(levels, cs, lw), f
        assert len(seen[f]) == sum(levels)
    if cs in (4, 8):
        assert max(max(lv) for lv, _ in _TREES) > 2 * cs
    assert [f for _, f in started] == list(range(len(_TREES)))           # slots are refilled in file order
    assert [s for s, _ in started[:min(slots, len(_TREES))]] == list(range(min(slots, len(_TREES))))
    assert max(widths) == min(slots, len(_TREES)) and sum(widths) == sum(sum(lv) for lv, _ in _TREES)


def test_lockstep_keeps_rows_busy_until_the_queue_is_empty():
    """Five files on three slots: three rows per step until fewer than three files are left."""
    files = [([1, 4, 6], False), ([1, 2], False), ([1, 9, 9], True), ([1, 3], False), ([1, 5, 5, 5], False)]
    seen, started, widths = _drive(files, 3, 4)
    assert [f for _, f in started] == [0, 1, 2, 3, 4] and [s for s, _ in started] == [0, 1, 2, 1, 1]
    first_narrow = next(k for k, w in enumerate(widths) if w < 3)
    assert all(w < 3 for w in widths[first_narrow:]) and widths[-1] == 1
    # slot 1 runs file 1 (3 nodes), file 3 (4 nodes), then file 4: the queue is empty from step 7, and the first slot to fall idle is
    # slot 0, when file 0's 11 nodes are done
    assert first_narrow == 11 and len(widths) == 7 + 16


def test_streams_flag():
    from scp_amd.cli import get_decode_octattn_args
    assert get_decode_octattn_args([]).streams == 1
    assert get_decode_octattn_args(["--streams", "16"]).streams == 16
    assert get_decode_octattn_args(["--streams", "64"]).streams == 64
    for bad in ("0", "-1", "65", "x", "2.5"):
        with pytest.raises(SystemExit):
            get_decode_octattn_args(["--streams", bad])


class _Model:
    cfg = octattn_cfg()


def _write(tmp_path, name, **over):
    from scp_amd import native
    from scp_amd.decoder import SIDECAR
    side = dict(model="OctAttention", type="kitti", lidar_level=8, mullevel=False, spher=True, cylin=False, n_points=10, n_nodes=12,
                bin_nums=[100.0], z_offset=0.0, quant=None, profile=native.numeric_profile("OctAttention", None, decodable=True),
                context_size=_Model.cfg.model.context_size, level_wise=False, sequential=False, depth=8)
    side.update(over)
    p = tmp_path / name
    p.write_bytes(b"\x00" * 16)
    if over.get("no_side") is None:
        with open(str(p) + SIDECAR, "w") as f:
            json.dump(side, f)
    return str(p)


@pytest.mark.parametrize("over,match", [(dict(profile="octattn/1:x"), "--decodable"), (dict(no_side=True), "--decodable"),
                                        (dict(mullevel=True), "multi-level"), (dict(sequential=True), "--sequential"),
                                        (dict(context_size=512), "context size 512")],
                         ids=["default_profile", "no_side_info", "multi_level", "sequential", "context_size"])
def test_batch_with_one_undecodable_file_is_refused_before_decoding(tmp_path, monkeypatch, over, match):
    """The refusal names the file and comes before any decoder (or device) is touched: good files stand before and after the bad one."""
    from scp_amd import decoder, native
    good1, bad, good2 = _write(tmp_path, "a_8_100_0.bin"), _write(tmp_path, "b_8_100_0.bin", **over), _write(tmp_path, "c_8_100_0.bin")
    monkeypatch.setattr(decoder.OctAttnBatchDecoder, "__init__", lambda *a, **k: pytest.fail("a decoder was built"))
    with pytest.raises(native.ScpError, match=match) as e:
        decoder.decode_octattn_files([good1, bad, good2], _Model(), streams=2)
    assert "b_8_100_0.bin" in str(e.value)
    with pytest.raises(native.ScpError, match="streams"):
        decoder.decode_octattn_files([good1], _Model(), streams=0)
    assert decoder.decode_octattn_files([], _Model(), streams=4) == []
