"""The coding tail of a frame - everything between "the logits table exists" and "the result dict is returned" ("The coding
tail") - seen from outside: public entry points of both encoders, and recorders around the functions of scp_amd.native the tail launches.
With every option on, all entry points write the same stream and the same entries; the launches come in the one order the stream format
allows; an option that is off launches nothing; a batch hands every frame its own entries.

Nothing here knows how the encoders are organised inside: the file passes unchanged on the commit before the tail became one function."""
from types import SimpleNamespace

import pytest
import torch

from cfgs import octattn_cfg
from test_gpu_ringlod import GENERAL
from test_gpu_ringrate import dev, ehem_model
from test_gpu_temper import CONFIGS, frames

pytestmark = pytest.mark.gpu

TAIL = ("force_rows", "temper_sweep", "temper_choose", "scale_rows", "softmax_cdf", "rate_segments")
OPTIONS = ("rate", "temper", "ring_lod")
ZERO_DROPS = (GENERAL[0], (0, 0, 0))
_SHARED = {}


def ehem(mullevel, level, **kw):
    from scp_amd.encoder import FrameEncoder
    return FrameEncoder(ehem_model(), "kitti", level, spher=True, mullevel=mullevel, device=dev(), **kw)


def octattn(**kw):
    from scp_amd.encoder import OctAttnFrameEncoder
    from scp_amd.models import OctAttention
    from scp_amd.weights import fill_weights
    if "octattn" not in _SHARED:
        _SHARED["octattn"] = fill_weights(OctAttention(octattn_cfg()), 0).to(dev())
    return OctAttnFrameEncoder(_SHARED["octattn"], "kitti", 12, spher=True, device=dev(), **kw)


def third_frame():
    """The OctAttention frame of test_gpu_temper, and the third frame of a batch: a further seed at the subsampling of `frames()`."""
    from scp_amd.synth import synth_frame
    if "third" not in _SHARED:
        _SHARED["third"] = synth_frame(6)[::30].copy()
    return _SHARED["third"]


def record_tail(monkeypatch):
    """Wrap the six launches of the tail; every wrapper notes its name and calls through.  -> the list of names, in call order."""
    from scp_amd import native
    calls = []

    def wrap(name, fn):
        def recorder(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return recorder

    for name in TAIL:
        monkeypatch.setattr(native, name, wrap(name, getattr(native, name)))
    return calls


def recorded(calls, fn):
    """fn() -> (its result, the launches it made)."""
    calls.clear()
    res = fn()
    return res, list(calls)


def ints_of(enc, xyz):
    """encode_ints from the encoder's own device quantiser, with the infos the integers were made with."""
    qs, bin_num, z_off = enc.quantize(torch.from_numpy(xyz).to(dev()))
    infos = [SimpleNamespace(**q) for q in enc.quant_info()]
    return enc.encode_ints(qs, bin_num, z_off, len(xyz), infos=infos)


def ehem_entry_points(enc, a, b):
    """Every way a FrameEncoder codes the frames a and b -> name: [result of a, result of b]."""
    return {"encode": [enc.encode(a), enc.encode(b)],
            "encode_ints": [ints_of(enc, a), ints_of(enc, b)],
            "encode_async": [enc.finish(h) for h in [enc.encode_async(a), enc.encode_async(b)]],
            "front_async": [enc.finish(enc.encode_async(x, front=enc.front_async(x))) for x in (a, b)],
            "encode_batch_async": enc.finish_batch(enc.encode_batch_async([a, b]))}


# ------------------------------------------------------------------------------------------------------------------ 1. all options at once
@pytest.mark.parametrize("mullevel,level", CONFIGS)
def test_all_options_at_once_give_one_stream_and_one_set_of_entries_on_every_entry_point(mullevel, level):
    a, b = frames()
    enc = ehem(mullevel, level, rate=True, temper="code", ring_lod=GENERAL)
    got = ehem_entry_points(enc, a, b)
    want = got["encode"]
    assert want[0]["bytes"] != want[1]["bytes"] and all(len(w["bytes"]) > 100 for w in want)
    for w in want:
        assert w["temper"]["mode"] == "code" and w["ring_lod"]["implied_rows"] > 0 and w["rate"]["bad_rows"] == 0
    for name, res in got.items():
        assert len(res) == 2
        for r, w in zip(res, want):
            assert r["bytes"] == w["bytes"], name
            for key in OPTIONS:
                assert r[key] == w[key], (name, key)                              # dicts of plain numbers: bit-identical floats


# ------------------------------------------------------------------------------------------------------------------ 2. the order
@pytest.mark.parametrize("temper", ["code", "report"])
def test_the_tail_launches_force_temper_cdf_rate_in_that_order(temper, monkeypatch):
    a, b = frames()
    enc = ehem(False, 12, rate=True, temper=temper, ring_lod=GENERAL)
    calls = record_tail(monkeypatch)
    want = [n for n in TAIL if temper == "code" or n != "scale_rows"]
    one, seq = recorded(calls, lambda: enc.encode(a))
    assert seq == want
    asy, seq = recorded(calls, lambda: enc.finish(enc.encode_async(a)))
    assert seq == want and asy["bytes"] == one["bytes"]
    bat, seq = recorded(calls, lambda: enc.finish_batch(enc.encode_batch_async([a, b])))
    assert seq == want and bat[0]["bytes"] == one["bytes"]


def test_the_octattention_tail_launches_temper_cdf_rate_in_that_order(monkeypatch):
    xyz = third_frame()
    enc = octattn(rate=True, temper="report")
    calls = record_tail(monkeypatch)
    want = ["temper_sweep", "temper_choose", "softmax_cdf", "rate_segments"]
    one, seq = recorded(calls, lambda: enc.encode(xyz))
    assert seq == want
    asy, seq = recorded(calls, lambda: enc.finish(enc.encode_async(xyz)))
    assert seq == want and asy["bytes"] == one["bytes"] and asy["rate"] == one["rate"] and asy["temper"] == one["temper"]


# ------------------------------------------------------------------------------------------------------------------ 3. options off
@pytest.mark.parametrize("mullevel,level", CONFIGS)
def test_a_plain_ehem_encoder_launches_the_cdf_alone_and_reports_nothing(mullevel, level, monkeypatch):
    a, b = frames()
    off = ehem_entry_points(ehem(mullevel, level, temper=None, ring_lod=ZERO_DROPS), a, b)
    enc = ehem(mullevel, level)
    calls = record_tail(monkeypatch)
    for name, fn in (("encode", lambda: [enc.encode(a), enc.encode(b)]),
                     ("encode_ints", lambda: [ints_of(enc, a), ints_of(enc, b)]),
                     ("encode_async", lambda: [enc.finish(h) for h in [enc.encode_async(a), enc.encode_async(b)]]),
                     ("front_async", lambda: [enc.finish(enc.encode_async(x, front=enc.front_async(x))) for x in (a, b)])):
        res, seq = recorded(calls, fn)
        assert seq == ["softmax_cdf", "softmax_cdf"], name
        assert [r["bytes"] for r in res] == [o["bytes"] for o in off[name]] and not any(k in r for r in res for k in OPTIONS), name
    res, seq = recorded(calls, lambda: enc.finish_batch(enc.encode_batch_async([a, b])))
    assert seq == ["softmax_cdf"]
    assert [r["bytes"] for r in res] == [o["bytes"] for o in off["encode_batch_async"]] and not any(k in r for r in res for k in OPTIONS)
    assert res[0]["bytes"] == off["encode"][0]["bytes"] != res[1]["bytes"]


def test_a_plain_octattention_encoder_launches_the_cdf_alone_and_reports_nothing(monkeypatch):
    xyz = third_frame()
    same = octattn(temper=None, ring_lod=ZERO_DROPS)
    off = [same.encode(xyz), same.finish(same.encode_async(xyz))]
    enc = octattn()
    calls = record_tail(monkeypatch)
    for fn, o in ((lambda: enc.encode(xyz), off[0]), (lambda: enc.finish(enc.encode_async(xyz)), off[1])):
        res, seq = recorded(calls, fn)
        assert seq == ["softmax_cdf"]
        assert res["bytes"] == o["bytes"] == off[0]["bytes"] and len(res["bytes"]) > 100 and not any(k in res for k in OPTIONS)


# ------------------------------------------------------------------------------------------------------------------ 4. the cuts of a batch
@pytest.mark.parametrize("option,kw", [("rate", dict(rate=True)), ("temper", dict(temper="report")), ("ring_lod", dict(ring_lod=GENERAL))])
@pytest.mark.parametrize("mullevel,level", CONFIGS)
def test_each_option_alone_is_cut_per_frame_in_a_batch_of_three(mullevel, level, option, kw):
    three = frames() + [third_frame()]
    enc = ehem(mullevel, level, **kw)
    want = [enc.encode(f) for f in three]
    # three frames of different sizes: the middle frame's cuts have neither end at 0 nor at the total
    assert len({w["n_nodes"] for w in want}) == 3 and len({tuple(w["level_sizes"]) for w in want}) == 3
    got = enc.finish_batch(enc.encode_batch_async(three))
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g["bytes"] == w["bytes"] and g[option] == w[option]
        assert not any(k in g for k in OPTIONS if k != option)
