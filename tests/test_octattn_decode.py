"""OctAttention decoder, host side (no GPU): window bookkeeping, the side-info fields of decodable streams, and the refusals that need
no device."""
import json
import types

import pytest

from scp_amd import native
from scp_amd.decoder import SIDECAR, _refuse_octattn, decode_octattn_file, octattn_chunks, octattn_window_of, read_sidecar, write_sidecar


def _rows(chunks, cs):
    """(chunk, window, position) of every node of a frame, by the encoder's rule: each chunk front-padded with cs - 1 rows and cut
    into consecutive windows of cs rows."""
    out = []
    for ci, n in enumerate(chunks):
        seq = [None] * (cs - 1) + list(range(n))
        for w in range(0, len(seq), cs):
            for p, r in enumerate(seq[w:w + cs]):
                if r is not None:
                    out.append((ci, w // cs, p))
    return out


@pytest.mark.parametrize("sizes,level_wise", [([1, 8, 40, 300], False), ([1, 8, 40, 300], True), ([1, 8, 1023, 1024], True),
                                              ([1, 2047], False), ([1], True), ([1, 7, 2048, 5], False), ([1024, 1024, 3], True)])
@pytest.mark.parametrize("cs", [1024, 4])
def test_window_of_every_node_follows_the_encoder(sizes, level_wise, cs):
    chunks = octattn_chunks(sizes, level_wise)
    assert sum(chunks) == sum(sizes) and len(chunks) == (len(sizes) if level_wise else 1)
    got = [(ci,) + octattn_window_of(r, cs) for ci, n in enumerate(chunks) for r in range(n)]
    assert got == _rows(chunks, cs)


def test_window_rule_edges():
    cs = 1024
    assert octattn_window_of(0, cs) == (0, cs - 1)          # the first node closes the pad window
    assert octattn_window_of(1, cs) == (1, 0)
    assert octattn_window_of(cs, cs) == (1, cs - 1)
    assert octattn_window_of(cs + 1, cs) == (2, 0)


def _enc(**kw):
    e = dict(data_type="kitti", lidar_level=10, mullevel=False, spher=True, cylin=False, context_size=1024, level_wise=False, decodable=True)
    e.update(kw)
    return types.SimpleNamespace(**e)


def _res(**kw):
    r = dict(n_points=100, n_nodes=321, bin_num=2001.0, z_offset=0.0, depth=10, sequential=False)
    r.update(kw)
    return r


def test_sidecar_round_trip_of_the_decodable_fields(tmp_path):
    out = str(tmp_path / "a.bin")
    side = write_sidecar(out, _enc(level_wise=True), _res(), "OctAttention")
    back = read_sidecar(out)
    assert back == json.loads(json.dumps(side))
    assert back["context_size"] == 1024 and back["level_wise"] is True and back["sequential"] is False and back["depth"] == 10
    assert back["profile"] == native.numeric_profile("OctAttention", decodable=True) and back["profile"].startswith("octattn/1d:")
    for k in ("model", "type", "lidar_level", "mullevel", "spher", "cylin", "n_points", "n_nodes", "bin_nums", "z_offset", "quant", "profile"):
        assert k in back                                     # the existing keys are all still there
    _refuse_octattn(out, back)                               # a decodable stream passes the checks


def test_profiles_differ():
    assert native.numeric_profile("OctAttention") != native.numeric_profile("OctAttention", decodable=True)
    assert native.numeric_profile("OctAttention").startswith("octattn/1:")


def test_ehem_sidecar_has_no_octattn_fields(tmp_path):
    out = str(tmp_path / "e.bin")
    side = write_sidecar(out, types.SimpleNamespace(data_type="kitti", lidar_level=12, mullevel=False, spher=True, cylin=False), _res(), "EHEM")
    assert "context_size" not in side and "level_wise" not in side and "sequential" not in side


@pytest.mark.parametrize("case,msg", [("none", "--decodable"), ("default", "--decodable"), ("sequential", "--sequential"),
                                      ("mullevel", "multi-level"), ("ehem", "not OctAttention")])
def test_refusals_without_a_gpu(tmp_path, case, msg):
    out = str(tmp_path / "s.bin")
    with open(out, "wb") as f:
        f.write(b"\x00" * 16)
    if case != "none":
        write_sidecar(out, _enc(mullevel=case == "mullevel", decodable=case != "default"), _res(sequential=case == "sequential"),
                      "EHEM" if case == "ehem" else "OctAttention")
    with pytest.raises(native.ScpError, match=msg):
        decode_octattn_file(out, model=None)


def test_decodable_flag_is_refused_where_it_does_not_apply():
    from scp_amd.cli import refuse_unsupported
    a = types.SimpleNamespace(spher_circle=False, level_wise=False, preproc_path="", metrics=False, type="kitti", spher=True, cylin=False,
                              sequential=False, decodable=True)
    refuse_unsupported(a, "OctAttention", False)
    with pytest.raises(native.ScpError, match="EHEM streams are decodable already"):
        refuse_unsupported(a, "EHEM", False)
    with pytest.raises(native.ScpError, match="multi-level"):
        refuse_unsupported(a, "OctAttention", True)
    a.sequential = True
    with pytest.raises(native.ScpError, match="--sequential"):
        refuse_unsupported(a, "OctAttention", False)
