"""The attention output reaches scp_swin_post_attn in the FRAGMENT ORDER of the post-attention kernels (include/scp.h: SCP_LDO_FRAG; per
128-row tile and plane [32 chunks of 8 channels][128 rows][8 bf16]) instead of rows.  The hand-over moves bytes, it computes nothing: every
test here asserts BIT equality against the row-major hand-over (native.set_attn_o("rows") / SCP_ATTN_O=rows)."""
import numpy as np
import pytest
import torch

from cfgs import ehem_cfg
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from scp_amd import native
    native.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ehem(dev):
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    return fill_weights(EHEM(ehem_cfg()), 0).to(dev)


@pytest.fixture(scope="module")
def pw(dev):
    from scp_amd import native
    g = torch.Generator().manual_seed(21)
    rn = lambda *sh, s=1.0: (torch.randn(sh, generator=g) * s).to(dev)
    return native.PostAttnWeights(rn(256, 256, s=0.05), rn(256, s=0.1), 1 + rn(256, s=0.1), rn(256, s=0.1), rn(1024, 256, s=0.05), rn(1024, s=0.1),
                                  rn(256, 1024, s=0.03), rn(256, s=0.1))


def _wtab(lps, dev):
    rows, base = [], 0
    for lp in lps:
        rows += [[base, lp]] * (lp // 512)
        base += lp
    return torch.tensor(rows, dtype=torch.int32, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16)


# (padded sequence lengths, shift, real lengths or None): one window; two sequences, unshifted and shifted; a `valid` vector whose second
# sequence (520 real rows of 1024) leaves the query tiles 640.. of its run pure padding - one of them wraps under the shift
CASES = [([512], 0, None), ([512, 1536], 0, None), ([512, 1536], 256, None), ([512, 1024], 0, [512, 520]), ([512, 1024], 256, [512, 520])]


@pytest.mark.parametrize("lps,shift,real", CASES)
def test_attention_planes_and_post_attn_equal_the_row_major_hand_over(dev, pw, lps, shift, real):
    """The o planes written in fragment order, un-permuted on the host, are the row-major planes element for element (rows of skipped
    padding tiles excepted: nobody writes them), and scp_swin_post_attn gives the same rows from either - whole launch and tile list."""
    from scp_amd import native
    g = torch.Generator().manual_seed(100 * len(lps) + shift + (7 if real else 0))
    T = sum(lps)
    qkv = (torch.randn((T, 768), generator=g) * 2.0).to(dev)
    table = (torch.randn((1023, 4), generator=g) * 0.5).to(dev)
    x = torch.randn((T, 256), generator=g).to(dev)
    wtab = _wtab(lps, dev)
    kv = native.KvPlanes(qkv[:, 256:512], qkv[:, 512:])
    valid = None
    written = torch.ones(T, dtype=torch.bool, device=dev)
    if real:
        valid = torch.zeros(T, device=dev)
        base = 0
        for c, lp in zip(real, lps):
            valid[base:base + c] = 1.0
            base += lp
        # a query tile is skipped iff its first row is padding (real rows are a prefix of a sequence's run)
        written = (valid.view(-1, 128)[:, 0] != 0).repeat_interleave(128)
        assert int((~written).sum()) >= 128
    rows = native.swin_attention_packed_planes(qkv[:, :256], kv, table, wtab, shift, split=True, valid=valid)
    frag = native.swin_attention_packed_planes(qkv[:, :256], kv, table, wtab, shift, split="frag", valid=valid)
    assert isinstance(frag, native.FragAct) and frag.t.shape == (2, T // 128, 32, 128, 8)
    back = frag.rows()
    assert torch.equal(_bits(back.t[:, written]), _bits(rows.t[:, written, :256]))
    # the host permutation is its own inverse pair
    assert torch.equal(_bits(native.FragAct.from_rows(back).t), _bits(frag.t))
    # post-attention on both forms (unwritten rows made equal first: they are don't-care inputs of don't-care rows)
    rows.t[:, ~written] = 0
    frag = native.FragAct.from_rows(rows)
    tiles = torch.arange(T // 128, dtype=torch.int32, device=dev)
    tiles = torch.cat((tiles[:2], tiles[3:])).contiguous()                      # tile 2 omitted
    L = native.lib()
    try:
        for wide in (0, 1):                                                     # the chain kernel and the wide kernel (launches this short run the latter)
            L.scp_rc_set_wide(wide)
            want = native.swin_post_attn(rows, x, pw)
            assert torch.equal(native.swin_post_attn(frag, x, pw), want), wide
            xa, xb = x.clone(), x.clone()
            native.swin_post_attn(rows, xa, pw, out=xa, tiles=tiles)
            native.swin_post_attn(frag, xb, pw, out=xb, tiles=tiles)
            assert torch.equal(xa, xb) and torch.equal(xb[256:384], x[256:384]) and torch.equal(xb[:256], want[:256]), wide
    finally:
        L.scp_rc_set_wide(-1)


@pytest.mark.parametrize("M", [1, 33, 512])
def test_wide_and_chain_kernels_read_fragment_order(dev, pw, M):
    """Both post-attention kernels (the decoder's wide kernel, the chain kernel) on fragment-ordered planes: the row-major result, ragged
    last tile included (rows behind M are never read as rows: the kernels repeat row M - 1)."""
    from scp_amd import native
    L = native.lib()
    g = torch.Generator().manual_seed(M)
    x, o = torch.randn((M, 256), generator=g).to(dev) * 2.0, torch.randn((M, 256), generator=g).to(dev)
    rows = native.split_rows(o)
    frag = native.FragAct.from_rows(rows)
    try:
        for wide in (1, 0):
            L.scp_rc_set_wide(wide)
            want = native.swin_post_attn(rows, x, pw)
            assert torch.equal(native.swin_post_attn(frag, x, pw), want), wide
            xc = x.clone()
            assert native.swin_post_attn(frag, xc, pw, out=xc) is xc and torch.equal(xc, want), wide
    finally:
        L.scp_rc_set_wide(-1)


def test_packed_forward_is_identical_under_both_hand_overs(dev, ehem):
    from scp_amd import native
    z = golden("logits_ehem_b2_c256")
    data, pos = torch.from_numpy(z["data"].astype(np.int64)), torch.from_numpy(z["pos"])
    if data.dim() == 3:
        data, pos = data[None], pos[None]
    B, c = data.shape[:2]
    ctx = data.reshape(B * c, 12).to(torch.uint8).to(dev)
    p = pos.transpose(1, 2).reshape(B * c, 3).contiguous().to(dev)
    out = {}
    prev = native.set_attn_o("frag")
    try:
        for mode in ("frag", "rows"):
            native.set_attn_o(mode)
            ev, od = ehem.forward_packed(ctx, p, [c] * B)
            out[mode] = (ev.clone(), od.clone())
    finally:
        native.set_attn_o(prev)
    assert torch.equal(out["frag"][0], out["rows"][0]) and torch.equal(out["frag"][1], out["rows"][1])
    assert bool(torch.isfinite(out["frag"][0]).all())


def test_short_frame_round_trip_is_byte_identical_under_both_hand_overs(dev, ehem):
    """One short multi-level frame through the encoder and the decoder under each hand-over: the same bytes, the same numeric profile, the
    same decoded occupancy codes."""
    from scp_amd import native
    from scp_amd.decoder import FrameDecoder
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    xyz = synth_frame(4)[::60].copy()                       # 2000 points
    got = {}
    prev = native.set_attn_o("frag")
    try:
        for mode in ("frag", "rows"):
            native.set_attn_o(mode)
            enc = FrameEncoder(ehem, "kitti", 12, spher=True, mullevel=True, device=dev)
            res = enc.encode(xyz)
            dec = FrameDecoder(ehem, 12, mullevel=True, polar=True, device=dev)
            shells = dec.decode(res["bytes"], res["n_levels"], res["pos_mm"])
            got[mode] = (res["bytes"], [torch.cat(codes).cpu().numpy() for codes, _ in shells], native.numeric_profile("EHEM"))
    finally:
        native.set_attn_o(prev)
    a, b = got["frag"], got["rows"]
    assert a[0] == b[0] and a[2] == b[2]
    assert len(a[1]) == len(b[1]) == 3 and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))
