"""OctAttention context model on MI355X (drop-in for models/oct_attention.py + models/attention_model.py).

`OctAttention(cfg).forward(data, pos)` with data int64 [B,c,4,3] = (occ, level, octant) x (ggp, gp, p, self) and
pos float32 [B,c,4,3] returns logits [B,c,255].  state_dict keys match the reference.
The dual-stream causal attention of attention_model.py:58-95 runs in one HIP kernel (csrc/octattn.hip); unlike
the reference, forward() is a pure function (it does not edit `data` in place, Appendix B-13).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import native
from .. import ops as _ops
from ..ops import linear as _linear

# False (tests only): the dense layers read fp32 rows and convert them in every tile (the round-2 form: identical bits)
PLANES = True


def linear(x, w, b=None, act=None, residual=None, scales=None):
    """OctAttention scales its embeddings by sqrt(600): the bf16x3 split (16-bit operands) leaves 1.8e-3 on the logits here, above
    the 1e-3 tolerance, so its dense layers run on the f16x3 kernel (22-bit operands, row scaled: the accuracy of an fp32 chain);
    the K = 12 position layer stays on the exact fp32 kernel."""
    return _linear(x, w, b, act=act, residual=residual, precise=True, scales=scales)


_KV_OFF = 640            # column of the value block inside the stacked key | value projection (600 rounded up to a multiple of 128)


def _kv_cat(a, D):
    """([2 * _KV_OFF, D] weight, [2 * _KV_OFF] bias) of the stacked key | value projection: rows [0, D) = key, [_KV_OFF, _KV_OFF + D) = value."""
    w = torch.zeros((2 * _KV_OFF, D), dtype=torch.float32, device=a.mlp_key.weight.device)
    b = torch.zeros((2 * _KV_OFF,), dtype=torch.float32, device=w.device)
    w[:D] = a.mlp_key.weight.detach()
    w[_KV_OFF:_KV_OFF + D] = a.mlp_value.weight.detach()
    b[:D] = a.mlp_key.bias.detach()
    b[_KV_OFF:_KV_OFF + D] = a.mlp_value.bias.detach()
    return w, b


class _PosEnc(nn.Module):
    def __init__(self, d_model, max_len):
        super().__init__()
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe)


class _Attn(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.mlp_key = nn.Linear(d, d)
        self.mlp_query = nn.Linear(d, d)
        self.mlp_value = nn.Linear(d, d)


class _Layer(nn.Module):
    def __init__(self, d, hid):
        super().__init__()
        self.attn = _Attn(d)
        self.linear1 = nn.Linear(d, hid)
        self.linear2 = nn.Linear(hid, d)
        self.norm1 = nn.LayerNorm(d, eps=1e-5)
        self.norm2 = nn.LayerNorm(d, eps=1e-5)


class _Transformer(nn.Module):
    def __init__(self, d, hid, n_layers, ctx):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(d, hid) for _ in range(n_layers)])
        self.position_enc = _PosEnc(d, ctx)


class OctAttention(nn.Module):
    def __init__(self, cfg, decodable=False):
        super().__init__()
        self.cfg = cfg
        m = cfg.model
        self.heads = m.head_num
        self.embed_dimension = 4 * (m.occ_embed_dim + m.level_embed_dim + m.octant_embed_dim + m.abs_pos_embed_dim)
        self.transformer_encoder = _Transformer(self.embed_dimension, m.hidden_dimension, m.layer_num, m.context_size)
        self.occ_enc = nn.Embedding(m.token_num + 1, m.occ_embed_dim)
        self.level_enc = nn.Embedding(m.max_octree_level + 1, m.level_embed_dim)
        self.octant_enc = nn.Embedding(9, m.octant_embed_dim)
        self.abs_pos_embed_dim = m.abs_pos_embed_dim
        if self.abs_pos_embed_dim:
            self.abs_pos_enc = nn.Linear(3, self.abs_pos_embed_dim)
        self.decoder0 = nn.Linear(self.embed_dimension, self.embed_dimension)
        self.decoder1 = nn.Linear(self.embed_dimension, m.token_num)
        mask = (torch.triu(torch.ones(m.context_size, m.context_size)) == 1).transpose(0, 1)
        self.register_buffer("mask", mask.float().masked_fill(mask == 0, float("-inf")).masked_fill(mask == 1, 0.0))
        # the numeric profile (native.numeric_profile): False = octattn/1 (the f16x3 attention with a launch-wide V scale, the default
        # encoder's bits); True = octattn/1d, the decodable profile: each logits row depends on its own window's rows 0..t only
        # (csrc/octattn_rowinv.hip), so OctAttnFrameDecoder can rebuild it one node at a time (OctAttnStepper)
        self.decodable = bool(decodable)
        self.eval()

    @classmethod
    def load_from_checkpoint(cls, path, cfg=None, map_location="cpu"):
        m = cls(cfg)
        sd = torch.load(path, map_location=map_location)
        m.load_state_dict(sd["state_dict"] if "state_dict" in sd else sd, strict=True)
        return m

    def _embed_torch(self, data, pos, cap):
        """The input stage as a sequence of torch index operations - the executable specification of csrc/octattn_embed.hip (tests
        compare the two bit for bit) and the path of the rows form (PLANES = False)."""
        B, c = data.shape[:2]
        data = data.long()
        occ, level, octant = data[..., 0], data[..., 1], data[..., 2]
        level = level - torch.clip(level[:, :, -1:] - cap, 0, None)           # oct_attention.py:57-61, out of place
        level = torch.clip(level, 0, self.cfg.model.max_octree_level)
        oe = F.embedding(occ, self.occ_enc.weight)
        ue = oe.clone()
        ue[:, :, -1] = self.occ_enc.weight[255]
        le = F.embedding(level, self.level_enc.weight)
        te = F.embedding(octant, self.octant_enc.weight)
        parts, parts_u = [oe, le, te], [ue, le, te]
        if self.abs_pos_embed_dim:
            pe = linear(pos, self.abs_pos_enc.weight, self.abs_pos_enc.bias)
            parts.append(pe)
            parts_u.append(pe)
        D = self.embed_dimension
        # both streams travel as one [2, B, c, D] tensor (0: known, 1: unknown): every layer they share runs as one launch
        E = torch.stack((torch.cat(parts, 3).reshape(B, c, D), torch.cat(parts_u, 3).reshape(B, c, D))) * math.sqrt(D)
        return E + self.transformer_encoder.position_enc.pe[:c]

    def profile_string(self):
        return native.numeric_profile("OctAttention", None, decodable=self.decodable)

    def _check_decodable(self, c=None):
        D = self.embed_dimension
        if not PLANES or D > _KV_OFF or D % 4 or D // self.heads > 152 or not self.abs_pos_embed_dim or \
                (c is not None and c > self.transformer_encoder.position_enc.pe.shape[0]):
            raise native.ScpError("the decodable OctAttention profile needs the planes path, embedding width <= 640 (a multiple of 4), head "
                                  "width <= 152, the position embedding and windows within the position table")

    @torch.no_grad()
    def forward(self, data, pos=None, capture_kv=None):
        """capture_kv (decodable profile only): a list that receives every layer's known-stream key | value projection [B, c, 1280]
        (key in columns [0, D), value in [640, 640 + D)) - the rows a decoder's cache holds (OctAttnStepper.prefill)."""
        if not data.is_cuda:
            raise native.ScpError("OctAttention runs on the MI355X only (no CPU fallback)")
        B, c = data.shape[:2]
        cap = 10 if self.cfg.train.type == "obj" else 12
        D = self.embed_dimension
        planes = PLANES
        n = B * c
        pa = None                                      # planes of E, when the kernel that produced E wrote them
        pe_tab = self.transformer_encoder.position_enc.pe
        dec = self.decodable
        if dec:
            self._check_decodable(c)
            if pos is None:
                raise native.ScpError("the decodable OctAttention profile needs positions")
        elif capture_kv is not None:
            raise native.ScpError("capture_kv: decodable profile only")
        if planes and D <= 768 and D % 4 == 0 and pos is not None and c <= pe_tab.shape[0]:
            # the whole input stage in ONE kernel (csrc/octattn_embed.hip): three embedding lookups x four ancestors, the position
            # Linear, concatenation, sqrt(D) scale, position table - both streams - and the f16x3 operand of the first dense layers
            ctx8 = data.reshape(n, 12)
            ctx8 = ctx8 if ctx8.dtype == torch.uint8 else ctx8.to(torch.uint8)
            ap = self.abs_pos_enc if self.abs_pos_embed_dim else None
            E, pa = native.octattn_embed(ctx8.contiguous(), pos.reshape(n, 4, 3).float().contiguous(), c, self.occ_enc.weight, self.level_enc.weight,
                                         self.octant_enc.weight, None if ap is None else ap.weight, None if ap is None else ap.bias, pe_tab, cap,
                                         self.cfg.model.max_octree_level)
            E = E.reshape(2, B, c, D)
        else:
            E = self._embed_torch(data, pos, cap)

        def lin(a, x, w, b, act=None, residual=None, rows=None, scales=None, row_max=None):
            if planes:
                return native.linear_split_f16(a if rows is None else a.rows(*rows), _ops._split16(w), b, _ops._ACT[act], residual, row_max=row_max)
            return linear(x, w, b, act=act, residual=residual, scales=scales)

        for lyr in self.transformer_encoder.layers:
            a = lyr.attn
            E2 = E.reshape(-1, D)
            rs = rsq = None
            if planes:
                if pa is None:                         # the embedding stage's output: one standalone pass
                    pa = native.SplitActF16(E2 if E2.is_contiguous() else E2.contiguous())
            elif E.is_contiguous():
                # the three projections read the same rows: one pass for their power-of-two row scales (the query takes the unknown stream's half)
                rs = native.RowScales(E2)
                rsq = rs.rows(n, 2 * n)
            if planes and D <= _KV_OFF:
                # key | value as ONE product (round 4): the two [600, 600] weights stacked with 40 zero rows behind each (N = 1280 = five
                # 256-wide tiles, 256 x 256 tile configuration - half the LDS fill per flop of the 128 x 128 one): 1 339 against 2 x 887 us
                # at M = 262 144 (tools/mb_oa_cfg.py); same products in the same k order: identical bits.  The attention kernels take the
                # two column slices with their row stride.
                wkv, bkv = _ops.derived(a, "kv_cat", [a.mlp_key.weight, a.mlp_key.bias, a.mlp_value.weight, a.mlp_value.bias], lambda: _kv_cat(a, D))
                # round 5: the maxima the next kernels scale by come out of the producing GEMM's epilogue (one zeroed buffer per layer): max |v| of the
                # known stream for the attention kernel's V planes, the row maxima of linear1's output for linear2 - no pass over either tensor
                mxw = torch.zeros(2 * n + 1, dtype=torch.int32, device=E.device)
                vmax, h1max = mxw[2 * n:], mxw[:2 * n]
                if dec:                                # no V scale at all: the row-invariant attention reads v in fp32
                    vmax = None
                    kv = native.linear_split_f16(pa, _ops._split16(wkv), bkv, cfg=1).reshape(2, B, c, wkv.shape[0])
                    if capture_kv is not None:
                        capture_kv.append(kv[0])
                else:
                    kv = native.linear_split_f16(pa, _ops._split16(wkv), bkv, cfg=1, col_max=(vmax, _KV_OFF, _KV_OFF + D, n)).reshape(2, B, c, wkv.shape[0])
                key, val = kv[..., :D], kv[..., _KV_OFF:_KV_OFF + D]
            else:
                vmax = h1max = None
                key = lin(pa, E, a.mlp_key.weight, a.mlp_key.bias, scales=rs).reshape(2, B, c, D)
                val = lin(pa, E, a.mlp_value.weight, a.mlp_value.bias, scales=rs).reshape(2, B, c, D)
            q_u = lin(pa, E[1], a.mlp_query.weight, a.mlp_query.bias, rows=(n, 2 * n), scales=rsq).reshape(B, c, D)
            att = torch.empty_like(E)
            if dec:
                native.octattn_attention_rowinv(q_u, key[0], val[0], self.heads, k_u=key[1], v_u=val[1], out=att[0], out_u=att[1])
            else:
                native.octattn_attention(q_u, key[0], key[1], val[0], val[1], self.heads, out=att[0], out_u=att[1], vmax=vmax)
            # norm(x + residual) in one pass; with `planes` the same pass writes the f16x3 operand of the layer that reads the result
            E, p1 = native.layernorm_add(att, E, lyr.norm1.weight, lyr.norm1.bias, 1e-5, planes=True) if planes else \
                (native.layernorm_add(att, E, lyr.norm1.weight, lyr.norm1.bias, 1e-5), None)
            h1 = lin(p1, E, lyr.linear1.weight, lyr.linear1.bias, act="relu", row_max=h1max)
            y2 = linear(h1, lyr.linear2.weight, lyr.linear2.bias, residual=E.reshape(h1.shape[:-1] + (D,)),
                        scales=None if h1max is None else native.RowScales.from_max(h1max)).reshape(E.shape)
            E, pa = native.layernorm_add(y2, None, lyr.norm2.weight, lyr.norm2.bias, 1e-5, planes=True) if planes else \
                (native.layernorm_add(y2, None, lyr.norm2.weight, lyr.norm2.bias, 1e-5), None)
        emu = E[1]
        if planes:
            d0 = native.linear_split_f16(pa.rows(n, 2 * n), _ops._split16(self.decoder0.weight), self.decoder0.bias, native.ACT_RELU)
            return linear(d0, self.decoder1.weight, self.decoder1.bias).reshape(B, c, -1)
        return linear(linear(emu, self.decoder0.weight, self.decoder0.bias, act="relu"), self.decoder1.weight, self.decoder1.bias)


def _pad_rows(n, device):
    """The front padding of a chunk (encoder._front): context rows (255, 0, 0) x 4, positions 0."""
    ctx = torch.zeros((n, 12), dtype=torch.uint8, device=device)
    ctx[:, 0::3] = 255
    return ctx, torch.zeros((n, 4, 3), dtype=torch.float32, device=device)


class OctAttnStepper:
    """Incremental evaluation of ONE window under the decodable profile (the decoder's hot path): per layer a cache of the known stream's
    key | value rows < t and the unknown stream's query of row t.  For the window's row t:
      unknown(ctx, pos) -> logits [1, 255]: the unknown stream (own occupancy unknown) through the three layers and the two decoder layers;
                           its attention reads the cached rows < t plus its own k_u, v_u;
      known(ctx, pos)   -> the known stream of row t (own occupancy decoded) through the layers: its key | value rows go into the cache,
                           its attention is q_u[t] (cached by `unknown`) against the cached rows <= t.  t advances by one.
    Every launch is the batched forward's kernel on one row and each of them is row-invariant, so each logits row is bit-identical to the
    same row of OctAttention.forward under the decodable profile (tests/test_gpu_octattn_decode.py)."""

    def __init__(self, model):
        model._check_decodable()
        if not model.decodable:
            raise native.ScpError("OctAttnStepper: the model runs the default (non-decodable) profile; set model.decodable = True")
        self.m = model
        p = next(model.parameters())
        self.device = p.device
        self.cs = model.cfg.model.context_size
        self.D = model.embed_dimension
        nl = len(model.transformer_encoder.layers)
        self.kv = torch.zeros((nl, self.cs, 2 * _KV_OFF), dtype=torch.float32, device=self.device)
        self.q = torch.zeros((nl, 1, self.D), dtype=torch.float32, device=self.device)
        self.h1max = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.t = 0

    def reset(self, pad):
        """Start a window: pad=True - the first window of a chunk, whose rows 0 .. cs - 2 are the front padding (their cache rows are the
        same for every chunk: computed once per model by a batched forward, then copied); pad=False - an empty window."""
        if pad and self.cs > 1:
            kv_pad = self.prefill_pad()
            self.kv[:, :self.cs - 1].copy_(kv_pad)
            self.t = self.cs - 1
        else:
            self.t = 0

    def prefill_pad(self):
        m = self.m

        def build():
            ctx, pos = _pad_rows(self.cs - 1, self.device)
            cap = []
            m(ctx.reshape(1, -1, 4, 3), pos.reshape(1, -1, 4, 3), capture_kv=cap)
            return torch.stack([k[0] for k in cap])
        return _ops.derived(m, "decodable_pad_kv", list(m.parameters()) + list(m.buffers()), build)

    def _embed(self, ctx, pos):
        m, t = self.m, self.t
        ap = m.abs_pos_enc
        cap = 10 if m.cfg.train.type == "obj" else 12
        pe = m.transformer_encoder.position_enc.pe[t:t + 1]
        return native.octattn_embed(ctx, pos, 1, m.occ_enc.weight, m.level_enc.weight, m.octant_enc.weight, ap.weight, ap.bias, pe, cap,
                                    m.cfg.model.max_octree_level)

    def _kv(self, lyr):
        a = lyr.attn
        return _ops.derived(a, "kv_cat", [a.mlp_key.weight, a.mlp_key.bias, a.mlp_value.weight, a.mlp_value.bias], lambda: _kv_cat(a, self.D))

    def _ffn(self, lyr, att, E):
        """norm1(att + E) -> linear1 / ReLU -> linear2 + residual -> norm2: the batched forward's launches on one row."""
        E, p1 = native.layernorm_add(att, E, lyr.norm1.weight, lyr.norm1.bias, 1e-5, planes=True)
        self.h1max.zero_()
        h1 = native.linear_split_f16(p1, _ops._split16(lyr.linear1.weight), lyr.linear1.bias, native.ACT_RELU, None, row_max=self.h1max)
        y2 = linear(h1, lyr.linear2.weight, lyr.linear2.bias, residual=E, scales=native.RowScales.from_max(self.h1max))
        return native.layernorm_add(y2, None, lyr.norm2.weight, lyr.norm2.bias, 1e-5, planes=True)

    @torch.no_grad()
    def unknown(self, ctx, pos):
        """ctx uint8 [1, 12], pos float32 [1, 4, 3] of the window's row t (own occupancy: any value) -> logits float32 [1, 255]."""
        if self.t >= self.cs:
            raise native.ScpError("OctAttnStepper: the window is full (reset it)")
        m, D, t = self.m, self.D, self.t
        E2, pa2 = self._embed(ctx, pos)
        E, pa = E2[1], pa2.rows(1, 2)
        for l, lyr in enumerate(m.transformer_encoder.layers):
            a = lyr.attn
            wkv, bkv = self._kv(lyr)
            kvu = native.linear_split_f16(pa, _ops._split16(wkv), bkv, cfg=1)
            native.linear_split_f16(pa, _ops._split16(a.mlp_query.weight), a.mlp_query.bias, native.ACT_NONE, None, out=self.q[l])
            att = torch.empty((1, D), dtype=torch.float32, device=self.device)
            native.octattn_attention_rowinv(self.q[l], self.kv[l, :, :D], self.kv[l, :, _KV_OFF:_KV_OFF + D], m.heads, k_u=kvu[:, :D],
                                            v_u=kvu[:, _KV_OFF:_KV_OFF + D], out_u=att, q0=t, q1=t + 1, qoff=t)
            E, pa = self._ffn(lyr, att, E)
        d0 = native.linear_split_f16(pa, _ops._split16(m.decoder0.weight), m.decoder0.bias, native.ACT_RELU)
        return linear(d0, m.decoder1.weight, m.decoder1.bias)

    @torch.no_grad()
    def known(self, ctx, pos):
        """The same row with its own occupancy decoded (ctx[0, 9]): its key | value rows join the cache; t advances."""
        m, D, t = self.m, self.D, self.t
        E2, pa2 = self._embed(ctx, pos)
        E, pa = E2[0], pa2.rows(0, 1)
        layers = m.transformer_encoder.layers
        for l, lyr in enumerate(layers):
            wkv, bkv = self._kv(lyr)
            native.linear_split_f16(pa, _ops._split16(wkv), bkv, cfg=1, out=self.kv[l, t:t + 1])
            if l == len(layers) - 1:                   # the last layer's known stream feeds nothing
                break
            att = torch.empty((1, D), dtype=torch.float32, device=self.device)
            native.octattn_attention_rowinv(self.q[l], self.kv[l, :, :D], self.kv[l, :, _KV_OFF:_KV_OFF + D], m.heads, out=att, q0=t, q1=t + 1,
                                            qoff=t)
            E, pa = self._ffn(lyr, att, E)
        self.t = t + 1


class OctAttnBatchStepper(OctAttnStepper):
    """OctAttnStepper for `slots` independent windows, stepped together: a call takes the slots it serves (`slot_ids`, B of them) and one
    row per slot - row b is row t[slot_ids[b]] of that slot's window.  Every dense launch is the batched forward's kernel on B rows
    (they are row-invariant: per-row scales, tile picked by N alone); the attention is the one-row-per-stream kernel
    (native.octattn_attention_rowinv_step), which reads each row's position and cache slot from device arrays.  So the launch count of
    a call does not depend on B, no call waits for the device, and the logits row of slot s at row t is bit-identical to that row of
    OctAttention.forward under the decodable profile whatever the other slots hold or do.
    State: cache [slots, layers, cs, 1280], the unknown stream's query per layer [slots, D], t int32 [slots] on the device (`t_dev`)
    with a host mirror (`t`)."""

    def __init__(self, model, slots):
        model._check_decodable()
        if not model.decodable:
            raise native.ScpError("OctAttnBatchStepper: the model runs the default (non-decodable) profile; set model.decodable = True")
        if slots < 1:
            raise native.ScpError("OctAttnBatchStepper: at least one slot")
        self.m = model
        self.device = next(model.parameters()).device
        self.cs = model.cfg.model.context_size
        if self.cs > 1024:
            raise native.ScpError("OctAttnBatchStepper: windows of at most 1024 rows (the step kernel keeps a row's scores in LDS)")
        self.D = model.embed_dimension
        self.slots = int(slots)
        self.nl = len(model.transformer_encoder.layers)
        dev = self.device
        self.kv = torch.zeros((self.slots, self.nl, self.cs, 2 * _KV_OFF), dtype=torch.float32, device=dev)
        self._kv_rows = self.kv.view(-1, 2 * _KV_OFF)
        self.q = torch.zeros((self.nl, self.slots, self.D), dtype=torch.float32, device=dev)
        self.h1max = torch.zeros((self.slots,), dtype=torch.int32, device=dev)
        self.t_dev = torch.zeros((self.slots,), dtype=torch.int32, device=dev)
        self.t = [0] * self.slots
        self._ones = torch.ones((self.slots,), dtype=torch.int32, device=dev)
        self._ids = {}

    def _slot_ids(self, slot_ids):
        """slot_ids (a sequence of distinct slot numbers) -> (the tuple, int32 and int64 device tensors).  The tensors are made once per
        distinct tuple (one small host-to-device copy), so a decoder that serves the same set of slots step after step uploads nothing."""
        key = tuple(int(s) for s in slot_ids)
        ent = self._ids.get(key)
        if ent is None:
            if not key or len(set(key)) != len(key) or min(key) < 0 or max(key) >= self.slots:
                raise native.ScpError(f"OctAttnBatchStepper: slot ids {key} are not distinct slots of 0 .. {self.slots - 1}")
            i64 = torch.tensor(key, dtype=torch.int64, device=self.device)
            ent = self._ids[key] = (key, i64.to(torch.int32), i64)
        return ent

    def reset(self, slot_ids, pad):
        """Start a window in each of the slots (OctAttnStepper.reset)."""
        key, _, i64 = self._slot_ids(slot_ids)
        t = 0
        if pad and self.cs > 1:
            kv_pad = self.prefill_pad()
            for s in key:
                self.kv[s, :, :self.cs - 1].copy_(kv_pad)
            t = self.cs - 1
        self.t_dev.index_fill_(0, i64, t)
        for s in key:
            self.t[s] = t

    def _embed(self, ctx, pos, ts):
        # scp_octattn_embed takes row r's position-table row as pe[r % c]: the table rows gathered by t with c = B give every row its own
        m, B = self.m, ctx.shape[0]
        ap = m.abs_pos_enc
        cap = 10 if m.cfg.train.type == "obj" else 12
        pe = m.transformer_encoder.position_enc.pe.index_select(0, ts)
        return native.octattn_embed(ctx, pos, B, m.occ_enc.weight, m.level_enc.weight, m.octant_enc.weight, ap.weight, ap.bias, pe, cap,
                                    m.cfg.model.max_octree_level)

    def _ffn(self, lyr, att, E):
        B = att.shape[0]
        h1max = self.h1max[:B]
        E, p1 = native.layernorm_add(att, E, lyr.norm1.weight, lyr.norm1.bias, 1e-5, planes=True)
        h1max.zero_()
        h1 = native.linear_split_f16(p1, _ops._split16(lyr.linear1.weight), lyr.linear1.bias, native.ACT_RELU, None, row_max=h1max)
        y2 = linear(h1, lyr.linear2.weight, lyr.linear2.bias, residual=E, scales=native.RowScales.from_max(h1max))
        return native.layernorm_add(y2, None, lyr.norm2.weight, lyr.norm2.bias, 1e-5, planes=True)

    def _rows(self, slot_ids, ctx, pos):
        ent = self._slot_ids(slot_ids)
        B = len(ent[0])
        if ctx.shape != (B, 12) or pos.shape != (B, 4, 3):
            raise native.ScpError(f"OctAttnBatchStepper: ctx [{B}, 12] and pos [{B}, 4, 3] expected (one row per slot)")
        return ent + (B,)

    @torch.no_grad()
    def unknown(self, slot_ids, ctx, pos):
        """ctx uint8 [B, 12], pos float32 [B, 4, 3]: row b = row t of slot slot_ids[b]'s window -> logits float32 [B, 255]."""
        key, i32, i64, B = self._rows(slot_ids, ctx, pos)
        if any(self.t[s] >= self.cs for s in key):
            raise native.ScpError("OctAttnBatchStepper: a window is full (reset it)")
        m, D = self.m, self.D
        E2, pa2 = self._embed(ctx, pos, self.t_dev.index_select(0, i64))
        E, pa = E2[1], pa2.rows(B, 2 * B)
        for l, lyr in enumerate(m.transformer_encoder.layers):
            a = lyr.attn
            wkv, bkv = self._kv(lyr)
            kvu = native.linear_split_f16(pa, _ops._split16(wkv), bkv, cfg=1)
            q = native.linear_split_f16(pa, _ops._split16(a.mlp_query.weight), a.mlp_query.bias, native.ACT_NONE, None)
            self.q[l].index_copy_(0, i64, q)
            att = torch.empty((B, D), dtype=torch.float32, device=self.device)
            native.octattn_attention_rowinv_step(q, self.kv[:, l, :, :D], self.kv[:, l, :, _KV_OFF:_KV_OFF + D], self.t_dev, i32, m.heads,
                                                 k_u=kvu[:, :D], v_u=kvu[:, _KV_OFF:_KV_OFF + D], out_u=att)
            E, pa = self._ffn(lyr, att, E)
        d0 = native.linear_split_f16(pa, _ops._split16(m.decoder0.weight), m.decoder0.bias, native.ACT_RELU)
        return linear(d0, m.decoder1.weight, m.decoder1.bias)

    @torch.no_grad()
    def known(self, slot_ids, ctx, pos):
        """The same rows with their own occupancy decoded (ctx[:, 9]): row b's key | value rows go into row t of ITS slot's cache; the
        t of every slot served advances by one."""
        key, i32, i64, B = self._rows(slot_ids, ctx, pos)
        m, D = self.m, self.D
        ts = self.t_dev.index_select(0, i64)
        E2, pa2 = self._embed(ctx, pos, ts)
        E, pa = E2[0], pa2.rows(0, B)
        row = i64 * (self.nl * self.cs) + ts                # cache row of (slot, layer 0, t) in the [slots * layers * cs, 1280] view
        layers = m.transformer_encoder.layers
        for l, lyr in enumerate(layers):
            wkv, bkv = self._kv(lyr)
            kvk = native.linear_split_f16(pa, _ops._split16(wkv), bkv, cfg=1)
            self._kv_rows.index_copy_(0, row + l * self.cs, kvk)
            if l == len(layers) - 1:                   # the last layer's known stream feeds nothing
                break
            att = torch.empty((B, D), dtype=torch.float32, device=self.device)
            native.octattn_attention_rowinv_step(self.q[l].index_select(0, i64), self.kv[:, l, :, :D], self.kv[:, l, :, _KV_OFF:_KV_OFF + D],
                                                 self.t_dev, i32, m.heads, out=att)
            E, pa = self._ffn(lyr, att, E)
        self.t_dev.index_add_(0, i64, self._ones[:B])
        for s in key:
            self.t[s] += 1
