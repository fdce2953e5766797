"""Frame decoder: bitstream -> occupancy codes -> quantised points, the inverse of scp_amd/encoder.py.

Counterpart of decode_ehem.py:56-189 / decode_ehem_mullevel.py:56-189.  The octree is regenerated breadth first: the nodes of
level L+1 are the set children of level L in (parent order, child digit) = Morton order, so context rows and node origins are
known before their occupancy symbol is decoded.  Per window of <= 8192 nodes the model runs in two phases (EHEM.decode):
even-node logits -> decode the even symbols -> odd-node logits given them -> decode the odd symbols; the integer CDFs come
from the same device kernel the encoder used (csrc/cdf.hip) and the symbols from the host range decoder (csrc/rangecoder.cpp).
Side information = what the reference stores: the `.bin` file name (levels, bin_num, z_offset) and the `.dat` (min, max) pairs.
Like the reference decoder, the last BFS node of every multi-level shell is not coded (Octree.py:259-262) and stays unknown.
Phase 1 (ancestors only) runs once per level for all its windows; phase 2 is sequential per window (the bitstream interleaves
them).  Decoding is not on the metric path.
"""
import json
import math
import os

import numpy as np
import torch

from . import native

KITTI = "kitti"
SIDECAR = ".scp.json"


def extract_info(binfile):
    """decode_ehem.py:20-27 / decode_ehem_mullevel.py:20-27: everything the reference's decoders know about a stream - coordinate
    system from the file name, (levels, bin_num, z_offset) = its last three `_` fields (integers: the encoder wrote
    `int(z_offset)`), and the per-level (min, max) pairs from `<binfile>.dat` for the polar systems."""
    name = os.path.basename(binfile)
    spher, cylin = "spher" in name, "cylin" in name
    n_levels, bin_num, z_offset = (int(x) for x in name[:-len(".bin")].split("_")[-3:])
    pos_mm = torch.load(binfile + ".dat").numpy() if (spher or cylin) else np.zeros((0, 2), np.float32)
    return spher, cylin, pos_mm, n_levels, bin_num, z_offset


def write_sidecar(outfile, enc, res, model_name):
    """`<outfile>.scp.json` - what the reference's two side-info carriers cannot hold (an extension; the `.bin` / `.dat` pair stays
    exactly the reference's): lidar level and dataset type (the reference decoder takes the level count for the lidar level,
    decode_ehem.py:218), each shell's own bin_num (the file name has the first shell's only, but every shell de-quantises its
    angles with its own), the un-truncated z offset, `quant` = per shell the (qs[3], offset[3]) the integers were made with when the encoder quantised the
    frame itself (None on the --preproc_path / encode_ints paths: the dataset rules of `shell_qs` then apply, and `--type obj`, whose
    per-axis-minimum offset exists nowhere else, cannot be de-quantised), and the numeric profile of the kernels that produced the CDFs."""
    side = dict(model=model_name, type=enc.data_type, lidar_level=int(enc.lidar_level), mullevel=bool(enc.mullevel),
                spher=bool(enc.spher), cylin=bool(enc.cylin), n_points=int(res["n_points"]), n_nodes=int(res["n_nodes"]),
                bin_nums=[float(b) for b in res.get("bin_nums", [res["bin_num"]])],
                z_offset=float(res["z_offset"]), quant=res.get("quant"),
                profile=native.numeric_profile(model_name, getattr(enc, "profile", None), decodable=getattr(enc, "decodable", False)))
    if model_name == "OctAttention":
        # additive fields (OctAttnFrameDecoder): the window length, whether every level is its own chunk, the one-window-per-node mode,
        # and the octree depth the positions are normalised by
        side.update(context_size=int(enc.context_size), level_wise=bool(enc.level_wise), sequential=bool(res.get("sequential", False)),
                    depth=int(res["depth"]) if "depth" in res else None)
    if getattr(enc, "temper", None) == "code":
        # a tempered stream ("Temperature"): the grid as float32 bit patterns and one grid index per (level, phase) group in
        # level order - the side information the decoder scales its rows by
        t = res["temper"]
        side["temper"] = dict(betas_u32=[int(b) for b in t["grid_u32"]], index=[int(g["index"]) for g in t["groups"]])
    if getattr(enc, "ring_lod", None) is not None:
        # a ring-LOD stream ("Ring LOD"): one drop per ring and, per shell, the integer thresholds on the radial axis - the
        # integers the decoder finds the implied nodes and the cell sizes with (the ring edges in metres are not part of the rule)
        r = res["ring_lod"]
        side["ring_lod"] = dict(drops=[int(d) for d in r["drops"]], thresholds=[[int(t) for t in shell] for shell in r["thresholds"]])
    with open(outfile + SIDECAR, "w") as f:
        json.dump(side, f)
    return side


TEMPER_TOKEN = "temper"


def is_tempered(binfile):
    """A stream whose rows were scaled by per-level inverse temperatures says so in its file name: the field `temper` where
    FrameEncoder.outfile puts it - directly in front of the coordinate token, or of the last three fields of a Cartesian name
    (`..._temper_spher_<levels>_<bin>_<z>.bin`).  A `temper` field anywhere else belongs to the original file's own name."""
    fields = os.path.basename(binfile)[:-len(".bin")].split("_")
    k = len(fields) - 4
    if k >= 0 and fields[k] in ("spher", "cylin"):
        k -= 1
    return k >= 0 and fields[k] == TEMPER_TOKEN


def stream_temper(binfile, side, n_levels):
    """The inverse temperatures of a stream -> None (a plain stream: any `temper` entry of its side-info file is ignored), or float32
    [2 * n_levels]: the value of group 2 l + p (level l of the file's level list, phase p).  A tempered stream without the table cannot
    be decoded: refused with the reason."""
    if not is_tempered(binfile):
        return None
    if side is None:
        raise native.ScpError(f"{binfile}: a tempered stream (`_{TEMPER_TOKEN}_` in its name) without its side-info file ({SIDECAR}), which "
                              "holds the inverse temperatures the encoder scaled its rows by")
    t = side.get("temper")
    if not isinstance(t, dict) or "betas_u32" not in t or "index" not in t:
        raise native.ScpError(f"{binfile}: a tempered stream whose side-info file has no `temper` entry (betas_u32, index)")
    def ints(name):
        v = t[name]
        if not isinstance(v, list) or not all(isinstance(x, int) and not isinstance(x, bool) for x in v):
            raise native.ScpError(f"{binfile}: the side-info file's `temper` entry: `{name}` is not a list of integers")
        return v

    betas, index = ints("betas_u32"), ints("index")
    if len(index) != 2 * n_levels:
        raise native.ScpError(f"{binfile}: the side-info file's `temper` entry holds {len(index)} indices, a stream of {n_levels} levels has "
                              f"{2 * n_levels} (one per level and phase)")
    if not 1 <= len(betas) <= native.TEMPER_MAX_NT or not all(0 <= b < 2 ** 32 for b in betas):
        raise native.ScpError(f"{binfile}: the side-info file's `temper` grid holds {len(betas)} values: 1 .. {native.TEMPER_MAX_NT} float32 bit "
                              "patterns expected")
    grid = np.array(betas, np.uint32).view(np.float32)
    if not (np.isfinite(grid).all() and (grid > 0).all()):
        raise native.ScpError(f"{binfile}: the side-info file's `temper` grid holds a value that is not finite and positive")
    for i in index:
        if not 0 <= i < len(grid):
            raise native.ScpError(f"{binfile}: temper index {i} out of range: the side-info file's grid has {len(grid)} values")
    return grid[index]


RINGLOD_TOKEN = "ringlod"


def is_ringlod(binfile):
    """A stream coded with a truncation depth per range ring says so in its file name: the field `ringlod` where FrameEncoder.outfile
    puts it - in front of `temper` (if there), which stands in front of the coordinate token
    (`..._ringlod[_temper]_spher_<levels>_<bin>_<z>.bin`).  A `ringlod` field anywhere else belongs to the original file's own name."""
    fields = os.path.basename(binfile)[:-len(".bin")].split("_")
    k = len(fields) - 4
    if k >= 0 and fields[k] in ("spher", "cylin"):
        k -= 1
    if k >= 0 and fields[k] == TEMPER_TOKEN:
        k -= 1
    return k >= 0 and fields[k] == RINGLOD_TOKEN


def stream_ringlod(binfile, side, n_levels, mullevel):
    """The ring-LOD table of a stream -> None (a name without the field: any `ring_lod` entry of its side-info file is ignored), or
    dict(drops tuple, thresholds: one tuple per shell).  A ring-LOD stream without a well-formed table cannot be decoded - the decoder
    would not know which rows are implied -: refused with the reason, before anything is decoded."""
    if not is_ringlod(binfile):
        return None
    if side is None:
        raise native.ScpError(f"{binfile}: a ring-LOD stream (`_{RINGLOD_TOKEN}_` in its name) without its side-info file ({SIDECAR}), which "
                              "holds the drops and the integer thresholds the encoder cut its rings with")
    t = side.get("ring_lod")
    if not isinstance(t, dict) or "drops" not in t or "thresholds" not in t:
        raise native.ScpError(f"{binfile}: a ring-LOD stream whose side-info file has no `ring_lod` entry (drops, thresholds)")

    def ints(v, name):
        if not isinstance(v, list) or not all(isinstance(x, int) and not isinstance(x, bool) for x in v):
            raise native.ScpError(f"{binfile}: the side-info file's `ring_lod` entry: `{name}` is not a list of integers")
        return v

    drops, shells = ints(t["drops"], "drops"), t["thresholds"]
    depths = shell_depths(n_levels, mullevel)
    if not isinstance(shells, list) or len(shells) != len(depths):
        raise native.ScpError(f"{binfile}: the side-info file's `ring_lod` entry holds the thresholds of "
                              f"{len(shells) if isinstance(shells, list) else 'no'} shells, the stream has {len(depths)}")
    if not 1 <= len(drops) <= native.RINGLOD_MAX_RINGS:
        raise native.ScpError(f"{binfile}: the side-info file's `ring_lod` entry holds {len(drops)} drops: 1 .. {native.RINGLOD_MAX_RINGS} rings expected")
    for s, thr in enumerate(shells):
        ints(thr, f"thresholds[{s}]")
        if len(thr) != len(drops) - 1:
            raise native.ScpError(f"{binfile}: the side-info file's `ring_lod` entry holds {len(drops)} drops for the {len(thr)} thresholds of "
                                  f"shell {s}: one more drop than thresholds expected")
        if any(not 0 <= x <= 2 ** 31 - 1 for x in thr) or any(b < a for a, b in zip(thr, thr[1:])):
            raise native.ScpError(f"{binfile}: the side-info file's `ring_lod` thresholds of shell {s} are negative, beyond 2^31 - 1 or descending: {thr}")
    top = min(native.RINGLOD_MAX, min(depths) - 1)
    for d in drops:
        if not 0 <= d <= top:
            raise native.ScpError(f"{binfile}: ring-LOD drop {d} out of range: 0 .. {top} for shells {depths} levels deep")
    return dict(drops=tuple(drops), thresholds=[tuple(thr) for thr in shells])


def read_sidecar(binfile):
    p = binfile + SIDECAR
    if not os.path.exists(p):
        return None
    with open(p) as f:
        return json.load(f)


def shell_qs(data_type, lidar_level, mullevel):
    f = (lambda l: 400 / (2 ** l - 1)) if data_type == KITTI else (lambda l: 2 ** (18 - l))
    return [f(lidar_level + k) for k in range(3)] if mullevel else [f(lidar_level)]


def dequantise_leaves(leaves, qs, bin_num, z_offset, spher, cylin, data_type=KITTI):
    """Leaf integers -> Cartesian points, decode_ehem.py:237-253 (`pt_rec * qs + offset`, then spher2cart / cylin2cart,
    data_preprocess.py:186-229), float64 on the device."""
    from . import metrics
    if spher:
        q, off = [qs, 2 * math.pi / (bin_num - 1), math.pi / (bin_num - 1)], [0.0, 0.0, 0.0]
    elif cylin:
        q, off = [qs, 2 * math.pi / (bin_num - 1), qs], [0.0, 0.0, float(z_offset)]
    else:
        o = -200.0 if data_type == KITTI else -float(2 ** 17)
        q, off = [qs, qs, qs], [o, o, o]
    return metrics.dequantize(leaves, q, off, spher=spher, cylin=cylin)


def octattn_window_of(r, cs):
    """OctAttention's window rule (encoder._chunk_rows): node r of a chunk (front-padded with cs - 1 rows) is predicted at position
    (r + cs - 1) % cs of window (r + cs - 1) // cs.  -> (window, position)."""
    return divmod(r + cs - 1, cs)


def octattn_chunks(level_sizes, level_wise):
    """The chunk lengths of a frame: one chunk of every node, or (level_wise) one per octree level."""
    return [int(n) for n in level_sizes] if level_wise else [int(sum(level_sizes))]


def _refuse_octattn(binfile, side):
    """The OctAttention streams OctAttnFrameDecoder cannot decode, refused with the reason."""
    if side is None or "profile" not in side:
        raise native.ScpError(f"{binfile}: no side-info file ({SIDECAR}): the default OctAttention profile cannot be decoded bit for bit (its "
                              "attention scales V by a maximum over the whole launch) - re-encode with --decodable")
    if side.get("model") != "OctAttention":
        raise native.ScpError(f"{binfile}: an {side.get('model')} stream, not OctAttention")
    if not str(side["profile"]).startswith("octattn/1d:"):
        raise native.ScpError(f"{binfile}: coded under the default OctAttention profile {side['profile']!r}, which cannot be decoded bit for bit "
                              "(its attention scales V by a maximum over the whole launch) - re-encode with --decodable")
    if side.get("mullevel"):
        raise native.ScpError(f"{binfile}: multi-level OctAttention streams (three shells) are not decodable")
    if side.get("sequential"):
        raise native.ScpError(f"{binfile}: a --sequential stream: each node's window slides, so the decoder has no cache to keep")
    want = native.numeric_profile("OctAttention", None, decodable=True)
    if side["profile"] != want:
        raise native.ScpError(f"{binfile}: coded under numeric profile {side['profile']!r}, this process runs {want!r}: the integer CDFs would "
                              "differ and the range decoder would desynchronise")
    for k in ("context_size", "level_wise", "depth", "n_nodes"):
        if side.get(k) is None:
            raise native.ScpError(f"{binfile}: side-info file without `{k}`")


def decode_octattn_file(binfile, model, device=None):
    """An OctAttention stream written with `--decodable` -> dict(codes [n_nodes] uint8 occupancy in BFS order, leaves int64 [U, 3],
    points [U, 3] float64 Cartesian).  Everything the decoder needs beyond the stream comes from the `.scp.json` side-info file."""
    side = read_sidecar(binfile)
    _refuse_octattn(binfile, side)
    if side["context_size"] != model.cfg.model.context_size:
        raise native.ScpError(f"{binfile}: coded with context size {side['context_size']}, the model has {model.cfg.model.context_size}")
    with open(binfile, "rb") as f:
        stream = f.read()
    dec = OctAttnFrameDecoder(model, side["depth"], level_wise=side["level_wise"], device=device)
    codes, leaves = dec.decode(stream, side["n_nodes"])
    return _octattn_result(side, codes, leaves, dec.stats)


def _octattn_result(side, codes, leaves, stats):
    """Decoded codes and leaf integers -> the dict decode_octattn_file returns (the leaves de-quantised by the side-info's rule)."""
    spher, cylin = side["spher"], side["cylin"]
    data_type, quant = side["type"], side.get("quant")
    if data_type == "obj" and quant:
        # the steps and offset the integers were made with: encode.py's --type obj rule (qs 1, the frame's per-axis minimum), or the
        # encoder's own quantiser
        from . import metrics
        pts = metrics.dequantize(leaves, quant[0]["qs"], quant[0]["offset"], spher=spher, cylin=cylin)
    else:
        # KITTI / Ford: the reference decoder's rule with the side-info's (un-truncated) z offset; obj without `quant`: the
        # encoder's fixed rule (qs 2^(18 - L), offset -2^17: OctAttnFrameEncoder.cart_offset)
        qs = shell_qs(data_type, side["lidar_level"], False)[0]
        pts = dequantise_leaves(leaves, qs, side["bin_nums"][0], side["z_offset"], spher, cylin, data_type)
    return dict(codes=[codes], leaves=[leaves], points=pts, spher=spher, cylin=cylin, stats=stats)


class _Stamps:
    """Wall seconds per stage, for all four decoders: `stats` is None (nothing is measured, no synchronisation) or a dict that collects
    them (bench.py --decode), assignable from outside at any time; every stamp then costs a device synchronisation."""
    stats = None

    def _t0(self):
        if self.stats is None:
            return 0.0
        import time
        torch.cuda.synchronize()
        return time.perf_counter()

    def _stamp(self, key, t0):
        if self.stats is None:
            return t0
        import time
        torch.cuda.synchronize()
        t = time.perf_counter()
        self.stats[key] = self.stats.get(key, 0.0) + (t - t0)
        return t


class OctAttnFrameDecoder(_Stamps):
    """The inverse of OctAttnFrameEncoder(decodable=True).  The octree is regenerated breadth first; a level's children, their context
    rows (occ, level, octant) x (ggp, gp, p, self) and positions come from one launch (native.decode_expand_octattn) once the level is
    decoded.  Node by node (the window rule of `octattn_window_of`; with `level_wise` every level is its own chunk): the unknown pass of
    OctAttnStepper gives the logits row, the encoder's CDF kernel its integer CDF, one pinned copy brings it to the host range decoder,
    and the known pass with the decoded symbol extends the window's cache."""

    def __init__(self, model, depth, level_wise=False, device=None):
        self.model = model
        self.depth = int(depth)
        self.level_wise = bool(level_wise)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.context_size = model.cfg.model.context_size
        self._pin = torch.empty(256, dtype=torch.int16, pin_memory=True)

    def decode(self, stream, n_nodes):
        """-> (occupancy codes uint8 [n_nodes] in BFS order, leaf integer coordinates int64 [U, 3])."""
        from . import ops
        from .models.oct_attention import OctAttnStepper
        import time
        dev, cs = self.device, self.context_size
        dec = native.AcDecoder(stream)
        prev = self.model.decodable
        self.model.decodable = True
        try:
            with ops.frozen_weights():
                st = OctAttnStepper(self.model)
                ctx = torch.tensor([[255, 0, 0] * 3 + [255, 1, 1]], dtype=torch.uint8, device=dev)     # the root: level 1, octant 1
                apos = torch.zeros((1, 4, 3), dtype=torch.int32, device=dev)
                pos = torch.zeros((1, 4, 3), dtype=torch.float32, device=dev)
                codes, done, r = [], 0, 0
                stream_ = torch.cuda.current_stream(dev)
                for L in range(1, self.depth + 1):
                    n = ctx.shape[0]
                    if done + n > n_nodes:
                        raise native.ScpError(f"the octree has more than the side-info's {n_nodes} nodes: stream and side-info disagree")
                    if L == 1 or self.level_wise:
                        r = 0
                    syms = np.empty(n, np.int64)
                    t = time.perf_counter() if self.stats is not None else 0.0
                    if self.stats is not None:
                        torch.cuda.synchronize()
                    for i in range(n):
                        w, p = octattn_window_of(r, cs)
                        if r == 0 or p == 0:
                            st.reset(pad=(w == 0))
                        crow, prow = ctx[i:i + 1], pos[i:i + 1]
                        logits = st.unknown(crow, prow)
                        t = self._stamp("model_step", t)
                        self._pin.copy_(native.softmax_cdf(logits, want_lohi=False, want_cdf=True)["cdf"][0], non_blocking=True)
                        stream_.synchronize()
                        t = self._stamp("cdf_d2h", t)
                        s = dec.next(self._pin.numpy())
                        t = self._stamp("range_decoder", t)
                        syms[i] = s
                        crow[0, 9] = s
                        st.known(crow, prow)
                        t = self._stamp("model_step", t)
                        r += 1
                    done += n
                    occ8, ctx, apos, pos = native.decode_expand_octattn(torch.from_numpy(syms).to(dev), ctx, apos, L, self.depth)
                    t = self._stamp("expansion", t)
                    codes.append(occ8)
                if done != n_nodes:
                    raise native.ScpError(f"decoded {done} nodes, the side-info says {n_nodes}")
        finally:
            self.model.decodable = prev
        return torch.cat(codes), apos[:, 3].long()


def decode_octattn_files(binfiles, model, streams=1, device=None):
    """Several OctAttention streams written with `--decodable`, decoded `streams` at a time in lockstep (OctAttnBatchDecoder): one model
    step serves one node of every stream in flight.  -> the dicts decode_octattn_file returns, in the order of `binfiles`, each with
    the bits the one-stream decoder gives.  The streams share the model; they may differ in depth, coordinate system, data type, lidar
    level and `level_wise`.  Every side-info file is read and checked before anything is decoded."""
    if streams < 1:
        raise native.ScpError("decode_octattn_files: streams >= 1 expected")
    binfiles = [str(b) for b in binfiles]
    sides = []
    for binfile in binfiles:
        side = read_sidecar(binfile)
        _refuse_octattn(binfile, side)
        if side["context_size"] != model.cfg.model.context_size:
            raise native.ScpError(f"{binfile}: coded with context size {side['context_size']}, the model has {model.cfg.model.context_size}")
        sides.append(side)
    if not binfiles:
        return []
    jobs = []
    for binfile, side in zip(binfiles, sides):
        with open(binfile, "rb") as f:
            jobs.append(dict(name=binfile, stream=f.read(), n_nodes=side["n_nodes"], depth=side["depth"], level_wise=side["level_wise"]))
    dec = OctAttnBatchDecoder(model, min(int(streams), len(jobs)), device=device)
    return [_octattn_result(side, codes, leaves, dec.stats) for side, (codes, leaves) in zip(sides, dec.decode(jobs))]


class OctAttnLockstep:
    """The host bookkeeping of the lockstep decoder, free of any device state (tests drive it with made-up level sizes).  `slots`
    slots each hold one file's position: level L, node i of the level's n, row r of the chunk (`level_wise`: a chunk per level).
    A step visits one node of every active slot; its window and position follow `octattn_window_of` exactly as in
    OctAttnFrameDecoder.decode.  Idle slots take the pending files in file order (`refill`, lowest idle slot first)."""

    def __init__(self, n_files, slots, context_size, level_wise):
        self.cs = int(context_size)
        self.level_wise = [bool(x) for x in level_wise]
        assert len(self.level_wise) == n_files and slots >= 1
        self.pending = list(range(n_files))[::-1]
        self.file = [None] * slots
        self.L = [0] * slots
        self.n = [0] * slots
        self.i = [0] * slots
        self.r = [0] * slots

    def refill(self):
        """-> [(slot, file)] newly started: level 1, the root node alone."""
        new = []
        for s in range(len(self.file)):
            if self.file[s] is None and self.pending:
                self.file[s] = self.pending.pop()
                self.L[s], self.n[s], self.i[s], self.r[s] = 1, 1, 0, 0
                new.append((s, self.file[s]))
        return new

    def active(self):
        return tuple(s for s, f in enumerate(self.file) if f is not None)

    def step(self):
        """One node of every active slot (no slot may sit at the end of its level) -> [(slot, file, node index in its level, window,
        position, reset, pad)]: reset = the slot's window starts here, pad = with the chunk's front padding."""
        rows = []
        for s, f in enumerate(self.file):
            if f is None:
                continue
            assert self.i[s] < self.n[s]
            w, p = octattn_window_of(self.r[s], self.cs)
            reset = self.r[s] == 0 or p == 0
            rows.append((s, f, self.i[s], w, p, reset, reset and w == 0))
            self.i[s] += 1
            self.r[s] += 1
        return rows

    def level_ends(self):
        """The slots whose level is decoded: each needs next_level() or finish() before the next step."""
        return [s for s, f in enumerate(self.file) if f is not None and self.i[s] == self.n[s]]

    def next_level(self, slot, n):
        self.L[slot] += 1
        self.n[slot], self.i[slot] = int(n), 0
        if self.level_wise[self.file[slot]]:
            self.r[slot] = 0

    def finish(self, slot):
        self.file[slot] = None


class OctAttnBatchDecoder(_Stamps):
    """OctAttnFrameDecoder for several streams at once.  Slot s of an OctAttnBatchStepper holds the window of one stream; in one step
    every active slot decodes exactly one node: one `unknown` over the active slots, one CDF launch on [B, 255], ONE pinned
    device-to-host copy of the B CDF rows and one stream synchronisation, B range-decoder calls (each stream has its own decoder),
    ONE host-to-device copy of the B symbols, one `known`.  Each slot's current level (context rows, positions) lies in its region
    of one device arena; the step's rows are gathered by a device index array that is advanced on the device, so the host work of a
    step beyond the B range-decoder calls does not grow with B.  A slot that finishes a level expands it for itself
    (native.decode_expand_octattn, one host sync) and goes on in the next step; a slot whose frame is complete takes the next
    pending file.  Each stream's symbols, codes and leaves are those of OctAttnFrameDecoder, bit for bit."""

    def __init__(self, model, streams, device=None):
        self.model = model
        self.slots = int(streams)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.context_size = model.cfg.model.context_size
        self.steps = 0
        self._pin = torch.empty((self.slots, 256), dtype=torch.int16, pin_memory=True)
        self._pin_sym = torch.empty((self.slots,), dtype=torch.uint8, pin_memory=True)

    def decode(self, jobs):
        """jobs: dicts(name, stream bytes, n_nodes, depth, level_wise) -> [(codes uint8 [n_nodes] in BFS order, leaves int64 [U, 3])] in
        the order of `jobs`."""
        from . import ops
        from .models.oct_attention import OctAttnBatchStepper
        import time
        dev, cs, S = self.device, self.context_size, self.slots
        prev = self.model.decodable
        self.model.decodable = True
        try:
            with ops.frozen_weights():
                st = OctAttnBatchStepper(self.model, S)
                sched = OctAttnLockstep(len(jobs), S, cs, [j["level_wise"] for j in jobs])
                cap = max(max(int(j["n_nodes"]) for j in jobs), 1)       # a level holds at most all of a frame's nodes
                ctx_a = torch.empty((S * cap, 12), dtype=torch.uint8, device=dev)
                pos_a = torch.empty((S * cap, 4, 3), dtype=torch.float32, device=dev)
                cur = torch.zeros((S,), dtype=torch.int64, device=dev)   # arena row of each slot's next node
                one = torch.ones((S,), dtype=torch.int64, device=dev)
                root = torch.tensor([255, 0, 0] * 3 + [255, 1, 1], dtype=torch.uint8, device=dev)     # the root: level 1, octant 1
                decs, syms, apos, codes, done = [None] * S, [None] * S, [None] * S, [None] * S, [0] * S
                results = [None] * len(jobs)
                pin_np, sym_np = self._pin.numpy(), self._pin_sym.numpy()
                stream_ = torch.cuda.current_stream(dev)

                def start(s, f):
                    decs[s] = native.AcDecoder(jobs[f]["stream"])
                    syms[s], codes[s], done[s] = np.empty(1, np.int64), [], 0
                    apos[s] = torch.zeros((1, 4, 3), dtype=torch.int32, device=dev)
                    ctx_a[s * cap].copy_(root)
                    pos_a[s * cap].zero_()
                    cur[s:s + 1].fill_(s * cap)

                for s, f in sched.refill():
                    start(s, f)
                act = sched.active()
                t = time.perf_counter() if self.stats is not None else 0.0
                if self.stats is not None:
                    torch.cuda.synchronize()
                while act:
                    rows = sched.step()
                    for pad in (True, False):
                        ids = [r[0] for r in rows if r[5] and r[6] == pad]
                        if ids:
                            st.reset(ids, pad)
                    B = len(act)
                    a64 = st._slot_ids(act)[2]
                    idx = cur.index_select(0, a64)
                    crow, prow = ctx_a.index_select(0, idx), pos_a.index_select(0, idx)
                    logits = st.unknown(act, crow, prow)
                    t = self._stamp("model_step", t)
                    self._pin[:B].copy_(native.softmax_cdf(logits, want_lohi=False, want_cdf=True)["cdf"], non_blocking=True)
                    stream_.synchronize()
                    t = self._stamp("cdf_d2h", t)
                    for b, (s, _, i, _, _, _, _) in enumerate(rows):
                        sym_np[b] = syms[s][i] = decs[s].next(pin_np[b])
                    t = self._stamp("range_decoder", t)
                    crow[:, 9] = self._pin_sym[:B].to(dev, non_blocking=True)
                    st.known(act, crow, prow)
                    cur.index_add_(0, a64, one[:B])
                    self.steps += 1
                    t = self._stamp("model_step", t)
                    ends = sched.level_ends()
                    for s in ends:
                        f, L, job = sched.file[s], sched.L[s], jobs[sched.file[s]]
                        n, lo = sched.n[s], s * cap
                        done[s] += n
                        occ8, cctx, apos[s], cpos = native.decode_expand_octattn(torch.from_numpy(syms[s]).to(dev), ctx_a[lo:lo + n], apos[s], L,
                                                                                 job["depth"])
                        codes[s].append(occ8)
                        m = cctx.shape[0]
                        if L == job["depth"]:
                            if done[s] != job["n_nodes"]:
                                raise native.ScpError(f"{job['name']}: decoded {done[s]} nodes, the side-info says {job['n_nodes']}")
                            results[f] = (torch.cat(codes[s]), apos[s][:, 3].long())
                            decs[s] = syms[s] = apos[s] = codes[s] = None
                            sched.finish(s)
                            continue
                        if done[s] + m > job["n_nodes"]:
                            raise native.ScpError(f"{job['name']}: the octree has more than the side-info's {job['n_nodes']} nodes: stream and "
                                                  "side-info disagree")
                        if m == 0:
                            raise native.ScpError(f"{job['name']}: decoded {done[s]} nodes, the side-info says {job['n_nodes']}")
                        ctx_a[lo:lo + m].copy_(cctx)
                        pos_a[lo:lo + m].copy_(cpos)
                        cur[s:s + 1].fill_(lo)
                        syms[s] = np.empty(m, np.int64)
                        sched.next_level(s, m)
                    if ends:
                        for s, f in sched.refill():
                            start(s, f)
                        act = sched.active()
                        t = self._stamp("expansion", t)
        finally:
            self.model.decodable = prev
        return results


def _ehem_job(binfile, lidar_level=None, data_type=None, mullevel=False, profile=None):
    """Everything decode_file knows about a stream before it decodes it: the side information of `extract_info`, the `.scp.json` (its
    numeric profile checked against this process's), the reference's rules where it is missing, and the stream's bytes."""
    spher, cylin, pos_mm, n_levels, bin_num, z_offset = extract_info(binfile)
    side = read_sidecar(binfile)
    if side is not None:
        prof = native.numeric_profile(side.get("model", "EHEM"), profile)
        if side["profile"] != prof:
            raise native.ScpError(f"{binfile}: coded under numeric profile {side['profile']!r}, this process runs {prof!r}: the "
                                  "integer CDFs would differ and the range decoder would desynchronise")
        lidar_level = side["lidar_level"] if lidar_level is None else lidar_level
        data_type = side["type"] if data_type is None else data_type
        z_offset = side["z_offset"]
    data_type = data_type or ("ford" if "ford" in binfile else KITTI)                       # decode_ehem.py:241
    if lidar_level is None:
        lidar_level = n_levels // 3 - 1 if mullevel else n_levels                            # the reference's rule
    qs = shell_qs(data_type, lidar_level, mullevel)
    if side is not None and len(side["bin_nums"]) == len(qs):
        bins = side["bin_nums"]
    else:
        bins = [bin_num] + [round((bin_num - 1) * qs[0] / q) + 1 for q in qs[1:]]
    temper = stream_temper(binfile, side, n_levels)
    ring_lod = stream_ringlod(binfile, side, n_levels, mullevel)
    with open(binfile, "rb") as f:
        stream = f.read()
    return dict(name=binfile, stream=stream, side=side, temper=temper, ring_lod=ring_lod, spher=spher, cylin=cylin, polar=spher or cylin, pos_mm=pos_mm, n_levels=n_levels,
                bin_num=bin_num, z_offset=z_offset, lidar_level=lidar_level, data_type=data_type, mullevel=mullevel, qs=qs, bins=bins)


def _obj_without_quant(binfile):
    return native.ScpError(f"{binfile}: --type obj streams are quantised with the frame's per-axis minimum as offset "
                           "(data_preprocess.py:31-37), which only the sidecar's `quant` entry records - it is missing here")


def check_lod(lod, depths):
    """--lod K of a stream whose shells are `depths` levels deep: 0 .. the shallowest depth - 1, or refused with the reason."""
    if isinstance(lod, bool) or not isinstance(lod, int) or not 0 <= lod <= min(depths) - 1:
        raise native.ScpError(f"lod {lod!r} outside 0 .. {min(depths) - 1}: the shells of this stream are {list(depths)} levels deep and LOD K "
                              "stops a tree after its level depth - K, of which there is at least one")
    return lod


def _ehem_result(job, shells, lod=0):
    """The decoded shells [(codes per level, leaf integers)] of a job -> the dict decode_file returns.  lod = K >= 1: the shells carry
    their LOD-K cell origins as a third entry; `points` are the cells' centres (metrics.lod_centres) through the same dequantiser, and
    the dict gains lod, cells (per shell) and levels_decoded (the levels of all shells that were decoded)."""
    binfile, side, spher, cylin, data_type = job["name"], job["side"], job["spher"], job["cylin"], job["data_type"]
    full = shells
    ring = job.get("ring_lod") is not None
    if ring:
        # a ring-LOD stream: the shells carry J(leaf, 0) as a third entry - every leaf is the origin of a terminal cell of size 2^j (j = 0:
        # the leaf itself), and the point written is the cell's centre, origin + (2^j - 1) / 2 per axis (exact in float64)
        shells = [(c, lv.to(torch.float64) + ((torch.bitwise_left_shift(torch.ones_like(j, dtype=torch.int64), j.long()) - 1).to(torch.float64) / 2)[:, None])
                  for c, lv, j in full]
    if lod:
        from . import metrics
        shells = [(c, metrics.lod_centres(cells, lod)) for c, _, cells in full]
    # KITTI / Ford: the reference decoder's own rule (steps from the integer bin_num in float64, decode_ehem.py:237-249) - the cloud it
    # would write.  obj: there is no rule (the offset is the frame's per-axis minimum): the sidecar's `quant` entry, or nothing.
    quant = side.get("quant") if side is not None else None
    if data_type == "obj" and quant is not None and len(quant) == len(shells):
        from . import metrics
        pts = [metrics.dequantize(lv, qd["qs"], qd["offset"], spher=spher, cylin=cylin) for (_, lv), qd in zip(shells, quant)]
    elif data_type == "obj":
        raise _obj_without_quant(binfile)
    else:
        pts = [dequantise_leaves(lv, q, b, job["z_offset"], spher, cylin, data_type) for (_, lv), q, b in zip(shells, job["qs"], job["bins"])]
    out = dict(codes=[torch.cat(c) for c, _ in shells], leaves=[lv for _, lv in shells], points=torch.cat(pts),
               spher=spher, cylin=cylin, n_levels=job["n_levels"], bin_num=job["bin_num"], z_offset=job["z_offset"],
               lidar_level=job["lidar_level"])
    if lod:
        out.update(leaves=[lv for _, lv, _ in full], lod=lod, cells=[cells for _, _, cells in full], levels_decoded=sum(len(c) for c, _, _ in full))
    if ring:
        out.update(leaves=[lv for _, lv, _ in full], cell_j=[j for _, _, j in full], ring_lod=job["ring_lod"])
    return out


def _refuse_ringlod_mode(job, what):
    """--lod / --streams on a ring-LOD stream: refused with the reason (plain and tempered files in those modes are unaffected)."""
    if job.get("ring_lod") is not None:
        raise native.ScpError(f"{job['name']}: a ring-LOD stream with {what}: its cells have mixed sizes already, and the lockstep driver and "
                              "previews of such trees are not part of this library - decode it alone, in full (--streams 1, --lod 0)")


def decode_attr(binfile, out, mullevel=False):
    """--attr: the reflectance layer of a decoded stream ("Reflectance").  Reads `<stream>.attr`, checks it against the decoded
    geometry and adds to `out` (decode_file's dict): attr_values (per shell device uint8 [U_s], in the order of `leaves`), reflectance
    (float32 [U], float32(value / scale), in the order of `points`), attr_Q and attr_scale.  Runs per file, after the geometry."""
    import os
    from . import attr
    if out.get("lod"):
        raise native.ScpError(f"--attr with --lod {out['lod']}: a preview has cells, not leaves, and the attribute layer codes one value per leaf")
    if out.get("ring_lod") is not None:
        raise native.ScpError(f"--attr: {binfile} is a ring-LOD stream, whose cells have mixed sizes - such streams carry no attribute layer")
    path = binfile + ".attr"
    if not os.path.exists(path):
        raise native.ScpError(f"--attr: {path} is missing - encode with encode*.py --attr to write it next to the stream")
    with open(path, "rb") as f:
        data = f.read()
    info = {}
    try:
        values = attr.decode_shells(data, out["leaves"], shell_depths(out["n_levels"], mullevel), info)
    except native.ScpError as e:
        raise native.ScpError(f"--attr: {path}: {e}") from None
    out.update(attr_values=values, attr_Q=info["Q"], attr_scale=info["scale"], reflectance=(torch.cat(values).double() / float(info["scale"])).float())
    return out


def decode_color(binfile, out, mullevel=False):
    """--color: the colour layer of a decoded stream ("Colour").  Reads `<stream>.color`, checks every shell's depth and leaf
    count against the decoded geometry and adds to `out` (decode_file's dict): colors (device uint8 [U,3], in the order of `points`) and
    color_Q.  Runs per file, after the geometry."""
    import os
    from . import color
    if out.get("lod"):
        raise native.ScpError(f"--color with --lod {out['lod']}: a preview has cells, not leaves, and the weights of a cut tree are unknown to the decoder")
    if out.get("ring_lod") is not None:
        raise native.ScpError(f"--color: {binfile} is a ring-LOD stream, whose cells have mixed sizes - such streams carry no colour layer")
    path = binfile + ".color"
    if not os.path.exists(path):
        raise native.ScpError(f"--color: {path} is missing - encode with encode.py --type obj --color to write it next to the stream")
    with open(path, "rb") as f:
        data = f.read()
    info = {}
    try:
        values = color.decode_shells(data, out["leaves"], shell_depths(out["n_levels"], mullevel), info)
    except native.ScpError as e:
        raise native.ScpError(f"--color: {path}: {e}") from None
    out.update(colors=torch.cat(values), color_Q=info["Q"])
    return out


def decode_file(binfile, model, lidar_level=None, data_type=None, mullevel=False, device=None, profile=None, lod=0, attr=False, color=False):
    """A stream file written by the encode CLIs -> dict(codes per shell, leaves per shell, points [U,3] float64 Cartesian).
    Side information exactly as the reference's decoders take it (`extract_info`); the `.scp.json` written next to the stream
    supplies what that cannot carry.  Without it the reference's own rules apply: lidar level = the level count (decode_ehem.py:218),
    integer z offset, and - for the two outer shells - bin numbers extrapolated from the first shell's.
    lod = K >= 1 (at most the shallowest shell's depth - 1): a preview - the tree stops after level D - K and `points` holds the centres
    of the cells of size 2^K those levels describe ("Depth report"); a multi-level stream decodes its first two shells in
    full, since the range decoder has to pass them, and stops the last one early.  The dict gains lod, cells (int64 origins per shell)
    and levels_decoded (over all shells: D - K for one tree); `leaves` holds None for the shell that stopped.  lod = 0 is the path without the option.
    attr: also decode `<stream>.attr` (`decode_attr`): the dict gains reflectance (float32 [U], in the order of `points`) and attr_values
    (uint8 per shell); not with lod >= 1.  Without it nothing of the attribute layer is read, launched or allocated.
    color: also decode `<stream>.color` (`decode_color`): the dict gains colors (uint8 [U,3], in the order of `points`) and color_Q; not
    with lod >= 1.  Without it nothing of the colour layer is read, launched or allocated."""
    if attr and lod:
        raise native.ScpError(f"--attr with --lod {lod}: a preview has cells, not leaves, and the attribute layer codes one value per leaf")
    if color and lod:
        raise native.ScpError(f"--color with --lod {lod}: a preview has cells, not leaves, and the weights of a cut tree are unknown to the decoder")
    job = _ehem_job(binfile, lidar_level, data_type, mullevel, profile)
    if lod:
        _refuse_ringlod_mode(job, f"--lod {lod}")
    dec = FrameDecoder(model, job["lidar_level"], mullevel=mullevel, polar=job["polar"], device=device, profile=profile)
    out = _ehem_result(job, dec.decode(job["stream"], job["n_levels"], job["pos_mm"], lod, temper=job["temper"], ring_lod=job["ring_lod"]), lod)
    if attr:
        out = decode_attr(binfile, out, mullevel)
    return decode_color(binfile, out, mullevel) if color else out


def shell_depths(n_levels, mullevel):
    """The octree depths of a stream's shells: one tree, or the three of a multi-level frame (decode_ehem_mullevel.py:199)."""
    if mullevel:
        m = n_levels // 3
        return [m - 1, m, m + 1]
    return [n_levels]


def last_coded_level(depth, pos_mm, mullevel, polar):
    """The last chunk is the deepest level with coded rows: a one-leaf shell's last level holds the dropped node alone, its (min, max)
    row still carries the build's initial words (min > max), and the clip and the epsilon-free division move up one level."""
    if mullevel and polar and depth > 1 and float(pos_mm[depth - 1][0]) > float(pos_mm[depth - 1][1]):
        return depth - 1
    return depth


def ehem_level_params(L, depth, last_coded, pos_mm, lidar_level, mullevel, polar):
    """(lv, ancestor level clamp, mn, den) of the model inputs of level L of a tree of `depth` levels."""
    last = L == last_coded
    lv = min(L, lidar_level) if last else L                                # encode_dataset_ehem.py:86 clips the last chunk
    if polar:
        mn, mx = float(pos_mm[L - 1][0]), float(pos_mm[L - 1][1])
        eps = 0.0 if (mullevel and last) else 1e-9
        return lv, (lidar_level if last else 255), mn, mx - mn + eps
    return lv, (lidar_level if last else 255), 0.0, float(2 ** depth)


def window_lengths(rows, cs):
    """The windows of a level with `rows` coded nodes."""
    return [min(cs, rows - i) for i in range(0, rows, cs)]


def chunk_steps(steps, max_tokens=1_000_000, max_rows=None):
    """Cut a round (steps[k] = the window lengths of step k) into the runs of WHOLE steps that one phase-1 forward takes:
    [(first step, one past the last)].  A run holds at most `max_tokens` real tokens and `max_rows` rows of the padded layout
    (encoder.MAX_PACKED_ROWS: the bounds of the encoder's own packed forwards, encoder.chunk_windows); a step is never split - one step of
    64 slots x 8192 tokens fits both bounds, and a step that did not would go alone."""
    if max_rows is None:
        from .encoder import MAX_PACKED_ROWS as max_rows
    out, i = [], 0
    while i < len(steps):
        j, tok, rows = i, 0, 0
        while j < len(steps):
            t = sum(steps[j])
            r = sum(-(-(c + (c & 1)) // 512) * 512 for c in steps[j])
            if j > i and (tok + t > max_tokens or rows + r > max_rows):
                break
            tok += t
            rows += r
            j += 1
        out.append((i, j))
        i = j
    return out


def _stage_rows(c, nst):
    """Rows of a window of c nodes in every cross stage (models/packed.py: StageLayout - every stage pads a window to x512 rows)."""
    rows, L = [], (c + (c & 1)) // 2
    for _ in range(nst):
        rows.append(-(-L // 512) * 512)
        L = (L + 1) // 2
    return rows


class _EhemRounds(_Stamps):
    """What both EHEM decoders do alike with the windows of a ROUND - one level of one stream (FrameDecoder) or the current level of every
    stream in flight (EhemBatchDecoder), as `steps`: steps[k] = [(column, window length)], window k of every column that has one.  The
    even-node logits of a window depend on ancestors only (ehem.py:92-115), so phase 1 runs ONCE over all windows of the round as a packed
    forward (in runs of whole steps under the encoder's bounds, `chunk_steps`) - bit-identical to one-window launches (every kernel is
    per-row / per-window deterministic: tests/test_gpu_e2e.py::test_full_frame_packed_forward_is_batch_invariant) and 10 - 50 x better at
    filling the GPU - with one CDF launch, one pinned copy and ehem_phase2_prepare on the side stream while the copy travels.  Phase 2
    needs the decoded even symbols and every bitstream interleaves its windows (evens, odds, evens, ...), so it runs step by step on the
    step's slice of the run's phase-1 state, with the plan of the step's lengths (the slice IS that plan's layout: the windows of a step
    are adjacent in every stage).  All state is per instance: several decoders may run on threads, each on its own stream."""

    def __init__(self, model, device=None, profile=None, max_tokens=1_000_000, max_rows=None, coder_threads=1):
        self.model = model
        self.profile = profile        # native.NumericProfile: must be the one the stream was coded under (None: process default)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.context_size = model.cfg.model.context_size
        self.max_tokens, self.max_rows = max_tokens, max_rows        # the bounds of one phase-1 forward (the encoder's; tests lower them)
        self.steps = 0
        self._plans = {}              # packed plans by their window lengths (`_plan`)
        self._pin = [None, None]      # pinned staging of the CDF rows (grown on demand)
        self._pin_po = None           # pinned staging of a step's even symbols on their way up
        self._side = None             # side stream of ehem_phase2_prepare (created on first use, on the decoding thread's device)
        self._pool = None             # range-decoder threads for the windows of a step (independent streams; ctypes releases the GIL)
        if int(coder_threads) > 1:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=min(int(coder_threads), 16))
        self.prepare_ahead = os.environ.get("SCP_DEC_PREP", "1") != "0"       # A/B switch: 0 = everything of phase 2 after the even symbols

    def _plan(self, lengths):
        """The packed plan of a list of window lengths (index maps depend on the lengths only).  Kept are the lists that repeat: ONE window
        of any length (every window's phase 2 in a one-stream level, and a frame decoded again has the same tail windows), small windows
        only (the one-node and few-node levels every tree starts with) and full windows only (the inner steps of the large levels)."""
        from .models.packed import PackedPlan
        key = tuple(lengths)
        p = self._plans.get(key)
        if p is None:
            p = PackedPlan(list(key), device=self.device)
            if len(key) == 1 or max(key) <= 64 or min(key) == self.context_size:
                if len(self._plans) >= 256:
                    self._plans.clear()
                self._plans[key] = p
        return p

    def _cdf_to_host(self, cdf_dev, then=None, slot=0):
        """int16 CDF rows -> numpy, through a pinned buffer with an asynchronous copy: `then()` (launches for the side stream) runs on the host while
        the GPU finishes phase 1 and the copy; returns (rows, then's result).  The rows are a view of pinned buffer `slot` (0: a run's phase-1 rows,
        1: a step's phase-2 rows): consumed before the slot's next use."""
        n = cdf_dev.numel()
        if self._pin[slot] is None or self._pin[slot].numel() < n:
            self._pin[slot] = torch.empty(max(n, 1 << 20), dtype=torch.int16, pin_memory=True)
        host = self._pin[slot][:n].view(cdf_dev.shape)
        host.copy_(cdf_dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        r = then() if then is not None else None
        ev.synchronize()
        return host.numpy(), r

    def _prepare(self, st, plan):
        """Start the symbol-independent part of phase 2 (models/packed.py: ehem_phase2_prepare) on the side stream, behind everything the current
        stream holds so far (phase 1); returns (prep, event).  The host decodes the even symbols meanwhile; phase 2 waits for the event."""
        from .models.packed import ehem_phase2_prepare
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            prep = ehem_phase2_prepare(self.model, st, plan)
            done = torch.cuda.Event()
            done.record(self._side)
        return prep, done

    def _run_coders(self, decs, grp, rows):
        """One range-decoder call per window of a step: decs[col].run(rows_of_that_window) for (col, rows) in order -> the symbols."""
        if self._pool is None or len(grp) < 2:
            return [decs[col].run(r) for (col, _), r in zip(grp, rows)]
        return list(self._pool.map(lambda a: decs[a[0][0]].run(a[1]), zip(grp, rows)))

    def _evens_to_device(self, evens, qps):
        """The even symbols of a step's windows -> int64 device tensor [sum qps] in the cross layout (each window's rows padded to its x512
        rows with zeros behind the real ones): one asynchronous copy out of a pinned buffer, whose previous contents were consumed - a
        step's phase-2 rows are read back, with a synchronisation, before the next step gets here."""
        Q = sum(qps)
        if self._pin_po is None or self._pin_po.numel() < Q:
            self._pin_po = torch.empty(max(Q, 8192), dtype=torch.int64, pin_memory=True)
        h = self._pin_po[:Q].numpy()
        q0 = 0
        for even, qp in zip(evens, qps):
            h[q0:q0 + even.shape[0]] = even
            h[q0 + even.shape[0]:q0 + qp] = 0
            q0 += qp
        po = torch.empty(Q, dtype=torch.int64, device=self.device)
        po.copy_(self._pin_po[:Q], non_blocking=True)
        return po

    def _step_rows(self, st, prep, run):
        """The rows of every step of a run (its steps' [(column, window length)]) in the run's phase-1 state `st` and preparation `prep`
        (or None) -> per step (state, preparation or None, cross-layout rows of every window).  Views only, cut while the CDF rows travel
        and the host has nothing else to do; a step of one-node windows is stepped over like any other.  A one-step run IS its step."""
        from .models.packed import phase2_prep_window
        nst = len(self.model.swin_cross_transformer.layers)
        out, bases = [], [0] * nst                                              # first row of the current step in every cross stage
        for grp in run:
            per = [_stage_rows(c, nst) for _, c in grp]
            rows = [sum(r) for r in zip(*per)]
            if len(run) == 1:
                out.append((st, prep, [p[0] for p in per]))
                continue
            q0, q1 = bases[0], bases[0] + rows[0]
            out.append((dict(a1=st["a1"][q0:q1], a2=st["a2"][q0:q1], pre_occ=st["pre_occ"][q0:q1]),
                        None if prep is None else phase2_prep_window(prep, bases, rows), [p[0] for p in per]))
            bases = [b + r for b, r in zip(bases, rows)]
        return out

    def _scale(self, rows, lengths, betas):
        """A tempered round: the logits rows of consecutive windows (`lengths` rows each) times their windows' inverse temperatures, in place -
        the encoder's own product (native.scale_rows).  Nothing is launched when every value is 1 (x * 1.0f is x, bit for bit)."""
        from itertools import accumulate
        if all(b == 1.0 for b in betas):
            return
        native.scale_rows(rows, list(accumulate(lengths, initial=0)), np.asarray(betas, np.float32))

    def _force(self, rows, implied, row0, lengths, odd):
        """A ring-LOD round: the logits rows of the implied nodes become the encoder's forced row (native.force_rows), in place.  rows: the
        phase-1 (odd False) or phase-2 rows of consecutive windows of `lengths` nodes whose first input row is row0; implied: the round's
        mask in the row order of `ctx` - a window's phase-1 rows are its nodes 0, 2, .., its phase-2 rows its nodes 1, 3, .."""
        idx, o = [], row0
        for c in lengths:
            idx.append(np.arange(o + (1 if odd else 0), o + c, 2, dtype=np.int64))
            o += c
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        if idx.shape[0] > rows.shape[0]:
            raise native.ScpError(f"ring LOD: {rows.shape[0]} logits rows for {idx.shape[0]} nodes of the round")
        if idx.shape[0]:
            native.force_rows(rows[:idx.shape[0]], implied[torch.from_numpy(idx).to(self.device)].contiguous())

    def _decode_round(self, decs, steps, ctx, posn, sym, first, temper=None, implied=None):
        """The windows of a round.  decs[col]: the column's range decoder; steps: EhemLockstep.layout's; ctx uint8 [T, 12] (own occupancy =
        255 placeholder) / posn f32 [T, 3]: the round's inputs in window order; the symbols of column col go to sym[first[col]:] (host
        int64: they stay on the host until the round is complete, a step sends only its even symbols up).  Runs the SAME packed kernels as
        the encoder: encoder and decoder must produce bit-identical integer CDFs.  A window of one node has no phase 2.
        temper: per column the inverse temperatures (phase 1, phase 2) of a tempered stream, (1, 1) for a plain one in the same round; None
        (no tempered stream in the round) adds nothing.
        implied: uint8 device mask [T] in the row order of `ctx` - the implied nodes of a ring-LOD stream, whose phase-1 and phase-2 rows
        are forced before anything else reads them; the range decoder then returns symbol 0 for them by itself.  None adds nothing."""
        from itertools import accumulate
        from .models.packed import ehem_phase1_packed, ehem_phase2_packed
        cs, model = self.context_size, self.model
        t_row = 0
        t = self._t0()
        for k0, k1 in chunk_steps([[c for _, c in st] for st in steps], self.max_tokens, self.max_rows):
            lengths = [c for st in steps[k0:k1] for _, c in st]
            ntok = sum(lengths)
            plan = self._plan(lengths)
            prob1, st = ehem_phase1_packed(model, ctx[t_row:t_row + ntok], posn[t_row:t_row + ntok], plan)
            t = self._stamp("phase1_model", t)
            prob1 = prob1.contiguous()
            if implied is not None:
                self._force(prob1, implied, t_row, lengths, odd=False)
            if temper is not None:
                self._scale(prob1, [(c + 1) // 2 for c in lengths], [temper[col][0] for st_ in steps[k0:k1] for col, _ in st_])
            cdf1_dev = native.softmax_cdf(prob1, want_lohi=False, want_cdf=True)["cdf"]
            # the run's query stream + pre_attn_mlp: one packed pass over all windows, launched while the CDF rows travel
            ahead = self.prepare_ahead and max(lengths) > 1

            def then():
                prep, done = self._prepare(st, plan) if ahead else (None, None)
                return done, self._step_rows(st, prep, steps[k0:k1])

            cdf1, (done, views) = self._cdf_to_host(cdf1_dev, then)
            t = self._stamp("cdf_d2h", t)
            e0, step_row = 0, t_row
            for k, (stw, pwin, qps) in zip(range(k0, k1), views):
                grp = steps[k]
                row0, step_row = step_row, step_row + sum(c for _, c in grp)          # the step's first input row
                ends = list(accumulate(((c + 1) // 2 for _, c in grp), initial=e0))
                evens = self._run_coders(decs, grp, [cdf1[a:b] for a, b in zip(ends, ends[1:])])
                e0 = ends[-1]
                for (col, c), even in zip(grp, evens):
                    r0 = first[col] + k * cs
                    sym[r0:r0 + c:2] = even
                t = self._stamp("range_decoder", t)
                if max(c for _, c in grp) > 1:
                    po = self._evens_to_device(evens, qps)
                    t = self._stamp("index_ops", t)
                    pw = plan if k1 - k0 == 1 else self._plan([c for _, c in grp])       # a one-step run: the step's plan is the run's
                    if done is not None:
                        torch.cuda.current_stream(self.device).wait_event(done)
                        done = None
                    prob2 = ehem_phase2_packed(model, stw, pw, po, prep=pwin).contiguous()
                    odd = [(col, c) for col, c in grp if c > 1]
                    if implied is not None:
                        self._force(prob2, implied, row0, [c for _, c in grp], odd=True)
                    if temper is not None:
                        self._scale(prob2, [c // 2 for _, c in odd], [temper[col][1] for col, _ in odd])
                    t = self._stamp("phase2_model", t)
                    cdf2, _ = self._cdf_to_host(native.softmax_cdf(prob2, want_lohi=False, want_cdf=True)["cdf"], slot=1)
                    t = self._stamp("cdf_d2h", t)
                    ends = list(accumulate((c // 2 for _, c in odd), initial=0))
                    for (col, c), o in zip(odd, self._run_coders(decs, odd, [cdf2[a:b] for a, b in zip(ends, ends[1:])])):
                        r0 = first[col] + k * cs
                        sym[r0 + 1:r0 + c:2] = o
                    t = self._stamp("range_decoder", t)
                self.steps += 1
            t_row += ntok


class FrameDecoder(_EhemRounds):
    """One stream: the tree driver (`_decode_tree`, native.decode_expand) over the round engine, a level = a round of one column.  A
    phase-1 forward takes the engine's default bounds (1 000 000 tokens, encoder.MAX_PACKED_ROWS padded rows); a level holds at most as
    many nodes as the frame has points (about 120 000), so no level of a supported frame reaches them and every level is one run."""

    def __init__(self, model, lidar_level=12, mullevel=False, polar=True, device=None, profile=None):
        super().__init__(model, device=device, profile=profile)
        self.lidar_level = lidar_level
        self.mullevel = mullevel
        self.polar = polar            # spherical / cylindrical: positions normalised with the .dat (min, max) pairs

    def _decode_level(self, dec, ctx, pos, n_total, temper=None, implied=None):
        """All windows of one level -> int64 device tensor [n_total]: the symbols of the ctx.shape[0] coded nodes, -1 behind them (the dropped last
        node of a multi-level shell).  ctx uint8 [n, 12], pos f32 [n, 3]; implied: the level's ring-LOD mask, uint8 [n], or None."""
        sym = np.full(n_total, -1, np.int64)
        steps = [[(0, c)] for c in window_lengths(ctx.shape[0], self.context_size)]
        self._decode_round([dec], steps, ctx, pos, sym, [0], None if temper is None else [temper], implied)
        return torch.from_numpy(sym).to(self.device)

    def _decode_tree(self, dec, depth, pos_mm, lod=0, stop=False, temper=None, ring=None):
        """One octree: returns (codes per level as device uint8 tensors, leaf integer coordinates [U,3]).  lod = K >= 1: a third entry,
        the origins of the level-(depth - K + 1) nodes (int64 [C,3], leaf units, node order) - what the symbols of level depth - K name;
        with `stop` the tree ends there (the levels below are not decoded, the leaves are None).  temper: float32 [2 * depth], the
        tree's inverse temperatures (level 1 phase 1, level 1 phase 2, ...) of a tempered stream.  ring: (thresholds, drops) of this tree
        in a ring-LOD stream - the nodes of level L with J(origin, depth - L + 1) > 0 are implied and their rows forced; a third entry,
        J(leaf, 0) uint8 [U], says how large the cell is that every leaf stands for.
        Level state: pos int32 [n,3] node origins, anc uint8 [n,9] = (level, octant, symbol) of (ggp, gp, p) with pad = (0, 0, 255), octant uint8 [n];
        the children of a decoded level and the model inputs of the level they form come from one launch (native.decode_expand)."""
        dev = self.device
        anc = torch.tensor([[0, 0, 255] * 3], dtype=torch.uint8, device=dev)
        octant = torch.ones(1, dtype=torch.uint8, device=dev)
        pos = torch.zeros((1, 3), dtype=torch.int32, device=dev)

        last_coded = last_coded_level(depth, pos_mm, self.mullevel, self.polar)

        def level_params(L):
            return ehem_level_params(L, depth, last_coded, pos_mm, self.lidar_level, self.mullevel, self.polar)

        # level 1: the root
        lv, clamp, mn, den = level_params(1)
        ctx = torch.tensor([[0, 0, 255] * 3 + [lv, 1, 255]], dtype=torch.uint8, device=dev)
        posn = ((pos.double() - mn) / den).float() if self.polar else (pos.double() / den).float()
        codes = []
        t = self._t0()
        for L in range(1, depth + 1):
            n = pos.shape[0]
            last = L == depth
            rows = n - (1 if (self.mullevel and last) else 0)                  # the dropped last node is never coded
            t = self._stamp("tree_expansion", t)
            beta = None if temper is None else (float(temper[2 * L - 2]), float(temper[2 * L - 1]))
            implied = None
            if ring is not None and rows > 0 and depth - L + 1 <= max(ring[1]):       # (a node larger than every terminal cell is never implied)
                implied = native.ringlod_cells(pos[:rows], ring[0], ring[1], start=depth - L + 1).clamp_(max=1)
            sym = self._decode_level(dec, ctx[:rows], posn[:rows], n, beta, implied) if rows > 0 else torch.full((n,), -1, dtype=torch.int64, device=dev)
            t = self._t0()
            # children in (parent, digit) order; occupancy 1..255, 0 = unknown (dropped node)
            if last:
                lvn, clamp, mn, den = 0, 255, 0.0, 1.0
            else:
                lvn, clamp, mn, den = level_params(L + 1)
            occ8, pos, anc, octant, ctx, posn = native.decode_expand(sym, pos, anc, octant, L, depth - L, lvn, clamp, self.polar and not last, mn, den)
            codes.append(occ8)
            if lod and L == depth - lod:
                cells = pos.long()
                if stop:
                    return codes, None, cells
            if last:
                if ring is not None:
                    return codes, pos.long(), native.ringlod_cells(pos, ring[0], ring[1])
                return (codes, pos.long(), cells) if lod else (codes, pos.long())

    def decode(self, stream, n_levels, pos_mm, lod=0, temper=None, ring_lod=None):
        """stream: bytes; temper: a tempered stream's inverse temperatures (decoder.stream_temper: float32 [2 * n_levels]); n_levels: total level count from the file name; pos_mm: [n_levels,2] array from the .dat file.
        Returns list of (codes_per_level, leaf_points int64 [U,3]) - one entry per shell.  lod = K >= 1 (at most the shallowest shell's
        depth - 1): every entry gains the origins of the shell's LOD-K cells; the shells of a multi-level stream are coded one after the
        other, so those before the last are decoded in full (the range decoder has to pass them) and only the last one stops after its
        level depth - K, its leaves None."""
        dec = native.AcDecoder(stream)
        depths = shell_depths(n_levels, self.mullevel)
        lod = check_lod(lod, depths)
        if ring_lod is not None and lod:
            raise native.ScpError("a ring-LOD stream has no --lod preview: its cells have mixed sizes already")
        out, off = [], 0
        from . import ops
        with native.use_profile(self.profile), ops.frozen_weights():            # (the weights do not change inside a frame: validated once per frame)
            for k, d in enumerate(depths):
                out.append(self._decode_tree(dec, d, pos_mm[off:off + d] if self.polar else None, lod, stop=lod > 0 and k == len(depths) - 1,
                                             temper=None if temper is None else temper[2 * off:2 * (off + d)],
                                             ring=None if ring_lod is None else (ring_lod["thresholds"][k], ring_lod["drops"])))
                off += d
        return out


# ------------------------------------------------------------------------------------------------ several EHEM streams in lockstep
class EhemLockstep:
    """The host bookkeeping of the lockstep EHEM decoder, free of any device state (tests drive it with made-up level sizes).  `slots`
    slots each hold one file's position: tree (of the file's 1 or 3), level L of the tree's depth, node count n of the level.  A ROUND
    decodes the current level of every active slot; its coded rows are n, or n - 1 on the last level of a tree whose last node is dropped
    (multi-level shells), and may be 0.  Within a round, STEP k holds window k of every slot that has more than k windows
    (`window_lengths`); the round's windows are ordered step-major, then slot, so the windows of a step are adjacent in every stage of
    the round's packed layout.  After a round every slot is advanced with its child count: the next level, the root of the file's next
    tree, or - the file done - idle, to be refilled in file order (lowest idle slot first, as OctAttnLockstep does)."""

    def __init__(self, depths, drops, slots, context_size):
        self.cs = int(context_size)
        self.depths = [[int(d) for d in ds] for ds in depths]
        self.drops = [bool(x) for x in drops]
        assert len(self.drops) == len(self.depths) and slots >= 1 and self.cs >= 1
        self.pending = list(range(len(self.depths)))[::-1]
        self.file = [None] * slots
        self.tree = [0] * slots
        self.L = [0] * slots
        self.n = [0] * slots

    def refill(self):
        """-> [(slot, file)] newly started: tree 0, level 1, the root node alone."""
        new = []
        for s in range(len(self.file)):
            if self.file[s] is None and self.pending:
                self.file[s] = self.pending.pop()
                self.tree[s], self.L[s], self.n[s] = 0, 1, 1
                new.append((s, self.file[s]))
        return new

    def active(self):
        return tuple(s for s, f in enumerate(self.file) if f is not None)

    def depth(self, slot):
        return self.depths[self.file[slot]][self.tree[slot]]

    def round(self):
        """The current level of every active slot, in slot order -> [(slot, file, tree, L, n, coded rows)] (nothing is advanced)."""
        out = []
        for s, f in enumerate(self.file):
            if f is not None:
                drop = self.drops[f] and self.L[s] == self.depth(s)
                out.append((s, f, self.tree[s], self.L[s], self.n[s], self.n[s] - (1 if drop else 0)))
        return out

    def advance(self, slot, m):
        """The slot's level is decoded and has m children -> "level" (on to the next level, m nodes), "tree" (the tree is complete: on to the
        root of the file's next tree) or "file" (the file is complete: the slot is idle)."""
        f = self.file[slot]
        if self.L[slot] < self.depth(slot):
            self.L[slot] += 1
            self.n[slot] = int(m)
            return "level"
        if self.tree[slot] + 1 < len(self.depths[f]):
            self.tree[slot] += 1
            self.L[slot], self.n[slot] = 1, 1
            return "tree"
        self.file[slot] = None
        return "file"

    @staticmethod
    def layout(rows, cs):
        """The layout of a round from the coded-row counts of its slots (one column each) -> (steps, wbase): steps[k] = [(column, window
        length)] of the columns with more than k windows, in column order - the round's window list is their concatenation; wbase int64
        [K, columns] (K >= 1) = the first row of window k of a column in the round's dense input arrays, -1 where there is none."""
        wins = [window_lengths(int(r), cs) for r in rows]
        K = max([len(w) for w in wins] + [1])
        wbase = np.full((K, len(wins)), -1, np.int64)
        steps, row = [], 0
        for k in range(max(len(w) for w in wins) if wins else 0):
            step = []
            for col, w in enumerate(wins):
                if len(w) > k:
                    step.append((col, w[k]))
                    wbase[k, col] = row
                    row += w[k]
            steps.append(step)
        return steps, wbase


# range-decoder threads of the lockstep decoder (1 = the calls of a step one after the other on the decoding thread)
CODER_THREADS = int(os.environ.get("SCP_DEC_CODER_THREADS", "1"))


class EhemBatchDecoder(_EhemRounds):
    """FrameDecoder for several streams at once: the lockstep driver (scheduling: EhemLockstep) over the round engine.  A round = the
    current level of every stream in flight, a column each; per step every stream's own range decoder takes its window's even symbols,
    ONE phase 2 serves the step, and every stream decodes its odd symbols.  The decoded levels of all streams are expanded by one launch
    (native.decode_expand_batch) that writes the next round's model inputs in round order.  The packed forward is batch-invariant bit
    for bit, so every stream's CDF rows, symbols, codes and leaves are FrameDecoder's; per stream the bitstream order (window: evens,
    odds) is untouched.  max_tokens / max_rows: the bounds of one phase-1 forward (the encoder's; tests lower them).  coder_threads > 1:
    the range-decoder calls of a step run on a pool of that many threads, 16 at most.  `stats` also gets the counters `rounds`, `steps`."""

    def __init__(self, model, streams, device=None, profile=None, max_tokens=1_000_000, max_rows=None, coder_threads=CODER_THREADS):
        self.slots = int(streams)
        if not 1 <= self.slots <= 64:
            raise native.ScpError("EhemBatchDecoder: 1 .. 64 streams expected")
        super().__init__(model, device=device, profile=profile, max_tokens=max_tokens, max_rows=max_rows,
                         coder_threads=min(int(coder_threads), self.slots))
        self.rounds = 0
        self._pin_sym = None          # pinned staging of a round's symbols on their way up (`_upload_symbols`)

    # ---- per-file facts
    def _params(self, f, tree, L):
        """(lv, clamp, mn, den) of the model inputs of level L of tree `tree` of job f (FrameDecoder._decode_tree's level_params)."""
        j, d = self._jobs[f], self._depths[f][tree]
        off = sum(self._depths[f][:tree])
        mm = j["pos_mm"][off:off + d] if j["polar"] else None
        return ehem_level_params(L, d, last_coded_level(d, mm, j["mullevel"], j["polar"]), mm, j["lidar_level"], j["mullevel"], j["polar"])

    def _round_temper(self, info):
        """Per column of the round the (phase 1, phase 2) inverse temperatures of its stream's current level - every slot has its own table
        and its own level; a plain stream's are (1, 1) -, or None when no stream in the round is tempered."""
        if all(self._jobs[r[1]].get("temper") is None for r in info):
            return None
        out = []
        for s, f, tree, L, n, rows in info:
            tb = self._jobs[f].get("temper")
            g = 2 * (sum(self._depths[f][:tree]) + L - 1)
            out.append((1.0, 1.0) if tb is None else (float(tb[g]), float(tb[g + 1])))
        return out

    def _put_roots(self, ctx, posn, roots):
        """roots: [(input row, file, tree)] - the root's context row and normalised origin, as FrameDecoder._decode_tree makes them."""
        if not roots:
            return
        c = np.zeros((len(roots), 12), np.uint8)
        p = np.zeros((len(roots), 3), np.float32)
        for i, (_, f, tree) in enumerate(roots):
            lv, _, mn, den = self._params(f, tree, 1)
            c[i] = [0, 0, 255] * 3 + [lv, 1, 255]
            p[i] = np.float32((0.0 - mn) / den) if self._jobs[f]["polar"] else np.float32(0.0 / den)
        idx = torch.tensor([r for r, _, _ in roots], dtype=torch.int64, device=self.device)
        ctx.index_copy_(0, idx, torch.from_numpy(c).to(self.device))
        posn.index_copy_(0, idx, torch.from_numpy(p).to(self.device))

    def _refill(self, sched, decs, codes):
        for _, f in sched.refill():
            decs[f], codes[f] = native.AcDecoder(self._jobs[f]["stream"]), []

    def _upload_symbols(self, N, ends):
        """The round's symbols (the first N words of the pinned buffer; behind them the last parent row of every segment) in one copy, one
        scan of their child counts, the segment totals back -> (sym, cum, children per segment)."""
        C = len(ends)
        self._pin_sym[N:N + C] = torch.from_numpy(ends)
        up = torch.empty(N + C, dtype=torch.int64, device=self.device)
        up.copy_(self._pin_sym[:N + C], non_blocking=True)
        sym = up[:N]
        cum = torch.cumsum(native.popcount_table(self.device)[sym + 1], 0)
        tot = cum[up[N:]].cpu().numpy()
        return sym, cum, np.diff(tot, prepend=0)

    def _segment_table(self, info, state, ninfo, nwb, first, cfirst):
        """The table of native.decode_expand_batch for the decoded round `info` (state[col]: what EhemLockstep.advance said), given the next
        round `ninfo` and its layout: a segment whose slot goes on with its tree gets its next level's scalars, coded rows and window
        starts; one whose tree is complete only yields child state (the leaves)."""
        ncol_of = {r[0]: i for i, r in enumerate(ninfo)}
        seg = np.zeros(len(info), native.EXPAND_SEG)
        wbk = np.full((nwb.shape[0], len(info)), -1, np.int64)
        for col, (s, f, tree, L, n, _) in enumerate(info):
            if state[col] == "level":
                lvn, clamp, mn, den = self._params(f, tree, L + 1)
                coded, polar = ninfo[ncol_of[s]][5], self._jobs[f]["polar"]
                wbk[:, col] = nwb[:, ncol_of[s]]
            else:
                lvn, clamp, mn, den, coded, polar = 0, 255, 0.0, 1.0, 0, False
            seg[col] = (first[col], n, cfirst[col], coded, L, self._depths[f][tree] - L, lvn, clamp, 1 if polar else 0, 0, mn, den)
        return seg, wbk

    def _next_parents(self, info, ninfo, nwb, cfirst, m, state_dev, roots_dev):
        """The parents of the next round, slot-major: a slot that goes on takes its children where the launch put them, a slot at a root (a
        new tree or file) the root row -> (pos, anc, octant), [(input row, file, tree)] of the roots with a coded row."""
        col_of = {r[0]: i for i, r in enumerate(info)}
        pieces, roots = [], []
        for nc, (s, f, tree, L, n, rows) in enumerate(ninfo):
            if L > 1:
                pieces.append((int(cfirst[col_of[s]]), int(m[col_of[s]])))
            else:
                pieces.append(None)
                if rows > 0:
                    roots.append((int(nwb[0, nc]), f, tree))
        if pieces and all(p is not None for p in pieces) and sum(p[1] for p in pieces) == state_dev[0].shape[0]:
            return state_dev, roots                                  # every segment goes on: its children are the next parents as they lie
        if not pieces:
            return state_dev, roots
        return tuple(torch.cat([a[p[0]:p[0] + p[1]] if p is not None else r for p in pieces]) for a, r in zip(state_dev, roots_dev)), roots

    def decode(self, jobs):
        """jobs: dicts(name, stream bytes, n_levels, pos_mm, polar, mullevel, lidar_level) -> per job the list FrameDecoder.decode returns:
        (codes per level, leaf integers int64 [U, 3]) of every shell."""
        from . import ops
        dev, cs = self.device, self.context_size
        self._jobs = jobs
        self._depths = depths = [shell_depths(j["n_levels"], j["mullevel"]) for j in jobs]
        sched = EhemLockstep(depths, [j["mullevel"] for j in jobs], self.slots, cs)
        decs, codes, shells = [None] * len(jobs), [None] * len(jobs), [[] for _ in jobs]
        results = [None] * len(jobs)
        roots_dev = (torch.zeros((1, 3), dtype=torch.int32, device=dev), torch.tensor([[0, 0, 255] * 3], dtype=torch.uint8, device=dev),
                     torch.ones(1, dtype=torch.uint8, device=dev))
        with native.use_profile(self.profile), ops.frozen_weights():
            t = self._t0()
            self._refill(sched, decs, codes)
            info = sched.round()
            steps, wb = EhemLockstep.layout([r[5] for r in info], cs)
            pos, anc, octant = (r.repeat(len(info), *([1] * (r.dim() - 1))) for r in roots_dev)
            T = sum(r[5] for r in info)
            ctx = torch.empty((T, 12), dtype=torch.uint8, device=dev)
            posn = torch.empty((T, 3), dtype=torch.float32, device=dev)
            self._put_roots(ctx, posn, [(int(wb[0, col]), r[1], r[2]) for col, r in enumerate(info) if r[5] > 0])
            while info:
                self.rounds += 1
                ns = np.array([r[4] for r in info], np.int64)
                first = np.cumsum(ns) - ns
                N = int(ns.sum())
                if self._pin_sym is None or self._pin_sym.numel() < N + len(info):
                    self._pin_sym = torch.empty(max(N + len(info), 1 << 16), dtype=torch.int64, pin_memory=True)
                buf = self._pin_sym[:N].numpy()
                buf[:] = -1
                t = self._stamp("tree_expansion", t)
                if steps:
                    self._decode_round([decs[r[1]] for r in info], steps, ctx, posn, buf, [int(x) for x in first], self._round_temper(info))
                t = self._t0()
                sym, cum, m = self._upload_symbols(N, first + ns - 1)
                cfirst = np.cumsum(m) - m
                state = []
                for col, (s, f, tree, L, n, _) in enumerate(info):
                    if L < depths[f][tree] and m[col] == 0:
                        raise native.ScpError(f"{jobs[f]['name']}: level {L} of a tree of {depths[f][tree]} levels decodes to no children: stream and "
                                              "side information disagree")
                    state.append(sched.advance(s, m[col]))
                self._refill(sched, decs, codes)
                ninfo = sched.round()
                nsteps, nwb = EhemLockstep.layout([r[5] for r in ninfo], cs)
                seg, wbk = self._segment_table(info, state, ninfo, nwb, first, cfirst)
                occ8, cpos, canc, coct, ctx, posn = native.decode_expand_batch(sym, pos, anc, octant, cum, seg, cs, wbk, int(m.sum()),
                                                                               sum(r[5] for r in ninfo))
                for col, (s, f, tree, L, n, _) in enumerate(info):
                    codes[f].append(occ8[first[col]:first[col] + n].clone())          # (a copy: the round's arrays are not kept alive)
                    if state[col] != "level":
                        shells[f].append((codes[f], cpos[cfirst[col]:cfirst[col] + m[col]].long()))
                        codes[f] = []
                    if state[col] == "file":
                        results[f], decs[f], codes[f] = shells[f], None, None
                (pos, anc, octant), roots = self._next_parents(info, ninfo, nwb, cfirst, m, (cpos, canc, coct), roots_dev)
                self._put_roots(ctx, posn, roots)
                info, steps = ninfo, nsteps
            self._stamp("tree_expansion", t)
        if self.stats is not None:
            self.stats["rounds"], self.stats["steps"] = self.rounds, self.steps
        return results


def decode_files(binfiles, model, streams=1, lidar_level=None, data_type=None, mullevel=False, device=None, profile=None):
    """Several EHEM stream files decoded `streams` at a time in lockstep (EhemBatchDecoder) -> the dicts decode_file returns, in the order
    of `binfiles`, each with the bits the one-stream decoder gives (codes, leaves, points).  The streams share the model and `mullevel`;
    they may differ in depth, coordinate system, data type and lidar level.  Every file's name side info and `.scp.json` is read and
    checked, the numeric profile included, before anything is decoded."""
    if not 1 <= int(streams) <= 64:
        raise native.ScpError("decode_files: 1 .. 64 streams expected")
    jobs = [_ehem_job(str(b), lidar_level, data_type, mullevel, profile) for b in binfiles]
    for j in jobs:
        _refuse_ringlod_mode(j, "--streams (the lockstep decoder)")
        if j["data_type"] == "obj" and not (j["side"] or {}).get("quant"):
            raise _obj_without_quant(j["name"])                               # decode_file's refusal, before anything is decoded
    if not jobs:
        return []
    dec = EhemBatchDecoder(model, min(int(streams), len(jobs)), device=device, profile=profile)
    return [_ehem_result(j, shells) for j, shells in zip(jobs, dec.decode(jobs))]
