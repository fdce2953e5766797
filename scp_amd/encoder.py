"""Frame encoder: LiDAR frame -> range-coded occupancy bitstream, everything between on the MI355X.

This is the hot path of encode.py:85-160 (compress_ehem) / encode_mullevel.py:88-154 and of the datasets feeding it
(dataloaders/encode_dataset_ehem*.py), restructured for the device:

  xyz (H2D once) -> scp_quantize (1 or 3 shells) -> scp_geom_build (one launch sequence for all shells)
     -> scp_geom_context_ehem (ctx u8 [N,12], pos f32 [N,3], sym u8 [N])
     -> EHEM windows (<= 8192 nodes, equal-length windows batched) -> logits scattered straight into CODING ORDER
     -> scp_softmax_cdf over all N rows -> (c_low, c_high) pairs (4 B/node D2H) -> scp_ac_encode_lohi (host)

Per-window softmax, the [N,255] PMF table on the host, the int64 [N,4,6] records and the per-level Python loops of
the reference do not exist here.  The returned dict carries the same scalars the reference prints.
"""
import math
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import os

import numpy as np
import torch

from . import native

KITTI, FORD = "kitti", "ford"


def _wait_event(ev, poll_s=0.0005):
    """Wait for a CUDA / HIP event on a worker thread WITHOUT burning a core: hipEventSynchronize spins (measured on the GPU box with
    tools/host_cpu_threads.py: each of the two coder threads sat at 100 % of a core for the whole run - 130 of a rank's 200 CPU-ms per
    frame - blocking-sync flag or not), so the coder thread polls the event and sleeps in between.  The coder is off the critical path
    (frames in flight hide it); half a millisecond of extra latency per frame costs nothing."""
    while not ev.query():
        time.sleep(poll_s)


def level_qs(data_type, level):
    """encode_dataset_ehem.py:164 / encode_dataset_ehem_mullevel.py:162-185."""
    return 400 / (2 ** level - 1) if data_type == KITTI else 2 ** (18 - level)


class EncodePlan:
    """Window list + coding order for one frame (encode.py:109-136): pure host bookkeeping on level sizes."""

    def __init__(self, level_sizes, context_size):
        self.level_sizes = list(level_sizes)
        self.windows = []          # (row_start, length, coded_start)
        row = 0
        for n in self.level_sizes:
            for i in range(0, n, context_size):
                c = min(context_size, n - i)
                self.windows.append((row + i, c, row + i))   # inside a window: evens first, then odds
            row += n
        self.n_rows = row

    def groups(self, max_batch):
        """Windows of equal length, chunked to at most max_batch per model call."""
        by_len = {}
        for w in self.windows:
            by_len.setdefault(w[1], []).append(w)
        out = []
        for c in sorted(by_len, reverse=True):
            ws = by_len[c]
            for i in range(0, len(ws), max_batch):
                out.append((c, ws[i:i + max_batch]))
        return out

    def coding_order_device(self, dev):
        """coding_order() built with vectorised device ops (no per-window host loop over 577k rows)."""
        w = torch.as_tensor(np.asarray(self.windows, np.int64), device=dev)          # [W,3] (start, length, coded)
        start, c = w[:, 0], w[:, 1]
        ne = (c + 1) // 2
        wid = torch.repeat_interleave(torch.arange(len(self.windows), device=dev), c)
        pos = torch.arange(self.n_rows, device=dev) - start[wid]                        # coded position inside the window
        even = pos < ne[wid]
        return start[wid] + torch.where(even, 2 * pos, 2 * (pos - ne[wid]) + 1)

    def coding_order(self):
        """Row index (frame order) of every coded position - for tests and for the reference-compatible view."""
        order = np.empty(self.n_rows, np.int64)
        for start, c, coded in self.windows:
            ne = (c + 1) // 2
            order[coded:coded + ne] = start + np.arange(0, c, 2)
            order[coded + ne:coded + c] = start + np.arange(1, c, 2)
        return order


# scp_swin_ln_qkv addresses its K / V planes through one 32-bit buffer resource: 4 planes x Tp rows x 512 B must stay below 2^31, i.e. a
# packed forward holds at most 1 048 575 rows of the PADDED layout (every window owns a multiple of 512 rows)
MAX_PACKED_ROWS = 1_048_064


def chunk_windows(windows, max_tokens):
    """Cut a frame's window list into the chunks of one packed forward each: [(first window, one past the last)].  A chunk holds at most
    `max_tokens` real tokens AND at most MAX_PACKED_ROWS rows of the padded layout (a window of c nodes owns ceil((c + c % 2) / 512) * 512
    rows at stage 0: tail windows of a few nodes still cost 512 rows each, which a token bound alone does not see)."""
    out, i = [], 0
    while i < len(windows):
        j, tok, rows = i, 0, 0
        while j < len(windows):
            c = windows[j][1]
            r = -(-(c + (c & 1)) // 512) * 512
            if tok and (tok + c > max_tokens or rows + r > MAX_PACKED_ROWS):
                break
            tok += c
            rows += r
            j += 1
        out.append((i, j))
        i = j
    return out


class _PackedInts(list):
    """Per-shell integer clouds that are consecutive views of ONE buffer (`.packed`: the shells back to back)."""
    packed = None


def _quant_of(infos):
    """Per shell the quantiser's (qs[3], offset[3]) as plain floats: what de-quantisation needs and the reference's file name cannot
    carry exactly (decoder.write_sidecar)."""
    return [dict(qs=[float(v) for v in i.qs], offset=[float(v) for v in i.offset]) for i in infos]


def _as_tensor(x, dtype):
    """numpy array -> host tensor of `dtype` (a view when the array has that type already); a tensor is left as it is."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype)) if isinstance(x, np.ndarray) else x


def _upload_ints(hq, device):
    """One frame's host integers (per-shell clouds, `host_ints`) -> the per-shell device clouds.  Clouds that are views of one pinned
    buffer (`hq.packed`) go over in ONE asynchronous copy and come back as views of its device image (`.packed`: no concatenation
    kernel either).  The copy is made from the PINNED TENSOR itself, never from a numpy view of it: torch's host allocator records the
    stream use of a tensor it knows, so the block is not handed to the next frame's host_ints while this copy still reads it (a
    from_numpy view of the same memory is invisible to the allocator: the next frame's integers could overwrite this frame's in flight)."""
    packed = getattr(hq, "packed", None)
    if packed is None:       # plain per-shell arrays computed elsewhere: pageable memory, synchronous copies
        return [_as_tensor(q, np.int32).to(device) for q in hq]
    qcat = packed.to(device, non_blocking=True)
    qs, a = _PackedInts(), 0
    for q in hq:
        qs.append(qcat[a:a + q.shape[0]])
        a += q.shape[0]
    qs.packed = qcat
    return qs


# What an option that is on (key: `rate`, `temper`, `ring_lod` - its entry in the result dict) leaves in a frame's coding tail: dev - its device
# buffer, which has to reach the host; keep - what its launches use, referenced until they have run; entries(the buffer's host image, the
# frames' result dicts so far, the frames' cuts in the list of levels) -> every frame's entry; check(host image) - None, or what refuses a
# frame by raising: the synchronous calls run it in front of the range coder
_Record = namedtuple("_Record", "key dev keep entries check", defaults=(None,))


class _Tail:
    """A frame's or a batch's coding tail as `_FrontEnd._code_table` enqueued it: the table that is coded, its symbols, the (c_low, c_high)
    pairs, the `_Record`s in the order their buffers travel to the host and their entries appear in the result, cuts (a batch: the row
    bounds of its frames), implied (ring LOD: the mask of the forced rows), rows (the per-row bits, when kept); host: the records' host
    images once made, by `_CoderPipeline.submit` or by `_code_now`.  Whoever holds the tail holds everything its launches use."""

    def __init__(self, table, sym_coded, lohi, records, cuts, implied, rows):
        self.table, self.sym_coded, self.lohi, self.records, self.cuts, self.implied, self.rows = table, sym_coded, lohi, records, cuts, implied, rows
        self.host = None


def _code_now(tail):
    """The synchronous calls: the pairs to the host, then the records that can refuse the frame, then the range coder, then the other
    records.  -> (stream, the time in front of the coder, the time behind it)."""
    lohi = tail.lohi.cpu().numpy()
    early = [r.dev.cpu() if r.check else None for r in tail.records]
    for r, h in zip(tail.records, early):
        if r.check:
            r.check(h.numpy())
    t3 = time.perf_counter()
    stream = native.ac_encode_lohi(lohi)
    t4 = time.perf_counter()
    tail.host = [r.dev.cpu() if h is None else h for r, h in zip(tail.records, early)]
    return stream, t3, t4


def _finish(tail, metas, streams, times, debug=None):
    """The end of every entry point of both encoders: a tail whose host images are complete, per frame its `meta` fields (what the
    reference prints, what its file names and the side-info file carry) and its coded stream, the wall times -> per frame the result
    dict: the stream and its size, the meta fields, the times, `_debug` (device tensors: the synchronous calls only), every record's entry."""
    out = []
    for stream, meta in zip(streams, metas):
        bits = 8 * len(stream)
        out.append(dict(bytes=stream, bits=bits, bpp=bits / meta["n_points"], times=dict(times), **meta))
        if debug is not None:
            out[-1]["_debug"] = debug
    cuts = np.concatenate(([0], np.cumsum([len(m["level_sizes"]) for m in metas])))     # a batch's levels: the frames' level lists one after the other
    for r, h in zip(tail.records, tail.host):
        for res, entry in zip(out, r.entries(h.numpy(), out, cuts)):
            res[r.key] = entry
    return out


def parse_ring_lod(ring_lod):
    """The `ring_lod` argument of FrameEncoder, (ring edges, one drop per ring) -> (edges, drops) as tuples, or None when the option is
    off: None, or every drop 0 ("Ring LOD").  Edges in native.dist_edges' form - ascending from 0, the last ring open -,
    at most native.RINGLOD_MAX_RINGS of them; drops: integers 0 .. native.RINGLOD_MAX.  Anything else is refused with the reason."""
    if ring_lod is None:
        return None
    try:
        edges, drops = ring_lod
        drops = list(drops)
    except (TypeError, ValueError):
        raise native.ScpError(f"ring_lod: (ring edges, one drop per ring) expected, got {ring_lod!r}")
    try:
        edges = native.dist_edges(edges)
    except native.ScpError as e:
        raise native.ScpError(f"ring_lod: the ring edges are not ascending from 0 ({e})")
    if len(edges) > native.RINGLOD_MAX_RINGS:
        raise native.ScpError(f"ring_lod: {len(edges)} rings, at most {native.RINGLOD_MAX_RINGS} expected")
    if len(drops) != len(edges):
        raise native.ScpError(f"ring_lod: {len(drops)} drops for {len(edges)} rings (the edges {edges}, the last ring open): one drop per ring expected")
    for d in drops:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= d <= native.RINGLOD_MAX:
            raise native.ScpError(f"ring_lod: drop {d!r}: an integer 0 .. {native.RINGLOD_MAX} (the number of octree levels the ring leaves out) expected")
    drops = tuple(int(d) for d in drops)
    return (edges, drops) if any(drops) else None


def _rate_layout(level_sizes, context_size=None):
    """The segments of a coding-order table the rate report sums over (native.rate_segments), from level sizes alone (host bookkeeping,
    the windows of EncodePlan): -> (the n_seg + 1 row offsets, per level its segment indices).  context_size None: one segment per level
    (plain BFS coding order, OctAttention) - ([index],).  EHEM: two per window of context_size rows, in coding order the window's first
    (c + 1) // 2 rows (phase 1: the first siblings) and the rest (phase 2: the second siblings, predicted through the cross-attention
    encoder) - (phase-1 indices, phase-2 indices); a window of one row has an empty phase 2, a level of no rows no segment."""
    off, levels, row = [0], [], 0
    for n in level_sizes:
        if context_size is None:
            levels.append(([len(off) - 1],))
            off.append(row + n)
        else:
            p1, p2 = [], []
            for i in range(0, n, context_size):
                c = min(context_size, n - i)
                p1.append(len(off) - 1)
                off.append(row + i + (c + 1) // 2)
                p2.append(len(off) - 1)
                off.append(row + i + c)
            levels.append((p1, p2))
        row += n
    return off, levels


def _rate_sum(raw, idx):
    """Segments `idx` of the host records (numpy int64 [S,5]: rows, ideal_bits, table_bits, top1, bad_rows - the two sums as float64 bit
    patterns) added up: math.fsum, i.e. correctly rounded and therefore the same whatever else the launch held."""
    f = raw.view(np.float64)
    return dict(nodes=int(raw[idx, 0].sum()), ideal_bits=math.fsum(f[idx, 1]), table_bits=math.fsum(f[idx, 2]), top1=int(raw[idx, 3].sum()),
                bad_rows=int(raw[idx, 4].sum()))


def _rate_report(raw, levels, bits, n_points):
    """The `rate` entry of a result dict ("Rate report"): per level of `level_sizes` nodes / ideal_bits / table_bits / top1
    (EHEM: also under phase1 / phase2), the frame's totals, bits per point and per node, and what the range coder spent beyond its table."""
    out_levels, everything = [], []
    for parts in levels:
        idx = [i for p in parts for i in p]
        everything += idx
        entry = _rate_sum(raw, idx)
        entry.pop("bad_rows")
        if len(parts) == 2:
            for name, p in zip(("phase1", "phase2"), parts):
                entry[name] = _rate_sum(raw, p)
                entry[name].pop("bad_rows")
        out_levels.append(entry)
    total = _rate_sum(raw, everything)
    nodes = total["nodes"]
    return dict(levels=out_levels, ideal_bits=total["ideal_bits"], table_bits=total["table_bits"], bad_rows=total["bad_rows"],
                bpp_ideal=total["ideal_bits"] / n_points, bpp_table=total["table_bits"] / n_points,
                bits_per_node_ideal=total["ideal_bits"] / max(nodes, 1), coder_overhead_bits=bits - total["table_bits"])


def _temper_layout(level_sizes, context_size=None):
    """The groups of the per-level temperature ("Temperature") over `_rate_layout`'s segments: EHEM two per entry of
    level_sizes, (phase 1, phase 2) in level order - group 2 l + p; an empty phase still counts -, OctAttention (context_size None) one
    per level.  -> (row offsets of the segments, group of every segment, [(level, phase or None, rows)] per group)."""
    off, levels = _rate_layout(level_sizes, context_size)
    group = np.zeros(len(off) - 1, np.int32)
    meta = []
    for l, parts in enumerate(levels):
        for p, idx in enumerate(parts):
            if idx:
                group[idx] = len(meta)
            meta.append((l, p + 1 if len(parts) == 2 else None, int(sum(off[i + 1] - off[i] for i in idx))))
    return off, group, meta


def _temper_groups(raw, info):
    """The host image of a frame's temperature buffer (`_FrontEnd._temper_launch`) -> one dict per group: level, phase, rows, index,
    bits_unit, bits_chosen; with the report (`temper_sums`) also `sums`, the group's bits at every grid value - its segments added in segment order in
    float64, the device's own order."""
    S, G, nt = info["S"], info["G"], info["nt"]
    f = raw.view(np.float64)
    seg_bits, group_bits = f[:S * nt].reshape(S, nt), f[S * nt:S * nt + 2 * G].reshape(G, 2)
    choice = raw[S * nt + 2 * G:].view(np.int32)[:G]
    out = []
    for g, (level, phase, rows) in enumerate(info["meta"]):
        d = dict(level=level, phase=phase, rows=rows, index=int(choice[g]), bits_unit=float(group_bits[g, 0]), bits_chosen=float(group_bits[g, 1]))
        if info["sums"]:
            sums = np.zeros(nt)
            for i in np.flatnonzero(info["group"] == g):
                sums = sums + seg_bits[i]
            d["sums"] = [float(v) for v in sums]
        out.append(d)
    return out


def _temper_entries(raw, info, cuts):
    """Every frame's `temper` entry from the launch's host buffer: info["per_level"] groups per level, the frames' levels `cuts`."""
    groups, k = _temper_groups(raw, info), info["per_level"]
    return [_temper_entry(groups[k * a:k * b], info, level0=int(a)) for a, b in zip(cuts[:-1], cuts[1:])]


def _temper_entry(groups, info, level0=0):
    """The `temper` entry of a result dict from the frame's groups (a batch: its slice of the launch's, its first level `level0`)."""
    grid = info["grid"]
    groups = [dict(g, level=g["level"] - level0) for g in groups]
    return dict(mode=info["mode"], grid=[float(b) for b in grid], grid_u32=[int(b) for b in grid.view(np.uint32)], unit=info["unit"],
                groups=groups, ideal_bits_unit=math.fsum(g["bits_unit"] for g in groups),
                ideal_bits_chosen=math.fsum(g["bits_chosen"] for g in groups), side_bits=8 * len(groups),
                moved=sum(g["index"] != info["unit"] for g in groups))


class _CoderPipeline:
    """The asynchronous tail of a frame, shared by both encoders' `*_async` calls: the model part of consecutive frames on alternating
    streams (lanes), the (c_low, c_high) pairs D2H on a copy stream, the serial host range coder on a worker thread (ctypes releases the
    GIL) - so the caller can enqueue the next frame while this one is being coded.  Created at an encoder's first asynchronous call."""

    def __init__(self, device, lanes_env):
        self.pool = ThreadPoolExecutor(max_workers=2)
        self.copy_stream = torch.cuda.Stream(device=device)
        # the front part of a frame (stage G with its small D2H syncs, the window plans) is launch-bound: on a side stream the syncs wait
        # for stage G only, not for the previous frames' model kernels queued on a lane; high priority: its tiny kernels slip in between
        # the model's
        self.front_stream = torch.cuda.Stream(device=device, priority=-1)
        # Lanes: consecutive frames run their model part on alternating streams, so the launch gaps and tails of one frame's
        # kernels are filled by the other's (the kernels are whole-GPU persistent launches: they interleave rather than
        # co-run).  One lane keeps every frame on the caller's stream.  Two lanes, with four frames in flight, measured on OctAttention:
        # 56.3 against 47.8 frames/s at L12, 23.1 against 21.0 at L14; three lanes: no better.
        self.lanes = [torch.cuda.Stream(device=device) for _ in range(max(1, int(os.environ.get(lanes_env, "2"))))]
        self._lane_i = 0

    def lane(self, caller):
        """The stream of this frame's model part, ordered behind whatever the caller's stream holds now."""
        if len(self.lanes) == 1:
            return caller
        main = self.lanes[self._lane_i % len(self.lanes)]
        self._lane_i += 1
        main.wait_stream(caller)
        return main

    def submit(self, main, tail, fills0):
        """tail: the frame's `_Tail`, enqueued on `main` (the last thing of its model part).  -> future of the coded stream, or - tail.cuts:
        row bounds of the frames of a batch - of the list of every frame's own stream.  fills0: native.CACHE_FILLS before the frame began.
        The pairs and, in the tail's order, the buffer of every record ride to pinned host tensors (one per call: the worker reads them
        after this returns) on the copy stream - no wait on this thread; the records' images are left in `tail.host` and are complete
        once the future is."""
        done = torch.cuda.Event()
        done.record(main)
        if native.CACHE_FILLS != fills0:               # device-side caches were built while this call ran (first frames only):
            main.synchronize()                         # finish them before anything is enqueued on another lane
        images = []
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(done)
            for dev in [tail.lohi] + [r.dev for r in tail.records]:
                images.append(torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True))
                images[-1].copy_(dev, non_blocking=True)
                dev.record_stream(self.copy_stream)
            copied = torch.cuda.Event(blocking=True)      # the coder thread SLEEPS until the pairs have landed (a default event spins a core)
            copied.record()
        host, tail.host, cuts = images[0], images[1:], tail.cuts

        def work():
            _wait_event(copied)
            h = host.numpy()
            if cuts is None:
                return native.ac_encode_lohi(h)
            return [native.ac_encode_lohi(h[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]

        return self.pool.submit(work)


class _FrontEnd:
    """What both encoders do alike in front of their models: the quantiser's parameters per rho shell, stage G's segment list, the
    device quantiser, and the lazily created coding pipeline of the asynchronous calls."""
    LANES_ENV = None                      # the environment variable that sets the number of lanes (read at the first asynchronous call)
    RATE_PHASES = False                   # EHEM: the report's segments follow the two-phase coding order of the windows
    ring_lod = None                       # off until __init__ says otherwise (`outfile` is also asked of encoders made without it)

    def __init__(self, model, data_type, lidar_level, spher, cylin, mullevel, max_batch, device, host_transform, rate=False, rate_rows=False,
                 temper=None, temper_grid=None, ring_lod=None):
        self.model = model
        # ring LOD ("Ring LOD"): None - nothing is launched or allocated and every stream is the one without the option;
        # (edges, drops) - every range ring leaves out its own number of octree levels
        self.ring_lod = parse_ring_lod(ring_lod)
        self._ring_thr = None                 # per tree of the last build its integer thresholds
        # per-level temperature ("Temperature"): None - nothing is launched or allocated; "report" - every result dict gains
        # `temper`, the stream's bytes stay; "code" - the table is scaled by the chosen inverse temperatures before it is coded
        if temper not in (None, "report", "code"):
            raise native.ScpError(f"temper={temper!r}: None, 'report' or 'code' expected")
        self.temper = temper
        self.temper_grid, self.temper_unit = native.temper_grid(temper_grid) if temper else (None, None)
        self.temper_sums = temper == "report"     # every group of `temper` also carries its bits at every grid value (the CLIs' --temper_report)
        self.rate = bool(rate)                # every result dict gains `rate` (one more read of the logits table per frame; the stream's bytes stay)
        # with rate: the synchronous calls keep the per-row bits of their last frame on the device (two float64 per coded row) for
        # FrameEncoder.ring_rate; off, the rate kernels allocate and launch exactly what they did before the option existed
        self.rate_rows = bool(rate_rows)
        self._rate_rows = None                # (row_ideal, row_table, plan) of the last synchronous encode, while its geometry stands
        # strict-identity switch (CLI --host_transform, SCP_XFORM=numpy): the float -> integer step of the reference on the host
        # (numpy float32 arctan2 / arccos, data_preprocess.py:42-70) instead of the device transform, whose float64 atan2 / acos is
        # more accurate and therefore gives other integers for a few points per frame.  Everything after the
        # integers is bit-exact on the device either way.
        self.host_transform = (os.environ.get("SCP_XFORM", "") == "numpy") if host_transform is None else bool(host_transform)
        self.data_type = data_type
        self.lidar_level = lidar_level
        self.mode = native.CYLIN if cylin else (native.SPHER if spher else native.CART)
        self.spher, self.cylin = spher and not cylin, cylin
        self.mullevel = mullevel
        self.max_batch = max_batch
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.context_size = model.cfg.model.context_size
        self.geom = native.Geom()
        self.cart_offset = -200.0 if data_type == KITTI else -float(2 ** 17)
        self._infos = []                      # the last quantiser call's per-shell info (quant_info)
        self._pipe = None

    def shells(self):
        L = self.lidar_level
        return [([0, 0], L), ([0, 1], L + 1), ([1], L + 2)] if self.mullevel else [(None, L)]

    def _quant_args(self):
        """(quantisation step of every shell, Cartesian offset): the arguments of every quantiser, host or device."""
        return [level_qs(self.data_type, lv) for _, lv in self.shells()], 0.0 if self.mullevel else self.cart_offset

    def _segments(self, clouds):
        """Geom.build's segment list [(offset, count, path, mullevel)] for integer clouds that lie back to back in one buffer: one frame's
        shells, or those of several frames, frame after frame."""
        paths = [path for path, _ in self.shells()]
        segs, off = [], 0
        for k, q in enumerate(clouds):
            segs.append((off, q.shape[0], paths[k % len(paths)], self.mullevel))
            off += q.shape[0]
        return segs

    def _build_xyz(self, frames):
        """Device transform: stage G1 + G2 of the frames as ONE launch sequence (scp_geom_build_xyz: every point transformed once, keys
        for all shells and the sort's first histogram out of one kernel, two host read-backs) -> the info of every (frame, shell)."""
        return self.geom.build_xyz(list(frames), self.mode, *self._quant_args(), [(path, self.mullevel) for path, _ in self.shells()])

    def _quantize_device(self, xyz_dev):
        """The device quantiser, shell by shell -> per-shell integer clouds (device int32 [P,3]); their infos in `_infos`."""
        qs, offset = self._quant_args()
        out = [native.quantize(xyz_dev, self.mode, q, offset) for q in qs]
        self._infos = [o[1] for o in out]
        return [o[0] for o in out]

    def quant_info(self):
        """Per shell the (qs[3], offset[3]) the last quantiser call made its integers with - the cylindrical z offset (the frame's z
        minimum) included: what a decoder needs to de-quantise (OctAttnFrameEncoder.encode_ints(..., quant=))."""
        return _quant_of(self._infos)

    def _pipeline(self):
        if self._pipe is None:
            self._pipe = _CoderPipeline(self.device, self.LANES_ENV)
        return self._pipe

    def _begin_async(self):
        """-> (now, the caller's stream, the lane of this frame's model part, native.CACHE_FILLS before the frame began)."""
        caller = torch.cuda.current_stream(self.device)
        return time.perf_counter(), caller, self._pipeline().lane(caller), native.CACHE_FILLS

    def _code_table(self, table, sym_coded, level_sizes, ring=None, plan=None, cuts=None, keep_rows=False):
        """The coding tail of a frame, the one place that states its order ("The coding tail"; the decoders force and scale in
        the same order): on the current stream 1. the implied rows forced, 2. the temperatures swept, chosen and - "code" - applied,
        3. the CDF kernel, 4. the rate kernels - each reads the table its predecessors left, so what is reported is what is coded.
        table: the logits in coding order; sym_coded: the coded symbols; level_sizes: the levels of the frame, or of a batch's frames one
        after the other; ring, plan: EHEM's ring state of `pre` (None: the option is off) and its plan; cuts: the row bounds of a batch's
        frames; keep_rows: the per-row bits are kept.  An option that is off launches and allocates nothing.  -> the frame's `_Tail`."""
        forced, implied = self._ring_force(table, sym_coded, ring, plan, cuts) if ring is not None else (None, None)
        temper = self._temper_launch(table, sym_coded, level_sizes)
        lohi = native.softmax_cdf(table, sym_coded)["lohi"]
        rate, rows = self._rate_launch(table, sym_coded, lohi, level_sizes, keep_rows)
        return _Tail(table, sym_coded, lohi, [r for r in (rate, temper, forced) if r is not None], cuts, implied, rows)

    def _rate_launch(self, table, sym_coded, lohi, level_sizes, keep_rows):
        """rate=True: the rate kernels, right behind the CDF launch that wrote `lohi` -> (the `rate` record: the device records
        of native.rate_segments; keep_rows: the per-row bits (row_ideal, row_table), else None); (None, None) when the report is off."""
        if not self.rate:
            return None, None
        off, levels = _rate_layout(level_sizes, self.context_size if self.RATE_PHASES else None)
        r = native.rate_segments(table, sym_coded, lohi, off, want_rows=keep_rows)
        entries = lambda raw, frames, cuts: [_rate_report(raw, levels[a:b], f["bits"], f["n_points"]) for f, a, b in zip(frames, cuts[:-1], cuts[1:])]
        return _Record("rate", r["raw"], r["keep"], entries), ((r["row_ideal"], r["row_table"]) if keep_rows else None)

    def _temper_launch(self, table, sym_coded, level_sizes):
        """temper="report" / "code": sweep and choice between the model and the CDF launch; "code" then scales the table in place, so
        that everything behind this call sees the table that is coded.  -> the `temper` record (device buffer int64: the sweep's segment
        bits, the groups' bits at unit and at the choice, the choices - one copy brings them to the host); None when the option is off."""
        if not self.temper:
            return None
        off, group, meta = _temper_layout(level_sizes, self.context_size if self.RATE_PHASES else None)
        S, G, nt = len(off) - 1, len(meta), len(self.temper_grid)
        raw = torch.zeros(S * nt + 2 * G + (G + S * nt + 1) // 2, dtype=torch.int64, device=table.device)
        ints = raw[S * nt + 2 * G:].view(torch.int32)
        seg_bits, seg_bad = raw[:S * nt].view(torch.float64).view(S, nt), ints[G:G + S * nt].view(S, nt)
        sw = native.temper_sweep(table, sym_coded, off, self.temper_grid, out=(seg_bits, seg_bad))
        ch = native.temper_choose(seg_bits, seg_bad, sw["seg_off"], table.shape[0], group, G, self.temper_grid, self.temper_unit,
                                  out=(ints[:G], raw[S * nt:S * nt + 2 * G].view(torch.float64).view(G, 2)))
        if self.temper == "code":
            native.scale_rows(table, sw["seg_off"], ch["seg_beta"])
        info = dict(S=S, G=G, nt=nt, meta=meta, group=group, mode=self.temper, grid=self.temper_grid, unit=self.temper_unit,
                    sums=self.temper_sums, per_level=2 if self.RATE_PHASES else 1)
        return _Record("temper", raw, (sw["keep"], ch["keep"], ch["seg_beta"]), lambda h, frames, cuts: _temper_entries(h, info, cuts))

    def _temper_token(self, base):
        """The file-name token of a tempered stream, in front of the coordinate token (decoder.stream_temper looks for it)."""
        return base + "_temper" if self.temper == "code" else base

    def _ring_token(self, base):
        """The file-name token of a ring-LOD stream, in front of `temper` / the coordinate token (decoder.stream_ringlod looks for it)."""
        return base + "_ringlod" if self.ring_lod is not None else base


class FrameEncoder(_FrontEnd):
    LANES_ENV = "SCP_LANES"
    RATE_PHASES = True

    def __init__(self, model, data_type=KITTI, lidar_level=12, spher=True, cylin=False, mullevel=False, max_batch=8,
                 device=None, packed=True, max_tokens=1_000_000, host_transform=None, profile=None, rate=False, rate_rows=False,
                 temper=None, temper_grid=None, ring_lod=None):
        if mullevel and not (spher or cylin):
            # encode_dataset_ehem_mullevel.py:97-186 has a cylindrical and a spherical branch only
            raise native.ScpError("--mullevel needs --spher or --cylin (the reference has no Cartesian multi-level path)")
        super().__init__(model, data_type, lidar_level, spher, cylin, mullevel, max_batch, device, host_transform, rate, rate_rows,
                         temper, temper_grid, ring_lod)
        if self.ring_lod is not None:
            if self.mode == native.CART:
                raise native.ScpError("ring_lod: Cartesian coordinates have no radial axis to cut rings on - encode with --spher or --cylin")
            if data_type not in (KITTI, FORD):
                raise native.ScpError(f"ring_lod: --type {data_type} has no LiDAR sensor at the origin to measure a range from")
        self.profile = profile          # native.NumericProfile of THIS encoder (None: the process default); current around every launch
        self.packed = packed            # one packed forward for all windows (default) vs one forward per group of equal windows
        self.max_tokens = max_tokens
        self._front_pool = None         # front_async's one thread

    # ------------------------------------------------------------------------------------------ stage G
    def host_ints(self, xyz):
        """The strict-identity front end: numpy [P,>=3] float32 -> (per-shell int32 arrays, infos) exactly as the reference computes
        them (scp_amd/data_preproc/data_preprocess.py: host_quantize).  Runs on the host; the CLI calls it on its reader thread."""
        from .data_preproc.data_preprocess import host_quantize_shells
        xyz = np.ascontiguousarray(xyz.cpu().numpy() if isinstance(xyz, torch.Tensor) else xyz, np.float32)
        out = host_quantize_shells(xyz, self.mode, *self._quant_args())
        # the shells' integers back to back in ONE pinned buffer (this runs on the reader / prefetch thread): the launch thread then issues a
        # single asynchronous host -> device copy and no concatenation kernel; the list holds numpy views of the buffer
        n = [q.shape[0] for q, _ in out]
        buf = torch.empty((sum(n), 3), dtype=torch.int32, pin_memory=torch.cuda.is_available())
        views, a = _PackedInts(), 0
        for (q, _), k in zip(out, n):
            v = buf[a:a + k].numpy()
            v[...] = q
            views.append(v)
            a += k
        views.packed = buf
        return views, [i for _, i in out]

    def quantize(self, xyz_dev, ints=None):
        """xyz -> list of per-shell integer clouds (device int32 [P,3]) + (bin_num, z_offset)."""
        if self.host_transform or ints is not None:
            hq, self._infos = ints if ints is not None else self.host_ints(xyz_dev)
            qs = _upload_ints(hq, self.device)
        else:
            qs = self._quantize_device(xyz_dev)
        first = self._infos[0]
        return qs, first.bin_num, (first.offset[2] if self.cylin else 0.0)

    def _reconstructed(self, infos=None):
        """The de-quantised leaves of the octree of the last `encode` / `preprocess` call, one float64 [U_s,3] device tensor per shell."""
        from . import metrics
        pts = []
        for s, info in enumerate(infos or self._infos):   # infos: per shell, anything with .qs[3] and .offset[3] (tests: the oracle's)
            leaves = self.geom.leaves(s)
            if self.ring_lod is not None:                 # the cloud a ring-LOD decoder writes: the centre of every leaf's terminal cell
                leaves = self.ring_centres(leaves, s)[0]
            pts.append(metrics.dequantize(leaves, info.qs, info.offset, spher=self.spher, cylin=self.cylin,
                                          f32=not self.mullevel).double())
        return pts

    # ------------------------------------------------------------------------------------------ ring LOD
    def ring_centres(self, leaves, s):
        """The leaves (device int32 [U,3]) of tree s of the geometry just built -> (centres of their terminal cells, float64 [U,3]: origin
        + (2^j - 1) / 2 per axis, exact; j uint8 [U]).  A snapped leaf is its cell's origin, so J(leaf, 0) is the cell's size."""
        j = native.ringlod_cells(leaves, self._ring_thr[s], self.ring_lod[1])
        return leaves.to(torch.float64) + ((torch.bitwise_left_shift(torch.ones_like(j, dtype=torch.int64), j.long()) - 1).to(torch.float64) / 2)[:, None], j

    def _ring_snap(self, q, clouds, infos):
        """ring_lod: the integer clouds `clouds` (consecutive row ranges of q, one per tree of the build to come: every frame's shells) with
        their quantiser infos -> (q snapped, out of place: every point on the origin of its terminal cell; the state `_ring_mask`
        completes).  One launch for all clouds, each with the thresholds of its own shell's step and offset."""
        edges, drops = self.ring_lod
        if len(infos) != len(clouds):
            raise native.ScpError(f"ring_lod: {len(clouds)} integer clouds but the quantiser infos of {len(infos)}: the thresholds need every "
                                  "shell's step and offset - quantise with this encoder (quantize / host_ints) or pass encode_ints(..., infos=)")
        if len(clouds) > native.RINGLOD_MAX_TABLES:
            raise native.ScpError(f"ring_lod: a batch holds at most {native.RINGLOD_MAX_TABLES} (frame, shell) trees")
        thr = [native.ringlod_thresholds(edges, i.qs[0], i.offset[0]) for i in infos]
        cuts = np.concatenate(([0], np.cumsum([int(c.shape[0]) for c in clouds])))
        # a tree is as deep as its cloud's largest coordinate has bits (scp_geom_build), and the snap must leave that bit alone: one read-back
        top = torch.stack([c.max() if c.numel() else torch.zeros((), dtype=c.dtype, device=c.device) for c in clouds]).cpu().tolist()
        depths = [int(v).bit_length() for v in top]
        if max(drops) > min(depths) - 1:
            raise native.ScpError(f"ring_lod: a drop of {max(drops)} levels, but the shells of this frame are {depths} levels deep: at most "
                                  f"{max(min(depths) - 1, 0)}, a tree keeps at least its root level")
        segs = [(int(a), int(b - a), 0, k) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
        j, snapped = native.ringlod_cells(q, thr, drops, segs=segs, snapped=True)
        return snapped, dict(thr=thr, j_points=j, point_cuts=cuts, x0=snapped[:, 0])

    def _ring_mask(self, ring, n_frames=1):
        """The implied rows of the geometry just built from snapped clouds, in frame order: a node of level L in a tree of depth D is
        implied iff J(origin, D - L + 1) > 0 - it lies inside a terminal cell, so its only child is child 0 and its symbol 0."""
        g, (edges, drops) = self.geom, self.ring_lod
        depths = [int(i.depth) for i in g.info]
        nd = g.nodes(("level", "pos"))
        segs = [(int(i.node_base), int(i.n_nodes), int(i.depth), s) for s, i in enumerate(g.info)]
        jn = native.ringlod_cells(nd["pos"], ring["thr"], drops, level=nd["level"], segs=segs)
        node_of_row = torch.cat([torch.arange(int(i.node_base), int(i.node_base) + g.rows(s), device=self.device) for s, i in enumerate(g.info)])
        # a multi-level cloud holds every point of the frame and the build keeps those of its rho shell (the top bits of axis 0 equal the
        # shell's path, which the snap leaves alone): `snapped` counts the points a tree holds, once each
        j_own, cuts = [], ring["point_cuts"]
        for s, (_, _, path, _) in enumerate(g.segments):
            j, path = ring["j_points"][int(cuts[s]):int(cuts[s + 1])], list(path or [])
            if path:
                bits = 0
                for p in path:
                    bits = (bits << 1) | int(p)
                j = j[torch.bitwise_right_shift(ring["x0"][int(cuts[s]):int(cuts[s + 1])], depths[s] - len(path)) == bits]
            j_own.append(j)
        ring.update(mask_rows=(jn[node_of_row] > 0).to(torch.uint8), leaves=[int(i.n_leaves) for i in g.info], n_frames=n_frames, j_own=j_own)
        self._ring_thr = ring["thr"]
        return ring

    def _ring_force(self, table, sym_coded, ring, plan, row_cuts=None):
        """ring_lod: the implied rows of the coding-order table forced to symbol 0, directly behind the model and in front of everything
        that reads the table (temper, CDF, rate).  ring: the state of `pre`.  -> (the `ring_lod` record - device int64 counters: [0] the
        implied rows whose symbol is NOT 0, the encoder's check of its own tree, then per frame its implied rows and its points per
        j = 0 .. RINGLOD_MAX -, the mask of the implied rows in coding order)."""
        F, K1 = ring["n_frames"], native.RINGLOD_MAX + 1
        mask = ring["mask_rows"][plan.coding_order_device(self.device)].contiguous()
        buf = torch.zeros(1 + F + F * K1, dtype=torch.int64, device=self.device)
        native.force_rows(table, mask, sym_coded, buf[:1])
        row_cuts = [0, plan.n_rows] if row_cuts is None else [int(c) for c in row_cuts]
        ns = len(ring["thr"]) // F
        for f in range(F):
            buf[1 + f] = mask[row_cuts[f]:row_cuts[f + 1]].sum()
            buf[1 + F + f * K1:1 + F + (f + 1) * K1] = torch.bincount(torch.cat(ring["j_own"][f * ns:(f + 1) * ns]).long(), minlength=K1)[:K1]
        return _Record("ring_lod", buf, (mask, ring), lambda h, frames, cuts: self._ring_entries(h, ring), self._ring_check), mask

    @staticmethod
    def _ring_check(h):
        """An implied row with a symbol other than 0: the tree is not the one the rule describes, and nothing of the frame is handed out."""
        if int(h[0]) != 0:
            raise native.ScpError(f"ring_lod: {int(h[0])} implied rows of the octree carry a symbol other than 0: the tree that was built is not "
                                  "the tree of the snapped points (internal error: nothing was written)")

    def _ring_entries(self, h, ring):
        """The host image of `_ring_force`'s counters and the state -> the `ring_lod` entry of every frame: edges, drops, thresholds and
        leaves per shell, snapped (points per j), implied_rows."""
        self._ring_check(h)
        edges, drops = self.ring_lod
        F, K1 = ring["n_frames"], native.RINGLOD_MAX + 1
        ns = len(ring["thr"]) // F
        return [dict(edges=list(edges), drops=list(drops), thresholds=[list(t) for t in ring["thr"][f * ns:(f + 1) * ns]],
                     snapped=[int(v) for v in h[1 + F + f * K1:1 + F + f * K1 + max(drops) + 1]], implied_rows=int(h[1 + f]),
                     leaves=ring["leaves"][f * ns:(f + 1) * ns]) for f in range(F)]

    def distortion_report(self, xyz_dev, edges=None, infos=None):
        """Where the D1 error of the frame just encoded goes (metrics.distortion_report on the cloud `distortion` measures): per range
        ring of `edges` (None: metrics.default_edges of the data type; other types must give edges) and, for the reconstructed points, per
        rho shell - `b_to_a["groups"][g]` holds exactly the leaves of shell g.  Sensor at the origin.  The dict gains `shell_leaves`."""
        from . import metrics
        edges = metrics.default_edges(self.data_type) if edges is None else edges
        pts = self._reconstructed(infos)
        group = torch.cat([torch.full((p.shape[0],), g, dtype=torch.int32, device=p.device) for g, p in enumerate(pts)])
        rep = metrics.distortion_report(xyz_dev[:, :3], torch.cat(pts), edges, quant_group=group, n_groups=len(pts))
        rep["shell_leaves"] = [int(p.shape[0]) for p in pts]
        return rep

    def _ring_frame(self, who, xyz_dev, edges, infos):
        """What `ring_rate` and `depth_report` (who) start from: the refusals of an encoder or a call that kept no rows; then the resolved
        edges, the reconstructed points per shell, the (shell, ring) bin of every one of them in leaf order, and the input points per
        ring (device int64 [rings])."""
        from . import metrics
        if not (self.rate and self.rate_rows):
            raise native.ScpError(f"{who} needs the per-row bits of the frame: make the encoder with rate=True and rate_rows=True (rate alone "
                                  "keeps per-level sums only)")
        if self._rate_rows is None:
            raise native.ScpError(f"{who}: no frame to report on - call it after a synchronous encode / encode_ints (the asynchronous and "
                                  "batch calls, and the record files of --preproc_path, leave no geometry and no rows behind)")
        edges = native.dist_edges(metrics.default_edges(self.data_type) if edges is None else edges)
        pts = self._reconstructed(infos)
        group = torch.cat([torch.full((p.shape[0],), g, dtype=torch.int32, device=p.device) for g, p in enumerate(pts)])
        bins = native.ring_bins(torch.cat(pts), edges, group, len(pts))
        points = torch.bincount(native.ring_bins(xyz_dev[:, :3], edges), minlength=len(edges))
        return edges, pts, bins, points

    def _share_args(self):
        """The arguments of native.rate_leaf_share for the frame whose rows `_rate_rows` holds: the node columns of the geometry, what
        every node cost (ideal, table), the segment table and the number of leaves."""
        row_ideal, row_table, plan = self._rate_rows
        g, dev = self.geom, self.device
        nd = g.nodes(("occ", "level", "parent"))
        # coding order -> frame-order row -> node: the rows of the segments lie back to back, a drop_last segment's last node has none
        node_of_row = torch.cat([torch.arange(int(i.node_base), int(i.node_base) + g.rows(s), device=dev) for s, i in enumerate(g.info)])
        bits_ideal, bits_table = native.node_bits(plan.coding_order_device(dev), node_of_row, row_ideal, row_table, g.total_nodes)
        return (nd["occ"], nd["level"], nd["parent"], bits_ideal, bits_table, native.share_table(g.info), sum(int(i.n_leaves) for i in g.info))

    def ring_rate(self, xyz_dev, edges=None, infos=None):
        """What every range ring and rho shell of the frame just encoded costs ("Rate per ring"): every node's ideal and
        coded-table bits are handed to the leaves below it in equal parts (csrc/ringrate.hip), and the leaves are summed over the bins of
        `distortion_report` - the reconstructed point's ring of `edges` (None: metrics.default_edges) and its shell.  Callable after a
        synchronous `encode` / `encode_ints` of an encoder made with rate=True and rate_rows=True, like `distortion_report`; the
        asynchronous and batch calls rebuild the geometry before they finish and keep no rows.  -> plain Python: edges,
        groups[shell][ring] (leaves, ideal_bits, table_bits, max_ideal_bits, ideal / table bits per leaf), rings[ring] (the shells
        added with math.fsum, and `points`: the input points whose own range lies in the ring), total, shell_leaves."""
        from . import metrics
        edges, pts, bins, points = self._ring_frame("ring_rate", xyz_dev, edges, infos)
        share = native.rate_leaf_share(*self._share_args())
        raw = native.share_segments(share["cost_ideal"], share["cost_table"], bins, len(pts) * len(edges))["raw"]
        rep = metrics.ring_rate_dict(edges, raw.cpu().numpy(), points.cpu().tolist(), len(pts))
        rep["shell_leaves"] = [int(p.shape[0]) for p in pts]
        return rep

    def lod_cells(self, k):
        """The cells of LOD k of the geometry just built, per shell: device int32 [C_s,3] origins in leaf units, in node (Morton) order -
        the leaves for k = 0, the nodes of level D_s - k + 1 for 1 <= k <= D_s - 1 ("Depth report").  The node origins are
        checked against `(leaf >> k) << k` of the shell's leaves."""
        g = self.geom
        if k == 0:
            return [g.leaves(s) for s in range(len(g.info))]
        nd = g.nodes(("level", "pos"))
        cells = []
        for s, i in enumerate(g.info):
            if not 1 <= k <= int(i.depth) - 1:
                raise native.ScpError(f"lod_cells: LOD {k} of a shell of depth {int(i.depth)}: 0 .. {int(i.depth) - 1} expected")
            sl = slice(int(i.node_base), int(i.node_base + i.n_nodes))
            c = nd["pos"][sl][nd["level"][sl] == int(i.depth) - k + 1].contiguous()
            want = torch.unique_consecutive(torch.bitwise_left_shift(torch.bitwise_right_shift(g.leaves(s), k), k), dim=0)
            if c.shape != want.shape or not torch.equal(c, want):
                raise native.ScpError(f"lod_cells: the origins of shell {s}'s level-{int(i.depth) - k + 1} nodes are not (leaf >> {k}) << {k} of its leaves")
            cells.append(c)
        return cells

    def depth_report(self, xyz_dev, max_drop=4, edges=None, infos=None):
        """What every octree level of the frame just encoded costs and buys ("Depth report"): for every truncation depth
        k = 0 .. max_drop the bits of levels 1 .. D - k per range ring and rho shell (csrc/ringrate.hip: `ring_rate` with every leaf's
        chain of ancestors cut k levels short, on ring_rate's bins - those of the FINEST reconstructed leaf, so that the columns of
        different k compare) and the D1 error of the cloud those levels describe: the centres of the level-(D - k + 1) nodes, through the
        encoder's own dequantiser.  Callable where `ring_rate` is.  max_drop: 0 .. the shallowest shell's depth - 1.  -> plain Python:
        edges, shell_leaves, shell_depths, levels[k] = dict(drop, cells per shell, rate = the ring_rate form on plane k, distortion =
        metrics.distortion_report of the LOD-k points against the input with groups = shells, d1 = metrics.chamfer_psnr of the same
        pair)."""
        from . import metrics
        edges, pts, bins, points = self._ring_frame("depth_report", xyz_dev, edges, infos)
        depths = [int(i.depth) for i in self.geom.info]
        if isinstance(max_drop, bool) or not isinstance(max_drop, int) or not 0 <= max_drop <= min(depths) - 1:
            raise native.ScpError(f"depth_report: max_drop {max_drop!r} outside 0 .. {min(depths) - 1}: the shells of this frame are {depths} levels "
                                  "deep and a tree keeps at least its root level")
        share = native.rate_depth_share(*self._share_args(), max_drop)
        infos, S = infos or self._infos, len(pts)
        raw = native.share_segments_depth(share["cost_ideal"], share["cost_table"], bins, S * len(edges))["raw"].cpu().numpy()
        points = points.cpu().tolist()
        peak, cells, dist, d1 = metrics.PEAK.get(self.data_type, 1.0), [], [], []
        for k in range(max_drop + 1):
            ck = self.lod_cells(k)
            pk = [metrics.dequantize(metrics.lod_centres(c, k), info.qs, info.offset, spher=self.spher, cylin=self.cylin,
                                     f32=not self.mullevel).double() for c, info in zip(ck, infos)]
            gk = torch.cat([torch.full((p.shape[0],), g, dtype=torch.int32, device=p.device) for g, p in enumerate(pk)])
            cells.append([int(c.shape[0]) for c in ck])
            dist.append(metrics.distortion_report(xyz_dev[:, :3], torch.cat(pk), edges, quant_group=gk, n_groups=S))
            d1.append(metrics.chamfer_psnr(xyz_dev[:, :3], torch.cat(pk), peak))
        return metrics.depth_dict(edges, raw, points, S, cells, dist, d1, [int(p.shape[0]) for p in pts], depths)

    def distortion(self, xyz_dev, infos=None, normals=None):
        """Chamfer distance and D1 PSNR of the frame just encoded (the octree of the last `encode` / `preprocess` call) against
        its input cloud, on the device - what the reference gets from distChamfer + the pc_error tool
        (encode_dataset_ehem.py:170-171, encode_dataset_ehem_mullevel.py:141-144; scp_amd/metrics.py).  With `normals` (device [P,3], one
        per input point: metrics.estimate_normals or a gene_normals.py file) the dict gains the D2 (point-to-plane) PSNR `psnr_d2` and its
        two directions `mse_ab_d2`, `mse_ba_d2`."""
        from . import metrics
        quant, peak = torch.cat(self._reconstructed(infos)), metrics.PEAK.get(self.data_type, 1.0)
        d = metrics.chamfer_psnr(xyz_dev, quant, peak)
        if normals is not None:
            p2 = metrics.d2_psnr(xyz_dev, normals, quant, peak)
            d.update(psnr_d2=p2["psnr_d2"], mse_ab_d2=p2["mse_ab"], mse_ba_d2=p2["mse_ba"])
        return d

    # ------------------------------------------------------------------------------------------ reflectance
    def attr_leaves(self):
        """Per shell the leaves of the geometry just built that a decoder will know (device int32 [U_s,3], Morton order): a multi-level
        shell's last BFS node is never coded, so its children - the last popcount(occ) leaves - are left out."""
        g, occ, out = self.geom, None, []
        for s, i in enumerate(g.info):
            lv = g.leaves(s)
            if g.segments[s][3] and int(i.n_nodes) > 0:
                if occ is None:
                    occ = g.nodes(("occ",))["occ"]
                last = int(occ[int(i.node_base) + int(i.n_nodes) - 1].item())
                lv = lv[:lv.shape[0] - bin(last).count("1")].contiguous()
            out.append(lv)
        return out

    def _attr_frame(self, who, xyz_dev, refl_dev, ints):
        """The checks of the reflectance entries and what they code on: (leaves, depths, qs, refl, points)."""
        if self.ring_lod is not None:
            raise native.ScpError(f"{who} with ring_lod: the leaves of such a tree are snapped cells of mixed sizes, and an attribute "
                                  "layer for them is not part of this library")
        if not self.geom.info:
            raise native.ScpError(f"{who}: no frame to code - call it after a synchronous encode / preprocess")
        xyz_dev = xyz_dev[:, :3].to(torch.float32).contiguous()
        refl_dev = refl_dev.reshape(-1).to(torch.float32).contiguous()
        if refl_dev.shape[0] != xyz_dev.shape[0]:
            raise native.ScpError(f"{who}: {refl_dev.shape[0]} reflectances for {xyz_dev.shape[0]} points")
        infos = self._infos
        try:
            qs = self.quantize(xyz_dev, ints)[0]         # the integers the tree was built from (the same quantiser, the same input)
        finally:
            self._infos = infos
        return self.attr_leaves(), [int(i.depth) for i in self.geom.info], [q.contiguous() for q in qs], refl_dev, int(xyz_dev.shape[0])

    @staticmethod
    def _with_target(who, sweep, Q, target, steps, code):
        """target = (kind, value): sweep() -> the table, the step that meets the target, code(Q) at that step, and the report with
        `target`, `chosen_Q`, `met` and the table as `sweep`.  Without a target: code(Q), nothing else."""
        from . import attr
        if target is None:
            if steps is not None:
                raise native.ScpError(f"{who}: steps is the grid of a target's sweep - give target as well")
            return code(Q)
        kind, value = attr.check_target(target, f"{who}: target")
        if int(Q) != 1:
            raise native.ScpError(f"{who}: Q = {Q} together with a target - the target chooses the step, leave Q at 1")
        table = sweep()
        pick = attr.choose_step(table, kind, value)
        data, rep = code(pick["Q"])
        rep.update(target=(kind, value), chosen_Q=pick["Q"], met=pick["met"], sweep=table)
        return data, rep

    def attr_sweep(self, xyz_dev, refl_dev, scale=None, steps=None, ints=None):
        """What every step of a grid costs and loses on the reflectance of the frame just encoded ("Step sweep"), in one pass
        per shell: attr.sweep_shells' table.  Preconditions and arguments as encode_attr's; steps: native.sweep_steps (None: the default
        grid of 16).  The PSNR of the table is over leaf values, not the point-wise PSNR of `--metrics`."""
        from . import attr
        leaves, depths, qs, refl, _ = self._attr_frame("attr_sweep", xyz_dev, refl_dev, ints)
        return attr.sweep_shells(leaves, depths, qs, refl, attr.default_scale(self.data_type) if scale is None else scale, steps)

    def encode_attr(self, xyz_dev, refl_dev, Q=1, scale=None, ints=None, chunk=None, want_overhead=False, target=None, steps=None):
        """The reflectance of the frame just encoded ("Reflectance"): codes one 8-bit value per leaf of the octree of the last
        `encode` / `preprocess` call, as `distortion` measures that octree - callable after a synchronous call.  xyz_dev device float32
        [P,>=3] and refl_dev device float32 [P] are the frame; Q = 1 .. 255 the step (1: lossless on the leaf values); scale: 8-bit units
        per unit of reflectance (None: 255 for KITTI, 1 for Ford); ints: the host integers of the frame where the encoder was given them;
        chunk = N: a version-2 file whose payloads the device codes in chunks of N symbols (None: version 1, the host coder), want_overhead:
        attr.encode_shells' `chunk_overhead_bits`.  target = (kind, value), kind "psnr" / "bpp" / "linf": the step comes from a sweep over
        `steps` (attr_sweep, attr.choose_step) and Q stays 1; the report gains target, chosen_Q, met and the table as `sweep`.
        -> (the bytes of `<stream>.attr`, report): attr.encode_shells' report plus n_points, bits_per_point, bits_per_leaf."""
        from . import attr
        leaves, depths, qs, refl_dev, n_points = self._attr_frame("encode_attr", xyz_dev, refl_dev, ints)
        scale = attr.default_scale(self.data_type) if scale is None else scale

        def code(step):
            data, rep = attr.encode_shells(leaves, depths, qs, refl_dev, step, scale, chunk=chunk, want_overhead=want_overhead)
            n_leaves = sum(int(lv.shape[0]) for lv in leaves)
            rep.update(n_points=n_points, bits_per_point=rep["bits"] / max(n_points, 1), bits_per_leaf=rep["bits"] / max(n_leaves, 1))
            return data, rep

        return self._with_target("encode_attr", lambda: attr.sweep_shells(leaves, depths, qs, refl_dev, scale, steps), Q, target, steps, code)

    # ------------------------------------------------------------------------------------------ colour
    def _color_frame(self, who, q_dev, rgb_dev):
        """The checks of the colour entries and what they code on: (leaves, depths, qs, rgb)."""
        if self.ring_lod is not None:
            raise native.ScpError(f"{who} with ring_lod: the leaves of such a tree are snapped cells of mixed sizes, and a colour "
                                  "layer for them is not part of this library")
        if not self.geom.info:
            raise native.ScpError(f"{who}: no frame to code - call it after a synchronous encode_ints")
        if len(self.geom.info) != 1:
            raise native.ScpError(f"{who}: the colour layer codes the one tree of an object cloud, this frame has {len(self.geom.info)} shells")
        if q_dev.dim() != 2 or q_dev.shape[1] != 3 or rgb_dev.shape != q_dev.shape or rgb_dev.dtype != torch.uint8:
            raise native.ScpError(f"{who}: q int32 [P,3] and rgb uint8 [P,3] expected, got {tuple(q_dev.shape)} and {tuple(rgb_dev.shape)} "
                                  f"{rgb_dev.dtype}")
        return self.attr_leaves(), [int(i.depth) for i in self.geom.info], [q_dev.to(torch.int32).contiguous()], rgb_dev.contiguous()

    def color_sweep(self, q_dev, rgb_dev, steps=None):
        """What every step of a grid costs and loses on the colour of the object cloud just encoded ("Step sweep"), in one
        pass: color.sweep_shells' table.  Preconditions and arguments as encode_color's; steps: native.sweep_steps.  The PSNR of the
        table is over leaf colours, not the point-wise PSNR of `--metrics`."""
        from . import color
        return color.sweep_shells(*self._color_frame("color_sweep", q_dev, rgb_dev), steps)

    def encode_color(self, q_dev, rgb_dev, Q=1, chunk=None, want_overhead=False, target=None, steps=None):
        """The colour of the object cloud just encoded ("Colour"): codes one RGB triple per leaf of the octree of the last
        synchronous `encode_ints` call.  q_dev device int32 [P,3]: the integers that tree was built from; rgb_dev device uint8 [P,3]: the
        points' 8-bit colours (color.point_colors); Q = 1 .. 255 the step of the three planes (1: lossless on the leaf means); chunk = N /
        want_overhead: a version-2 (chunked) file and its report fields, as for encode_attr; target / steps: the step from a sweep
        (color_sweep, color.choose_step), as for encode_attr.
        -> (the bytes of `<stream>.color`, report): color.encode_shells' report plus n_points, bits_per_point, bits_per_leaf."""
        from . import color
        leaves, depths, qs, rgb = self._color_frame("encode_color", q_dev, rgb_dev)

        def code(step):
            data, rep = color.encode_shells(leaves, depths, qs, rgb, step, chunk=chunk, want_overhead=want_overhead)
            n_leaves = sum(int(lv.shape[0]) for lv in leaves)
            rep.update(n_points=int(q_dev.shape[0]), bits_per_point=rep["bits"] / max(int(q_dev.shape[0]), 1), bits_per_leaf=rep["bits"] / max(n_leaves, 1))
            return data, rep

        return self._with_target("encode_color", lambda: color.sweep_shells(leaves, depths, qs, rgb, steps), Q, target, steps, code)

    def preprocess(self, xyz_dev, ints=None):
        # (ring_lod snaps the integers between the quantiser and the build: the route of the integer inputs)
        if ints is None and not self.host_transform and self.ring_lod is None:
            self._infos = self._build_xyz([xyz_dev])
            pre = self._tables(self._infos[0].bin_num, self._infos[0].offset[2] if self.cylin else 0.0, xyz_dev.shape[0])
        else:
            qs, bin_num, z_off = self.quantize(xyz_dev, ints)
            pre = self.preprocess_ints(qs, bin_num, z_off, xyz_dev.shape[0])
        pre["bin_nums"] = [float(i.bin_num) for i in self._infos]      # every shell's own (the file name carries the first)
        pre["quant"] = self.quant_info()                               # the steps and offsets the integers were made with (sidecar)
        return pre

    def _tables(self, bin_num, z_offset, n_points):
        """ctx / pos / coded symbols of every segment of the geometry just built, one launch (scp_geom_context_ehem_all)."""
        pos_mode = native.POS_MINMAX_MUL if self.mullevel else (native.POS_POW2 if self.mode == native.CART else native.POS_MINMAX)
        self._rate_rows = None           # a new geometry: the rows ring_rate would join it with are the previous frame's
        ctx, pos, sym_coded, mm = self.geom.context_ehem_all(pos_mode, self.lidar_level, self.context_size)
        sizes = []
        for s in range(len(self.geom.info)):
            counts = self.geom.level_counts(s)
            if self.mullevel:
                counts[-1] -= 1          # Octree.py:259-262: the records drop the last BFS node
            sizes += counts
        return dict(ctx=ctx, pos=pos, sym_coded=sym_coded, pos_mm=mm, level_sizes=sizes, bin_num=bin_num, z_offset=z_offset, n_points=n_points)

    def preprocess_ints(self, qs, bin_num, z_offset, n_points):
        """qs: per-shell quantised integer clouds (device int32 [P_s,3]) - the entry point for already-quantised input
        (the reference's --preproc_path flow).  -> ctx/pos/sym device tensors for all shells, level sizes, meta."""
        packed = getattr(qs, "packed", None)
        q = packed if packed is not None else (torch.cat(qs) if len(qs) > 1 else qs[0])
        if self.ring_lod is None:
            self.geom.build(q.contiguous(), self._segments(qs))
            return self._tables(bin_num, z_offset, n_points)
        q, ring = self._ring_snap(q.contiguous(), qs, self._infos)
        self.geom.build(q, self._segments(qs))
        ring = self._ring_mask(ring)
        pre = self._tables(bin_num, z_offset, n_points)
        pre["ring"] = ring
        return pre

    def preprocess_records(self, records, bin_num, z_offset, n_points):
        """--preproc_path flow (encode_dataset_ehem.py:149-157 + :52-105): the reference's int64 [N,4,6] record files (one per
        shell) -> the same ctx/pos/sym tables the device octree path produces.  Pure index plumbing on the device."""
        L = self.lidar_level
        ctxs, poss, syms, mms, sizes = [], [], [], [], []
        for rec in records:
            r = (torch.from_numpy(np.ascontiguousarray(rec, np.int64)) if isinstance(rec, np.ndarray) else rec).to(self.device)
            lvl = r[:, 3, 1]
            depth = int(lvl.max())
            counts = torch.bincount(lvl, minlength=depth + 1)[1:]
            last = (lvl == depth)[:, None]
            levels = torch.where(last, torch.clamp(r[:, :, 1], max=L), r[:, :, 1])          # ehem:86 clips the last chunk
            ctx = torch.stack((levels, r[:, :, 2], r[:, :, 0] - 1), 2).reshape(-1, 12).to(torch.uint8)
            p = r[:, 3, 3:6]
            if self.mode == native.CART and not self.mullevel:
                pos = (p.double() / float(2 ** depth)).float()
                mm = torch.zeros((depth, 2), dtype=torch.int64, device=self.device)
            else:
                mn = torch.full((depth + 1,), 2 ** 62, dtype=torch.int64, device=self.device).scatter_reduce(0, lvl, p.min(1)[0], "amin")
                mx = torch.full((depth + 1,), -2 ** 62, dtype=torch.int64, device=self.device).scatter_reduce(0, lvl, p.max(1)[0], "amax")
                eps = torch.where((lvl == depth) & torch.tensor(self.mullevel, device=self.device), 0.0, 1e-9).double()
                pos = ((p - mn[lvl][:, None]).double() / ((mx - mn)[lvl].double() + eps)[:, None]).float()
                mm = torch.stack((mn[1:], mx[1:]), 1)
            ctxs.append(ctx); poss.append(pos.contiguous()); syms.append((r[:, 3, 0] - 1).to(torch.uint8)); mms.append(mm)
            sizes += counts.tolist()
        return dict(ctx=torch.cat(ctxs), pos=torch.cat(poss), sym=torch.cat(syms), pos_mm=torch.cat(mms), level_sizes=sizes,
                    bin_num=bin_num, z_offset=z_offset, n_points=n_points)

    def encode_records(self, records, bin_num, z_offset, n_points, timing=False):
        """Encode from the reference's preprocessed record files (list of int64 [N,4,6], one per shell)."""
        t0 = time.perf_counter()
        if self.ring_lod is not None:
            raise native.ScpError("ring_lod with record files (--preproc_path): the records hold a finished octree, and the option snaps the "
                                  "points before the tree is built")
        return self._encode_pre(self.preprocess_records(records, bin_num, z_offset, n_points), t0, timing)

    # ------------------------------------------------------------------------------------------ stage M + C
    def logits_in_coding_order(self, pre, plan):
        with native.use_profile(self.profile):
            return self._logits_in_coding_order(pre, plan)

    def profile_string(self):
        return native.numeric_profile("EHEM", self.profile)

    def _logits_in_coding_order(self, pre, plan):
        if self.packed:
            return self.logits_packed(pre, plan)
        N = plan.n_rows
        table = torch.empty((N, 255), dtype=torch.float32, device=self.device)
        ctx, pos = pre["ctx"], pre["pos"]
        for c, ws in plan.groups(self.max_batch):
            starts = [w[0] for w in ws]
            if len(ws) == 1:
                bctx, bpos = ctx[starts[0]:starts[0] + c][None], pos[starts[0]:starts[0] + c][None]
            else:
                bctx = torch.stack([ctx[s:s + c] for s in starts])
                bpos = torch.stack([pos[s:s + c] for s in starts])
            o1, o2 = self.model.forward_ctx(bctx, bpos)
            ne = (c + 1) // 2
            for b, (start, _, coded) in enumerate(ws):
                table[coded:coded + ne] = o1[b]
                if c > 1:
                    table[coded + ne:coded + c] = o2[b]
        return table

    def logits_packed(self, pre, plan):
        """All windows of the frame through ONE packed forward per chunk of <= max_tokens tokens (models/packed.py); the last layer
        of both probability heads writes its rows straight into the coding-order table (row stride 256 floats: 16-byte rows)."""
        full = torch.empty((plan.n_rows, 256), dtype=torch.float32, device=self.device)
        ctx, pos = pre["ctx"], pre["pos"]
        for r0, tok, pp in (pre.get("packed_plans") or self.packed_plans(plan)):
            self.model.forward_packed(ctx[r0:r0 + tok], pos[r0:r0 + tok], None, plan=pp, table=full[r0:])
        return full[:, :255]

    def packed_plans(self, plan):
        """The frame's windows cut into chunks of <= max_tokens tokens, each with its index maps: [(first row, tokens, PackedPlan)]."""
        from .models.packed import PackedPlan
        ws = plan.windows
        return [(ws[i][0], sum(w[1] for w in ws[i:j]), PackedPlan([w[1] for w in ws[i:j]], device=self.device))
                for i, j in chunk_windows(ws, self.max_tokens)]

    def encode(self, xyz, timing=False):
        """xyz: numpy / torch float32 [P,3].  Returns dict(bytes, bits, bpp, n_nodes, n_points, bin_num, z_offset,
        n_levels, pos_mm (numpy [n_levels,2]), times)."""
        t0 = time.perf_counter()
        xyz = _as_tensor(xyz, np.float32)
        ints = self.host_ints(xyz) if self.host_transform else None        # from the caller's copy (no D2H of a frame just uploaded)
        xyz_dev = xyz.to(self.device, non_blocking=True)
        return self._encode_pre(self.preprocess(xyz_dev, ints), t0, timing)

    def encode_ints(self, qs, bin_num, z_offset, n_points, timing=False, infos=None):
        """Encode from already-quantised integer coordinates (list of per-shell int32 [P_s,3] arrays / tensors).  infos: the quantiser
        infos the integers were made with (ring_lod takes its thresholds from their steps and offsets); None: the last quantiser call's."""
        t0 = time.perf_counter()
        if infos is not None:
            self._infos = list(infos)
        dq = [_as_tensor(q, np.int32).to(self.device) for q in qs]
        return self._encode_pre(self.preprocess_ints(dq, bin_num, z_offset, n_points), t0, timing)

    # ------------------------------------------------------------------------------------------ pipelined variant
    def _front(self, xyz, ints, caller, batch=False):
        """Stage G and the window plans of one frame - batch: of a list of frames as ONE sequence of levels (preprocess_batch) - on the
        front stream (a side stream: launch-bound work with two small D2H syncs, which runs under the previous frames' model kernels
        instead of in front of this frame's).  -> everything the model part needs + the event it waits for."""
        torch.cuda.set_device(self.device)                     # (the current device is per host thread: this may be the front thread)
        frames = [_as_tensor(x, np.float32) for x in (xyz if batch else [xyz])]
        if self.host_transform and ints is None and not batch:
            ints = self.host_ints(frames[0])                   # from the caller's copy (no D2H of a frame just uploaded)
        front_stream = self._pipeline().front_stream
        with torch.cuda.stream(front_stream):
            front_stream.wait_stream(caller)                   # whatever produced `xyz` on the caller's stream
            dev_frames = [x.to(self.device, non_blocking=True) for x in frames]
            pre, metas = self.preprocess_batch(dev_frames, ints) if batch else (self.preprocess(dev_frames[0], ints), None)
            plan = EncodePlan(pre["level_sizes"], self.context_size)
            if self.packed:
                pre["packed_plans"] = self.packed_plans(plan)
            sym_coded = self._sym_coded(pre, plan)
            ready = torch.cuda.Event()
            ready.record()
        return dict(pre=pre, metas=metas, plan=plan, sym_coded=sym_coded, ready=ready, dev_frames=dev_frames)

    def front_async(self, xyz, ints=None):
        """Start a frame's front part (stage G, plans) on the encoder's FRONT THREAD and return a future for `encode_async(..., front=)`.
        The front part blocks its host thread for most of a frame time - its ~35 small dependent kernels each wait for a gap between the
        whole-GPU model kernels of the frames in flight (33 - 43 ms per frame in `bench.py`, against 0.4 ms alone on the GPU) - so a loop that
        calls this one frame ahead keeps the launch thread free for the model part (ctypes and torch release the GIL while they wait).
        Call order = frame order: the front thread takes the frames one at a time (one `scp_geom` handle)."""
        self._pipeline()
        if self._front_pool is None:
            self._front_pool = ThreadPoolExecutor(max_workers=1)
        caller = torch.cuda.current_stream(self.device)
        return self._front_pool.submit(self._front, xyz, ints, caller)

    def _model_async(self, front, main, fills0, t0, cuts=None):
        """The model part and the coding tail of a front part on the lane `main`, the range coder behind them -> the handle.  The handle
        keeps the front part (everything allocated on the front stream: frames, tables, plans) and the tail (the logits table, the pairs,
        the options' buffers) referenced until finish(), i.e. past their last use on `main`, so the caching allocator cannot hand them
        out again early."""
        pre, plan = front["pre"], front["plan"]
        main.wait_event(front["ready"])
        with torch.cuda.stream(main):
            tail = self._code_table(self.logits_in_coding_order(pre, plan), front["sym_coded"], plan.level_sizes, pre.get("ring"), plan, cuts)
        return dict(future=self._pipeline().submit(main, tail, fills0), t0=t0, front=front, tail=tail)

    def encode_async(self, xyz, ints=None, front=None):
        """Like encode(), but the front part runs on the front stream, the model part on the next lane, and the D2H copy of the
        (c_low, c_high) pairs and the serial host range coder on a worker thread (_CoderPipeline), so the caller can enqueue the next
        frame while this one is being coded.  Returns a handle; `finish(handle)` blocks and returns the usual result dict.
        ints: the result of `host_ints(xyz)` when the caller has already computed it (strict-identity mode, CLI reader thread).
        front: the future `front_async(xyz, ints)` returned for this frame (then xyz / ints are not looked at again)."""
        t0, caller, main, fills0 = self._begin_async()
        return self._model_async(front.result() if front is not None else self._front(xyz, ints, caller), main, fills0, t0)

    # ------------------------------------------------------------------------------------------ batches of small frames
    def preprocess_batch(self, frames, ints=None):
        """Stage G of k frames at once: one scp_geom_build with every (frame, shell) as a segment - one radix sort, one tree pass - and
        the frames' context tables back to back.  Frames share nothing (encode.py:274-291 rebuilds everything per frame): the batch is
        ONE sequence of levels - the frames' level lists one after the other - for the window plan, the packed forward and the CDF
        kernel, and is cut into frames again in front of the range coder.  Returns (combined `pre`, per-frame meta).
        ints: per frame the result of `host_ints(frame)` when the caller has computed it already (strict-identity mode, a prefetch thread)."""
        ns = len(self.shells())
        if len(frames) * ns > 62:
            raise native.ScpError("a batch holds at most 62 (frame, shell) trees (SCP_MAX_SEGMENTS)")
        ring = None
        if self.host_transform or ints is not None or self.ring_lod is not None:
            qs_all, infos = [], []
            for f, xyz_dev in enumerate(frames):
                if self.host_transform or ints is not None:
                    hq, inf = ints[f] if ints is not None else self.host_ints(xyz_dev)
                    qs_all += _upload_ints(hq, self.device)
                else:                                  # ring_lod: the device quantiser, shell by shell, then the snap below
                    qs_all += self._quantize_device(xyz_dev)
                    inf = self._infos
                infos += inf
            q = torch.cat(qs_all).contiguous()
            if self.ring_lod is not None:
                q, ring = self._ring_snap(q, qs_all, infos)
            self.geom.build(q, self._segments(qs_all))
        else:
            infos = self._build_xyz(frames)
        self._infos = infos[-ns:]
        if ring is not None:
            ring = self._ring_mask(ring, len(frames))
        pre = self._tables(infos[0].bin_num, 0.0, 0)
        if ring is not None:
            pre["ring"] = ring
        metas, sizes, mm0 = [], pre["level_sizes"], 0
        depths = [i.depth for i in self.geom.info]
        for f, xyz_dev in enumerate(frames):
            fi = infos[f * ns:(f + 1) * ns]
            nl = sum(depths[f * ns:(f + 1) * ns])
            fsizes = sizes[mm0:mm0 + nl]
            metas.append(dict(bin_num=fi[0].bin_num, z_offset=(fi[0].offset[2] if self.cylin else 0.0), n_points=int(xyz_dev.shape[0]),
                              bin_nums=[float(i.bin_num) for i in fi], quant=_quant_of(fi), pos_mm=pre["pos_mm"][mm0:mm0 + nl],
                              level_sizes=fsizes, n_nodes=int(sum(fsizes))))
            mm0 += nl
        out = dict(ctx=pre["ctx"], pos=pre["pos"], sym_coded=pre["sym_coded"], level_sizes=sizes)
        if ring is not None:
            out["ring"] = pre["ring"]
        return out, metas

    def encode_batch_async(self, frames, ints=None):
        """k frames through ONE stage G, ONE packed forward and ONE CDF launch (the small-frame configurations: a level-12 frame has
        22 windows, far too few for an MI355X - BASELINE.json configs[1] is a batch of 16 of them), on the same streams as encode_async.
        The streams are byte-identical to the per-frame path (every kernel is per window / per row).  Returns a handle for finish_batch().
        ints: [host_ints(frame) for every frame] when the caller has them already (strict-identity mode)."""
        t0, caller, main, fills0 = self._begin_async()
        front = self._front(frames, ints, caller, batch=True)
        cuts = np.concatenate(([0], np.cumsum([m["n_nodes"] for m in front["metas"]])))
        return self._model_async(front, main, fills0, t0, cuts)

    def _sym_coded(self, pre, plan):
        """The coded symbols in coding order: written by the context kernel itself (scp_geom_context_ehem_all), or - for tables that
        did not come out of it (the --preproc_path record files) - gathered through the plan's coding-order index."""
        if pre.get("sym_coded") is not None:
            return pre["sym_coded"]
        return pre["sym"][plan.coding_order_device(self.device)].contiguous()

    @staticmethod
    def _meta(pre, n_nodes):
        """The result fields of one frame out of its `pre` (preprocess*), or out of its entry of preprocess_batch's per-frame list."""
        return dict(n_nodes=n_nodes, n_points=pre["n_points"], bin_num=pre["bin_num"], z_offset=pre["z_offset"], n_levels=len(pre["level_sizes"]),
                    pos_mm=pre["pos_mm"].cpu().numpy(), level_sizes=pre["level_sizes"], bin_nums=pre.get("bin_nums", [float(pre["bin_num"])]),
                    quant=pre.get("quant"))

    def finish_batch(self, h):
        metas = h["front"]["metas"]
        streams = h["future"].result()
        return _finish(h["tail"], [self._meta(m, m["n_nodes"]) for m in metas], streams, dict(total=(time.perf_counter() - h["t0"]) / len(metas)))

    def finish(self, h):
        stream = h["future"].result()
        meta = self._meta(h["front"]["pre"], h["front"]["plan"].n_rows)
        return _finish(h["tail"], [meta], [stream], dict(total=time.perf_counter() - h["t0"]))[0]

    def _encode_pre(self, pre, t0, timing):
        if timing:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        plan = EncodePlan(pre["level_sizes"], self.context_size)
        table = self.logits_in_coding_order(pre, plan)
        sym_coded = self._sym_coded(pre, plan)
        if timing:
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        keep_rows = self.rate and self.rate_rows and pre.get("sym_coded") is not None      # (record files: no geometry to join the rows with)
        tail = self._code_table(table, sym_coded, plan.level_sizes, pre.get("ring"), plan, keep_rows=keep_rows)
        self._rate_rows = (*tail.rows, plan) if keep_rows else None
        stream, t3, t4 = _code_now(tail)            # (raises before anything is coded when an implied row carries a symbol other than 0)
        debug = dict(table=table, sym_coded=sym_coded, pre=pre)
        if tail.implied is not None:
            debug["implied"] = tail.implied
        return _finish(tail, [self._meta(pre, plan.n_rows)], [stream], dict(geom=t1 - t0, model=t2 - t1, cdf=t3 - t2, coder=t4 - t3, total=t4 - t0),
                       debug)[0]

    def outfile(self, base, res):
        """encode.py:140-144 file name; a ring-LOD and a tempered stream say so in front of the coordinate token
        (`..._ringlod_temper_spher_<levels>_<bin>_<z>.bin`)."""
        base = self._temper_token(self._ring_token(base))
        if self.spher:
            base += "_spher"
        elif self.cylin:
            base += "_cylin"
        return base + "_" + str(res["n_levels"]) + "_" + str(int(res["bin_num"])) + "_" + str(int(res["z_offset"])) + ".bin"


class OctAttnFrameEncoder(_FrontEnd):
    """OctAttention path.  Same-level (encode.py:23-82 `compress` + dataloaders/encode_dataset.py:32-55): one BFS sequence,
    front-padded with context_size-1 rows (occ 255), cut into consecutive 1024-windows; node r is predicted at position
    (r+1023) % 1024 of window (r+1023) // 1024.  Plain BFS coding order.  `--cylin` is wired here (the reference forgot to, SURVEY B-7).

    Multi-level / level-wise (encode_mullevel.py:23-86 `compress` + dataloaders/encode_dataset_mullevel.py:27-119): the frame is a
    LIST of sequences ("chunks") - one per rho shell ([0,0] at qs(L), [0,1] at qs(L+1), [1] at qs(L+2); records without the last
    BFS node, Octree.py:259-262), and with `level_wise` one per octree level of every shell - each front-padded and windowed on
    its own, positions divided by 2^(the shell's deepest level); the PMF rows of the chunks are stacked in order
    (`probabilities[:-1023]`) and coded as one stream.  File name `<base>[_spher]_<chunks>_<bin_num>_0.bin`."""

    LANES_ENV = "SCP_LANES_OCTATTN"

    def __init__(self, model, data_type=KITTI, lidar_level=12, spher=True, cylin=False, max_batch=128, device=None, mullevel=False,
                 level_wise=False, named=False, host_transform=None, decodable=False, rate=False, temper=None, temper_grid=None, ring_lod=None):
        if parse_ring_lod(ring_lod) is not None:
            raise native.ScpError("OctAttention: ring_lod is not available - its decoder has no forced rows; the EHEM encoders have the option")
        if temper == "code":
            raise native.ScpError("OctAttention: temper='code' is not available - the decodable profile decodes one node per step, and a "
                                  "tempered form of it is not part of this library; temper='report' measures what it would save")
        # decodable=True: the octattn/1d numeric profile (models/oct_attention.py) - every PMF row a function of its own window's rows
        # 0..t, so OctAttnFrameDecoder can reproduce it node by node; the default (octattn/1) keeps the round-6 bits
        self.decodable = bool(decodable)
        if self.decodable and mullevel:
            raise native.ScpError("--decodable: multi-level OctAttention streams (three shells) have no decoder; encode with encode.py")
        if mullevel and (cylin or not spher):
            # encode_dataset_mullevel.py:76-86: the three-shell records exist for --spher only
            raise native.ScpError("OctAttention multi-level encoding needs --spher (encode_dataset_mullevel.py:76)")
        super().__init__(model, data_type, lidar_level, spher, cylin, mullevel, max_batch, device, host_transform, rate,
                         temper=temper, temper_grid=temper_grid)
        self.level_wise = level_wise
        self.named = named or mullevel        # encode_mullevel.py's file-name scheme (also for its single-shell Cartesian input)

    def quantize(self, xyz_dev):
        if self.host_transform:
            from .data_preproc.data_preprocess import host_quantize_shells
            out = host_quantize_shells(np.ascontiguousarray(xyz_dev.cpu().numpy(), np.float32), self.mode, *self._quant_args())
            self._infos = [i for _, i in out]
            qs = [torch.from_numpy(q).to(self.device) for q, _ in out]
        else:
            qs = self._quantize_device(xyz_dev)
        return qs, self._infos[0].bin_num

    def profile_string(self):
        return native.numeric_profile("OctAttention", None, decodable=self.decodable)

    def encode(self, xyz, timing=False, sequential=False):
        t0 = time.perf_counter()
        xyz = _as_tensor(xyz, np.float32)
        xyz_dev = xyz.to(self.device)
        if not self.host_transform:
            bin_num = self.build_from_xyz(xyz_dev)
            return self.encode_ints(None, bin_num, xyz_dev.shape[0], t0, sequential=sequential, front=self._front(None), quant=self.quant_info())
        qs, bin_num = self.quantize(xyz_dev)
        return self.encode_ints(qs, bin_num, xyz_dev.shape[0], t0, sequential=sequential, quant=self.quant_info())

    def _sequential_rows(self, seq_ctx, seq_pos, N, table):
        """`--sequential` (encode.py:38-41,55-56): a window starts at EVERY row of the padded sequence and only the prediction
        of its last position is kept, i.e. node r is predicted from its full 1023-node history (window r .. r + 1023).
        The reference's loop runs past the last full window with shrinking windows that all end at the last node and
        overwrite its row; the last one (that node alone) wins - reproduced.  ~context_size x the model calls of the default
        mode: batches of `max_batch` windows are gathered with a strided view, one forward each."""
        cs = self.context_size
        wc = seq_ctx.unfold(0, cs, 1).permute(0, 2, 1)               # [N, cs, 12] view: window i = rows i .. i + cs - 1
        wp = seq_pos.unfold(0, cs, 1).permute(0, 3, 1, 2)            # [N, cs, 4, 3]
        for b0 in range(0, N, self.max_batch):
            b1 = min(N, b0 + self.max_batch)
            out = self.model(wc[b0:b1].reshape(b1 - b0, cs, 4, 3), wp[b0:b1].contiguous())
            table[b0:b1] = out[:, -1]
        if cs > 1:
            table[N - 1] = self.model(seq_ctx[-1:].reshape(1, 1, 4, 3), seq_pos[-1:].reshape(1, 1, 4, 3))[0, -1]

    def build_from_xyz(self, xyz_dev):
        """Device transform: stage G1 + G2 in one launch sequence (scp_geom_build_xyz) -> bin_num of the first shell."""
        self._infos = self._build_xyz([xyz_dev])
        return self._infos[0].bin_num

    def _front(self, qs):
        """stage G + the front-padded context sequences (encode_dataset.py:32-55 / encode_dataset_mullevel.py:44-73) on the
        current stream.  qs: one integer cloud, or the list of per-shell clouds; None: the geometry has been built already
        (build_from_xyz).  -> (chunks [(seq_ctx, seq_pos, n)], sym, N)."""
        if qs is not None:
            if not isinstance(qs, (list, tuple)):
                qs = [qs]
            if len(qs) != len(self.shells()):
                raise native.ScpError(f"expected {len(self.shells())} integer cloud(s), got {len(qs)}")
            self.geom.build((torch.cat(qs) if len(qs) > 1 else qs[0]).contiguous(), self._segments(qs))
        segs = self.geom.segments
        cs = self.context_size
        pad_ctx = torch.zeros((cs - 1, 12), dtype=torch.uint8, device=self.device)
        pad_ctx[:, 0::3] = 255
        pad_pos = torch.zeros((cs - 1, 4, 3), dtype=torch.float32, device=self.device)
        chunks, syms = [], []
        for s in range(len(segs)):
            ctx, pos, sym = self.geom.context_octattn(s)
            counts = self.geom.level_counts(s)
            if self.mullevel:
                counts[-1] -= 1                      # the records drop the last BFS node (Octree.py:259-262)
                if counts[-1] == 0:                  # ... and with it the deepest level (the kernel's positions are over 2^(max level present))
                    counts.pop()
            syms.append(sym)
            cuts = counts if self.level_wise else [ctx.shape[0]]
            a = 0
            for n in cuts:
                chunks.append((torch.cat((pad_ctx, ctx[a:a + n])), torch.cat((pad_pos, pos[a:a + n])), n))
                a += n
        sym = torch.cat(syms) if len(syms) > 1 else syms[0]
        return chunks, sym, int(sym.shape[0])

    def _chunk_rows(self, chunks, table):
        """Default mode: consecutive windows of context_size over every padded chunk; all windows of the frame (whatever chunk they belong to)
        share batched forwards.  Round 6: a chunk's shorter TAIL window rides in the same forwards, padded behind its last row to a full window
        - the model is causal (attention_model.py:58-95: row i attends to rows <= i; everything else is per row), so the rows in front of the
        padding come out as in a forward of the short window alone (bit for bit under the decodable profile; under the default one the
        attention's launch-wide V scale makes them agree to rounding only), and the frame saves that forward's ~45 launches on one window (1 ms of a
        15 ms L12 frame)."""
        cs = self.context_size
        full_c, full_p, dst = [], [], []       # windows + (table row of the window's first real node, leading pad rows, real rows in the window)
        row = 0
        for seq_ctx, seq_pos, n in chunks:
            total = n + cs - 1
            n_full = total // cs
            for w in range(n_full):
                full_c.append(seq_ctx[w * cs:(w + 1) * cs])
                full_p.append(seq_pos[w * cs:(w + 1) * cs])
                lo = max(w * cs - (cs - 1), 0)
                dst.append((row + lo, lo + (cs - 1) - w * cs, cs))
            k = total - n_full * cs
            if k:
                # (padding rows: the front padding's rows - valid embedding indices - and zero positions)
                full_c.append(torch.cat((seq_ctx[n_full * cs:], seq_ctx[:cs - k])))
                full_p.append(torch.cat((seq_pos[n_full * cs:], torch.zeros_like(seq_pos[:cs - k]))))
                lo = n_full * cs - (cs - 1)
                dst.append((row + max(lo, 0), max(-lo, 0), k))
            row += n
        # forwards of EQUAL size (round 6): 286 windows under max_batch = 128 ran as 128 + 128 + 30 - the short third forward fills the chip
        # badly (26.4 - 26.7 frames/s at L14 --cylin) - and run as 96 + 96 + 94 (27.2)
        nfw = -(-len(dst) // self.max_batch) if dst else 0
        step = -(-len(dst) // nfw) if nfw else 1
        for b0 in range(0, len(dst), step):
            b1 = min(len(dst), b0 + step)
            contiguous = len(chunks) == 1 and all(d[2] == cs for d in dst[b0:b1])
            if contiguous:                     # one sequence: its full windows are one contiguous block (no copy)
                d = chunks[0][0][b0 * cs:b1 * cs].reshape(b1 - b0, cs, 4, 3)
                p = chunks[0][1][b0 * cs:b1 * cs].reshape(b1 - b0, cs, 4, 3)
            else:
                d = torch.stack(full_c[b0:b1]).reshape(b1 - b0, cs, 4, 3)
                p = torch.stack(full_p[b0:b1])
            out = self.model(d, p).reshape(-1, 255)
            # consecutive full windows of one chunk cover consecutive table rows: one copy per run (the first window of a chunk
            # starts with its cs - 1 pad rows; a tail window ends its run with its real rows)
            i = 0
            while i < b1 - b0:
                j = i + 1
                while (j < b1 - b0 and dst[b0 + j - 1][2] == cs and dst[b0 + j][1] == 0 and
                       dst[b0 + j][0] == dst[b0 + j - 1][0] + cs - dst[b0 + j - 1][1]):
                    j += 1
                r0, skip, _ = dst[b0 + i]
                rows = (j - 1 - i) * cs + dst[b0 + j - 1][2] - skip
                table[r0:r0 + rows] = out[i * cs + skip:i * cs + skip + rows]
                i = j

    def _logits(self, chunks, N, sequential=False):
        """The frame's logits table [N,255] in coding order (plain BFS, chunk after chunk) on the current stream."""
        table = torch.empty((N, 255), dtype=torch.float32, device=self.device)
        prev = self.model.decodable
        self.model.decodable = self.decodable
        try:
            if sequential:
                row = 0
                for seq_ctx, seq_pos, n in chunks:
                    self._sequential_rows(seq_ctx, seq_pos, n, table[row:row + n])
                    row += n
            else:
                self._chunk_rows(chunks, table)
        finally:
            self.model.decodable = prev
        return table

    def _code_front(self, front, bin_num, n_points, quant, sequential=False):
        """What the synchronous and the asynchronous call share behind `_front`: the table, its coding tail on the current stream, and
        the frame's meta fields.  -> (tail, meta)."""
        chunks, sym, N = front
        sizes = [c[2] for c in chunks]
        tail = self._code_table(self._logits(chunks, N, sequential), sym, sizes)
        z_off = float(quant[0]["offset"][2]) if (quant and self.cylin) else 0.0
        return tail, dict(n_nodes=N, n_points=n_points, bin_num=bin_num, z_offset=z_off, quant=quant, n_levels=len(chunks), pos_mm=np.zeros((0, 2)),
                          level_sizes=sizes, depth=int(self.geom.info[0].depth), sequential=bool(sequential))

    def encode_ints(self, q, bin_num, n_points, t0=None, sequential=False, front=None, quant=None):
        """q: integer cloud (numpy / tensor int32 [P,3]) or the list of per-shell clouds of the multi-level form.  quant: per shell
        dict(qs, offset) the integers were made with (`quant_info()`), kept in the result - `z_offset` is its cylindrical z offset - for
        the side-info file; None: unknown (z offset 0)."""
        t0 = t0 or time.perf_counter()
        if front is None:
            qs = q if isinstance(q, (list, tuple)) else [q]
            qs = [_as_tensor(x, np.int32).to(self.device) for x in qs]
            front = self._front(qs)
        if sequential and self.decodable:
            raise native.ScpError("--decodable with --sequential: each node's window slides, so a decoder has no cache to keep")
        tail, meta = self._code_front(front, bin_num, n_points, quant, sequential)
        stream = _code_now(tail)[0]
        return _finish(tail, [meta], [stream], dict(total=time.perf_counter() - t0), dict(table=tail.table, sym_coded=tail.sym_coded))[0]

    def encode_async(self, xyz):
        """Like encode(), but stage G runs on the front stream, the model part on the next lane, and the D2H copy of the (c_low, c_high)
        pairs and the serial host range coder on a worker thread (_CoderPipeline): the caller can enqueue the next frame while this
        one is being coded.  `finish(handle)` blocks and returns the usual result dict."""
        t0, caller, main, fills0 = self._begin_async()
        xyz, pipe = _as_tensor(xyz, np.float32), self._pipeline()
        with torch.cuda.stream(pipe.front_stream):
            pipe.front_stream.wait_stream(caller)
            xyz_dev = xyz.to(self.device, non_blocking=True)
            if not self.host_transform:
                q, bin_num = None, self.build_from_xyz(xyz_dev)
            else:
                q, bin_num = self.quantize(xyz_dev)
            front = self._front(q)
            ready = torch.cuda.Event()
            ready.record()
        main.wait_event(ready)
        with torch.cuda.stream(main):
            tail, meta = self._code_front(front, bin_num, xyz_dev.shape[0], self.quant_info())
        # (the handle keeps what the front stream allocated - the frame, its integers, the context sequences - and the tail referenced
        # until finish(): see FrameEncoder._model_async)
        return dict(future=pipe.submit(main, tail, fills0), meta=meta, t0=t0, front=(xyz_dev, q, front), tail=tail)

    def finish(self, h):
        return _finish(h["tail"], [h["meta"]], [h["future"].result()], dict(total=time.perf_counter() - h["t0"]))[0]

    def outfile(self, base, res):
        """encode.py:24 (`<base>.bin`) / encode_mullevel.py:68-72 (`<base>[_spher|_cylin]_<chunks>_<bin_num>_0.bin`)."""
        if not self.named:
            return base + ".bin"
        if self.spher:
            base += "_spher"
        elif self.cylin:
            base += "_cylin"
        return base + "_" + str(res["n_levels"]) + "_" + str(int(res["bin_num"])) + "_0.bin"
