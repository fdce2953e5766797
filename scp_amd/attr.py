"""Reflectance layer ("Reflectance"): the host side of csrc/attr.hip - the 16 fixed tables, the table choice, the
`<stream>.attr` file, and the two drivers `encode_shells` / `decode_shells` that FrameEncoder.encode_attr and decode_file(attr=True) call.

The transform itself (leaf values, lifting, inverse, the coder's pairs) runs on the device in exact integers; what happens here is the
choice of one table per octree level (transmitted, so its float arithmetic need not be reproducible), the serial range coder, and bytes.
With chunk = N (a version-2 file, DESIGN.md 6, "Chunked payloads") the coder runs on the device too, on all chunks of a payload at once
(csrc/ac_chunks.hip); the readers take the version from the file."""
import struct

import numpy as np
import torch

from . import native

MAGIC, VERSION, VERSION_CHUNKED = b"SCPA", 1, 2                 # version 2: chunked payloads (include/scp.h, "Chunk-parallel range coder")
ALPHABET = native.ATTR_ALPHABET
RATIOS = (32, 64, 96, 128, 152, 176, 192, 208, 216, 224, 232, 238, 243, 247, 250, 253)
_TABLES = {}


def tables(alphabet=ALPHABET):
    """uint16 [16, alphabet + 1]: cdf rows of the 16 geometric tables over z = 2 |k| - (k > 0), built from integers only.  Row g: b_0 = 2^24,
    b_m = (b_(m-1) R[g]) >> 8, u[z] = b_((z+1)>>1), c[z] = 1 + ((65536 - alphabet) u[z]) // sum(u), the rest of 65536 to c[0];
    cdf = [0, cumsum(c)] with the last entry (65536) wrapped to 0.  alphabet: 511 (the reflectance layer, |k| <= 255) or 1021 (the colour
    layer, |k| <= 510: b_0 .. b_510)."""
    alphabet = int(alphabet)
    if alphabet not in (ALPHABET, native.COLOR_ALPHABET):
        raise native.ScpError(f"attr.tables: an alphabet of {ALPHABET} or {native.COLOR_ALPHABET} symbols expected, got {alphabet}")
    if alphabet not in _TABLES:
        out = np.zeros((len(RATIOS), alphabet + 1), np.uint16)
        for g, R in enumerate(RATIOS):
            b = [1 << 24]
            for _ in range((alphabet + 1) >> 1):
                b.append((b[-1] * R) >> 8)
            u = [b[(z + 1) >> 1] for z in range(alphabet)]
            su = sum(u)
            c = [1 + ((65536 - alphabet) * v) // su for v in u]
            c[0] += 65536 - sum(c)
            acc, row = 0, [0]
            for v in c:
                acc += v
                row.append(acc)
            out[g] = np.array(row, np.int64).astype(np.uint16)          # 65536 -> 0
        out.setflags(write=False)
        _TABLES[alphabet] = out
    return _TABLES[alphabet]


def table_counts(alphabet=ALPHABET):
    """int64 [16, alphabet]: the counts c[z] of every table (they sum to 65536 per row)."""
    t = tables(alphabet).astype(np.int64)
    hi = t[:, 1:].copy()
    hi[:, -1] = 65536
    return hi - t[:, :-1]


def choose_tables(hist, alphabet=ALPHABET):
    """hist int [D, alphabet] -> (choice int [D]: per context the table with the fewest bits sum_z hist[z] (16 - log2 c[z]), the lower index on a
    tie; bits float64 [D] under the choice)."""
    hist = np.asarray(hist, np.float64).reshape(-1, alphabet)
    cost = hist @ (16.0 - np.log2(table_counts(alphabet).astype(np.float64))).T   # [D, 16]
    choice = np.argmin(cost, axis=1)                                               # (the first minimum: the lower g)
    return choice.astype(np.int64), cost[np.arange(len(choice)), choice]


def chunk_count(n, N):
    """The chunks of a payload of n symbols at N symbols per chunk."""
    return -(-int(n) // int(N))


def chunked_blob(who, n, N, s):
    """pack's side of a version-2 payload: the shell's `lengths` (C integers) and `payload` (the C chunks back to back) -> the length
    table followed by the chunks, after both were found to fit the n symbols of the shell."""
    lengths, payload = [int(v) for v in s["lengths"]], bytes(s["payload"])
    if len(lengths) != chunk_count(n, N):
        raise native.ScpError(f"{who}: {len(lengths)} chunk lengths for {n} symbols in chunks of {N}, {chunk_count(n, N)} expected")
    if any(not 0 <= v < 1 << 32 for v in lengths) or sum(lengths) != len(payload):
        raise native.ScpError(f"{who}: the chunk lengths add up to {sum(lengths)}, the chunks hold {len(payload)} bytes")
    return np.asarray(lengths, "<u4").tobytes() + payload


def chunked_split(noun, k, n, N, blob):
    """unpack's side: the payload of shell k (n symbols, chunks of N) -> (lengths uint32 [C], the chunks back to back); a payload too
    short for its length table, or whose lengths do not add up to the rest, is refused."""
    C = chunk_count(n, N)
    if len(blob) < 4 * C:
        raise native.ScpError(f"{noun}: shell {k}'s payload of {len(blob)} bytes cannot hold the {C} chunk lengths of {n} symbols in chunks of {N}")
    lengths = np.frombuffer(blob[:4 * C], "<u4").astype(np.uint32)
    if int(lengths.sum(dtype=np.int64)) != len(blob) - 4 * C:
        raise native.ScpError(f"{noun}: shell {k}'s {C} chunk lengths add up to {int(lengths.sum(dtype=np.int64))}, its payload holds "
                              f"{len(blob) - 4 * C} bytes behind them")
    return lengths, blob[4 * C:]


def read_chunk_size(r):
    """The chunk size behind the fixed header of a version-2 file (r: its Reader)."""
    N = struct.unpack("<I", r.take(4, "the chunk size"))[0]
    if not native.CHUNK_MIN <= N <= native.CHUNK_MAX:
        raise native.ScpError(f"{r.noun}: a version-{VERSION_CHUNKED} file with a chunk size of {N} symbols, outside {native.CHUNK_MIN} .. 2^20")
    return N


def pack(Q, scale, shells, chunk=None):
    """shells: per shell dict(D, U, root, tables (D indices for j = D .. 1), payload bytes) -> the bytes of `<stream>.attr`.  chunk = N:
    a version-2 file - the shells with U >= 2 hold `lengths` (one per chunk of N symbols) and, as `payload`, the chunks back to back;
    None: version 1."""
    if not 1 <= int(Q) <= 255 or not 1 <= int(scale) <= 1 << 20 or len(shells) > 255:
        raise native.ScpError(f"attr.pack: Q {Q} outside 1 .. 255, scale {scale} outside 1 .. 2^20 or {len(shells)} shells")
    head, body = [MAGIC + struct.pack("<BBIB", VERSION if chunk is None else VERSION_CHUNKED, int(Q), int(scale), len(shells))], []
    if chunk is not None:
        head.append(struct.pack("<I", native.check_chunk(chunk, "attr.pack: chunk size")))
    for s in shells:
        D, U = int(s["D"]), int(s["U"])
        head.append(struct.pack("<BI", D, U))
        if U >= 1:
            head.append(struct.pack("<B", int(s["root"])))
        if U >= 2:
            idx = [int(t) for t in s["tables"]]
            if len(idx) != D or not all(0 <= t < len(RATIOS) for t in idx):
                raise native.ScpError(f"attr.pack: {D} table indices below {len(RATIOS)} expected, got {idx}")
            blob = bytes(s["payload"]) if chunk is None else chunked_blob("attr.pack", U - 1, chunk, s)
            head.append(bytes(idx) + struct.pack("<I", len(blob)))
            body.append(blob)
    return b"".join(head + body)


class Reader:
    """Bounds-checked reads from the bytes of a layer's file; noun ("attribute file", "colour file") opens its refusals."""

    def __init__(self, data, noun):
        self.data, self.noun, self.pos = bytes(data), noun, 0

    def take(self, n, what):
        if self.pos + n > len(self.data):
            raise native.ScpError(f"{self.noun}: truncated in {what} ({len(self.data)} bytes)")
        self.pos += n
        return self.data[self.pos - n:self.pos]

    def end(self):
        if self.pos != len(self.data):
            raise native.ScpError(f"{self.noun}: {len(self.data) - self.pos} bytes behind the last payload")


def unpack(data, info=None):
    """The bytes of `<stream>.attr` -> (Q, scale, shells as `pack` takes them); anything else is refused with the reason.  info: a dict
    that receives the file's `version` and `chunk` (N of a version-2 file, whose shells with U >= 2 carry `lengths`; None for version 1)."""
    r = Reader(data, "attribute file")
    take = r.take
    if take(4, "the magic") != MAGIC:
        raise native.ScpError("attribute file: no 'SCPA' magic - not written by encode*.py --attr")
    version, Q, scale, n = struct.unpack("<BBIB", take(7, "the header"))
    if version not in (VERSION, VERSION_CHUNKED):
        raise native.ScpError(f"attribute file: version {version}, this library reads versions {VERSION} and {VERSION_CHUNKED}")
    chunk = read_chunk_size(r) if version == VERSION_CHUNKED else None
    if info is not None:
        info.update(version=version, chunk=chunk)
    if not 1 <= Q <= 255 or not 1 <= scale <= 1 << 20:
        raise native.ScpError(f"attribute file: Q {Q} outside 1 .. 255 or scale {scale} outside 1 .. 2^20")
    shells = []
    for k in range(n):
        D, U = struct.unpack("<BI", take(5, f"shell {k}"))
        s = dict(D=D, U=U, root=None, tables=[], payload=b"", length=0)
        if U >= 1:
            s["root"] = take(1, f"shell {k}'s root value")[0]
        if U >= 2:
            if not 1 <= D <= native.MAX_DEPTH:
                raise native.ScpError(f"attribute file: shell {k} of depth {D}")
            s["tables"] = list(take(D, f"shell {k}'s table indices"))
            if any(t >= len(RATIOS) for t in s["tables"]):
                raise native.ScpError(f"attribute file: shell {k} names table {max(s['tables'])} of {len(RATIOS)}")
            s["length"] = struct.unpack("<I", take(4, f"shell {k}'s payload length"))[0]
        shells.append(s)
    for k, s in enumerate(shells):
        s["payload"] = take(s.pop("length"), f"shell {k}'s payload")
        if chunk is not None and s["U"] >= 2:
            s["lengths"], s["payload"] = chunked_split("attribute file", k, s["U"] - 1, chunk, s["payload"])
    r.end()
    return Q, scale, shells


def level_contexts(counts):
    """level_counts [D + 1] (n_0 = U .. n_D = 1) -> uint8 [U - 1]: the context (level - 1) of every coefficient in coding order."""
    counts = [int(c) for c in counts]
    D = len(counts) - 1
    return np.concatenate([np.full(counts[j - 1] - counts[j], j - 1, np.uint8) for j in range(D, 0, -1)] + [np.zeros(0, np.uint8)])


def symbols_to_coefficients(z):
    """z = 2 |k| - (k > 0) -> k (int16)."""
    z = np.asarray(z, np.int32)
    return np.where(z & 1, (z + 1) >> 1, -(z >> 1)).astype(np.int16)


def default_scale(data_type):
    """255 for KITTI (reflectance in [0, 1]), 1 for Ford (0 .. 255 already)."""
    return 1 if data_type == "ford" else 255


def encode_payload(f, pairs, alphabet, chunk=None, want_overhead=False):
    """f: what a forward entry returns (k, ctx, hist), pairs: the layer's pairs entry -> (choice int [contexts], ideal bits float64
    [contexts], the payload): one table per context, the device's (c_low, c_high) pairs, then chunk = None (version 1): the host range
    coder on the pairs, the payload bytes; chunk = N (version 2): the device coder on all chunks at once - the pairs stay on the device -
    and the payload as dict(lengths uint32 [C], payload: the chunks back to back, serial_bytes: with want_overhead the size of the
    version-1 payload of the same pairs, which costs a host coder run, else None)."""
    choice, bits = choose_tables(f["hist"].cpu().numpy(), alphabet)
    dev_tabs = torch.from_numpy(tables(alphabet)[choice].view(np.int16).copy()).to(f["k"].device)
    lohi = pairs(f["k"], f["ctx"], dev_tabs)
    if chunk is None:
        return choice, bits, native.ac_encode_lohi(lohi.cpu().numpy())
    lengths, data = native.ac_chunks_encode(lohi, chunk)
    serial = len(native.ac_encode_lohi(lohi.cpu().numpy())) if want_overhead else None
    return choice, bits, dict(lengths=lengths, payload=data, serial_bytes=serial)


def chunk_report(chunk, p):
    """The chunked fields of a shell's report from encode_payload's version-2 payload p: chunk, chunks, and - where the serial size was
    asked for - chunk_overhead_bits = the length table + the version-2 chunks - the version-1 payload of the same pairs."""
    C = int(p["lengths"].shape[0])
    rep = dict(chunk=int(chunk), chunks=C)
    if p["serial_bytes"] is not None:
        rep["chunk_overhead_bits"] = 8 * (4 * C + len(p["payload"]) - p["serial_bytes"])
    return rep


def shells_on_geometry(noun, shells, leaves, depths):
    """The shells of an unpacked file against the decoded geometry: per shell (k, shell, leaves as contiguous int32, U, D), after the
    shell count and the shell's D and U were found to be the geometry's.  A generator: every check runs when the caller's loop reaches it,
    the shell count's at the first step."""
    if len(shells) != len(leaves):
        raise native.ScpError(f"{noun}: {len(shells)} shells, the geometry stream has {len(leaves)}")
    for k, (s, lv, D) in enumerate(zip(shells, leaves, depths)):
        U, D = int(lv.shape[0]), int(D)
        if s["D"] != D or s["U"] != U:
            raise native.ScpError(f"{noun}: shell {k} was coded on {s['U']} leaves of depth {s['D']}, the geometry stream decodes to "
                                  f"{U} leaves of depth {D} - it belongs to another stream")
        yield k, s, lv.to(torch.int32).contiguous(), U, D


def decode_payload(noun, k, payload, table_of, lv, D, channels, alphabet, chunk=None, lengths=None):
    """The payload of shell k (U >= 2 leaves lv) -> its coefficients, device int16 [channels, U - 1].  table_of: per context channel * D +
    (level - 1) the index of its table.  Every coefficient's context follows from the level counts of the tree alone - so with chunk = N
    and the chunk lengths (a version-2 file) all chunks are decoded at once on the device, where contexts, symbols and the symbol ->
    coefficient map stay."""
    U = int(lv.shape[0])
    counts = native.attr_level_counts(lv, D)
    if chunk is not None:
        reps = (counts[:-1] - counts[1:]).flip(0).clamp(min=0)                  # levels D .. 1
        level = torch.repeat_interleave(torch.arange(D - 1, -1, -1, dtype=torch.uint8, device=lv.device), reps)
        if level.shape[0] != U - 1:
            raise native.ScpError(f"{noun}: shell {k}'s leaves are not a Morton-ordered set ({level.shape[0]} coefficients for {U} leaves)")
        ctx = torch.cat([level + c * D for c in range(channels)])
        z = native.ac_chunks_decode(payload, lengths, chunk, tables(alphabet), table_of, ctx, alphabet + 1).to(torch.int32)
        return torch.where((z & 1) != 0, (z + 1) >> 1, -(z >> 1)).to(torch.int16).reshape(channels, U - 1)
    level = level_contexts(counts.cpu().numpy())
    if level.shape[0] != U - 1:
        raise native.ScpError(f"{noun}: shell {k}'s leaves are not a Morton-ordered set ({level.shape[0]} coefficients for {U} leaves)")
    ctx = np.concatenate([level + np.uint8(c * D) for c in range(channels)])
    z = native.AcDecoder(payload, Lp=alphabet + 1).run_ctx(tables(alphabet)[table_of], ctx)
    return torch.from_numpy(symbols_to_coefficients(z).reshape(channels, U - 1)).to(lv.device)


def encode_shells(leaves, depths, qs, refl, Q=1, scale=255, chunk=None, want_overhead=False):
    """leaves: per shell device int32 [U_s,3] in Morton order (Geom.leaves, a multi-level shell's unknown leaves dropped); depths: per
    shell; qs: per shell the quantised points, device int32 [P,3]; refl device float32 [P].  -> (bytes of the attribute file, report):
    report = dict(Q, scale, shells = [dict(U, depth, bits, level_bits (ideal bits under the chosen table, levels D .. 1), tables, root)],
    bits, values (per shell device uint8 [U]: the leaf values that were coded), counts (int32 [U]: points per leaf), decoded (uint8 [U]:
    what a decoder gets back - `values` itself at Q = 1)).  chunk = N: a version-2 file, every payload cut into chunks of N symbols
    that the device codes at once (None: version 1, the host coder); the report gains `chunk` and every coded shell `chunk`, `chunks` and,
    with want_overhead (a host coder run per shell), `chunk_overhead_bits`."""
    Q, scale = int(Q), int(scale)
    if chunk is not None:
        chunk = native.check_chunk(chunk, "attribute chunk size")
    if not 1 <= Q <= 255:
        raise native.ScpError(f"attribute step Q = {Q} outside 1 .. 255")
    if not 1 <= scale <= 1 << 20:
        raise native.ScpError(f"attribute scale {scale} outside 1 .. 2^20")
    packed, rep, values, counts, decoded = [], [], [], [], []
    for lv, D, q in zip(leaves, depths, qs):
        U, D = int(lv.shape[0]), int(D)
        a, cnt = native.attr_leaf_values(q, refl, lv, D, scale)
        values.append(a)
        counts.append(cnt)
        if U == 0:
            packed.append(dict(D=D, U=0))
            rep.append(dict(U=0, depth=D, bits=0, level_bits=[], tables=[], root=None))
            decoded.append(a)
            continue
        f = native.attr_forward(lv, a, D, Q)
        root = int(f["root"].item())
        if U == 1:
            packed.append(dict(D=D, U=1, root=root))
            rep.append(dict(U=1, depth=D, bits=0, level_bits=[], tables=[], root=root))
            decoded.append(a)
            continue
        choice, bits, payload = encode_payload(f, native.attr_pairs, ALPHABET, chunk, want_overhead)
        order = list(range(D - 1, -1, -1))                                       # the file lists j = D .. 1
        extra = {}
        if chunk is not None:
            extra, nbytes = chunk_report(chunk, payload), 4 * len(payload["lengths"]) + len(payload["payload"])
            packed.append(dict(D=D, U=U, root=root, tables=[int(choice[c]) for c in order], lengths=payload["lengths"], payload=payload["payload"]))
        else:
            nbytes = len(payload)
            packed.append(dict(D=D, U=U, root=root, tables=[int(choice[c]) for c in order], payload=payload))
        rep.append(dict(U=U, depth=D, bits=8 * nbytes, level_bits=[float(bits[c]) for c in order],
                        tables=[int(choice[c]) for c in order], root=root, **extra))
        decoded.append(a if Q == 1 else native.attr_inverse(lv, D, Q, root, f["k"]))
    data = pack(Q, scale, packed, chunk)
    report = dict(Q=Q, scale=scale, shells=rep, bits=8 * len(data), values=values, counts=counts, decoded=decoded)
    if chunk is not None:
        report["chunk"] = chunk
    return data, report


TARGET_KINDS = ("psnr", "bpp", "linf")


def check_target(target, who="target"):
    """(kind, value) of a rate or quality target -> (kind, float value): kind is one of TARGET_KINDS, value finite and >= 0."""
    try:
        kind, value = target
        value = float(value)
    except (TypeError, ValueError):
        raise native.ScpError(f"{who}: a pair (kind, value) expected, got {target!r}") from None
    if kind not in TARGET_KINDS:
        raise native.ScpError(f"{who}: unknown kind {kind!r}, one of {', '.join(TARGET_KINDS)} expected")
    if not np.isfinite(value) or value < 0:
        raise native.ScpError(f"{who}: {kind}={value} - a finite value >= 0 expected")
    return kind, value


def leaf_psnr(sse, n):
    """10 log10(255^2 n / sse) over n leaf values with the squared error sse; inf at zero error (and for no value at all)."""
    return float("inf") if sse == 0 or n == 0 else 10.0 * float(np.log10(255.0 ** 2 * n / sse))


def sweep_rows(steps, channels, frame_bytes, shells):
    """The table of a frame's sweep: steps [G]; frame_bytes the header and shell records `pack` writes for the frame (no payload);
    shells: per coded shell (U, hist [G, contexts, alphabet], sse [G, channels], linf [G, channels]) as host arrays, per uncoded shell
    (U, None, None, None).  -> per step dict(Q, table_bits, est_bits, sse, linf, leaves, psnr) and, for more than one channel, sse_rgb /
    linf_rgb / psnr_rgb per channel.  PSNR is over leaf values - what the layer codes against what it returns."""
    U_all = sum(int(s[0]) for s in shells)
    rows = []
    for g, Q in enumerate(steps):
        table_bits, nbytes = 0.0, int(frame_bytes)
        sse, linf = [0] * channels, [0] * channels
        for U, hist, s2, smax in shells:
            if hist is None:
                continue
            bits = float(choose_tables(hist[g], hist.shape[-1])[1].sum())
            table_bits += bits
            nbytes += int(np.ceil(bits / 8.0))
            sse = [a + int(b) for a, b in zip(sse, s2[g])]
            linf = [max(a, int(b)) for a, b in zip(linf, smax[g])]
        row = dict(Q=int(Q), table_bits=table_bits, est_bits=8 * nbytes, sse=sum(sse), linf=max(linf), leaves=U_all,
                   psnr=leaf_psnr(sum(sse), channels * U_all))
        if channels > 1:
            row.update(sse_rgb=sse, linf_rgb=linf, psnr_rgb=[leaf_psnr(v, U_all) for v in sse])
        rows.append(row)
    return rows


def record_bytes(D, U):
    """The bytes of a shell's record in the header of `<stream>.attr`: D, U, the root (U >= 1), D table indices and the payload length
    (U >= 2)."""
    return 5 + (1 if U >= 1 else 0) + (D + 4 if U >= 2 else 0)


def sweep_shells(leaves, depths, qs, refl, scale=255, steps=None):
    """One pass per shell over a grid of steps (native.attr_sweep; DESIGN.md 6, "Step sweep"), summed over the shells of a frame since a
    file has one Q.  Arguments as encode_shells'; steps: native.sweep_steps.  -> dict(steps, points, leaves, rows): per step Q, table_bits
    (choose_tables on that step's histograms, summed over contexts and shells, float64), est_bits (8 x (the header and shell-record bytes
    of a version-1 file + ceil(table_bits / 8) per coded shell)), sse, linf, leaves, psnr = 10 log10(255^2 leaves / sse) - the PSNR over
    LEAF VALUES, what the layer codes against what it returns, not the point-wise nearest-neighbour PSNR of --metrics."""
    scale = int(scale)
    if not 1 <= scale <= 1 << 20:
        raise native.ScpError(f"attribute scale {scale} outside 1 .. 2^20")
    grid = native.sweep_steps(steps)
    if len(leaves) > 255:
        raise native.ScpError(f"attr.sweep_shells: {len(leaves)} shells, an attribute file holds at most 255")
    frame_bytes, shells = 4 + 7, []
    for lv, D, q in zip(leaves, depths, qs):
        U, D = int(lv.shape[0]), int(D)
        frame_bytes += record_bytes(D, U)
        if U < 2:
            shells.append((U, None, None, None))
            continue
        a, _ = native.attr_leaf_values(q, refl, lv, D, scale)
        s = native.attr_sweep(lv, a, D, grid)
        shells.append((U, s["hist"].cpu().numpy(), s["sse"].cpu().numpy(), s["linf"].cpu().numpy()))
    return dict(steps=[int(v) for v in grid], points=int(refl.shape[0]), leaves=sum(s[0] for s in shells),
                rows=sweep_rows(grid, 1, frame_bytes, shells))


def choose_step(sweep, kind, value):
    """The step of a sweep table (sweep_shells) for a target: psnr - the largest step whose leaf PSNR is >= value; linf - the largest step
    whose largest error (over the channels) is <= value; bpp - the smallest step whose est_bits <= value x points.  Every row is looked
    at: the error need not grow with the step.  No step qualifies: the smallest step for psnr / linf, the largest for bpp, met = False.
    -> dict(kind, value, Q, index, met).  A pure host function."""
    kind, value = check_target((kind, value), "choose_step")
    rows = sweep["rows"]
    if not rows:
        raise native.ScpError("choose_step: an empty sweep table")
    if kind == "psnr":
        ok = [i for i, r in enumerate(rows) if r["psnr"] >= value]
    elif kind == "linf":
        ok = [i for i, r in enumerate(rows) if r["linf"] <= value]
    else:
        ok = [i for i, r in enumerate(rows) if r["est_bits"] <= value * sweep["points"]]
    by_q = sorted(range(len(rows)), key=lambda i: rows[i]["Q"])
    if ok:
        i = (min if kind == "bpp" else max)(ok, key=lambda i: rows[i]["Q"])
    else:
        i = by_q[-1] if kind == "bpp" else by_q[0]
    return dict(kind=kind, value=value, Q=int(rows[i]["Q"]), index=i, met=bool(ok))


def decode_shells(data, leaves, depths, info=None):
    """The bytes of an attribute file + the decoded geometry (per shell device int32 / int64 [U,3] leaves in the decoder's order, and the
    depths) -> per shell the device uint8 [U] leaf values.  D and U of every shell must be the geometry's.  info: a dict that receives
    the file's Q and scale.  The file's version decides the coder: version 1 the host's, version 2 (chunked) the device's."""
    meta = {}
    Q, scale, shells = unpack(data, meta)
    if info is not None:
        info.update(Q=Q, scale=scale)
    out = []
    for k, s, lv, U, D in shells_on_geometry("attribute file", shells, leaves, depths):
        if U == 0:
            out.append(torch.empty(0, dtype=torch.uint8, device=lv.device))
            continue
        if U == 1:
            out.append(torch.full((1,), s["root"], dtype=torch.uint8, device=lv.device))
            continue
        table_of = [s["tables"][D - 1 - c] for c in range(D)]                    # context c is level c + 1; the file lists j = D .. 1
        coef = decode_payload("attribute file", k, s["payload"], table_of, lv, D, 1, ALPHABET, meta["chunk"], s.get("lengths"))
        out.append(native.attr_inverse(lv, D, Q, s["root"], coef[0]))
    return out


def point_values(refl, scale):
    """The 8-bit value of every reflectance (device float32 [P]) as scp_attr_leaf_values takes it: int64 [P]."""
    r = refl.double()
    v = torch.floor(r * float(scale) + 0.5).clamp(0.0, 255.0)
    return torch.where(torch.isfinite(r), v, torch.zeros_like(v)).to(torch.int64)


def reflectance_psnr(xyz, refl, points, values, scale):
    """The reflectance PSNR of a decoded frame: xyz [P,3] / refl [P] the input, points [U,3] / values uint8 [U] the decoded cloud (device
    tensors).  Both directions through native.nn_error_split's indices (the lowest index among equally near points), errors in 8-bit
    units, PSNR = 10 log10(255^2 / max(mse_ab, mse_ba)); the sums are over int64 squares, hence exact.  -> dict(psnr, mse_ab, mse_ba)."""
    v = point_values(refl.to(torch.float32), scale)
    w = values.to(torch.int64)
    ab = native.nn_error_split(xyz[:, :3], points, (0.0,))["idx"].long()
    ba = native.nn_error_split(points, xyz[:, :3], (0.0,))["idx"].long()
    mse_ab = float(torch.sum((v - w[ab]) ** 2).item()) / v.shape[0]
    mse_ba = float(torch.sum((w - v[ba]) ** 2).item()) / w.shape[0]
    worst = max(mse_ab, mse_ba)
    return dict(psnr=float("inf") if worst == 0 else 10.0 * float(np.log10(255.0 ** 2 / worst)), mse_ab=mse_ab, mse_ba=mse_ba)
