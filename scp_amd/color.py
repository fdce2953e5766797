"""Colour layer ("Colour"): the host side of csrc/color.hip - the `<stream>.color` file, the two drivers `encode_shells` /
`decode_shells` that FrameEncoder.encode_color and decode_file(color=True) call, and the colour PSNR.

Leaf means, the YCoCg-R transform, the lifting of the three planes, its inverse and the coder's pairs run on the device in exact integers;
here are the 8-bit value of a reader's float colour, the choice of one of attr.py's 16 tables (its 1021-symbol form) per context channel * D
+ (level - 1), which is transmitted, the serial range coder, and bytes."""
import struct

import numpy as np
import torch

from . import attr, native

MAGIC, VERSION, TRANSFORM_YCOCG_R = b"SCPC", 1, 1
ALPHABET = native.COLOR_ALPHABET


def point_colors(rgb):
    """The 8-bit colour of every point: float [P,3] (device or host tensor) -> uint8 [P,3], clamp(floor(c + 0.5), 0, 255), 0 where c is not
    finite.  float32 + 0.5 is exact up to 2^23, far beyond the clamp."""
    c = rgb.to(torch.float32)
    v = torch.floor(c.double() + 0.5).clamp(0.0, 255.0)
    return torch.where(torch.isfinite(c), v, torch.zeros_like(v)).to(torch.uint8).contiguous()


def pack(Q, shells, chunk=None):
    """shells: per shell dict(D, U, root (Y, Co, Cg), tables (3 D indices, channel-major, levels D .. 1), payload bytes) -> the bytes of
    `<stream>.color`.  chunk = N: a version-2 file - the shells with U >= 2 hold `lengths` (one per chunk of N symbols) and, as
    `payload`, the chunks back to back; None: version 1."""
    if not 1 <= int(Q) <= 255 or len(shells) > 255:
        raise native.ScpError(f"color.pack: Q {Q} outside 1 .. 255 or {len(shells)} shells")
    head, body = [MAGIC + struct.pack("<BBBB", VERSION if chunk is None else attr.VERSION_CHUNKED, int(Q), TRANSFORM_YCOCG_R, len(shells))], []
    if chunk is not None:
        head.append(struct.pack("<I", native.check_chunk(chunk, "color.pack: chunk size")))
    for s in shells:
        D, U = int(s["D"]), int(s["U"])
        head.append(struct.pack("<BI", D, U))
        if U >= 1:
            y, co, cg = (int(v) for v in s["root"])
            if not (0 <= y <= 255 and -255 <= co <= 255 and -255 <= cg <= 255):
                raise native.ScpError(f"color.pack: roots {(y, co, cg)} outside Y 0 .. 255, Co / Cg -255 .. 255")
            head.append(struct.pack("<Bhh", y, co, cg))
        if U >= 2:
            idx = [int(t) for t in s["tables"]]
            if len(idx) != 3 * D or not all(0 <= t < len(attr.RATIOS) for t in idx):
                raise native.ScpError(f"color.pack: {3 * D} table indices below {len(attr.RATIOS)} expected, got {idx}")
            blob = bytes(s["payload"]) if chunk is None else attr.chunked_blob("color.pack", 3 * (U - 1), chunk, s)
            head.append(bytes(idx) + struct.pack("<I", len(blob)))
            body.append(blob)
    return b"".join(head + body)


def unpack(data, info=None):
    """The bytes of `<stream>.color` -> (Q, shells as `pack` takes them); anything else is refused with the reason.  info: a dict that
    receives the file's `version` and `chunk` (N of a version-2 file, whose shells with U >= 2 carry `lengths`; None for version 1)."""
    r = attr.Reader(data, "colour file")
    take = r.take
    if take(4, "the magic") != MAGIC:
        raise native.ScpError("colour file: no 'SCPC' magic - not written by encode.py --color")
    version, Q, transform, n = struct.unpack("<BBBB", take(4, "the header"))
    if version not in (VERSION, attr.VERSION_CHUNKED):
        raise native.ScpError(f"colour file: version {version}, this library reads versions {VERSION} and {attr.VERSION_CHUNKED}")
    if transform != TRANSFORM_YCOCG_R:
        raise native.ScpError(f"colour file: unknown colour transform {transform}, this library knows {TRANSFORM_YCOCG_R} (YCoCg-R)")
    if not 1 <= Q <= 255:
        raise native.ScpError(f"colour file: Q {Q} outside 1 .. 255")
    chunk = attr.read_chunk_size(r) if version == attr.VERSION_CHUNKED else None
    if info is not None:
        info.update(version=version, chunk=chunk)
    shells = []
    for k in range(n):
        D, U = struct.unpack("<BI", take(5, f"shell {k}"))
        s = dict(D=D, U=U, root=None, tables=[], payload=b"", length=0)
        if U >= 1:
            s["root"] = struct.unpack("<Bhh", take(5, f"shell {k}'s root values"))
            if not all(-255 <= v <= 255 for v in s["root"]):
                raise native.ScpError(f"colour file: shell {k}'s roots {s['root']} outside Y 0 .. 255, Co / Cg -255 .. 255")
        if U >= 2:
            if not 1 <= D <= native.MAX_DEPTH:
                raise native.ScpError(f"colour file: shell {k} of depth {D}")
            s["tables"] = list(take(3 * D, f"shell {k}'s table indices"))
            if any(t >= len(attr.RATIOS) for t in s["tables"]):
                raise native.ScpError(f"colour file: shell {k} names table {max(s['tables'])} of {len(attr.RATIOS)}")
            s["length"] = struct.unpack("<I", take(4, f"shell {k}'s payload length"))[0]
        shells.append(s)
    for k, s in enumerate(shells):
        s["payload"] = take(s.pop("length"), f"shell {k}'s payload")
        if chunk is not None and s["U"] >= 2:
            s["lengths"], s["payload"] = attr.chunked_split("colour file", k, 3 * (s["U"] - 1), chunk, s["payload"])
    r.end()
    return Q, shells


def _file_order(D):
    """The contexts channel * D + (level - 1) in the order the file lists them: channel-major, levels D .. 1."""
    return [c * D + j for c in range(3) for j in range(D - 1, -1, -1)]


def encode_shells(leaves, depths, qs, rgb, Q=1, chunk=None, want_overhead=False):
    """leaves: per shell device int32 [U_s,3] in Morton order; depths: per shell; qs: per shell the integer points, device int32 [P,3];
    rgb device uint8 [P,3].  -> (bytes of the colour file, report): report = dict(Q, shells = [dict(U, depth, bits, level_bits ([3][D]:
    ideal bits under the chosen table per channel, levels D .. 1), tables (likewise), roots)], bits, values (per shell device uint8 [U,3]:
    the leaf means that were coded), counts (int32 [U]), decoded (uint8 [U,3]: what a decoder gets back - `values` itself at Q = 1)).
    chunk = N / want_overhead: a version-2 file and its report fields, as in attr.encode_shells."""
    Q = int(Q)
    if chunk is not None:
        chunk = native.check_chunk(chunk, "colour chunk size")
    if not 1 <= Q <= 255:
        raise native.ScpError(f"colour step Q = {Q} outside 1 .. 255")
    packed, rep, values, counts, decoded = [], [], [], [], []
    for lv, D, q in zip(leaves, depths, qs):
        U, D = int(lv.shape[0]), int(D)
        mean, ycc, cnt = native.color_leaf_values(q, rgb, lv, D)
        values.append(mean)
        counts.append(cnt)
        decoded.append(mean)
        if U == 0:
            packed.append(dict(D=D, U=0))
            rep.append(dict(U=0, depth=D, bits=0, level_bits=[], tables=[], roots=None))
            continue
        f = native.color_forward(lv, ycc, D, Q)
        roots = [int(v) for v in f["root"].cpu().tolist()]
        if U == 1:
            packed.append(dict(D=D, U=1, root=roots))
            rep.append(dict(U=1, depth=D, bits=0, level_bits=[], tables=[], roots=roots))
            continue
        choice, bits, payload = attr.encode_payload(f, native.color_pairs, ALPHABET, chunk, want_overhead)    # [3 D], by context
        order = _file_order(D)
        extra = {}
        if chunk is not None:
            extra, nbytes = attr.chunk_report(chunk, payload), 4 * len(payload["lengths"]) + len(payload["payload"])
            packed.append(dict(D=D, U=U, root=roots, tables=[int(choice[c]) for c in order], lengths=payload["lengths"], payload=payload["payload"]))
        else:
            nbytes = len(payload)
            packed.append(dict(D=D, U=U, root=roots, tables=[int(choice[c]) for c in order], payload=payload))
        rep.append(dict(U=U, depth=D, bits=8 * nbytes, level_bits=[[float(bits[c]) for c in order[ch * D:(ch + 1) * D]] for ch in range(3)],
                        tables=[[int(choice[c]) for c in order[ch * D:(ch + 1) * D]] for ch in range(3)], roots=roots, **extra))
        if Q != 1:
            decoded[-1] = native.color_inverse(lv, D, Q, roots, f["k"])
    data = pack(Q, packed, chunk)
    report = dict(Q=Q, shells=rep, bits=8 * len(data), values=values, counts=counts, decoded=decoded)
    if chunk is not None:
        report["chunk"] = chunk
    return data, report


def record_bytes(D, U):
    """The bytes of a shell's record in the header of `<stream>.color`: D, U, the roots (U >= 1), 3 D table indices and the payload length
    (U >= 2)."""
    return 5 + (5 if U >= 1 else 0) + (3 * D + 4 if U >= 2 else 0)


def sweep_shells(leaves, depths, qs, rgb, steps=None):
    """One pass per shell over a grid of steps (native.color_sweep; DESIGN.md 6, "Step sweep").  Arguments as encode_shells'; steps:
    native.sweep_steps.  -> dict(steps, points, leaves, rows) as attr.sweep_shells, with sse / linf / psnr over the three channels
    (psnr = 10 log10(255^2 3 leaves / sum(sse)), linf the largest error of any channel) and sse_rgb / linf_rgb / psnr_rgb per channel.
    The PSNR is over LEAF COLOURS - the leaf means the layer codes against what it returns - not the point-wise PSNR of --metrics."""
    grid = native.sweep_steps(steps)
    if len(leaves) > 255:
        raise native.ScpError(f"color.sweep_shells: {len(leaves)} shells, a colour file holds at most 255")
    frame_bytes, shells = 4 + 4, []
    for lv, D, q in zip(leaves, depths, qs):
        U, D = int(lv.shape[0]), int(D)
        frame_bytes += record_bytes(D, U)
        if U < 2:
            shells.append((U, None, None, None))
            continue
        mean, ycc, _ = native.color_leaf_values(q, rgb, lv, D)
        s = native.color_sweep(lv, ycc, mean, D, grid)
        shells.append((U, s["hist"].cpu().numpy(), s["sse"].cpu().numpy(), s["linf"].cpu().numpy()))
    return dict(steps=[int(v) for v in grid], points=int(rgb.shape[0]), leaves=sum(s[0] for s in shells),
                rows=attr.sweep_rows(grid, 3, frame_bytes, shells))


choose_step = attr.choose_step


def decode_shells(data, leaves, depths, info=None):
    """The bytes of a colour file + the decoded geometry (per shell device int32 / int64 [U,3] leaves in the decoder's order, and the
    depths) -> per shell the device uint8 [U,3] leaf colours.  D and U of every shell must be the geometry's.  info: a dict that
    receives the file's Q.  The file's version decides the coder: version 1 the host's, version 2 (chunked) the device's."""
    meta = {}
    Q, shells = unpack(data, meta)
    if info is not None:
        info.update(Q=Q)
    out = []
    for k, s, lv, U, D in attr.shells_on_geometry("colour file", shells, leaves, depths):
        if U == 0:
            out.append(torch.empty((0, 3), dtype=torch.uint8, device=lv.device))
            continue
        coef = torch.empty((3, 0), dtype=torch.int16, device=lv.device)
        if U >= 2:
            by_ctx = dict(zip(_file_order(D), s["tables"]))
            coef = attr.decode_payload("colour file", k, s["payload"], [by_ctx[c] for c in range(3 * D)], lv, D, 3, ALPHABET, meta["chunk"],
                                       s.get("lengths"))
        out.append(native.color_inverse(lv, D, Q, s["root"], coef))
    return out


Y4 = (2126, 7152, 722)                     # BT.709 luma in units of 1 / 10000
CHUNK = 1 << 20


def _sums(a, b):
    """uint8 [n,3] colours a and b -> the exact sums of squared differences (R, G, B, y4) as Python integers; chunks of at most 2^20 points
    keep every int64 partial sum below 2^63 (a y4 difference is at most 2 550 000)."""
    tot = [0, 0, 0, 0]
    w = torch.tensor(Y4, dtype=torch.int64, device=a.device)
    for i in range(0, a.shape[0], CHUNK):
        d = a[i:i + CHUNK].to(torch.int64) - b[i:i + CHUNK].to(torch.int64)
        part = torch.cat([(d * d).sum(0), ((d * w).sum(1) ** 2).sum().reshape(1)]).cpu().tolist()
        tot = [t + int(p) for t, p in zip(tot, part)]
    return tot


def color_psnr(xyz, rgb, points, decoded):
    """The colour PSNR of a decoded cloud: xyz [P,3] / rgb [P,3] the input (rgb as the reader returns it, or its uint8 point colours), points
    [U,3] / decoded uint8 [U,3] the decoded cloud (device tensors).  Both directions through native.nn_error_split's indices (the lowest
    index among equally near points).  -> dict(psnr_y, psnr_rgb, sse_ab / sse_ba (R, G, B, y4 as exact integers), n_ab, n_ba): mse =
    sum / n (/ 1e8 for luma), PSNR = 10 log10(255^2 / max(mse_ab, mse_ba)), inf at zero error; psnr_rgb over the mean of the channels."""
    v = rgb if rgb.dtype == torch.uint8 else point_colors(rgb)
    w = decoded
    ab = native.nn_error_split(xyz[:, :3], points, (0.0,))["idx"].long()
    ba = native.nn_error_split(points, xyz[:, :3], (0.0,))["idx"].long()
    s_ab, s_ba = _sums(v, w[ab]), _sums(w, v[ba])
    n_ab, n_ba = int(v.shape[0]), int(w.shape[0])

    def psnr(mse_ab, mse_ba):
        worst = max(mse_ab, mse_ba)
        return float("inf") if worst == 0 else 10.0 * float(np.log10(255.0 ** 2 / worst))

    return dict(psnr_y=psnr(s_ab[3] / n_ab / 1e8, s_ba[3] / n_ba / 1e8),
                psnr_rgb=psnr(sum(s_ab[:3]) / 3 / n_ab, sum(s_ba[:3]) / 3 / n_ba), sse_ab=s_ab, sse_ba=s_ba, n_ab=n_ab, n_ba=n_ba)
