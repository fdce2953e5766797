"""A correctly rounded numpy restatement of the device quantiser (csrc/geom.hip: transform_kernel + quantize_kernel, and their copies
front_transform_kernel / quant1 behind scp_geom_build_xyz), for tests that hold the device to DESIGN.md 2.1 bit for bit.

The recipe, operation by operation: float32 products and sums in the reference's order, IEEE float32 sqrt, x + float32(1e-9),
atan2 / acos evaluated in float64 and rounded ONCE to float32, the float32 `+ 6.2831855f` wrap of negative phi, the float32 division
z / rho, float32 bin_num, float32 `6.2831855f / (bin - 1)` and `3.1415927f / (bin - 1)` widened to float64, rint(((double)t - off) / qs)
in float64.  The Cartesian branch is quantize_kernel's float32 one.

A float64 libm is not correctly rounded itself, so a value whose float64 result lies next to a float32 rounding midpoint may round
either way: `ambiguous` marks those (2^-45 relative, about 5e-7 of all values) and only they may be left out of a bit comparison.
`explained` decides whether an integer that differs from a numpy-made fixture is one that numpy's documented float32 error can flip."""
from collections import namedtuple

import numpy as np

F32 = np.float32
TWO_PI_F = F32(6.2831855)
PI_F = F32(3.1415927)
ANGULAR = {"spher": (1, 2), "cylin": (1,), "cart": ()}

Quantised = namedtuple("Quantised", "q tr bin_num qs offset max_coord min_coord v64 raw64")


def _transform(xyz, mode):
    """-> (tr float32 [n,3], v64 [n,3], raw64 [n,3]).  raw64: the float64 function values that are rounded to float32 (atan2 before
    the wrap, acos; NaN in columns that hold no function value).  v64: the same with the wrap applied in float64 (rho / z columns: tr)."""
    xyz = np.ascontiguousarray(xyz, F32)
    if mode == "cart":
        return xyz.copy(), xyz.astype(np.float64), np.full(xyz.shape, np.nan)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(under="ignore"):
        s = x * x + y * y
        if mode == "spher":
            s = s + z * z
    rho = np.sqrt(s)
    xe = x + F32(1e-9)
    phi_raw = np.arctan2(y.astype(np.float64), xe.astype(np.float64))
    phi = phi_raw.astype(F32)
    neg = phi < 0
    phi = np.where(neg, phi + TWO_PI_F, phi).astype(F32)
    phi64 = np.where(neg, phi_raw + np.float64(TWO_PI_F), phi_raw)
    raw = np.full(xyz.shape, np.nan)
    raw[:, 1] = phi_raw
    if mode == "spher":
        ratio = (z / rho).astype(F32)
        th_raw = np.arccos(ratio.astype(np.float64))
        c, c64 = th_raw.astype(F32), th_raw
        raw[:, 2] = th_raw
    else:
        c, c64 = z, z.astype(np.float64)
    tr = np.stack([rho, phi, c], 1).astype(F32)
    assert tr.dtype == F32 and rho.dtype == F32 and phi.dtype == F32
    return tr, np.stack([rho.astype(np.float64), phi64, c64], 1), raw


def cr_transform(xyz, mode):
    """float32 [n,3] Cartesian -> float32 [n,3] (rho, phi, theta | z), every value the correctly rounded one of the kernel's recipe."""
    return _transform(xyz, mode)[0]


def cr_quantise(xyz, qs, mode, cart_offset=-200.0):
    """-> Quantised(q int32 [n,3], tr, bin_num, qs[3], offset[3], max_coord, min_coord, v64, raw64): the integers, and everything
    scp_quant_info reports, as the kernels compute them."""
    tr, v64, raw = _transform(xyz, mode)
    if mode == "cart":
        qsf, offf = F32(qs), F32(cart_offset)
        q = np.rint(((tr - offf) / qsf).astype(F32)).astype(np.int32)
        return Quantised(q, tr, 0.0, [float(qs)] * 3, [float(cart_offset)] * 3, int(q.max()), int(q.min()), v64, raw)
    binf = F32(np.rint(F32(tr[:, 0].max() / F32(qs))) + F32(1))
    assert type(binf) is F32
    q_phi = F32(TWO_PI_F / F32(binf - F32(1)))
    q_th = F32(PI_F / F32(binf - F32(1)))
    qsv = [float(qs), float(q_phi), float(q_th) if mode == "spher" else float(qs)]
    off = [0.0, 0.0, float(tr[:, 2].min()) if mode == "cylin" else 0.0]
    q = np.rint((tr.astype(np.float64) - np.array(off)) / np.array(qsv)).astype(np.int32)
    return Quantised(q, tr, float(binf), qsv, off, int(q.max()), int(q.min()), v64, raw)


def depth_of(max_coord):
    """Smallest D with 2^D > max_coord (the tree depth scp_geom_build derives from the largest integer)."""
    return int(max_coord).bit_length()


def ambiguous(v64):
    """True where a float64 function value lies within 2^-45 relative (128 float64 ulp) of a float32 rounding midpoint: only there
    can a float64 atan2 / acos that is a few ulp off round to another float32 than the exact value does."""
    v = np.asarray(v64, np.float64)
    ok = np.isfinite(v)
    w = np.where(ok, v, 0.0)
    f = w.astype(F32)
    up = (f.astype(np.float64) + np.nextafter(f, F32(np.inf)).astype(np.float64)) / 2
    dn = (f.astype(np.float64) + np.nextafter(f, F32(-np.inf)).astype(np.float64)) / 2
    d = np.minimum(np.abs(w - up), np.abs(w - dn))
    return ok & (d <= np.abs(w) * 2.0 ** -45)


def explained(mode, col, q_cr, q_other, v64, t, off, qs):
    """For coordinates (arrays, all of column `col`) whose correctly rounded integer q_cr differs from a numpy-made q_other: true iff the
    column is angular, the difference is +-1, and the exact (v64 - off) / qs lies within 2.5 float32 ulp of t, divided by qs, of the
    half-integer between the two integers.  2.5 = numpy within 2 ulp of the correctly rounded value + the 0.5 ulp
    of the correct rounding itself."""
    q_cr, q_other = np.asarray(q_cr, np.int64), np.asarray(q_other, np.int64)
    if col not in ANGULAR[mode]:
        return np.zeros(q_cr.shape, bool)
    half = (q_cr + q_other) / 2.0
    exact = (np.asarray(v64, np.float64) - off) / qs
    ulp = np.spacing(np.abs(np.asarray(t, F32))).astype(np.float64)
    return (np.abs(q_cr - q_other) == 1) & (np.abs(exact - half) <= 2.5 * ulp / qs)


def unexplained(mode, ref, q_other):
    """-> (differing coordinates per column [3], number of differing points, number of differing coordinates NOT explained)."""
    q_other = np.asarray(q_other).astype(np.int64)
    diff = ref.q.astype(np.int64) != q_other
    bad = 0
    for k in range(3):
        m = diff[:, k]
        if m.any():
            ok = explained(mode, k, ref.q[m, k], q_other[m, k], ref.v64[m, k], ref.tr[m, k], ref.offset[k], ref.qs[k])
            bad += int((~ok).sum())
    return diff.sum(0).tolist(), int(diff.any(1).sum()), bad


def n_ambiguous(ref):
    return int(ambiguous(ref.raw64).sum())


# tests/golden/frame_ints.npz (numpy-made) against cr_quantise of synth_frame(0) / ford_like(synth_frame(0)): (fixture, mode, step,
# Cartesian offset, differing coordinates per column, differing points).  Both sides are fixed data; test_quantiser_ref.py re-derives them.
FRAME_INTS_CASES = [("q_spher_L12", "spher", 400 / (2 ** 12 - 1), -200.0, [0, 0, 853], 853),
                    ("q_spher_L16", "spher", 400 / (2 ** 16 - 1), 0.0, [0, 0, 0], 0),
                    ("q_spher_L17", "spher", 400 / (2 ** 17 - 1), 0.0, [0, 0, 0], 0),
                    ("q_spher_L18", "spher", 400 / (2 ** 18 - 1), 0.0, [0, 6, 0], 6),
                    ("q_cylin_L14", "cylin", 400 / (2 ** 14 - 1), -200.0, [0, 0, 0], 0),
                    ("q_cart_L12", "cart", 400 / (2 ** 12 - 1), -200.0, [0, 0, 0], 0),
                    ("q_spher_ford_L17", "spher", 2.0, 0.0, [0, 42, 68], 110),
                    ("q_spher_ford_L18", "spher", 1.0, 0.0, [0, 62, 132], 194),
                    ("q_spher_ford_L19", "spher", 0.5, 0.0, [0, 148, 277], 425)]
FRAME_DIFF_POINTS = {name: pts for name, _, _, _, _, pts in FRAME_INTS_CASES}


def _crafted(mode):
    rows = []
    for r in (1.0, 37.5):
        rows += [(r, 0, 0), (-r, 0, 0), (0, r, 0), (0, -r, 0), (0, 0, r), (0, 0, -r),
                 (-r, -0.0, 1),
                 (-r, 1e-30, 0.5), (-r, -1e-30, 0.5), (-r, 1e-40, 0.5), (-r, -1e-40, 0.5),      # the +-pi seam, normal and denormal y
                 (r, -1e-30, 0),                                                             # -tiny phi -> + 2 pi: the top bin
                 (r, 1e-40, 2), (r, -1e-40, 2),                                              # denormal phi, denormal negative phi
                 (-1e-9, r, 0.25), (-1e-9, -r, 0.25),                                        # x + 1e-9f == 0 exactly
                 (-1e-12, r, 1), (1e-4, 1e-4, r), (1e-2, 0, r), (1e-2, 0, -r),               # next to the poles
                 (r, r, r), (-r, -r, -r)]
    rows += [(119.9, 0.01, -25), (-119.9, -0.01, 2), (3, 4, 0), (3, 4, 0), (1e-20, 1e-20, 1), (2.5, -2.5, -1.73)]
    if mode == "cylin":
        rows.append((0, 0, 0))          # rho = 0, phi = 0; undefined (0 / 0) in spherical mode, so only here
    with np.errstate(under="ignore"):
        return np.array(rows, np.float64).astype(F32)


def edge_points(mode="spher"):
    """Points on the axes, at the +-pi seam, next to the poles and with denormal coordinates, embedded at rows 2000.. of a thinned
    synthetic frame (a sensible bin_num, a ragged last workgroup)."""
    from scp_amd.synth import synth_frame
    base = synth_frame(5)[::30][:4001]
    return np.ascontiguousarray(np.concatenate([base[:2000], _crafted(mode), base[2000:]]), F32)
