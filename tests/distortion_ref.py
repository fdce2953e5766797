"""A numpy float64 statement of the distortion report's definitions (include/scp.h: scp_nn_error_split_f64, scp_dist_segments_f64;
csrc/distreport.hip), independent of the device code, for tests that hold the device to it.

  neighbour   d2(i,j) = (dx*dx + dy*dy) + dz*dz with dx = a_i.x - b_j.x ..., written out elementwise so that numpy rounds as the device
              does; j*(i) = argmin_j, and numpy's argmin returns the FIRST minimum, i.e. the lowest index among equals.
  split       e = b_j* - a_i; the frame straight from its definition: r^ = (x,y,z)/rho, phi^ = (-y,x,0)/s, theta^ = (xz, yz, -s2)/(rho s)
              with (x,y,z) = a_i - view.  s == 0: an axis point, components 0.
  bin         ring = the largest r with rho2 >= E_r * E_r (searchsorted on the squares, side="right"); bin = group * R + ring.
  record      counts, the maximum and the histogram exactly (np.frexp for the exponent), every sum with math.fsum - the correctly rounded
              sum, which no summation order of the device can be further from than its own rounding error."""
import math

import numpy as np

CHUNK = 512
SUMS = ("sum_sq", "sum_r2", "sum_phi2", "sum_theta2", "sum_r")


def sqdist_rows(q, p):
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(a, b):
    """-> (idx int64 [na], d2 float64 [na]): the lowest index among the nearest points of b, and its squared distance."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    idx, d2 = [], []
    for s in range(0, len(a), CHUNK):
        d = sqdist_rows(a[s:s + CHUNK], b)
        j = np.argmin(d, axis=1)
        idx.append(j)
        d2.append(d[np.arange(len(j)), j])
    return np.concatenate(idx), np.concatenate(d2)


def split(a, b, idx, view=(0.0, 0.0, 0.0)):
    """-> (comp float64 [na,3] = (e_r, e_phi, e_theta), axis bool [na], rho2 float64 [na])."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    v = np.asarray(view, np.float64)
    e = b[idx] - a
    x, y, z = a[:, 0] - v[0], a[:, 1] - v[1], a[:, 2] - v[2]
    s2 = x * x + y * y
    rho2 = s2 + z * z
    s, rho = np.sqrt(s2), np.sqrt(rho2)
    axis = s == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        e_r = (e[:, 0] * x + e[:, 1] * y + e[:, 2] * z) / rho
        e_phi = (e[:, 1] * x - e[:, 0] * y) / s
        e_theta = (e[:, 0] * x * z + e[:, 1] * y * z - e[:, 2] * s2) / (rho * s)
    comp = np.stack((e_r, e_phi, e_theta), 1)
    comp[axis] = 0.0
    return comp, axis, rho2


def ring(rho2, edges):
    esq = np.asarray(edges, np.float64) * np.asarray(edges, np.float64)
    return np.searchsorted(esq, rho2, side="right") - 1


def bucket(d2):
    """Histogram bucket of every d2: 0 for d2 == 0, else clamp(floor(log2 d2) + 41, 1, 63)."""
    d2 = np.asarray(d2, np.float64)
    _, ex = np.frexp(d2)                      # d2 = m 2^ex with 0.5 <= m < 1: floor(log2 d2) = ex - 1
    return np.where(d2 == 0.0, 0, np.clip(ex.astype(np.int64) - 1 + 41, 1, 63))


def record(d2, comp, axis):
    """The scp_dist_seg record of one bin's rows, as a dict."""
    framed = ~axis
    return dict(rows=int(len(d2)), axis_rows=int(axis.sum()),
                sum_sq=math.fsum(d2), sum_r2=math.fsum(comp[framed, 0] ** 2), sum_phi2=math.fsum(comp[framed, 1] ** 2),
                sum_theta2=math.fsum(comp[framed, 2] ** 2), sum_r=math.fsum(comp[framed, 0]), abs_r=math.fsum(np.abs(comp[framed, 0])),
                max_sq=float(d2.max()) if len(d2) else 0.0, hist=np.bincount(bucket(d2), minlength=64).astype(np.int64))


def records(d2, comp, axis, bins, n_bins):
    return [record(d2[bins == k], comp[bins == k], axis[bins == k]) for k in range(n_bins)]


def direction(a, b, edges, group=None, n_groups=1, view=(0.0, 0.0, 0.0)):
    """Everything scp_nn_error_split_f64 + scp_dist_segments_f64 give for one direction."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    idx, d2 = nearest(a, b)
    comp, axis, rho2 = split(a, b, idx, view)
    g = np.zeros(len(a), np.int64) if group is None else np.asarray(group, np.int64)
    bins = g * len(edges) + ring(rho2, edges)
    return dict(idx=idx, d2=d2, comp=comp, axis=axis, bin=bins, records=records(d2, comp, axis, bins, n_groups * len(edges)))
