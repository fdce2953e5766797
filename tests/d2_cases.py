"""Input clouds of the D2 tests (tests/test_d2_ref.py checks on the CPU that the reference alone keeps every one of them inside the
exclusion cap; tests/test_gpu_d2.py runs the device on them).  All float64 arrays of float32-representable values."""
import functools

import numpy as np

SIZES = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025)
VIEW = (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def near4096():
    """The 4096 points of synth_frame(0) nearest the sensor, nearest first: with radius 1.0 and max_nn 30 no point has fewer than 3
    neighbours, no 30th / 31st neighbour tie and no eigenvalue gap below 1e-2."""
    from scp_amd.synth import synth_frame
    xyz = synth_frame(0)[:, :3].astype(np.float64)
    r2 = (xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2]
    out = xyz[np.argsort(r2, kind="stable")[:4096]].copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gauss(n, seed=21):
    """A Gaussian cluster (sigma 0.3 m, off the sensor): from a few hundred points on, far more than max_nn lie within 1 m of any."""
    rng = np.random.default_rng(seed)
    out = (rng.standard_normal((n, 3)) * 0.3 + np.array([5.0, 3.0, 1.0])).astype(np.float32).astype(np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tie_lattice():
    """8 x 8 x 4 lattice, spacing 1 x 1 x 2, shuffled: from an interior point the squared distances are 0 (1 point), 1 (4), 2 (4), 4 (6)
    and 5 (16), so the 30th and the 31st neighbour tie exactly at 5 and the lower index must win.  The vertical spacing keeps the
    smallest eigenvalue apart, so the normals stay comparable."""
    rng = np.random.default_rng(22)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    out = (g * np.array([1.0, 1.0, 2.0]) + np.array([3.0, -2.0, 1.0]))[rng.permutation(len(g))]
    out.setflags(write=False)
    return out


def normal_cases():
    """(id, cloud, radius, max_nn, cap on the excluded share)"""
    cases = []
    for n in SIZES:
        cases.append((f"near-{n}", near4096()[:n], 1.0, 30, 0.02))
        cases.append((f"gauss-{n}", gauss(n), 1.0, 30, 0.02))
    cases.append(("near-4096", near4096(), 1.0, 30, 0.0))
    for k in (1, 3, 30, 32):
        cases.append((f"gauss-1025-nn{k}", gauss(1025), 1.0, k, 0.02))
    cases.append(("near-1025-nn32", near4096()[:1025], 1.0, 32, 0.02))
    cases.append(("gauss-1025-r0.06", gauss(1025), 0.06, 30, 0.02))        # some points keep fewer than 3 neighbours
    cases.append(("near-1025-reversed", near4096()[:1025][::-1].copy(), 1.0, 30, 0.02))
    cases.append(("gauss-1025-reversed", gauss(1025)[::-1].copy(), 1.0, 30, 0.02))
    cases.append(("tie-lattice", tie_lattice(), 3.0, 30, 0.02))
    return cases


def unit_rows(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.sqrt((v * v).sum(1))[:, None]


def tie_pairs():
    """(id, a, n_a, b) for na, nb in {1, 255, 256, 257, 1025}, na != nb: points on a coarse grid (exact ties, shared points and duplicates
    inside a cloud), except two tie-free random pairs."""
    out = []
    sizes = (1, 255, 256, 257, 1025)
    for na in sizes:
        for nb in sizes:
            if na == nb:
                continue
            rng = np.random.default_rng(1000 * na + nb)
            if (na, nb) in ((257, 1025), (1025, 255)):
                a, b = rng.random((na, 3)) * 4.0, rng.random((nb, 3)) * 4.0
            else:
                a, b = rng.integers(0, 9, (na, 3)) * 0.5, rng.integers(0, 9, (nb, 3)) * 0.5 + 0.25 * rng.integers(0, 2, (nb, 1))
            out.append((f"{na}x{nb}", a, unit_rows(rng, na), b))
    return out
