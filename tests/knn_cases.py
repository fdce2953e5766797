"""Windows of the kNN tests, each the smallest that still has the edge it is named for (tests/test_knn_cases.py asserts on the CPU that
it has; tests/test_gpu_knn.py runs the device on them).  Every window is a float32 array [n, C]; `exact` ones have coordinates whose
distances the kernel's fp32 arithmetic (and its f16x3 split) computes without a single rounding, so their neighbour lists are THE
lists under (distance ascending, index ascending)."""
import collections
import functools

import numpy as np

K = 20
LADDER = (1, 7, 19, 20, 21, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 2049)
FEATURE_C = (144, 192)
GENERIC_C = (5, 8, 64, 145, 200)

# group: the launches a case can share ("pos", "f144", "f192": packed launches of that width; "generic": the dense entry point only)
# family: what the CPU tests ask of it; misaligned: the device copy starts one float behind a 16-byte boundary
Case = collections.namedtuple("Case", "name group family exact x misaligned")


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


# --------------------------------------------------------------------------------------------------------------- positions
@functools.lru_cache(maxsize=None)
def lattice_cloud():
    """synth_frame(0) snapped to a 2^10 lattice over its bounding cube, made unique, in Morton order: int64 [P, 3] in 0 .. 1023."""
    from scp_amd.synth import synth_frame
    xyz = synth_frame(0).astype(np.float64)
    lo = xyz.min(0)
    ext = (xyz.max(0) - lo).max()
    q = np.minimum(1023, np.floor((xyz - lo) / ext * 1024.0)).astype(np.int64)
    q = np.unique(q, axis=0)
    key = np.zeros(len(q), np.int64)
    for b in range(10):
        for c in range(3):
            key |= ((q[:, c] >> b) & 1) << (3 * b + c)
    q = q[np.argsort(key, kind="stable")]
    q.setflags(write=False)
    return q


def lattice_window(n, start=None):
    """n consecutive Morton-ordered lattice points starting a third into the cloud (raw integers)."""
    q = lattice_cloud()
    start = len(q) // 3 if start is None else start
    assert start + n <= len(q)
    return q[start:start + n]


def position_cases():
    out = [Case("morton-lattice-raw", "pos", "morton", True, _ro(lattice_window(2048)), False),
           Case("morton-lattice", "pos", "morton", True, _ro(lattice_window(2048) * 2.0 ** -10), False)]
    for n in LADDER:
        out.append(Case(f"lattice-{n}", "pos", "lattice", True, _ro(lattice_window(n) * 2.0 ** -10), False))
    out.append(Case("lattice-8192", "pos", "lattice", True, _ro(lattice_window(8192) * 2.0 ** -10), False))
    out.append(Case("all-equal", "pos", "degenerate", True, _ro(np.tile([[0.25, 0.5, 0.75]], (300, 1))), False))
    i = np.arange(300)
    two = np.where((i % 25 == 3)[:, None], [[0.5, 0.5, 0.25]], [[0.125, 0.75, 0.5]])       # 12 copies of one point among 288 of another
    out.append(Case("two-clusters-of-duplicates", "pos", "degenerate", True, _ro(two), False))
    line = np.stack([2.0 * i, np.ones(300), -3.0 * np.ones(300)], 1)                       # collinear, two apart: i - m and i + m tie
    out.append(Case("line", "pos", "degenerate", True, _ro(line), False))
    return out


def dense_batch():
    """B = 3 items of n = 1000 lattice points for the dense entry point: the last 32-point box of every item holds 8 points."""
    P = len(lattice_cloud())
    return _ro(np.stack([lattice_window(1000, s) for s in (P // 3, P // 2, P // 5)]) * 2.0 ** -10)


# --------------------------------------------------------------------------------------------------------------- features, exact
def scaled_integers(n, C, seed):
    """Integers 0 .. 3 times a power of two 2^e per row, e in -2 .. 3; row 0 is zero, row 5 repeats row 2, row 9 is twice row 4.
    Everything is a multiple of 2^-2 below 2^5: fp32 sums of 200 such products are exact, and so is the f16x3 split (xb = 0)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 4, (n, C)).astype(np.float64)
    e = rng.integers(-2, 4, n)
    e[[2, 4]] = (3, 0)
    v[2] = 3.0                                             # rows 2 and 5, equal, are the farthest of most rows: a 20th / 21st tie even at n = 21
    x = v * (2.0 ** e)[:, None]
    x[0] = 0.0
    if n > 9:
        x[5] = x[2]
        x[9] = 2.0 * x[4]
    return x


def feature_exact_cases():
    return [Case(f"scaled-int-c{C}-{n}", f"f{C}", "scaled-int", True, _ro(scaled_integers(n, C, 100 * C + n)), False)
            for C in FEATURE_C for n in (21, 300, 513, 2049)]


# --------------------------------------------------------------------------------------------------------------- features, inexact
def _ar1(rng, n, C, rho):
    """A stationary smooth walk of unit variance per column: x_t = rho x_(t-1) + sqrt(1 - rho^2) noise."""
    z = rng.standard_normal((n, C))
    out = np.empty((n, C))
    out[0] = z[0]
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, n):
        out[t] = rho * out[t - 1] + s * z[t]
    return out


def siblings(n, C, seed, shared=128):
    """Octree siblings share their parent's part of the feature row: the first `shared` columns are equal inside runs of 1 .. 8
    consecutive rows (a smooth walk from run to run); the other columns are a smooth walk plus noise, row by row."""
    rng = np.random.default_rng(seed)
    shared = min(shared, C - 1)
    runs = []
    while sum(runs) < n:
        runs.append(int(rng.integers(1, 9)))
    rid = np.repeat(np.arange(len(runs)), runs)[:n]
    x = np.empty((n, C))
    x[:, :shared] = _ar1(rng, len(runs), shared, 0.98)[rid]
    x[:, shared:] = _ar1(rng, n, C - shared, 0.95) + 0.25 * rng.standard_normal((n, C - shared))
    return x


def mixed_magnitude(n, C, seed):
    """siblings with every row scaled by 2^e, e in -12 .. 12; row 1 is zero and row 3 has one feature 2^20 times the others."""
    rng = np.random.default_rng(seed + 1)
    x = siblings(n, C, seed) * (2.0 ** rng.integers(-12, 13, n))[:, None]
    x[1] = 0.0
    x[3] = siblings(n, C, seed)[3] * 2.0 ** -10
    x[3, 7] = 2.0 ** 10
    return x


def offset(n, C, seed):
    """siblings plus, in every column, ten times that column's spread: 2 x.y - |x|^2 - |y|^2 cancels four digits."""
    x = siblings(n, C, seed)
    return (x - x.mean(0)[None, :]) + 10.0 * x.std(0)[None, :]


INEXACT = {"siblings": siblings, "mixed-magnitude": mixed_magnitude, "offset": offset}


def feature_inexact_cases():
    out = []
    for C in FEATURE_C:
        for fam, fn in INEXACT.items():
            for n in (300, 2049):
                out.append(Case(f"{fam}-c{C}-{n}", f"f{C}", fam, False, _ro(fn(n, C, 7 * C + n)), False))
    out.append(Case("siblings-c144-8192", "f144", "siblings", False, _ro(siblings(8192, 144, 8192)), False))
    return out


# --------------------------------------------------------------------------------------------------------------- generic kernel
def generic_cases():
    out = []
    for C in GENERIC_C:
        out.append(Case(f"generic-scaled-int-c{C}", "generic", "scaled-int", True, _ro(scaled_integers(300, C, 300 + C)), False))
        out.append(Case(f"generic-siblings-c{C}", "generic", "siblings", False, _ro(siblings(300, C, 300 + C, shared=(C * 2) // 3)), False))
    out.append(Case("generic-misaligned-c144", "generic", "scaled-int", True, _ro(scaled_integers(300, 144, 144)), True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(position_cases() + feature_exact_cases() + feature_inexact_cases() + generic_cases())


def by_name(name):
    (c,) = [c for c in cases() if c.name == name]
    return c


def names(**want):
    return [c.name for c in cases() if all(getattr(c, k) == v for k, v in want.items())]


def device_mode(case, f16x3):
    """Which arithmetic serves the case: the f16x3 path exists for 144 / 192 features on a 16-byte aligned base only."""
    return "f16x3" if f16x3 and case.x.shape[1] in FEATURE_C and not case.misaligned else "f32"


# --------------------------------------------------------------------------------------------------------------- packed launches
def pack(windows):
    """Windows [n_w, C] -> (x float32 [T, C] with every window padded to a multiple of 512 rows, ctab int32 [T / 512, 2] = (first row
    of the chunk's sequence, its real length), bases)."""
    C = windows[0].shape[1]
    pad = [-(-len(w) // 512) * 512 for w in windows]
    x = np.zeros((sum(pad), C), np.float32)
    tab, bases, base = [], [], 0
    for w, p in zip(windows, pad):
        x[base:base + len(w)] = w
        tab += [[base, len(w)]] * (p // 512)
        bases.append(base)
        base += p
    return x, np.asarray(tab, np.int32), bases
