"""The pair sets of the chunk coder's tests (host only), and their chunks as the host coder writes them: what tests/test_gpu_ac_chunks.py
holds the device coder to.  Every set is built once per process and never modified; tests/test_chunk_format.py checks, without a GPU, that
the sets do what they are for."""
import functools

import numpy as np

CHUNKS = (64, 256, 4096)


def sizes(N):
    """One wave of chunks and less, and two sizes beyond one wave that end in a short chunk."""
    return (1, N - 1, N, N + 1, 2 * N, 64 * N + 1, 65 * N - 1)


def table_symbols(rng, n, alphabet):
    """n symbols spread over the 16 tables of an alphabet, drawn from each table's own distribution (so peaked tables code their common
    symbols) with a tenth drawn uniformly (so every table also codes its width-1 tail): (tables uint16 [16, Lp], ctx, sym)."""
    from scp_amd import attr
    tabs, counts = attr.tables(alphabet), attr.table_counts(alphabet)
    ctx = rng.integers(0, 16, size=n).astype(np.uint8)
    sym = rng.integers(0, alphabet, size=n)
    for g in range(16):
        at = np.nonzero(ctx == g)[0]
        own = rng.choice(alphabet, size=len(at), p=counts[g] / 65536.0)
        keep = rng.random(len(at)) < 0.1
        sym[at] = np.where(keep, sym[at], own)
    return tabs, ctx, sym.astype(np.int16)


def lohi_of(tabs, ctx, sym):
    row = tabs[ctx.astype(np.int64)]
    i = np.arange(len(sym))
    s = sym.astype(np.int64)
    return row[i, s].astype(np.uint32) | (row[i, s + 1].astype(np.uint32) << 16)          # (the last entry holds 65536 as 0)


@functools.lru_cache(maxsize=None)
def pairs(kind, n):
    """uint32 [n]: (a) `tab511` / `tab1021` random symbols under each of the 16 tables; (b) `width1` width-1 pairs at random positions;
    (c) `mid` pairs straddling the midpoint, `midbroken` the same with one off-centre symbol every few hundred; (d) `full` full-width
    pairs (c_high 65536 stored as 0); (e) `mixed` the sets interleaved in runs."""
    rng = np.random.default_rng(KINDS.index(kind) * 1000003 + n)
    if kind.startswith("tab"):
        out = lohi_of(*table_symbols(rng, n, int(kind[3:])))
    elif kind == "width1":
        lo = rng.integers(0, 65536, size=n).astype(np.uint32)
        out = lo | (((lo + 1) & 0xFFFF) << 16)
    elif kind in ("mid", "midbroken"):
        out = np.full(n, 0x7FFF | (0x8001 << 16), np.uint32)
        if kind == "midbroken":
            at = np.nonzero(rng.random(n) < 1.0 / 300)[0]
            lo = (0x7FF0 + rng.integers(0, 8, size=len(at))).astype(np.uint32)
            out[at] = lo | ((lo + 1 + rng.integers(0, 8, size=len(at)).astype(np.uint32)) << 16)
    elif kind == "full":
        out = np.zeros(n, np.uint32)
    else:
        parts = [pairs(k, n) for k in ("tab511", "width1", "midbroken", "full", "tab1021", "mid")]
        pick = (np.arange(n) // 37 + rng.integers(0, 6)) % 6
        out = np.choose(pick, parts).astype(np.uint32)
    out = np.ascontiguousarray(out, np.uint32)
    out.setflags(write=False)
    return out


KINDS = ("tab511", "tab1021", "width1", "mid", "midbroken", "full", "mixed")


@functools.lru_cache(maxsize=None)
def host_chunks(kind, n, N):
    from scp_amd import native
    p = pairs(kind, n)
    return tuple(native.ac_encode_lohi(p[b:b + N]) for b in range(0, n, N))
