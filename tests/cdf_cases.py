"""Rows of the CDF-kernel tests (tests/test_cdf_cases.py checks on the CPU, through the oracle alone, that they still have the edges they are
named for; tests/test_gpu_cdf.py runs csrc/cdf.hip on them).  Pure numpy: nothing here touches the device.

Trained probability heads emit peaked rows: a spread above 87 (float32 exponentials go subnormal, above 104 exactly zero), symbols of
width 1, -inf entries.  logit_rows has every such kind, pmf_rows the unnormalised rows of the scp_pmf_cdf path on which the float32
serial prefix sum depends on its order, place the row layouts the encoder and the decoders hand the kernel."""
import numpy as np

NSYMS = (2, 3, 16, 64, 65, 128, 129, 254, 255)
ROW_COUNTS = (1, 63, 64, 65, 129, 4003)                  # one row, around the 64-row tile, two tiles and a row, 62 tiles and a partial one
KINDS = ("flat", "normal", "normal8", "normal30", "normal1e4", "ramp", "huge", "neginf", "tie", "peaked")
PEAKED_KINDS = ("normal30", "normal1e4", "ramp", "huge", "neginf", "peaked")
FORCED = ("first", "last", "argmax", "zero")             # the symbol forced on row r: FORCED[(r // 10) % 4]
LAYOUTS = {"tight": (None, False), "ld256": (256, False), "ld256-misaligned": (256, True), "ld300": (300, False)}
RAMP_END = -104.0                                        # expf(-103.98) is half the smallest subnormal: the ramp ends in exact zeros


def kind_of(r):
    return np.asarray(r) % len(KINDS)


def softmax_f32(logits):
    """The float32 PMF csrc/cdf.hip defines, on the host: exp(x - max) in float32, a SERIAL float32 row sum in column order (np.cumsum is
    serial), a correctly rounded float32 division."""
    x = np.ascontiguousarray(logits, np.float32)
    with np.errstate(under="ignore"):
        e = np.exp(x - x.max(1, keepdims=True))
        return (e / np.cumsum(e, axis=1, dtype=np.float32)[:, -1:]).astype(np.float32)


def softmax_f64(logits):
    """The float64 reference of that PMF: exp(float64(float32(x - max))) normalised in float64.  The float32 rounding of the argument is part
    of the library's definition and is reproduced here."""
    x = np.ascontiguousarray(logits, np.float32)
    d = (x - x.max(1, keepdims=True)).astype(np.float32).astype(np.float64)
    with np.errstate(under="ignore"):
        e = np.exp(d)
    return e / e.sum(1, keepdims=True)


def logit_rows(n, nsym, seed):
    """float32 logits [n, nsym] and symbols uint8 [n].  Row r is of kind KINDS[r % 10]:
      flat       zeros
      normal     N(0,1)
      normal8    N(0,1) * 8
      normal30   N(0,1) * 30: the spread exceeds 87, exponentials go subnormal or zero
      normal1e4  N(0,1) * 1e4
      ramp       linspace(0, -104, nsym): walks through the whole subnormal band
      huge       one entry 1e30, in another column than the drawn symbol's: every other probability is an exact zero
      neginf     one to nsym - 1 entries -inf
      tie        the symbol ties exactly with the maximum (and with one other column)
      peaked     the symbol's logit 20 above its N(0,1) value
    and its symbol is forced by FORCED[(r // 10) % 4]: column 0, column nsym - 1, the row's argmax, a column whose float32 probability is
    an exact zero (where the row has one).  `tie` and `peaked` rows are built around their symbol: the last two leave theirs alone."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nsym)).astype(np.float32)
    sym = rng.integers(0, nsym, n).astype(np.int64)
    other = (sym + 1 + rng.integers(0, nsym - 1, n)) % nsym          # a column that is not the symbol's
    n_inf = 1 + rng.integers(0, nsym - 1, n)
    inf_key = rng.random((n, nsym))
    r = np.arange(n)
    k, f = kind_of(r), (r // len(KINDS)) % len(FORCED)
    sym[f == 0] = 0
    sym[f == 1] = nsym - 1
    other = np.where(other == sym, (sym + 1) % nsym, other)
    is_ = lambda name: k == KINDS.index(name)
    x[is_("flat")] = 0.0
    x[is_("normal8")] *= np.float32(8.0)
    x[is_("normal30")] *= np.float32(30.0)
    x[is_("normal1e4")] *= np.float32(1e4)
    x[is_("ramp")] = np.linspace(0.0, RAMP_END, nsym).astype(np.float32)
    m = is_("huge")
    x[r[m], other[m]] = np.float32(1e30)
    m = is_("neginf")
    x[m] = np.where(np.argsort(np.argsort(inf_key[m], axis=1), axis=1) < n_inf[m, None], -np.inf, x[m]).astype(np.float32)
    m = is_("tie")
    top = x.max(1) + np.float32(1.0)
    x[r[m], sym[m]] = top[m]
    x[r[m], other[m]] = top[m]
    m = is_("peaked")
    x[r[m], sym[m]] += np.float32(20.0)
    # the symbols that depend on the finished row
    free = ~(is_("tie") | is_("peaked"))
    m = free & (f == 2)
    sym[m] = x[m].argmax(1)
    p = softmax_f32(x)
    zero = p == 0.0
    m = free & (f == 3) & zero.any(1)
    sym[m] = zero[m].argmax(1)                                        # the first exact zero of the row
    assert np.isfinite(x.max(1)).all() and not np.isnan(x).any()
    x.setflags(write=False)
    sym = sym.astype(np.uint8)
    sym.setflags(write=False)
    return x, sym


def pmf_rows(n, nsym, seed):
    """Unnormalised float32 rows of the scp_pmf_cdf path, random * 2^randint(-24, 1) per element, and symbols: magnitudes 2^-24 .. 2 side by
    side, so every float32 prefix sum rounds and the serial column-order sum differs from any re-associated one."""
    rng = np.random.default_rng(seed)
    p = (rng.random((n, nsym)) * np.exp2(rng.integers(-24, 2, (n, nsym)).astype(np.float64))).astype(np.float32)
    p = np.maximum(p, np.float32(2.0 ** -60))                         # (random() may return 0.0: keep every entry positive)
    sym = rng.integers(0, nsym, n).astype(np.uint8)
    sym[:2] = (0, nsym - 1)[:n]
    p.setflags(write=False)
    sym.setflags(write=False)
    return p, sym


def cdf_from_f64_prefix_sums(pmf):
    """numpyAc's table with its float32 serial prefix sums replaced by float64 prefix sums rounded to float32 once (what a re-associated or
    more accurate sum tends to): uint16 [n, nsym + 1].  Where this differs from the oracle's table, summation order shows."""
    pmf = np.ascontiguousarray(pmf, np.float32)
    n, nsym = pmf.shape
    c = np.cumsum(pmf.astype(np.float64), axis=1).astype(np.float32)
    c = (c / c[:, -1:]).astype(np.float32)
    q = np.rint(np.hstack((np.zeros((n, 1)), c.astype(np.float64))) * (65536 - nsym)).astype(np.int64)
    return ((q + np.arange(nsym + 1)) & 0xFFFF).astype(np.uint16)


def widen(cdf):
    """uint16 table [n, nsym + 1] -> int64 with the wrapped last column (0) back at 65536."""
    c = np.asarray(cdf).view(np.uint16).astype(np.int64)
    c[:, -1] = np.where(c[:, -1] == 0, 65536, c[:, -1])
    return c


def pairs(cdf, sym):
    """(c_low, c_high as stored: 0 for the top symbol) of every row's symbol from a uint16 table."""
    c = np.asarray(cdf).view(np.uint16).astype(np.int64)
    r, s = np.arange(len(c)), np.asarray(sym, np.int64)
    nsym = c.shape[1] - 1
    return c[r, s], np.where(s == nsym - 1, 0, c[r, np.minimum(s + 1, nsym)])


def _address(t):
    return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data


def place(rows, ld=None, misalign=False):
    """The rows [n, nsym] (a numpy array or a torch tensor, on any device) embedded in a wider float32 buffer of NaNs: a view [n, nsym] of
    row stride ld (None: nsym) whose first element lies on a 16-byte boundary, or with `misalign` one float past one.  The layouts the
    kernel stages in differently are LAYOUTS: ld == nsym, the 256-float rows of the coding-order table (16-byte loads), the same rows at a
    misaligned base (which must fall back to the generic loop) and any other stride."""
    n, nsym = rows.shape
    ld = nsym if ld is None else int(ld)
    assert ld >= nsym
    size = n * ld + 8
    flat = rows.new_full((size,), float("nan")) if hasattr(rows, "new_full") else np.full(size, np.nan, np.float32)
    assert _address(flat) % 4 == 0
    off = (-(_address(flat) // 4)) % 4 + (1 if misalign else 0)
    view = flat[off:off + n * ld].reshape(n, ld)[:, :nsym]
    view[...] = rows
    assert (_address(view) % 16 == 4) if misalign else (_address(view) % 16 == 0)
    return view
