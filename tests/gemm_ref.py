"""Exact references for csrc/gemm_f16.hip (tests/test_gemm_f16_exact_gpu.py, tests/test_gemm_ref_cpu.py).

Operands are dyadic.  The WIDE set -- x in multiples of 1/8 within [-4, 4], w in multiples of 1/16 within [-1, 1], f16 bias and
residual in multiples of 1/8 within [-8, 8] -- makes every product a multiple of 2^-7 and keeps every partial sum of up to 6144 of
them below 2^15: 22 bits, exact in f32 in ANY summation order and any MFMA-internal grouping.  The f64 pre-activation x . w^T (+ bias)
is then the only value a correct f32 accumulator can hold, and
    bias / no bias     out = f16(pre)                       one round-to-nearest-even
    accumulate         out = f16(f16(pre) + r0)             the kernel's arithmetic: the product is rounded, added in f32, rounded again
    pair-f32           out = fl32(acc1 + fl32(bias + 2^-11 acc2))      acc1, acc2 exact, the f32 bias is NOT dyadic
    bias + GELU        f16(gelu64(pre) - A) <= out <= f16(gelu64(pre) + A) for |pre| <= 12, f16(pre) above, +-0 below
with A = ``gelu_tolerance()``: the error of gelu_f16.h's polynomial form, restated here in numpy with one rounding per fmaf and
measured against f64, plus an allowance for the hardware exponential.  The NARROW set (x within [-1, 1], w within [-1/2, 1/2], bias
within [-2, 2]) puts most pre-activations of a short K into GELU's interesting range, the negative tail included.
Two evaluations of the same expectations: numpy on the CPU (conv_ref.f16_bits / ordered: the definition), and torch f64 in row chunks
on the device for the cases too large for that (``rn16``: round-to-nearest-even onto the f16 grid by integer arithmetic in f64;
tests/test_gemm_ref_cpu.py holds the two against each other).  Everything cached here is shared between tests: read-only.
``work_items`` / ``tile_order`` are the library's own description of the persistent walk (evaluated on the host: no device needed)."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch

import conv_ref as R

# (denominator, largest numerator) of x, w and of bias / residual
WIDE = SimpleNamespace(name="wide", x=(8, 32), w=(16, 16), b=(8, 64))
NARROW = SimpleNamespace(name="narrow", x=(8, 8), w=(16, 8), b=(8, 16))
UNIT = 2.0 ** -7                 # every product, bias and residual is a multiple of it
GELU_RANGE = 12.0                # beyond it gelu_f16.h returns max(v, 0) exactly (tests/test_gemm_ref_cpu.py)
F16_TIE_TO_INF = 65520.0         # the tie between 65504 and 2^16: rounds to even, i.e. to inf
CPU_LIMIT = 1 << 21              # outputs up to which a case is checked with numpy on the CPU


# ------------------------------------------------------------------------------------------------ the kernel's schedule
def _tiles(m, n):
    return ((m + 255) // 256) * ((n + 255) // 256)


def work_items(m, n, grid):
    """[items, 2] = (list position of the tile, n-half 0 / 1 or -1 for the whole tile) of the persistent walk of ``grid`` workgroups;
    workgroup w runs items w, w + grid, ..."""
    from vlfm_amd import _lib

    L = _lib.lib()
    L.vlfm_gemm_f16_work_items.restype = ctypes.c_int
    out = np.full((2 * _tiles(m, n), 2), -7, np.int32)
    items = L.vlfm_gemm_f16_work_items(m, n, grid, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(out))
    assert items >= _tiles(m, n)
    return out[:items]


def tile_order(m, n, group_m=0):
    """[tiles, 2] = (m-tile, n-tile) of every list position; group_m = 0: the grouping the launcher uses."""
    from vlfm_amd import _lib

    L = _lib.lib()
    L.vlfm_gemm_f16_tile_order.restype = ctypes.c_int
    out = np.full((_tiles(m, n), 2), -7, np.int32)
    assert L.vlfm_gemm_f16_tile_order(m, n, group_m, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(out)) == len(out)
    return out


# ------------------------------------------------------------------------------------------------ operands
def _dyadic(g, shape, den_num):
    den, num = den_num
    return (torch.randint(-num, num + 1, shape, generator=g).float() / den).half()


@functools.lru_cache(maxsize=4)
def operands(M, N, K, narrow=False):
    """Seeded dyadic x [M, K], w [N, K], bias b [N], residual r0 [M, N] (wide set only): f16 CPU tensors."""
    s = NARROW if narrow else WIDE
    g = torch.Generator().manual_seed(((M * 1009 + N) * 1013 + K) * 2 + int(narrow))
    x, w, b = _dyadic(g, (M, K), s.x), _dyadic(g, (N, K), s.w), _dyadic(g, (N,), s.b)
    r0 = None if narrow else _dyadic(g, (M, N), WIDE.b)           # (the narrow set serves the GELU epilogue only)
    assert_budget(x, w, b)
    return SimpleNamespace(M=M, N=N, K=K, set=s.name, x=x, w=w, b=b, r0=r0)


def assert_budget(x, w, b=None):
    """The premise of exactness, from the operands alone: no partial sum of |x w| (+ |bias|), in units of 2^-7, reaches 24 bits --
    and all of them are multiples of that unit."""
    row = float(x.float().abs().sum(1).max()) * float(w.float().abs().max()) + (float(b.float().abs().max()) if b is not None else 0.0)
    assert row / UNIT < 2 ** 24, row
    for t, den in ((x, 8), (w, 16)) + (((b, 8),) if b is not None else ()):
        assert bool((t.float() * den == (t.float() * den).round()).all())


def pre_cpu(x, w, b=None, unit=UNIT):
    """x . w^T (+ b) in f64 on the CPU, checked to be what an f32 accumulator holds exactly."""
    pre = x.double().numpy() @ w.double().numpy().T
    if b is not None:
        pre = pre + b.double().numpy()
    assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
    assert unit is None or np.array_equal(pre / unit, np.round(pre / unit))
    return pre


# Value edges on one (130, 264, 64) problem.  K-slots 0..7 are reserved: the dyadic noise is zero there, the hand-made rows are zero
# everywhere else, so a hand-made x row meets a hand-made w row in the reserved slots only, noise meets hand-made rows in zeros, and
# every sum stays exact in f32 (at most two non-zero products, or noise alone).  Row EDGE_BIG of x is (256, 1), row EDGE_SMALL is
# 2^-12 in slot 2.  name -> (row, column, (slot, w value)..., bias, residual)
EDGE_SHAPE = (130, 264, 64)
EDGE_BIG, EDGE_SMALL = 3, 70
EDGE_COLUMNS = {
    "65504 + 15.9921875 -> 65504": (EDGE_BIG, 5, ((0, 255.875), (1, 15.9921875)), 0.0, 0.125),
    "65520, the tie -> inf": (EDGE_BIG, 6, ((0, 255.875), (1, 16.0)), 0.0, 0.125),
    "-(65504 + 15.9921875) -> -65504": (EDGE_BIG, 133, ((0, -255.875), (1, -15.9921875)), 0.0, -0.125),
    "-65520 -> -inf": (EDGE_BIG, 134, ((0, -255.875), (1, -16.0)), 0.0, 0.0),
    "65512 + bias 8 -> inf, 65504 without": (EDGE_BIG, 40, ((0, 255.875), (1, 8.0)), 8.0, 0.0),
    "accumulate 65504 + 65504 -> inf": (EDGE_BIG, 41, ((0, 255.875),), 0.0, 65504.0),
    "accumulate -65504 - 65504 -> -inf": (EDGE_BIG, 200, ((0, -255.875),), 0.0, -65504.0),
    "2^-24, the smallest subnormal": (EDGE_SMALL, 7, ((2, 2.0 ** -12),), 0.0, 0.0),
    "2^-25, a tie -> 0": (EDGE_SMALL, 8, ((2, 2.0 ** -13),), 0.0, 0.0),
    "3 * 2^-25, a tie -> 2^-23": (EDGE_SMALL, 135, ((2, 3 * 2.0 ** -13),), 0.0, 0.0),
    "-2^-24": (EDGE_SMALL, 260, ((2, -2.0 ** -12),), 0.0, 0.0),
}
# what the hand-made elements must come out as: ((epilogue, with bias), (row, column), f16 value)
_INF = float("inf")
EDGE_OUTCOMES = [
    (("bias", True), (3, 5), 65504.0), (("bias", True), (3, 6), _INF), (("bias", True), (3, 133), -65504.0), (("bias", True), (3, 134), -_INF),
    (("bias", True), (3, 40), _INF), (("bias", False), (3, 40), 65504.0), (("bias", False), (3, 6), _INF),
    (("bias", True), (70, 7), 2.0 ** -24), (("bias", True), (70, 8), 0.0), (("bias", True), (70, 135), 2.0 ** -23),
    (("bias", True), (70, 260), -2.0 ** -24), (("bias", False), (70, 7), 2.0 ** -24), (("bias", False), (70, 8), 0.0),
    (("bias_gelu", True), (3, 5), 65504.0), (("bias_gelu", True), (3, 6), _INF), (("bias_gelu", True), (3, 40), _INF),
    (("bias_gelu", True), (3, 133), 0.0), (("bias_gelu", True), (3, 134), 0.0),
    (("accumulate", True), (3, 41), _INF), (("accumulate", True), (3, 200), -_INF), (("accumulate", True), (3, 6), _INF),
    (("accumulate", True), (3, 5), 65504.0), (("accumulate", True), (70, 7), 2.0 ** -24), (("accumulate", True), (70, 8), 0.0),
    (("accumulate", True), (70, 135), 2.0 ** -23), (("accumulate", False), (3, 41), _INF), (("accumulate", False), (3, 200), -_INF),
    (("accumulate", False), (70, 260), -2.0 ** -24),
]


@functools.lru_cache(maxsize=None)
def edge_case():
    """Operands with f16 saturation, subnormal results and ties placed by hand (EDGE_COLUMNS), a NaN in the last row of x and
    another in the last row of w; ``pre`` / ``pre_nobias`` in f64 with NaN in exactly row M - 1 and column N - 1."""
    M, N, K = EDGE_SHAPE
    g = torch.Generator().manual_seed(65504)
    x, w, b, r0 = _dyadic(g, (M, K), WIDE.x), _dyadic(g, (N, K), WIDE.w), _dyadic(g, (N,), WIDE.b), _dyadic(g, (M, N), WIDE.b)
    x[:, :8] = 0
    w[:, :8] = 0
    x[EDGE_BIG] = 0
    x[EDGE_BIG, 0], x[EDGE_BIG, 1] = 256.0, 1.0
    x[EDGE_SMALL] = 0
    x[EDGE_SMALL, 2] = 2.0 ** -12
    r0[EDGE_SMALL] = 0
    for m, n, slots, bias, res in EDGE_COLUMNS.values():
        w[n] = 0
        for k, v in slots:
            w[n, k] = v
            assert float(w[n, k]) == v and abs(v) >= 2.0 ** -14            # an f16 number, and a normal one
        b[n], r0[m, n] = bias, res
    assert M - 1 not in (EDGE_BIG, EDGE_SMALL) and all(n != N - 1 for _, n, *_ in EDGE_COLUMNS.values())
    pre_nobias = pre_cpu(x, w, unit=None)
    pre = pre_cpu(x, w, b, unit=None)
    for p in (pre, pre_nobias):
        p[M - 1, :] = np.nan
        p[:, N - 1] = np.nan
    x, w = x.clone(), w.clone()
    x[M - 1, 20] = float("nan")
    w[N - 1, 33] = float("nan")
    return SimpleNamespace(M=M, N=N, K=K, x=x, w=w, b=b, r0=r0, pre=pre, pre_nobias=pre_nobias)


# ------------------------------------------------------------------------------------------------ numpy: the definition
def f16_bits(v):
    """conv_ref.f16_bits with f16's overflow: anything at or beyond the tie 65520 is +-inf (conv_ref's raises there)."""
    v = np.asarray(v, np.float64)
    big = np.abs(v) >= F16_TIE_TO_INF
    bits = R.f16_bits(np.where(big, 0.0, v))
    return np.where(big, np.where(v > 0, np.int16(0x7C00), np.int16(-0x0400)), bits).astype(np.int16)


def f16_value(v):
    return f16_bits(v).view(np.float16).astype(np.float64)


def shares(pre):
    """(inexact, tie): the fractions of ``pre`` that f16 cannot hold, and that lie exactly between two f16 numbers.  A midpoint
    mirrors its rounding h into the other neighbour, 2 pre - h, which no other inexact value does (|2 (pre - h)| < 1 ulp)."""
    h = f16_value(pre)
    inexact = (h != pre) & np.isfinite(h)
    with np.errstate(invalid="ignore"):
        mirror = np.where(inexact, 2.0 * pre - h, 0.0)
    tie = inexact & (f16_value(mirror) == mirror)
    return float(inexact.mean()), float(tie.mean())


def gelu64(pre):
    t = torch.from_numpy(np.ascontiguousarray(pre, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t * 0.5 ** 0.5))).numpy()


def gelu_shares(pre):
    """(within [-6, 6], within [-6, -1]): where GELU is neither the identity nor zero, and its negative tail."""
    return float((np.abs(pre) <= 6.0).mean()), float(((pre >= -6.0) & (pre <= -1.0)).mean())


def want_accumulate(pre, r0):
    """f16(pre) + r0, the value the second rounding sees: both addends are dyadic, their f32 sum is exact (asserted)."""
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(pre), np.nan, f16_value(np.nan_to_num(pre, nan=0.0)) + r0.double().numpy())
    ok = np.isfinite(s)
    assert np.array_equal(s[ok].astype(np.float32).astype(np.float64), s[ok])
    return s


def gelu_bounds(pre, A):
    """(lo, hi) in f64: the f16 result of the GELU epilogue lies between their roundings."""
    g = gelu64(np.clip(pre, -GELU_RANGE, GELU_RANGE))
    inner = np.abs(pre) <= GELU_RANGE
    outer = np.where(pre > 0, pre, 0.0)
    return np.where(inner, g - A, outer), np.where(inner, g + A, outer)


def _fail(what, bad, got_bits, exact, want_desc):
    i = tuple(int(v) for v in np.argwhere(bad)[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at [m, n] = {i}: got "
                         f"{got_bits[i].view(np.float16)!r}, exact {exact[i]!r} -> {want_desc(i)}")


def check_exact(got_bits, exact, what, row0=0):
    """``got_bits`` (int16) is ``exact`` (f64) rounded once to f16; -0 == +0; NaN in ``exact`` wants a NaN."""
    want = f16_bits(np.nan_to_num(exact, nan=0.0))
    nan = np.isnan(exact)
    got_nan = (got_bits & 0x7FFF) > 0x7C00
    bad = np.where(nan, ~got_nan, got_nan | (R.ordered(got_bits) != R.ordered(want)))
    print(f"{what}: {int(bad.sum())} of {bad.size} outputs differ from round_f16(f64)")
    if bad.any():
        _fail(f"{what} (rows from {row0})", bad, got_bits, exact, lambda i: f"f16 {want[i].view(np.float16)!r}")


def check_gelu(got_bits, pre, A, what, row0=0):
    nan = np.isnan(pre)
    lo, hi = gelu_bounds(np.nan_to_num(pre, nan=0.0), A)
    lo_b, hi_b = f16_bits(lo), f16_bits(hi)
    o = R.ordered(got_bits)
    got_nan = (got_bits & 0x7FFF) > 0x7C00
    bad = np.where(nan, ~got_nan, got_nan | (o < R.ordered(lo_b)) | (o > R.ordered(hi_b)))
    loose = int((R.ordered(hi_b) != R.ordered(lo_b)).sum())
    print(f"{what}: {int(bad.sum())} of {bad.size} outputs outside [f16(gelu - A), f16(gelu + A)]; the two differ at {loose}")
    if bad.any():
        _fail(f"{what} (rows from {row0})", bad, got_bits, pre,
              lambda i: f"gelu in [{lo[i]!r}, {hi[i]!r}] -> f16 [{lo_b[i].view(np.float16)!r}, {hi_b[i].view(np.float16)!r}]")


def want_pair_bits(acc1, acc2, bias):
    """fl32(acc1 + fl32(bias + 2^-11 acc2)) as int32 bit patterns [M, N]; bias f32 [N] or None (the kernel then adds 0.0f)."""
    a1, a2 = (acc1 + 0.0).astype(np.float32), (acc2 + 0.0).astype(np.float32)
    assert np.array_equal(a1.astype(np.float64), acc1) and np.array_equal(a2.astype(np.float64), acc2)
    low = a2 * np.float32(2.0 ** -11)
    mid = (bias if bias is not None else np.zeros(acc1.shape[1], np.float32)).astype(np.float32)[None, :] + low
    out = a1 + mid
    assert out.dtype == np.float32
    return out.view(np.int32)


# ------------------------------------------------------------------------------------------------ torch f64: the large cases
def rn16(t):
    """f64 tensor (any device) -> the f16 number nearest to each element, ties to even, as f64; +-inf from 65520 on.  Integer
    arithmetic on the exponent field and ONE torch.round (nearest even) of an exactly scaled value: no intermediate f32 rounding,
    which ``t.half()`` has."""
    bits = t.contiguous().view(torch.int64)
    e = ((bits >> 52) & 0x7FF) - 1023                                   # floor(log2 |t|); -1023 for 0 and f64 subnormals
    ulp = ((torch.clamp(e, min=-14, max=16) - 10 + 1023) << 52).view(torch.float64)
    r = torch.round(t / ulp) * ulp
    r = torch.where(r.abs() >= 65536.0, torch.copysign(torch.full_like(t, float("inf")), t), r)
    return torch.where(torch.isnan(t), t, r)


def shares_t(pre):
    h = rn16(pre)
    inexact = h != pre
    mirror = torch.where(inexact, 2.0 * pre - h, torch.zeros_like(pre))
    tie = inexact & (rn16(mirror) == mirror)
    return float(inexact.double().mean()), float(tie.double().mean())


def gelu_shares_t(pre):
    """``gelu_shares`` on a torch tensor (any device)."""
    return float((pre.abs() <= 6.0).double().mean()), float(((pre >= -6.0) & (pre <= -1.0)).double().mean())


def bad_exact_t(got, exact):
    """True where the f16 tensor ``got`` is not rn16(exact) (-0 == +0; a NaN is always bad)."""
    return ~(got.double() == rn16(exact))


def bad_gelu_t(got, pre, A):
    c = torch.clamp(pre, -GELU_RANGE, GELU_RANGE)
    g = 0.5 * c * (1.0 + torch.erf(c * 0.5 ** 0.5))
    inner = pre.abs() <= GELU_RANGE
    outer = torch.where(pre > 0, pre, torch.zeros_like(pre))
    lo, hi = rn16(torch.where(inner, g - A, outer)), rn16(torch.where(inner, g + A, outer))
    v = got.double()
    return ~((v >= lo) & (v <= hi))


# ------------------------------------------------------------------------------------------------ GELU: the tolerance A
_Q = [2.834908400e-06, -3.937762449e-05, 1.861798810e-04, 1.369373058e-04, -7.063421421e-03, 5.249617994e-02, 4.592081904e-01,
      1.151105165e+00]


def _fma32(a, b, c):
    """fmaf on f32 arrays: RN32(a b + c) with ONE rounding.  a b is exact in f64 (48 bits); the f64 sum is turned into its
    round-to-odd form with the error term of TwoSum, after which the rounding to f32 equals that of the exact value (53 >= 24 + 2)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def gelu_erf_f32(v):
    """csrc/gelu_f16.h's gelu_erf, operation by operation, on an f32 numpy array; exp2 is evaluated in f64 and rounded to f32 (the
    hardware's v_exp_f32 is about 1 ulp off that: ``gelu_tolerance`` allows for it).  Returns (gelu, 0.5 u e)."""
    v = np.asarray(v, np.float32)
    u = np.abs(v)
    q = np.full_like(u, np.float32(_Q[0]))
    for c in _Q[1:]:
        q = _fma32(q, u, np.full_like(u, np.float32(c)))
    p = (q.astype(np.float64) * u.astype(np.float64)).astype(np.float32)        # q * u: one rounding
    with np.errstate(under="ignore"):
        e = np.exp2(-p.astype(np.float64)).astype(np.float32)
    h = np.float32(-0.5) * u                                                     # exact
    return _fma32(h, e, np.maximum(v, np.float32(0.0))), (-h).astype(np.float64) * e.astype(np.float64)


@functools.lru_cache(maxsize=None)
def gelu_tolerance():
    """(A, restatement's max |error| against f64, max 0.5 u e) over [-12, 12]: every multiple of 2^-7 (what the dyadic operands
    produce) and 2^21 + 1 evenly spaced points.  A = error + 2^-22 max(0.5 u e): v_exp_f32's ~1 ulp (2^-23 relative, doubled) scales
    the subtracted term 0.5 u e and nothing else."""
    pts = np.concatenate([np.arange(-1536, 1537) * UNIT, np.linspace(-GELU_RANGE, GELU_RANGE, (1 << 21) + 1)]).astype(np.float32)
    got, term = gelu_erf_f32(pts)
    err = float(np.abs(got.astype(np.float64) - gelu64(pts.astype(np.float64))).max())
    return err + 2.0 ** -22 * float(term.max()), err, float(term.max())
