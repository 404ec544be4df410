"""Exact references for csrc/gemm_f32.hip (tests/test_gemm_f32_exact_gpu.py, tests/test_gemm_f32_ref_cpu.py): numpy on the CPU.

EXACT form (v_mfma_f32_32x32x2_f32): one fmaf per k, in the kernel's k order (``k_order``), from a zero accumulator -- ``fma_chain``, with
gemm_ref._fma32 (ONE rounding per step).  Random full-mantissa operands: every step rounds, so an element of another row, column or k,
a k taken twice or in another order shows in the last bit.
SPLIT form (three v_mfma_f32_32x32x16_f16 per product block): the kernel's contract is
    out = fmaf(acc2, 2^-11, acc1),   acc1 = hi_x . hi_w^T,   acc2 = hi_x . lo_w^T + lo_x . hi_w^T      (lo . lo is left out: documented)
with (hi, lo) = ``split_planes``.  ``dyadic_split_operands`` builds x = P/8 + j 2^-17, w = Q/16 + jw 2^-18 whose planes are exactly
(P/8, j/64) and (Q/16, jw/128): acc1 is a multiple of 2^-7, acc2 of 2^-10, and no partial sum of either reaches 24 bits of its unit, so
both are exact in f32 in ANY summation order and any MFMA-internal grouping (``assert_split_budget``, from the operands alone) and
``split_model`` is the only value a correct kernel can hold before its epilogue.
EPILOGUE, both forms, in f32: fl32(pre + bias) (0.0f without a bias), ReLU = fmaxf(., 0) or GELU, fl32(. + residual) (0.0f without one).
GELU has no single right answer (v_exp_f32): the pre-activation t IS known bit for bit, so the output lies in
[fl32(gelu64(t) - A + r), fl32(gelu64(t) + A + r)], A = gemm_ref.gelu_tolerance(), derived from the polynomial that gemm_f32.hip's gelu_erf
shares with gelu_f16.h (tests/test_gemm_f32_ref_cpu.py compares the coefficients in the kernel's source with gemm_ref._Q).
Comparisons are on bit patterns, -0 == +0; a NaN in the expectation asks for a NaN.  Everything cached here is read-only."""
import functools
from types import SimpleNamespace

import numpy as np

import gemm_ref as G

TK = 32                          # floats of K per tile of the kernel
SCALE = np.float32(2.0 ** -11)   # of the cross-term accumulator
# (M, N, K) of tests/test_gemm_f32_exact_gpu.py: the smallest at which each path of the kernel exists (tile 128 x 128, K-tile 32)
SHAPES = [(1, 1, 32), (130, 132, 64), (129, 131, 96), (385, 262, 64), (1100, 40, 32), (130, 68, 2048)]
MUTATION_SHAPE = (130, 132, 64)
SEED = 15838                     # of the dyadic operands: one at which the single output of (1, 1, 32) needs the final rounding too


# ------------------------------------------------------------------------------------------------ the split: planes and model
def split_planes(a):
    """split4 / split_f32_kernel, operation by operation: hi = f16(a) (one round-to-nearest-even), lo = f16((a - f32(hi)) * 2048) with
    the subtraction and the product in f32 (both exact while |a| < 65504).  f16 arrays."""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = a.astype(np.float16)
        rem = a - hi.astype(np.float32)
        lo = (rem * np.float32(2048.0)).astype(np.float16)
    assert rem.dtype == np.float32
    return hi, lo


def assert_split_budget(hx, lx, hw, lw):
    """The premise of exactness, from the planes alone (f64 arrays, no NaN): hi_x, lo_x, hi_w, lo_w are multiples of 1/8, 1/64, 1/16,
    1/128, so acc1 is a multiple of 2^-7 and acc2 of 2^-10; and the sum of the |products| of no output reaches 2^24 of those units.
    Returns the two largest sums in bits of their unit."""
    for t, den in ((hx, 8), (lx, 64), (hw, 16), (lw, 128)):
        assert np.array_equal(t * den, np.round(t * den)), den
    s1 = float((np.abs(hx) @ np.abs(hw).T).max()) * 2.0 ** 7
    s2 = float((np.abs(hx) @ np.abs(lw).T + np.abs(lx) @ np.abs(hw).T).max()) * 2.0 ** 10
    assert s1 < 2 ** 24 and s2 < 2 ** 24, (s1, s2)
    return np.log2(max(s1, 1.0)), np.log2(max(s2, 1.0))


def split_accumulators(x, w):
    """(acc1, acc2) of the split form as f32 arrays, each checked to be exact (assert_split_budget, and f64 -> f32 -> f64 is the
    identity).  A NaN operand is allowed: it is taken out for the premises and makes its row / column NaN."""
    planes = [p.astype(np.float64) for p in split_planes(x) + split_planes(w)]
    assert_split_budget(*[np.nan_to_num(p, nan=0.0) for p in planes])
    hx, lx, hw, lw = planes
    with np.errstate(invalid="ignore"):
        acc1, acc2 = hx @ hw.T, hx @ lw.T + lx @ hw.T
    for acc, unit in ((acc1, 2.0 ** -7), (acc2, 2.0 ** -10)):
        ok = ~np.isnan(acc)
        assert np.array_equal(acc[ok].astype(np.float32).astype(np.float64), acc[ok])
        assert np.array_equal(acc[ok] / unit, np.round(acc[ok] / unit))
    return acc1.astype(np.float32), acc2.astype(np.float32)


def split_model(x, w):
    """fmaf(acc2, 2^-11, acc1): what a correct split kernel holds before its epilogue, for operands that pass the premises."""
    acc1, acc2 = split_accumulators(x, w)
    with np.errstate(invalid="ignore"):
        return G._fma32(acc2, np.full_like(acc2, SCALE), acc1)


@functools.lru_cache(maxsize=None)
def dyadic_split_operands(M, N, K, narrow=False):
    """Seeded x = P/8 + j 2^-17 [M, K], w = Q/16 + jw 2^-18 [N, K] (f32), P in [-32, 32], Q in [-16, 16], j and jw in [-3, 3] and 0
    where P / Q is 0; bias b [N] and residual r [M, N] in multiples of 1/8 within [-8, 8].  |j| <= 3 keeps x within half an f16 ulp of
    P/8 even just below a power of two (where the ulp halves: 2^-15 = 4 * 2^-17 at 1/8), so the planes are exactly (P/8, j/64) and
    (Q/16, jw/128) -- asserted.  ``narrow`` (for GELU): P in [-8, 8], Q in [-4, 4], bias within [-2, 2], which keeps most
    pre-activations of K <= 2048 inside [-6, 6].  ``xc`` / ``wc`` are the coarse parts P/8, Q/16 alone."""
    rng = np.random.default_rng(SEED + ((M * 1009 + N) * 1013 + K) * 2 + int(narrow))
    pmax, qmax, bmax = (8, 4, 16) if narrow else (32, 16, 64)
    P, Q = rng.integers(-pmax, pmax + 1, (M, K)), rng.integers(-qmax, qmax + 1, (N, K))
    j, jw = rng.integers(-3, 4, (M, K)) * (P != 0), rng.integers(-3, 4, (N, K)) * (Q != 0)
    x64, w64 = P / 8.0 + j * 2.0 ** -17, Q / 16.0 + jw * 2.0 ** -18
    x, w = x64.astype(np.float32), w64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64) and np.array_equal(w.astype(np.float64), w64)
    for a, coarse, fine in ((x, P / 8.0, j / 64.0), (w, Q / 16.0, jw / 128.0)):
        hi, lo = split_planes(a)
        assert np.array_equal(hi.astype(np.float64), coarse) and np.array_equal(lo.astype(np.float64), fine)
    b = (rng.integers(-bmax, bmax + 1, N) / 8.0).astype(np.float32)
    r = (rng.integers(-64, 65, (M, N)) / 8.0).astype(np.float32)
    out = SimpleNamespace(M=M, N=N, K=K, x=x, w=w, b=b, r=r, xc=(P / 8.0).astype(np.float32), wc=(Q / 16.0).astype(np.float32))
    for a in vars(out).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def split_shares(c):
    """From the operands alone: (share of x with lo != 0, of w, share of outputs whose final fmaf(acc2, 2^-11, acc1) is inexact, share
    whose split result differs from fl32 of the full product x . w^T, largest partial sums of acc1 / acc2 in bits)."""
    (hx, lx), (hw, lw) = split_planes(c.x), split_planes(c.w)
    bits = assert_split_budget(*[p.astype(np.float64) for p in (hx, lx, hw, lw)])
    acc1, acc2 = split_accumulators(c.x, c.w)
    exact = acc1.astype(np.float64) + acc2.astype(np.float64) * 2.0 ** -11                # fits f64: 2^-21 units below 2^15
    model = split_model(c.x, c.w)
    full = (c.x.astype(np.float64) @ c.w.astype(np.float64).T).astype(np.float32)         # (products of 2^-35 units: exact in f64)
    return SimpleNamespace(lo_x=float((lx != 0).mean()), lo_w=float((lw != 0).mean()),
                           inexact=float((model.astype(np.float64) != exact).mean()), off_full=float((model != full).mean()), bits=bits)


# ------------------------------------------------------------------------------------------------ the exact form
def k_order(K):
    """The order in which the exact kernel feeds k to an accumulator: per K-tile of 32, for kk in 0..3, q in 0..3 the MFMA's k pair is
    (8 kk + q, 8 kk + 4 + q): lanes 0-31 first, lanes 32-63 second."""
    assert K % TK == 0
    return [t * TK + 8 * kk + half * 4 + q for t in range(K // TK) for kk in range(4) for q in range(4) for half in (0, 1)]


def fma_chain(x, w, order):
    """acc = fmaf(x[m, k], w[n, k], acc) for k in ``order``, from 0.0f: f32 [M, N], one rounding per step."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    with np.errstate(invalid="ignore"):
        for k in order:
            acc = G._fma32(x[:, k:k + 1], w[None, :, k], acc)
    return acc


@functools.lru_cache(maxsize=None)
def random_operands(M, N, K):
    """Seeded full-mantissa operands as in tests/test_gemm_f32_gpu.py: x = randn with four decades of column scales, w = 0.05 randn,
    bias and residual randn."""
    rng = np.random.default_rng((M * 7 + N * 3 + K) * 2 + 1)
    x = (rng.standard_normal((M, K)) * np.logspace(-2, 2, K)[None, :]).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    out = SimpleNamespace(M=M, N=N, K=K, x=x, w=w, b=rng.standard_normal(N).astype(np.float32),
                          r=rng.standard_normal((M, N)).astype(np.float32))
    for a in (out.x, out.w, out.b, out.r):
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the epilogue
def epilogue(pre32, bias=None, act=None, residual=None):
    """store_tile's arithmetic on the f32 value ``pre32`` [M, N].  None / "relu": the f32 result.  "gelu": (t, lo, hi), the f32
    pre-activation t and the f32 bounds of the result."""
    assert pre32.dtype == np.float32 and act in (None, "relu", "gelu")
    with np.errstate(invalid="ignore"):
        t = pre32 + (np.float32(0.0) if bias is None else np.asarray(bias, np.float32)[None, :])
        r = np.float32(0.0) if residual is None else np.asarray(residual, np.float32)
        assert t.dtype == np.float32
        if act == "gelu":
            A = G.gelu_tolerance()[0]
            g = G.gelu64(t.astype(np.float64)) + np.asarray(r, np.float64)
            return t, (g - A).astype(np.float32), (g + A).astype(np.float32)
        if act == "relu":
            t = np.fmax(t, np.float32(0.0))                   # fmaxf: a NaN becomes 0
        out = t + r
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def _ordered32(a):
    """f32 -> int64 in value order, one step per ulp, -0 == +0."""
    v = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(v >= 0, v, -(v & 0x7FFFFFFF))


def _report(what, bad, got, text, note):
    print(f"{what}: {int(bad.sum())} of {bad.size} outputs {text}")
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs {text}; first at [m, n] = {list(i)}: got {got[i]!r} "
                             f"({got[i].view(np.int32):#010x}), {note(i)}")


def check_bits(got, want, what):
    """``got`` equals ``want`` bit for bit (f32 [M, N]); -0 == +0; NaN in ``want`` asks for a NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape and got.ndim == 2, (got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), np.isnan(got) | (_ordered32(got) != _ordered32(want)))
    _report(what, bad, got, "differ", lambda i: f"want {want[i]!r} ({want[i].view(np.int32):#010x})")


def check_between(got, lo, hi, what):
    """lo <= got <= hi elementwise (f32 [M, N]); NaN in ``lo`` asks for a NaN."""
    got, lo, hi = (np.asarray(a, np.float32) for a in (got, lo, hi))
    assert got.shape == lo.shape == hi.shape and got.ndim == 2
    nan = np.isnan(lo)
    with np.errstate(invalid="ignore"):
        bad = np.where(nan, ~np.isnan(got), ~((got >= lo) & (got <= hi)))
    _report(what, bad, got, "differ", lambda i: f"want a value in the GELU bounds [{lo[i]!r}, {hi[i]!r}]")
