"""tests/gemm_f32_ref.py checked on its own, without a GPU: the premises under which the split model has one right answer, at every shape
of tests/test_gemm_f32_exact_gpu.py; that the comparisons report each of a list of wrong kernels (mutated models) as wrong; that the
GELU tolerance applies to gemm_f32.hip (same coefficients as gemm_ref._Q); and the representation bound of the hi / lo' split as it
really is -- 2^-23 |a| from 2^-12 on (attained), 2^-36 absolute below, hence at most 2^-22 |a| on [2^-14, 2^-12)."""
import re
from pathlib import Path

import numpy as np
import pytest

import gemm_f32_ref as F
import gemm_ref as G

KERNEL = Path(__file__).resolve().parent.parent / "vlfm_amd" / "csrc" / "gemm_f32.hip"
IDS = [f"{m}x{n}x{k}" for m, n, k in F.SHAPES]


# ------------------------------------------------------------------------------------------------ premises
@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_split_operands_have_one_right_answer_and_exercise_the_model(shape):
    """Budget and exactness (asserted inside dyadic_split_operands / split_accumulators, from the operands alone), and the shares that
    make the comparison mean something: lo != 0 in at least half of x and of w; the final fmaf inexact in at least 5 % of the outputs
    (for the single output of (1, 1, 32): in that output, which gemm_f32_ref.SEED sees to)."""
    for narrow in (False, True):
        c = F.dyadic_split_operands(*shape, narrow=narrow)
        s = F.split_shares(c)
        pre = F.epilogue(F.split_model(c.x, c.w), c.b)
        inside = float((np.abs(pre) <= 6.0).mean())
        print(f"{shape} {'narrow' if narrow else 'wide'}: lo != 0 in {s.lo_x:.2f} of x, {s.lo_w:.2f} of w; final fmaf inexact in "
              f"{s.inexact:.2f}; differs from fl32(x . w^T) in {s.off_full:.3f}; partial sums {s.bits[0]:.1f} / {s.bits[1]:.1f} bits; "
              f"|pre + bias| <= 6 in {inside:.2f}")
        assert max(s.bits) < 24
        assert s.lo_x >= 0.5 and s.lo_w >= 0.5
        if narrow:
            assert inside >= 0.5                 # what the GPU test asserts before it checks GELU on this set
        else:
            assert s.inexact >= 0.05
            assert c.M * c.N == 1 or s.off_full >= 0.02           # "implements the split model" is told from "is merely close to f32"


def test_coarse_operands_are_exact_in_any_order():
    """The arbiter of the exact form: x = P/8, w = Q/16 -- the f64 product is f32-exact and so is every partial sum."""
    for shape in F.SHAPES:
        c = F.dyadic_split_operands(*shape)
        G.assert_budget(_T(c.xc), _T(c.wc))
        pre = c.xc.astype(np.float64) @ c.wc.astype(np.float64).T
        assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
    c = F.dyadic_split_operands(*F.MUTATION_SHAPE)
    want = (c.xc.astype(np.float64) @ c.wc.astype(np.float64).T).astype(np.float32)
    F.check_bits(F.fma_chain(c.xc, c.wc, F.k_order(c.K)), want, "coarse, kernel order")
    F.check_bits(F.fma_chain(c.xc, c.wc, range(c.K - 1, -1, -1)), want, "coarse, descending")


def _T(a):
    import torch

    return torch.from_numpy(np.array(a))


def test_k_order_is_a_permutation_per_tile():
    order = F.k_order(96)
    assert order[:8] == [0, 4, 1, 5, 2, 6, 3, 7] and order[8:10] == [8, 12]
    for t in range(3):
        assert sorted(order[32 * t:32 * t + 32]) == list(range(32 * t, 32 * t + 32))


def test_split_planes_restate_the_kernel_on_known_values():
    a = np.array([0.0, -0.0, 1.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -23, 1 + 2.0 ** -12 + 2.0 ** -23, 2.0 ** -25, 2.0 ** -24,
                  3 * 2.0 ** -25, 65504.0, 7e4], np.float32)
    hi, lo = F.split_planes(a)
    assert hi.dtype == lo.dtype == np.float16
    want_hi = [0.0, -0.0, 1.0, 1.0, 1 + 2.0 ** -9, 1.0, 1.0, 0.0, 2.0 ** -24, 2.0 ** -23, 65504.0, np.inf]
    want_lo = [0.0, 0.0, 0.0, 1.0, -1.0, 2.0 ** -12, 0.5, 2.0 ** -14, 0.0, -2.0 ** -14, 0.0, -np.inf]
    assert np.array_equal(hi.astype(np.float64), want_hi) and np.array_equal(lo.astype(np.float64), want_lo)
    assert np.signbit(hi[1]) and not np.signbit(lo[1])


# ------------------------------------------------------------------------------------------------ mutations
def _caught(got, want, what):
    with pytest.raises(AssertionError, match=r"[1-9]\d* of \d+ outputs differ; first at \[m, n\]"):
        F.check_bits(got, want, what)


def test_wrong_split_kernels_are_reported():
    c = F.dyadic_split_operands(*F.MUTATION_SHAPE)
    (hx, lx), (hw, lw) = ([p.astype(np.float64) for p in F.split_planes(a)] for a in (c.x, c.w))
    want = F.split_model(c.x, c.w)
    F.check_bits(want.copy(), want, "the model itself")
    F.check_bits(want, np.where(want == 0, np.float32(-0.0), want), "-0 == +0")

    def model(acc1, acc2, scale=2.0 ** -11):
        a1, a2 = acc1.astype(np.float32), acc2.astype(np.float32)
        assert np.array_equal(a1, acc1) and np.array_equal(a2, acc2)
        return G._fma32(a2, np.full_like(a2, np.float32(scale)), a1)

    acc1, acc2 = hx @ hw.T, hx @ lw.T + lx @ hw.T
    F.check_bits(model(acc1, acc2), want, "the model, restated")
    _caught(model(acc1, hx @ lw.T), want, "cross term lo_x . hi_w dropped")
    _caught(model(acc1, lx @ hw.T), want, "cross term hi_x . lo_w dropped")
    _caught(model(acc1, acc2, 2.0 ** -10), want, "scale 2^-10")
    _caught(F.split_model(c.x[:, :-F.TK], c.w[:, :-F.TK]), want, "last K-tile skipped")
    _caught(model(acc1, hx @ lw.T + np.roll(lx, -1, axis=0) @ hw.T), want, "lo_x taken from row m + 1")
    _caught(model(acc1 + np.float32(2.0 ** -7) * (np.arange(want.size).reshape(want.shape) == want.size - 1), acc2), want,
            "one unit of acc1 in the last element")


def test_wrong_epilogues_are_reported():
    c = F.dyadic_split_operands(*F.MUTATION_SHAPE)
    pre = F.split_model(c.x, c.w)
    want = F.epilogue(pre, c.b, "relu", c.r)
    F.check_bits(np.maximum(pre + c.b[None, :], np.float32(0)) + c.r, want, "the epilogue, restated")
    _caught(np.maximum(pre, np.float32(0)) + c.b[None, :] + c.r, want, "bias added after the activation")
    _caught(np.maximum(pre + c.b[None, :] + c.r, np.float32(0)), want, "residual added before the activation")
    _caught(F.epilogue(pre, np.roll(c.b, 1), "relu", c.r), want, "bias shifted by one column")
    # GELU: the bounds hold the f32 restatement of the kernel's polynomial, and reject a value two ulp outside
    n = F.dyadic_split_operands(*F.MUTATION_SHAPE, narrow=True)
    t, lo, hi = F.epilogue(F.split_model(n.x, n.w), n.b, "gelu", n.r)
    got = G.gelu_erf_f32(t)[0] + n.r
    F.check_between(got, lo, hi, "gelu_erf restated in f32")
    with pytest.raises(AssertionError, match="outputs differ"):
        F.check_between(np.nextafter(np.nextafter(hi, np.float32(np.inf)), np.float32(np.inf)), lo, hi, "two ulp above")
    with pytest.raises(AssertionError, match="outputs differ"):
        F.check_between(0.5 * t * (1 + np.tanh(0.7978845608 * (t + 0.044715 * t ** 3))) + n.r, lo, hi, "tanh GELU")
    nan = t.copy()
    nan[3, 5] = np.nan
    tn, lon, hin = F.epilogue(nan, None, "gelu", None)
    with pytest.raises(AssertionError, match=r"1 of \d+ outputs differ; first at \[m, n\] = \[3, 5\]"):
        F.check_between(np.nan_to_num(lon), lon, hin, "a number where NaN is due")


def test_a_chain_in_another_k_order_is_reported():
    """Random full-mantissa operands: every step of the chain rounds, so the order shows -- which is what lets the GPU test pin it."""
    c = F.random_operands(*F.MUTATION_SHAPE)
    want = F.fma_chain(c.x, c.w, F.k_order(c.K))
    _caught(F.fma_chain(c.x, c.w, range(c.K)), want, "ascending k")
    _caught(F.fma_chain(np.roll(c.x, 1, axis=0), c.w, F.k_order(c.K)), want, "x rows shifted by one")
    # one fmaf per step is not "f64 product + f64 add, then cast" everywhere, but nearly: the two may differ in rare elements only
    acc = np.zeros_like(want)
    for k in F.k_order(c.K):
        acc = (c.x[:, k:k + 1].astype(np.float64) * c.w[None, :, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    print(f"twice-rounded chain differs from the fmaf chain in {int((acc != want).sum())} of {want.size} outputs")
    assert (acc != want).mean() < 1e-3


# ------------------------------------------------------------------------------------------------ GELU coefficients
def test_kernel_gelu_coefficients_are_the_reference_polynomial():
    """gemm_ref.gelu_tolerance() is derived from _Q; it applies to gemm_f32.hip only while its gelu_erf -- the one of gelu_f16.h, which
    it shares with gemm_f16.hip -- holds the same eight numbers, in the same Horner order."""
    kernel = KERNEL.read_text()
    assert '#include "gelu_f16.h"' in kernel and "t = gelu_erf(t);" in kernel and "float gelu_erf(" not in kernel
    body = re.search(r"float gelu_erf\(float v\) \{(.*?)\n\}", (KERNEL.parent / "gelu_f16.h").read_text(), re.S).group(1)
    first = re.findall(r"float q = ([-+0-9.e]+)f;", body)
    rest = re.findall(r"q = fmaf\(q, u, ([-+0-9.e]+)f\);", body)
    assert len(first) == 1 and len(rest) == 7
    assert [float(v) for v in first + rest] == G._Q
    assert "__builtin_amdgcn_exp2f(-(q * u))" in body and "fmaf(-0.5f * u, e, fmaxf(v, 0.0f))" in body


# ------------------------------------------------------------------------------------------------ the representation bound
def _rep_error(a):
    a = np.asarray(a, np.float32)
    hi, lo = F.split_planes(a)
    return np.abs(a.astype(np.float64) - (hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11))      # exact in f64


def _log_uniform(rng, lo_exp, hi_exp, n):
    """Full-mantissa f32 values of both signs, log-uniform in [2^lo_exp, 2^hi_exp)."""
    v = np.exp2(rng.uniform(lo_exp, hi_exp, n)).astype(np.float32)
    return np.where(rng.integers(0, 2, n) == 1, -v, v)


def test_split_representation_bound():
    """|a - (hi + 2^-11 lo')| <= 2^-23 |a| for 2^-12 <= |a| < 65504 -- NOT 2^-24: hi leaves a remainder of up to 13 significant bits, of
    which lo' keeps 11 -- and <= 2^-36 absolute below 2^-12, where lo' is f16-subnormal (which is 2^-22 |a| at 2^-14)."""
    rng = np.random.default_rng(23)
    worst = np.float32(1 + 2.0 ** -12 + 2.0 ** -23)
    scales = np.exp2(np.arange(-12, 16)).astype(np.float32)
    hand = np.concatenate([s * scales for s in (worst, -worst, np.float32(1 + 2.0 ** -12 - 2.0 ** -23), np.float32(1 + 3 * 2.0 ** -12 + 2.0 ** -23),
                                                np.float32(2 - 2.0 ** -12 - 2.0 ** -23), np.float32(1.0), np.float32(2 - 2.0 ** -23))])
    hand = hand[np.abs(hand) < 65504.0]
    for lo_exp, hi_exp in ((-12, -4), (-4, 4), (4, np.log2(65504.0))):
        a = np.concatenate([_log_uniform(rng, lo_exp, hi_exp, 2_000_000), hand])
        a = a[(np.abs(a) >= 2.0 ** -12) & (np.abs(a) < 65504.0)]
        rel = _rep_error(a) / np.abs(a.astype(np.float64))
        print(f"[2^{lo_exp}, 2^{hi_exp:.3f}): max relative representation error 2^{np.log2(rel.max()):.3f}")
        assert rel.max() <= 2.0 ** -23
        assert rel.max() > 2.0 ** -24                      # the old statement is false in every group
    # tight: the example attains it
    assert _rep_error(worst) == 2.0 ** -23 and float(worst) == 1 + 2.0 ** -12 + 2.0 ** -23
    hi, lo = F.split_planes(worst)
    assert float(hi) == 1.0 and float(lo) == 0.5            # the remainder 2^-12 + 2^-23 scales to the tie 2^-1 + 2^-12 -> even
    # below 2^-12: absolute
    small = np.array([2.0 ** -12 * (1 - 2.0 ** -24), 2.0 ** -13, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -24), 2.0 ** -14 + 2.0 ** -37,
                      2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -36, 2.0 ** -37, 2.0 ** -149, 0.0, 3.0e-6], np.float32)
    for lo_exp, hi_exp in ((-14, -12), (-26, -14), (-60, -26)):
        a = np.concatenate([_log_uniform(rng, lo_exp, hi_exp, 2_000_000), small, -small])
        a = a[np.abs(a) < 2.0 ** -12]
        err = _rep_error(a)
        print(f"[2^{lo_exp}, 2^{hi_exp}): max absolute representation error 2^{np.log2(err.max()):.3f}")
        assert err.max() <= 2.0 ** -36
        if lo_exp == -14:
            mid = (np.abs(a) >= 2.0 ** -14)
            rel = err[mid] / np.abs(a[mid].astype(np.float64))
            print(f"[2^-14, 2^-12): max relative representation error 2^{np.log2(rel.max()):.3f}")
            assert 2.0 ** -23 < rel.max() <= 2.0 ** -22     # looser than 2^-23 there, as documented
