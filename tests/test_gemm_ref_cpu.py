"""tests/gemm_ref.py checked on its own, without a GPU: the GELU tolerance A that tests/test_gemm_f16_exact_gpu.py imports, the
branches of the GELU expectation outside [-12, 12], the operand sets' shares of outputs that exercise the f16 rounding, and the torch
evaluation of the expectations (used for the large cases, on the device) against the numpy one (the definition)."""
import numpy as np
import pytest
import torch

import conv_ref as R
import gemm_ref as G

# the shapes of tests/test_gemm_f16_exact_gpu.py that do not depend on the device's CU count
SHAPES = [(1, 8, 64), (256, 256, 64), (255, 248, 128), (257, 264, 192), (300, 136, 256), (130, 384, 320), (257, 1408, 1408),
          (130, 264, 6144)]


def test_gelu_tolerance_is_measured_and_small():
    """A = the restated polynomial form's error against f64 + the allowance for v_exp_f32.  The header documents 2.8e-7 for the
    former; with max(0.5 u e) ~ 0.17 the allowance is ~4e-8: A must come out at or below 3.3e-7."""
    A, err, term = G.gelu_tolerance()
    print(f"gelu_erf restated in f32: max |error| vs f64 over [-12, 12] = {err:.4e}; max 0.5 u e = {term:.4f}; A = {A:.4e}")
    assert 1e-7 < err <= 2.8e-7 and 0.16 < term < 0.18
    assert A <= 3.3e-7


def test_gelu_restatement_is_the_identity_or_zero_beyond_12():
    """What the two outer branches of the GELU expectation rest on: for f32 v with 12 <= |v| <= 65504 the form returns max(v, 0)
    EXACTLY (the subtracted term is below half an ulp of v, or an exact zero)."""
    v = np.concatenate([np.linspace(12.0, 65504.0, 1 << 20), np.arange(1536, 4097) * G.UNIT, 2.0 ** np.arange(4, 16),
                        np.nextafter(np.float32(12.0), np.float32(13.0), dtype=np.float32)[None]]).astype(np.float32)
    v = v[v > 12.0]
    pos, _ = G.gelu_erf_f32(v)
    neg, _ = G.gelu_erf_f32(-v)
    assert np.array_equal(pos, v)
    assert not bool(neg.any())            # +-0


def test_fma32_rounds_once():
    """_fma32 against exact rational arithmetic on random f32 triples, cancellation and f32 ties included."""
    from fractions import Fraction

    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)
    c[::2] = rng.standard_normal(2000).astype(np.float32)
    got = G._fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i


def test_rn16_is_numpys_f64_to_f16():
    """The torch rounding used on the device for the large cases == numpy's direct f64 -> f16 conversion: on every f16 number, every
    midpoint between two of them (ties), their f64 neighbours (where a detour through f32 rounds twice), and random values."""
    h = np.arange(0, 0x7C00, dtype=np.int16).view(np.float16).astype(np.float64)
    mid = (h[:-1] + h[1:]) / 2
    pts = np.concatenate([h, mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf), [65519.99, 65520.0, 65521.0, 7e4, 1e-9, 0.0],
                          np.random.default_rng(3).standard_normal(200000) * 100])
    pts = np.concatenate([pts, -pts])
    got = G.rn16(torch.from_numpy(pts)).numpy()
    assert np.array_equal(got, G.f16_value(pts))
    assert np.array_equal(np.signbit(got), np.signbit(pts))
    t = torch.tensor([float("nan"), float("inf"), -float("inf")], dtype=torch.float64)
    r = G.rn16(t)
    assert bool(torch.isnan(r[0])) and r[1] == float("inf") and r[2] == -float("inf")


def test_f16_bits_saturates_at_the_tie():
    v = np.array([65504.0, 65519.9921875, 65520.0, -65519.9921875, -65520.0, 1e9, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -24])
    want = np.array([65504.0, 65504.0, np.inf, -65504.0, -np.inf, np.inf, 2.0 ** -24, 0.0, 2.0 ** -23, -2.0 ** -24])
    assert np.array_equal(G.f16_value(v), want)


def test_edge_case_expectations():
    """The hand-made elements of gemm_ref.edge_case(): what the f64 reference and the roundings defined here make of them is what
    their names say (gemm_ref.EDGE_OUTCOMES), and NaN is expected in exactly the last row and the last column."""
    c = G.edge_case()
    A = G.gelu_tolerance()[0]
    M, N, _ = G.EDGE_SHAPE
    assert np.isnan(c.pre[M - 1]).all() and np.isnan(c.pre[:, N - 1]).all() and int(np.isnan(c.pre).sum()) == M + N - 1
    assert int(torch.isnan(c.x).sum()) == 1 and int(torch.isnan(c.w).sum()) == 1
    clean = {True: np.nan_to_num(c.pre), False: np.nan_to_num(c.pre_nobias)}
    want = {}
    for wb in (True, False):
        want["bias", wb] = (G.f16_value(clean[wb]),) * 2
        want["accumulate", wb] = (G.f16_value(np.nan_to_num(G.want_accumulate(clean[wb], c.r0))),) * 2
    lo, hi = G.gelu_bounds(clean[True], A)
    want["bias_gelu", True] = (G.f16_value(lo), G.f16_value(hi))
    assert {k for k, _, _ in G.EDGE_OUTCOMES} == set(want)
    for key, (m, n), value in G.EDGE_OUTCOMES:
        assert want[key][0][m, n] == value == want[key][1][m, n], (key, m, n, value, want[key][0][m, n], want[key][1][m, n])
    for name, (m, n, _, _, _) in G.EDGE_COLUMNS.items():
        print(f"{name}: pre {c.pre[m, n]!r}, without bias {c.pre_nobias[m, n]!r}, r0 {float(c.r0[m, n])!r}")


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in SHAPES])
def test_operand_sets_exercise_the_rounding(shape):
    """From the reference alone: at least 5 % of a wide case's outputs need the one f16 rounding and 2 % are exact ties; at least
    30 % of a narrow K <= 192 case's pre-activations lie in [-6, 6] and 5 % in GELU's negative tail [-6, -1].  (1, 8, 64) has eight
    outputs: shares of eight say nothing, it is printed only.)  The torch evaluation agrees with the numpy one on the same case."""
    M, N, K = shape
    c = G.operands(M, N, K)
    pre = G.pre_cpu(c.x, c.w, c.b)
    assert float(np.abs(pre).max()) < 2 ** 15
    inexact, tie = G.shares(pre)
    cn = G.operands(M, N, K, narrow=True)
    pre_n = G.pre_cpu(cn.x, cn.w, cn.b)
    mid, tail = G.gelu_shares(pre_n)
    print(f"{shape}: wide inexact {inexact:.1%} ties {tie:.1%} max|pre| {np.abs(pre).max():.1f}; narrow in [-6, 6] {mid:.1%} in [-6, -1] "
          f"{tail:.1%}; accumulate inexact {G.shares(G.want_accumulate(pre, c.r0))[0]:.1%}")
    if M * N >= 1024:
        assert inexact >= 0.05 and tie >= 0.02
        if K <= 192:
            assert mid >= 0.30 and tail >= 0.05
    ti, tt = G.shares_t(torch.from_numpy(pre))
    assert (ti, tt) == pytest.approx((inexact, tie), abs=1e-12)
    assert G.gelu_shares_t(torch.from_numpy(pre_n)) == pytest.approx((mid, tail), abs=1e-12)
    A = G.gelu_tolerance()[0]
    # the torch forms flag exactly what the numpy checks flag: the right answer passes both, its neighbour one ulp up fails both
    for p, want, mask_t in ((pre, G.f16_bits(pre), G.bad_exact_t), (pre_n, G.f16_bits(G.gelu64(pre_n)), None)):
        bits = want.copy()
        if mask_t is not None:
            G.check_exact(bits, p, "exact, numpy")
            assert not bool(mask_t(torch.from_numpy(bits).view(torch.float16), torch.from_numpy(p)).any())
            bits[0, 0] += 1
            with pytest.raises(AssertionError):
                G.check_exact(bits, p, "one ulp up, numpy")
            assert int(mask_t(torch.from_numpy(bits).view(torch.float16), torch.from_numpy(p)).sum()) == 1
        else:
            G.check_gelu(bits, p, A, "gelu, numpy")
            assert not bool(G.bad_gelu_t(torch.from_numpy(bits).view(torch.float16), torch.from_numpy(p), A).any())
            lo, hi = G.gelu_bounds(p, A)
            up = R.ordered(G.f16_bits(hi)) + 1                   # one f16 step above the upper bound, everywhere
            bits = np.where(up >= 0, up, 0x8000 - up).astype(np.uint16).view(np.int16)
            bad_t = G.bad_gelu_t(torch.from_numpy(bits).view(torch.float16), torch.from_numpy(p), A)
            assert bool(bad_t.all())
            with pytest.raises(AssertionError):
                G.check_gelu(bits, p, A, "one ulp above the bound, numpy")
