"""-m gpu: vlfm_gemm_f32_nt and vlfm_split_f32_to_f16_pair (csrc/gemm_f32.hip) against references with ONE right answer, bit for bit
(tests/gemm_f32_ref.py; tests/test_gemm_f32_ref_cpu.py shows that those references report wrong kernels).

  exact form   random full-mantissa operands: the result is the f32 fma chain in the kernel's k order, then the epilogue's f32
               arithmetic.  The arbiter for the assumed order: coarse dyadic operands, whose result is the f64 product in ANY order.
  split form   dyadic operands whose hi / lo' planes are known exactly: the result is fmaf(acc2, 2^-11, acc1) with exact acc1, acc2
               (the split model), then the same epilogue.  The flag is cleared before every call and must stay 0.
  GELU         the pre-activation is known bit for bit; the output must lie within the f32 roundings of gelu64 -+ A (+ residual).
Shapes (gemm_f32_ref.SHAPES): the smallest at which each path exists -- one clamped element with scalar stores and a single K-tile,
2 x 2 tiles with M and N tails on the vector path, N % 4 == 3 and == 2 (scalar stores, scalar residual, scalar bias gather), 12 and 9
workgroups (the XCD remap with remainders 4 and 1), an odd number of K-tiles, 64 K-tiles.  Every launch writes into a buffer of NaNs
with 4096 sentinel floats on either side.  Around them: inputs left untouched, a bias 4 bytes off alignment, NaN confinement, the
boundary of the overflow flag, the split kernel on its value edges, and the refusals of the entry."""
import numpy as np
import pytest
import torch

import gemm_f32_ref as F

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4096, -777.25
UNWRITTEN = 0x7FC05A5A           # an f32 NaN: what C holds before a launch
PLANE_PATTERN = 0x7E5A           # an f16 NaN: the same for the planes
OWNER = "gemm-f32-exact-tests"   # a flag of our own
IDS = [f"{m}x{n}x{k}" for m, n, k in F.SHAPES]
TAIL_SHAPES = [(130, 132, 64), (129, 131, 96)]
# (name, activation, residual: None / "separate" / "in place"); all but the first with a bias
EPILOGUES = [("no epilogue", None, None), ("bias", None, None), ("bias + ReLU", "relu", None), ("bias + residual", None, "separate"),
             ("bias + ReLU + residual in place", "relu", "in place"), ("bias + GELU + residual", "gelu", "separate")]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _flag(dev):
    from vlfm_amd.vlm import ops

    return ops.gemm_f32_overflow_flag(dev, OWNER)


def _launch(x, w, b, act, r, mode, precision):
    """One launch into NaN-filled C inside a sentinel-filled flat buffer -> (C as numpy [M, N], the flag after the call).  ``mode``
    "in place": C holds the residual and is passed as the residual."""
    from vlfm_amd.vlm import ops

    M, N = x.shape[0], w.shape[0]
    flat = torch.full((2 * GUARD + M * N,), SENTINEL, dtype=torch.float32, device=x.device)
    out = flat[GUARD:GUARD + M * N].view(M, N)
    assert out.data_ptr() % 16 == 0
    out.view(torch.int32).fill_(UNWRITTEN)
    if mode == "in place":
        out.copy_(r)
    flag = _flag(x.device)
    flag.zero_()
    got = ops.linear_f32(x, w, b, act=act, residual={None: None, "separate": r, "in place": out}[mode], precision=precision, out=out,
                         owner=OWNER)
    assert got.data_ptr() == out.data_ptr()
    whole = flat.cpu().numpy()
    assert (whole[:GUARD] == SENTINEL).all(), "floats in front of C were written"
    assert (whole[GUARD + M * N:] == SENTINEL).all(), "floats behind C were written"
    return whole[GUARD:GUARD + M * N].reshape(M, N), int(flag.item())


def _check(got, pre32, b, act, r, what):
    if act == "gelu":
        _, lo, hi = F.epilogue(pre32, b, act, r)
        F.check_between(got, lo, hi, what)
    else:
        F.check_bits(got, F.epilogue(pre32, b, act, r), what)


def _run_epilogues(c, pre32, dev, precision, what, gelu=None):
    """Every epilogue on the operands ``c`` whose value before the epilogue is ``pre32``; ``gelu`` = (operands, pre32) for the GELU run
    where that uses a set of its own."""
    t = {id(s): [_dev(a, dev) for a in (s.x, s.w, s.b, s.r)] for s in (c,) + ((gelu[0],) if gelu else ())}
    for name, act, mode in EPILOGUES:
        s, p = gelu if (gelu and act == "gelu") else (c, pre32)
        x, w, b, r = t[id(s)]
        with_bias = name != "no epilogue"
        got, flag = _launch(x, w, b if with_bias else None, act, r, mode, precision)
        assert flag == 0, f"{what}, {name}: the overflow flag was raised"
        _check(got, p, s.b if with_bias else None, act, s.r if mode else None, f"{what}, {name}")


# ------------------------------------------------------------------------------------------------ exact form
@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_exact_form_is_the_fma_chain_and_the_f32_epilogue(gpu_device, shape):
    M, N, K = shape
    d = F.dyadic_split_operands(M, N, K)
    # the arbiter: P/8 . (Q/16)^T is exact in f32 whatever the order -- this fails on a wrong index, never on a wrong assumed order
    coarse, _ = _launch(_dev(d.xc, gpu_device), _dev(d.wc, gpu_device), None, None, None, None, "exact")
    want = d.xc.astype(np.float64) @ d.wc.astype(np.float64).T
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    F.check_bits(coarse, want.astype(np.float32), f"{shape} exact form, coarse dyadic operands against f64")
    c = F.random_operands(M, N, K)
    chain = F.fma_chain(c.x, c.w, F.k_order(K))
    try:
        _run_epilogues(c, chain, gpu_device, "exact", f"{shape} exact form")
    except AssertionError as e:
        raise AssertionError(f"{e}\n(the coarse dyadic operands of this shape came out exact, in any k order: the kernel's indexing holds; "
                             f"if 'no epilogue' is what differs, the fault lies in the k order assumed by gemm_f32_ref.k_order)") from e


# ------------------------------------------------------------------------------------------------ split form
@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_split_form_is_the_split_model_and_the_f32_epilogue(gpu_device, shape):
    from vlfm_amd.vlm import ops

    M, N, K = shape
    c, n = F.dyadic_split_operands(M, N, K), F.dyadic_split_operands(M, N, K, narrow=True)
    for s in (c, n):
        w = _dev(s.w, gpu_device)
        _flag(gpu_device).zero_()
        hi, lo = ops.split_weight(w, OWNER)
        want_hi, want_lo = F.split_planes(s.w)
        assert np.array_equal(hi.cpu().numpy().view(np.int16), want_hi.view(np.int16)), "hi plane of w"
        assert np.array_equal(lo.cpu().numpy().view(np.int16), want_lo.view(np.int16)), "lo plane of w"
        assert int(_flag(gpu_device).item()) == 0
    pre_n = F.split_model(n.x, n.w)
    inside = float((np.abs(F.epilogue(pre_n, n.b)) <= 6.0).mean())
    print(f"{shape} narrow: {inside:.1%} of the GELU pre-activations in [-6, 6]")
    assert inside >= 0.5
    _run_epilogues(c, F.split_model(c.x, c.w), gpu_device, "split", f"{shape} split form", gelu=(n, pre_n))


# ------------------------------------------------------------------------------------------------ around C
def _pre32(form, s):
    return F.fma_chain(s.x, s.w, F.k_order(s.K)) if form == "exact" else F.split_model(s.x, s.w)


def _operands(form, shape):
    return F.random_operands(*shape) if form == "exact" else F.dyadic_split_operands(*shape)


@pytest.mark.parametrize("form", ["exact", "split"])
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=["130x132x64", "129x131x96"])
def test_inputs_are_left_untouched(gpu_device, shape, form):
    """x, w, the bias, the planes and a residual that is not aliased come back bit for bit (the sentinels around C: every launch)."""
    from vlfm_amd.vlm import ops

    s = _operands(form, shape)
    x, w, b, r = (_dev(a, gpu_device) for a in (s.x, s.w, s.b, s.r))
    planes = ops.split_weight(w, OWNER) if form == "split" else ()
    before = [t.clone() for t in (x, w, b, r) + tuple(planes)]
    got, _ = _launch(x, w, b, "relu", r, "separate", form)
    for name, t, t0 in zip(("x", "w", "bias", "residual", "w_hi", "w_lo"), (x, w, b, r) + tuple(planes), before):
        a, a0 = (v.view(torch.int16 if v.dtype == torch.float16 else torch.int32) for v in (t, t0))
        assert torch.equal(a, a0), f"{name} was written"
    if form == "split":
        assert ops.split_weight(w, OWNER)[0].data_ptr() == planes[0].data_ptr()            # the launch used these planes
    F.check_bits(got, F.epilogue(_pre32(form, s), s.b, "relu", s.r), f"{shape} {form} form, bias + ReLU + separate residual")


@pytest.mark.parametrize("form", ["exact", "split"])
def test_bias_off_alignment_takes_the_scalar_gather(gpu_device, form):
    """N % 4 == 0 (vector stores) with a bias that starts 4 bytes behind a 16-byte boundary: the same bits as with an aligned bias."""
    shape = TAIL_SHAPES[0]
    s = _operands(form, shape)
    x, w, b = (_dev(a, gpu_device) for a in (s.x, s.w, s.b))
    odd = torch.full((s.N + 8,), 1.0e3, dtype=torch.float32, device=gpu_device)[1:s.N + 1]
    odd.copy_(b)
    assert s.N % 4 == 0 and odd.is_contiguous() and odd.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 0
    aligned, _ = _launch(x, w, b, None, None, None, form)
    got, _ = _launch(x, w, odd, None, None, None, form)
    F.check_bits(got, aligned, f"{shape} {form} form, bias 4 bytes off against the aligned bias")
    F.check_bits(got, F.epilogue(_pre32(form, s), s.b), f"{shape} {form} form, bias 4 bytes off")


@pytest.mark.parametrize("form", ["exact", "split"])
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=["130x132x64", "129x131x96"])
def test_nan_stays_in_its_row_and_column(gpu_device, shape, form):
    """A NaN in x[M - 1, 20] and one in w[N - 1, 33]: NaN in exactly row M - 1 and column N - 1 (the rows a padded tile row is clamped
    to), every other output as before, bit for bit; the split form raises its flag."""
    s = _operands(form, shape)
    M, N, K = shape
    x, w = np.array(s.x), np.array(s.w)
    x[M - 1, 20] = np.nan
    w[N - 1, 33] = np.nan
    pre = _pre32(form, type(s)(x=x, w=w, K=K))
    want = F.epilogue(pre, s.b, None, s.r)
    mask = np.zeros((M, N), bool)
    mask[M - 1, :] = True
    mask[:, N - 1] = True
    assert np.array_equal(np.isnan(want), mask)
    got, flag = _launch(_dev(x, gpu_device), _dev(w, gpu_device), _dev(s.b, gpu_device), None, _dev(s.r, gpu_device), "separate", form)
    assert np.array_equal(np.isnan(got), mask), f"{shape} {form} form: NaN is not confined to row {M - 1} and column {N - 1}"
    F.check_bits(got, want, f"{shape} {form} form, NaN in the last row of x and of w")
    assert flag == (1 if form == "split" else 0)
    _flag(gpu_device).zero_()


# ------------------------------------------------------------------------------------------------ the flag's boundary
@pytest.mark.parametrize("probe,raised", [(65504.0, 1), (float(np.nextafter(np.float32(65504.0), np.float32(0.0))), 0)],
                         ids=["65504", "below-65504"])
def test_split_flag_boundary(gpu_device, probe, raised):
    """x zero apart from x[M - 1, K - 1]: 65504 raises the flag, its f32 predecessor (hi = 65504, lo' = -8) does not and gives the
    split model's finite result."""
    M, N, K = TAIL_SHAPES[0]
    s = F.dyadic_split_operands(M, N, K)
    x = np.zeros((M, K), np.float32)
    x[M - 1, K - 1] = probe
    assert x[M - 1, K - 1] == np.float32(probe) and (raised == 1) == (probe >= 65504.0)
    got, flag = _launch(_dev(x, gpu_device), _dev(s.w, gpu_device), None, None, None, None, "split")
    assert flag == raised
    _flag(gpu_device).zero_()
    if not raised:
        want = F.split_model(x, s.w)
        assert np.isfinite(got).all() and bool(want[M - 1].any()) and not want[:M - 1].any()
        F.check_bits(got, want, f"split form, x[M - 1, K - 1] = {probe!r}")


# ------------------------------------------------------------------------------------------------ vlfm_split_f32_to_f16_pair
def _edge_values():
    rng = np.random.default_rng(257)
    special = [0.0, -0.0, 2.0 ** -149, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -14,
               float(np.nextafter(np.float32(2.0 ** -14), np.float32(0.0))), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -23,
               1 + 2.0 ** -12 + 2.0 ** -23, -(2.0 ** -25), -(1 + 2.0 ** -12 + 2.0 ** -23)]
    rest = np.exp2(rng.uniform(-20, 15, 257 - len(special))) * rng.choice([-1.0, 1.0], 257 - len(special))
    a = np.concatenate([special, rest]).astype(np.float32)
    assert a.size == 257 and a.size % 256 != 0 and np.signbit(a[1]) and a[2] == np.float32(2.0 ** -149) and a[2] > 0
    return a


def _split_on_device(a, dev, count=None):
    """vlfm_split_f32_to_f16_pair on ``a`` into pattern-filled planes with 64 spare elements -> (rc, hi bits, lo bits, flag)."""
    from vlfm_amd import _lib

    src = _dev(a, dev)
    hi = torch.full((a.size + 64,), PLANE_PATTERN, dtype=torch.int16, device=dev)
    lo = torch.full((a.size + 64,), PLANE_PATTERN, dtype=torch.int16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().vlfm_split_f32_to_f16_pair(src.data_ptr(), hi.data_ptr(), lo.data_ptr(), a.size if count is None else count,
                                                flag.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, hi.cpu().numpy(), lo.cpu().numpy(), int(flag.item())


def test_split_kernel_on_value_edges(gpu_device):
    """257 values (count % 256 != 0): +-0, f32 and f16 subnormals, the ties of f16's smallest steps, 2^-14 and its predecessor, the
    ties of lo', random full-mantissa values over 35 binades: both planes bit for bit, nothing behind element 256, flag 0.  Then
    65504, -65504, inf and NaN, each alone in the last place: flag 1."""
    from vlfm_amd import _lib

    a = _edge_values()
    want_hi, want_lo = (p.view(np.int16) for p in F.split_planes(a))
    rc, hi, lo, flag = _split_on_device(a, gpu_device)
    assert rc == _lib.VLFM_OK and flag == 0
    for name, got, want in (("hi", hi, want_hi), ("lo", lo, want_lo)):
        bad = got[:a.size] != want
        print(f"split kernel, {name} plane: {int(bad.sum())} of {bad.size} outputs differ")
        assert not bad.any(), (name, int(np.argmax(bad)), float(a[np.argmax(bad)]), hex(int(got[np.argmax(bad)]) & 0xFFFF),
                               hex(int(want[np.argmax(bad)]) & 0xFFFF))
        assert (got[a.size:] == PLANE_PATTERN).all(), f"{name} plane written behind element {a.size - 1}"
    for v in (65504.0, -65504.0, np.inf, np.nan):
        b = a.copy()
        b[-1] = v
        rc, hi, lo, flag = _split_on_device(b, gpu_device)
        assert rc == _lib.VLFM_OK and flag == 1, v
        assert np.array_equal(hi[:a.size - 1], want_hi[:-1]) and np.array_equal(lo[:a.size - 1], want_lo[:-1]), v
    rc, hi, lo, flag = _split_on_device(a, gpu_device, count=0)
    assert rc == _lib.VLFM_OK and flag == 0 and (hi == PLANE_PATTERN).all() and (lo == PLANE_PATTERN).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_gemm_f32_refusals(gpu_device):
    """VLFM_ERR_INVALID, and C untouched: K % 32 != 0, K == 0, activation 3, precision 2, x / w / c / residual 4 bytes off alignment,
    the split form without its planes or without the flag.  m == 0 or n == 0: VLFM_OK, nothing done."""
    from vlfm_amd import _lib

    L = _lib.lib()
    M, N, K = 64, 64, 64
    f32 = dict(dtype=torch.float32, device=gpu_device)

    def shifted(shape):
        n = int(np.prod(shape))
        t = torch.full((n + 8,), 3.0, **f32)[1:n + 1].view(shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t

    x, w, r = torch.ones((M, K), **f32), torch.ones((N, K), **f32), torch.ones((M, N), **f32)
    c = torch.full((M, N), SENTINEL, **f32)
    hi = torch.ones((N, K), dtype=torch.float16, device=gpu_device)
    lo = torch.zeros_like(hi)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    assert all(t.data_ptr() % 16 == 0 for t in (x, w, r, c, hi, lo))

    def call(x=x, w=w, r=r, c=c, m=M, n=N, k=K, act=0, prec=0, hi=hi, lo=lo, flag=flag):
        p = [t.data_ptr() if t is not None else None for t in (x, w, None, r, c)]
        q = [t.data_ptr() if t is not None else None for t in (hi, lo, flag)]
        return L.vlfm_gemm_f32_nt(*p, m, n, k, act, prec, *q, None)

    refused = {"K % 32 != 0": dict(k=48), "K == 0": dict(k=0), "activation 3": dict(act=3), "precision 2": dict(prec=2),
               "x off alignment": dict(x=shifted((M, K))), "w off alignment": dict(w=shifted((N, K))),
               "residual off alignment": dict(r=shifted((M, N))), "split without w_hi": dict(prec=1, hi=None),
               "split without w_lo": dict(prec=1, lo=None), "split without the flag": dict(prec=1, flag=None)}
    for name, kw in refused.items():
        assert call(**kw) == _lib.VLFM_ERR_INVALID, name
        assert "gemm_f32_nt" in _lib.last_error(), name
    odd_c = shifted((M, N))
    assert call(c=odd_c) == _lib.VLFM_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert call(m=0) == _lib.VLFM_OK and call(n=0) == _lib.VLFM_OK and call(m=0, prec=1) == _lib.VLFM_OK
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all()) and bool((odd_c == 3.0).all()) and int(flag.item()) == 0
    # ... and the same arguments, unmodified, are accepted: the refusals above are due to what each one changed
    assert call() == _lib.VLFM_OK and call(prec=1) == _lib.VLFM_OK
    torch.cuda.synchronize()
    assert bool((c == float(K) + 1.0).all()) and int(flag.item()) == 0             # 64 products of 1 and the residual 1
