"""Exact references for csrc/conv_nhwc.hip (tests/test_conv_nhwc_exact_gpu.py, tests/test_conv_host_cpu.py).

Operands are dyadic -- x in {-3, -2.75, ..., 3}, w in {-1, -1/2, 0, 0, 0, 1/2, 1}, bias in {-8, -7.875, ..., 8} -- so every product and
every partial sum is a multiple of 1/8 and, while |sum| < 1024, exact in f32 in ANY summation order: the f64 convolution on the
CPU is then the one value an f32 accumulator can hold, and the f16 output without activation is one round-to-nearest-even of it.
Multiples of 1/8 below 256 are f16 numbers themselves, so with these operands that rounding rarely has anything to do; the ``fine``
operands -- x in {-3, -3 + 1/64, ..., 3}, bias in multiples of 1/128, the same weights -- give sums in multiples of 1/128 (17 bits
below 1024: still exact in f32 in any order) of which about a third need the rounding, exact ties included.
Everything returned by ``case`` is cached and shared between tests: treat it as read-only."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch

# the five tile shapes (pixels x channels) the kernel is compiled for and, for each, the smallest layer found -- more than one tile,
# ragged in pixels and in channels, batch >= 2, odd height and width -- that pick_cfg gives it: (B, Ho, Wo, cout) of the OUTPUT
TILE_WITNESS = {
    (64, 64): (2, 5, 7, 72),            # M = 70
    (128, 64): (3, 17, 161, 72),        # M = 8211
    (128, 128): (3, 31, 117, 136),      # M = 10881
    (256, 64): (2, 55, 149, 136),       # M = 16390
    (64, 128): (3, 11, 163, 328),       # M = 5379
}
PRE_LIMIT = 1024.0      # what the pre-activations stay below (asserted): 13 bits in eighths, 17 bits in 1/128ths


def picked_tile(pixels, cin, cout, k):
    from vlfm_amd import _lib

    bm, bn = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().vlfm_conv_nhwc_tile(pixels, cin, cout, k, ctypes.byref(bm), ctypes.byref(bn)), "conv_nhwc_tile")
    return bm.value, bn.value


def input_size(out_size, stride):
    """The odd input height / width that gives ``out_size`` under 'same' padding (k = 1 and k = 3 alike)."""
    return out_size if stride == 1 else 2 * out_size - 1


@functools.lru_cache(maxsize=None)
def case(B, cin, cout, k, s, Ho, Wo, fine=False):
    """Dyadic operands of one layer (CPU, f16; x is [B, cin, H, W] with NHWC memory) and its exact pre-activations in f64:
    ``pre`` with the bias, ``pre_nobias`` without, both [B, Ho, Wo, cout] numpy arrays."""
    H, W = input_size(Ho, s), input_size(Wo, s)
    g = torch.Generator().manual_seed(((B * 131 + cin) * 131 + cout) * 131 + k * 7 + s * 3 + Ho * 1009 + Wo + 7919 * fine)
    xden = 64 if fine else 4          # x = integers / xden in [-3, 3]; a product is a multiple of 1 / (2 xden), and so is the bias
    # |x w| <= 3, so no partial sum in any order exceeds 3 K: with this it is an integer / (2 xden) of at most 24 bits
    assert 3 * k * k * cin * 2 * xden < 2 ** 24
    x = (torch.randint(-3 * xden, 3 * xden + 1, (B, H, W, cin), generator=g).double() / xden).half().permute(0, 3, 1, 2)
    levels = torch.tensor([-1.0, -0.5, 0.0, 0.0, 0.0, 0.5, 1.0])
    w = levels[torch.randint(0, 7, (cout, cin, k, k), generator=g)].half()
    b = (torch.randint(-8 * 2 * xden, 8 * 2 * xden + 1, (cout,), generator=g).double() / (2 * xden)).half()
    pre = torch.nn.functional.conv2d(x.double().contiguous(), w.double(), None, stride=s, padding=k // 2)
    assert pre.shape == (B, cout, Ho, Wo)
    pre_nobias = pre.permute(0, 2, 3, 1).contiguous().numpy()
    pre = pre_nobias + b.double().numpy()
    for p in (pre, pre_nobias):        # the premise of exactness, on the reference alone
        assert float(np.abs(p).max()) < PRE_LIMIT and np.array_equal(p * 2 * xden, np.round(p * 2 * xden))
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return SimpleNamespace(B=B, cin=cin, cout=cout, k=k, s=s, H=H, W=W, Ho=Ho, Wo=Wo, x=x, w=w, b=b, pre=pre, pre_nobias=pre_nobias)


def f16_bits(values_f64):
    """One round-to-nearest-even f64 -> f16 (numpy converts directly, without an f32 step), as int16 bit patterns."""
    with np.errstate(over="raise"):
        return values_f64.astype(np.float16).view(np.int16)


def silu_f64(pre):
    with np.errstate(over="ignore"):
        return pre / (1.0 + np.exp(-pre))


def ordered(bits):
    """int16 f16 bit patterns -> integers in value order, one step per f16 ulp (2^-24 in the subnormal range), -0 == +0."""
    v = np.asarray(bits).view(np.int16).astype(np.int32)
    return np.where(v >= 0, v, -(v & 0x7FFF))


def ulp_distance(got_bits, want_bits):
    """Elementwise |got - want| in f16 ulps; ``got`` must hold no NaN / inf (asserted)."""
    got = np.asarray(got_bits).view(np.int16)
    assert not bool(((got & 0x7C00) == 0x7C00).any()), "NaN or inf in the kernel's output"
    return np.abs(ordered(got) - ordered(want_bits))
