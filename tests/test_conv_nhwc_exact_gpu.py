"""vlfm_conv_nhwc_f16 (csrc/conv_nhwc.hip) against an f64 convolution on the CPU, bit for bit, on every tile shape pick_cfg can choose.

The operands are dyadic (tests/conv_ref.py): every product and partial sum is exact in f32 in any summation order, so the f64
pre-activation is the ONLY value a correct f32 accumulator can hold.
  * act = None, with and without bias: the output is pre rounded once to f16 -- compared as int16, -0 == +0.  A second rounding, a
    K-slot read twice or not at all, a wrong tap, a wrong bias lane, a row stored to the wrong pixel: all show.
  * SiLU: within ONE f16 ulp (2^-24 in the subnormal range) of silu(pre) evaluated in f64 and rounded once to f16.  Derived, not
    measured: v_exp_f32 and v_rcp_f32 are ~1 ulp of f32 each, scaling the argument by log2(e) costs |v| 2^-23 relative in the
    exponential (|v| < 1024 -- and beyond |v| ~ 20 the result is v or 0 whatever the exponential's last bits); together < 2^-13
    relative, far below half an f16 ulp (2^-12), so only a value next to a rounding tie can move, and by one.
Cases: per tile shape its witness layer (conv_ref.TILE_WITNESS: > 1 tile, ragged in pixels and channels, B >= 2, odd H and W; each
case asserts through vlfm_conv_nhwc_tile that it lands on the shape it is named for) as 3x3 / stride 1 / Cin 64 (plain staging),
3x3 / stride 2 / Cin 72 (GEN staging: every 16-byte slot decodes its own tap), 1x1 / stride 1 / Cin 64 (one K-tile: prologue only)
and 1x1 / stride 2 / Cin 128 (two K-tiles); on 64x64 also Cin 512 (72 K-tiles), Cin 8 (K = 72 padded to 128) and one pixel.
Around them: finer operands whose sums need the rounding, NaN-filled surroundings of sliced tensors, a repeat screen and the
argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

PATTERN = 0x7E5A        # an f16 NaN: what output buffers hold before a launch
TILES = list(R.TILE_WITNESS)
VARIANTS = [(3, 1, 64), (3, 2, 72), (1, 1, 64), (1, 2, 128)]       # (k, stride, cin)
# (tile, B, Ho, Wo, cin, cout, k, s)
CASES = [(t,) + R.TILE_WITNESS[t][:3] + (cin, R.TILE_WITNESS[t][3], k, s) for t in TILES for k, s, cin in VARIANTS] + [
    ((64, 64), 2, 5, 7, 512, 72, 3, 1),       # NT = 72: the long K loop
    ((64, 64), 2, 5, 7, 8, 72, 3, 1),         # K = 72 padded to 128 with zero weights: the second K-tile is mostly zero-page slots
    ((64, 64), 1, 1, 1, 16, 8, 3, 1),         # one pixel: eight of the nine taps are padding
    ((64, 64), 1, 1, 1, 16, 8, 1, 1),
]


def case_id(c):
    (bm, bn), B, Ho, Wo, cin, cout, k, s = c
    return f"tile{bm}x{bn}-B{B}x{Ho}x{Wo}-cin{cin}-cout{cout}-k{k}-s{s}"


def operands(c, dev):
    from vlfm_amd.vlm import det_ops

    rows, bias = det_ops.pack_conv_weight(c.w.to(dev), c.b.to(dev))
    return c.x.to(dev), rows, bias          # x keeps its NHWC memory across the copy


def nhwc_bits(y):
    """[B, C, H, W] f16 device tensor (any strides) -> [B, H, W, C] int16 numpy."""
    return y.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy()


def framework_silu(c, where):
    """What the framework's own f16 SiLU returns at one element (for the report when a comparison fails)."""
    v = torch.tensor([c.pre[where]], dtype=torch.float32, device="cuda").half()
    return float(torch.nn.functional.silu(v)[0])


def check_exact(got_bits, pre, what):
    want = R.f16_bits(pre)
    bad = R.ordered(got_bits) != R.ordered(want)
    print(f"{what}: {int(bad.sum())} of {bad.size} outputs differ from round_f16(f64)")
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at [b, y, x, n] = {i}: got "
                             f"{got_bits[i].view(np.float16)!r}, exact {pre[i]!r} -> f16 {want[i].view(np.float16)!r}")


def check_silu(got_bits, c, what):
    exact = R.silu_f64(c.pre)
    want = R.f16_bits(exact)
    d = R.ulp_distance(got_bits, want)
    flushed = (got_bits & 0x7FFF) == 0
    flushed &= (want & 0x7FFF) != 0
    print(f"{what}: max {int(d.max())} f16 ulp, {int((d == 1).sum())} of {d.size} one ulp off, {int(flushed.sum())} nonzero -> zero")
    if d.max() > 1:
        i = tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape))
        raise AssertionError(f"{what}: {int((d > 1).sum())} outputs beyond one f16 ulp, worst {int(d.max())} ulp at {i}: pre {c.pre[i]!r}, "
                             f"silu {exact[i]!r}, got {got_bits[i].view(np.float16)!r}, want {want[i].view(np.float16)!r}, the "
                             f"framework's f16 silu gives {framework_silu(c, i)!r}; {int(flushed.sum())} nonzero results came back zero")


def run_all_three(c, dev):
    from vlfm_amd.vlm import det_ops

    x, rows, bias = operands(c, dev)
    assert det_ops.conv_nhwc_supported(c.cin, c.cout, c.k, c.s) and x.shape == (c.B, c.cin, c.H, c.W)
    y = det_ops.conv_nhwc(x, rows, bias, c.k, c.s, None)
    assert y.shape == (c.B, c.cout, c.Ho, c.Wo)
    check_exact(nhwc_bits(y), c.pre, "bias, no activation")
    y = det_ops.conv_nhwc(x, rows, None, c.k, c.s, None)
    check_exact(nhwc_bits(y), c.pre_nobias, "no bias, no activation")
    y = det_ops.conv_nhwc(x, rows, bias, c.k, c.s, "silu")
    check_silu(nhwc_bits(y), c, "bias + SiLU")


@pytest.mark.parametrize("tile,B,Ho,Wo,cin,cout,k,s", CASES, ids=[case_id(c) for c in CASES])
def test_conv_is_exact_on_every_tile_shape(gpu_device, tile, B, Ho, Wo, cin, cout, k, s):
    assert R.picked_tile(B * Ho * Wo, cin, cout, k) == tile
    run_all_three(R.case(B, cin, cout, k, s, Ho, Wo), gpu_device)


@pytest.mark.parametrize("tile", TILES, ids=[f"tile{t[0]}x{t[1]}" for t in TILES])
@pytest.mark.parametrize("cin,s", [(64, 1), (72, 2)])
def test_conv_rounds_once(gpu_device, tile, cin, s):
    """Sums of the operands above are multiples of 1/8, mostly below 256: f16 numbers already, which a second rounding in the
    epilogue leaves alone.  With the fine operands (multiples of 1/64; sums in 1/128ths, still exact in f32 in any order) about
    a third of the outputs need the one rounding, exact ties (to even) among them -- which is also where SiLU in f32 may
    legitimately land one ulp from the f64 value: silu(v) of a large tie v lies just below the tie, its f32 value on it."""
    B, Ho, Wo, cout = R.TILE_WITNESS[tile]
    c = R.case(B, cin, cout, 3, s, Ho, Wo, fine=True)
    inexact = R.f16_bits(c.pre).view(np.float16).astype(np.float64) != c.pre
    assert inexact.mean() > 0.25
    run_all_three(c, gpu_device)


# (tile, cin, stride): 3x3 on the plain and on the GEN staging path, both strides
POISON = [(t, cin, s) for t in TILES for cin in (64, 72) for s in (1, 2)]


@pytest.mark.parametrize("tile,cin,s", POISON, ids=[f"tile{t[0]}x{t[1]}-cin{cin}-s{s}" for t, cin, s in POISON])
def test_conv_in_poisoned_surroundings(gpu_device, tile, cin, s):
    """Input and output are views [1 : B + 1, 8 : 8 + channels] of NHWC buffers with an image before, an image after and wider
    pixels.  Everything around the input is NaN: a 16-byte read outside the logical tensor -- also one that only meets zero weights,
    as in a padded K slot -- puts a NaN into the result.  Everything around the output must keep its bit pattern."""
    from vlfm_amd.vlm import det_ops

    B, Ho, Wo, cout = R.TILE_WITNESS[tile]
    assert R.picked_tile(B * Ho * Wo, cin, cout, 3) == tile
    c = R.case(B, cin, cout, 3, s, Ho, Wo)
    _, rows, bias = operands(c, gpu_device)
    c0, xp, op = 8, cin + 24, cout + 32
    xbuf = torch.full((B + 2, c.H, c.W, xp), float("nan"), dtype=torch.float16, device=gpu_device)
    x = xbuf.permute(0, 3, 1, 2)[1:B + 1, c0:c0 + cin]
    x.copy_(c.x.to(gpu_device))
    assert int(torch.isnan(xbuf).sum()) == xbuf.numel() - c.x.numel()
    for act in (None, "silu"):
        obuf = torch.full((B + 2, Ho, Wo, op), PATTERN, dtype=torch.int16, device=gpu_device)
        out = obuf.view(torch.float16).permute(0, 3, 1, 2)[1:B + 1, c0:c0 + cout]
        got = det_ops.conv_nhwc(x, rows, bias, 3, s, act, out=out)
        assert got.data_ptr() == out.data_ptr() == obuf.data_ptr() + 2 * (Ho * Wo * op + c0)
        whole = obuf.cpu().numpy()
        inside = whole[1:B + 1, :, :, c0:c0 + cout]
        if act is None:
            check_exact(inside, c.pre, "view, no activation")
        else:
            check_silu(inside, c, "view, SiLU")
        kept = whole == PATTERN
        kept[1:B + 1, :, :, c0:c0 + cout] = True
        assert bool(kept.all()), f"{int((~kept).sum())} elements outside the output view were overwritten, first at {np.argwhere(~kept)[0]}"


@pytest.mark.parametrize("tile", TILES, ids=[f"tile{t[0]}x{t[1]}" for t in TILES])
@pytest.mark.parametrize("cin,s", [(64, 1), (72, 2)])
def test_conv_repeats_bit_for_bit(gpu_device, tile, cin, s):
    from vlfm_amd.vlm import det_ops

    B, Ho, Wo, cout = R.TILE_WITNESS[tile]
    c = R.case(B, cin, cout, 3, s, Ho, Wo)
    x, rows, bias = operands(c, gpu_device)
    outs = [det_ops.conv_nhwc(x, rows, bias, 3, s, "silu") for _ in range(10)]
    assert len({o.data_ptr() for o in outs}) == 10
    check_silu(nhwc_bits(outs[0]), c, "first launch")
    first = outs[0].view(torch.int16)
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(o.view(torch.int16), first), f"launch {i} differs from launch 0"


def test_conv_argument_contract(gpu_device):
    """Calls outside the contract return VLFM_ERR_INVALID before any launch and leave the output untouched; batch 0 is a no-op."""
    from vlfm_amd import _lib

    L = _lib.lib()
    x = torch.zeros(2 * 4 * 4 * 64, dtype=torch.float16, device=gpu_device)
    w = torch.zeros(64 * 25 * 64, dtype=torch.float16, device=gpu_device)
    bias = torch.zeros(64, dtype=torch.float16, device=gpu_device)
    zero = torch.zeros(64, dtype=torch.float16, device=gpu_device)
    out = torch.full((2 * 4 * 4 * 64,), PATTERN, dtype=torch.int16, device=gpu_device)
    good = dict(batch=2, height=4, width=4, cin=64, cout=64, ksize=3, stride=1, x_pix=64, out_pix=64, act=1, zero=zero.data_ptr())

    def call(**changed):
        a = dict(good, **changed)
        return L.vlfm_conv_nhwc_f16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), a["zero"], a["batch"], a["height"],
                                    a["width"], a["cin"], a["cout"], a["ksize"], a["stride"], a["x_pix"], a["out_pix"], a["act"],
                                    None)

    refused = {
        "cout % 8 != 0": dict(cout=60),
        "x_pix_stride < cin": dict(x_pix=56),
        "out_pix_stride % 8 != 0": dict(out_pix=68),
        "stride 3": dict(stride=3),
        "ksize 5": dict(ksize=5),
        "act 2": dict(act=2),
        "null zero page": dict(zero=None),
        "2^41 input elements": dict(batch=4096, height=1024, width=1024, cin=512, x_pix=512),
        "exactly 2^31 input elements": dict(batch=4, height=1024, width=1024, cin=512, x_pix=512),
    }
    for what, changed in refused.items():
        assert call(**changed) == _lib.VLFM_ERR_INVALID, what
        assert _lib.last_error().startswith("conv_nhwc_f16"), what
    assert call(batch=0) == _lib.VLFM_OK
    torch.cuda.synchronize(gpu_device)
    assert bool((out == PATTERN).all())
    assert call() == _lib.VLFM_OK          # ... and the call they were all derived from is a valid one
    torch.cuda.synchronize(gpu_device)
    assert bool((out.view(torch.float16) == 0).all())
