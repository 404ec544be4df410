"""-m gpu: the two multi-scale deformable attention kernels of csrc/detect_ops.hip (GroundingDINO's encoder and decoder) against the
f64 four-tap reference of tests/detect_ref.py (which tests/test_detect_ref_cpu.py pins to transformers' module): sampling points
outside their level (zero padding), exactly on pixel centres, pixel edges, 0 and 1, levels of 1 x 1 and 1 x W, query counts that do
not fill a workgroup, other L and P than the shipped 4 x 4, large and equal logits."""
import pytest
import torch
import torch.nn.functional as F

import detect_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SMALL_LEVELS = [(5, 7), (3, 4), (1, 3), (1, 1)]
SHIPPED_LEVELS = [(60, 80), (30, 40), (15, 20), (8, 10)]


def _hf(value, shapes, start, loc, w):
    """transformers' own grid_sample formulation, f32, on the device of its inputs."""
    from transformers.models.grounding_dino.modeling_grounding_dino import MultiScaleDeformableAttention

    return MultiScaleDeformableAttention()(value, torch.tensor(shapes, device=value.device), shapes, start, loc, w, 64)


def _plain_case(dev, name, shapes, B, Q, heads, D, P, seed, exact=False, lo=-0.3, hi=1.3):
    from vlfm_amd.vlm import det_ops

    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    start, S = R.level_starts(shapes)
    value = torch.randn(B, S, heads, D, generator=g)
    loc = torch.rand(B, Q, heads, L, P, 2, generator=g) * (hi - lo) + lo
    if exact:
        for l, (hl, wl) in enumerate(shapes):
            for q, (cx, cy) in enumerate(zip(R.exact_coordinates(wl), R.exact_coordinates(hl))):
                loc[:, q, :, l, 0, 0], loc[:, q, :, l, 0, 1] = cx, cy
    w = torch.softmax(torch.randn(B, Q, heads, L * P, generator=g), -1).view(B, Q, heads, L, P)
    ref, _ = R.ms_deform_attn_f64(value, shapes, start, loc, w)
    vg, sg, lg, wg = value.to(dev), start.to(dev), loc.to(dev), w.to(dev)
    got = det_ops.ms_deform_attn(vg, shapes, sg, lg, wg).cpu()
    lib = _hf(vg, shapes, sg, lg, wg).cpu()
    err, err_lib = float((got.double() - ref).abs().max()), float((lib.double() - ref).abs().max())
    print(f"ms_deform_attn {name}: err={err:.3e} library f32={err_lib:.3e} bound=1e-5 (atol = rtol) max|ref|={float(ref.abs().max()):.2f}")
    assert got.shape == (B, Q, heads * D)
    assert torch.allclose(got, ref.float(), atol=1e-5, rtol=1e-5), err
    return value, start, loc, w


def test_plain_kernel_small_levels_outside_and_exact_coordinates(gpu_device):
    """(a) levels 5 x 7, 3 x 4, 1 x 3, 1 x 1, locations in [-0.3, 1.3] (about a third of the taps outside) and, in the first eight
    queries, one point per level exactly on 0, 1, the outermost pixel centres, the first pixel edges, half a pixel outside."""
    _plain_case(gpu_device, "(a) small levels", SMALL_LEVELS, 2, 37, 8, 32, 3, seed=1, exact=True)


def test_plain_kernel_less_than_one_workgroup(gpu_device):
    """(b) 60 outputs (heads 3, D = 20, one level, one point, one query): D neither 32 nor a multiple of 8."""
    _plain_case(gpu_device, "(b) one query", [(3, 4)], 1, 1, 3, 20, 1, seed=2)


def test_plain_kernel_shipped_geometry(gpu_device):
    """(c) the detector's four levels at batch 1."""
    _plain_case(gpu_device, "(c) shipped levels", SHIPPED_LEVELS, 1, 50, 8, 32, 4, seed=3, lo=-0.15, hi=1.15)


def test_plain_kernel_exact_zeros(gpu_device):
    """(d) all weights 0 -> exactly 0; every point outside every level (5.0, -5.0) -> exactly 0."""
    from vlfm_amd.vlm import det_ops

    value, start, loc, w = _plain_case(gpu_device, "(d) base", SMALL_LEVELS, 2, 5, 8, 32, 3, seed=4)
    args = (value.to(gpu_device), SMALL_LEVELS, start.to(gpu_device))
    assert bool((det_ops.ms_deform_attn(*args, loc.to(gpu_device), torch.zeros_like(w).to(gpu_device)) == 0).all())
    for far in (5.0, -5.0):
        assert bool((det_ops.ms_deform_attn(*args, torch.full_like(loc, far).to(gpu_device), w.to(gpu_device)) == 0).all())


# ------------------------------------------------------------------------------------------------ the fused kernel
HEADS, D = 8, 32
FUSED_LEVELS = {4: [(20, 27), (5, 7), (1, 3), (1, 1)], 2: [(9, 12), (1, 5)]}


def _fused_inputs(coords, L, P, B, Q, seed, logit_scale=1.0, equal_head=None):
    """Offsets drawn backwards from target locations uniform in [-0.3, 1.3]; in the first queries one point per level lands exactly
    on the coordinates of detect_ref.exact_coordinates (reference = target - offset / W with an exact offset)."""
    g = torch.Generator().manual_seed(seed)
    shapes = FUSED_LEVELS[L]
    start, S = R.level_starts(shapes)
    value = torch.randn(B, S, HEADS, D, generator=g)
    target = torch.rand(B, Q, HEADS, L, P, 2, generator=g, dtype=torch.float64) * 1.6 - 0.3
    ref = torch.rand(B, Q, L, coords, generator=g, dtype=torch.float64)
    if coords == 4:
        ref[..., 2:] = ref[..., 2:] * 0.5 + 0.1
    exact = []
    for l, (hl, wl) in enumerate(shapes):
        for q, (cx, cy) in enumerate(list(zip(R.exact_coordinates(wl), R.exact_coordinates(hl)))[:Q]):
            if coords == 2:     # offset (2, -1) pixels
                ref[:, q, l, 0], ref[:, q, l, 1] = float(torch.tensor(cx).float()) - 2.0 / wl, float(torch.tensor(cy).float()) + 1.0 / hl
            else:               # box 0.5 x 0.5, offset (2 P, -P): location = reference + (0.5, -0.25)
                ref[:, q, l] = torch.tensor([float(torch.tensor(cx).float()) - 0.5, float(torch.tensor(cy).float()) + 0.25, 0.5, 0.5])
            exact.append((q, l))
    ref = ref.float()
    r = ref.double()[:, :, None, :, None, :]
    if coords == 2:
        norm = torch.tensor([[float(wl), float(hl)] for hl, wl in shapes], dtype=torch.float64)[None, None, None, :, None, :]
        off = (target - r) * norm
    else:
        off = (target - r[..., :2]) * P * 2.0 / r[..., 2:]
    for q, l in exact:
        off[:, q, :, l, 0, 0], off[:, q, :, l, 0, 1] = (2.0, -1.0) if coords == 2 else (2.0 * P, -1.0 * P)
    logits = torch.randn(B, Q, HEADS, L * P, generator=g) * logit_scale
    if equal_head is not None:
        logits[:, :, equal_head] = 0.7
    ol = torch.cat([off.float().reshape(B, Q, -1), logits.reshape(B, Q, -1)], -1).contiguous()
    return shapes, start, S, value, ol, ref


def _outside_share(shapes, loc):
    """The share of the four taps of every sampling point that fall outside their level (f64 on the host)."""
    out = total = 0
    for l, (hl, wl) in enumerate(shapes):
        x0, y0 = torch.floor(loc[:, :, :, l, :, 0] * wl - 0.5), torch.floor(loc[:, :, :, l, :, 1] * hl - 0.5)
        for dy in (0, 1):
            for dx in (0, 1):
                inside = (x0 + dx >= 0) & (x0 + dx < wl) & (y0 + dy >= 0) & (y0 + dy < hl)
                out += int((~inside).sum())
                total += inside.numel()
    return out / total


def _fused_launch(dev, value, shapes, start, ol, ref, L, P, heads=HEADS, head_dim=D, coords=None):
    """The C entry point on an output over-allocated by one query row of SENTINEL.  Returns (status, buffer [B * Q + 1, 256])."""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import det_ops

    B, S = value.shape[:2]
    Q = ol.shape[1]
    sh = torch.tensor(shapes, dtype=torch.int32, device=dev)
    st = start.to(torch.int32).to(dev)
    vg, og, rg = value.to(dev), ol.to(dev), ref.to(dev)
    out = torch.full((B * Q + 1, HEADS * D), SENTINEL, dtype=torch.float32, device=dev)
    rc = _lib.lib().vlfm_ms_deform_attn_fused(vg.data_ptr(), sh.data_ptr(), st.data_ptr(), og.data_ptr(), rg.data_ptr(), B, Q, heads,
                                              head_dim, L, P, ref.shape[-1] if coords is None else coords, S, out.data_ptr(),
                                              det_ops._stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


def _fused_case(dev, coords, L, P, B, Q, seed, **kw):
    from vlfm_amd import _lib
    from vlfm_amd.vlm import det_ops

    shapes, start, S, value, ol, ref = _fused_inputs(coords, L, P, B, Q, seed, **kw)
    loc64, w64 = R.deform_locations_f64(ol, ref, shapes, HEADS, L, P)
    share = _outside_share(shapes, loc64)
    assert share >= 0.2, share
    want, _ = R.ms_deform_attn_fused_f64(value, shapes, start, ol, ref, L, P)
    # the module's own arithmetic in f32 on the device: softmax, the location formula, the grid_sample formulation
    vg, og, rg, sg = value.to(dev), ol.to(dev), ref.to(dev), start.to(dev)
    off = og[..., :HEADS * L * P * 2].view(B, Q, HEADS, L, P, 2)
    wts = F.softmax(og[..., HEADS * L * P * 2:].view(B, Q, HEADS, L * P), -1).view(B, Q, HEADS, L, P)
    spatial = torch.tensor(shapes, device=dev)
    if coords == 2:
        normalizer = torch.stack([spatial[..., 1], spatial[..., 0]], -1)
        loc = rg[:, :, None, :, None, :] + off / normalizer[None, None, None, :, None, :]
    else:
        loc = rg[:, :, None, :, None, :2] + off / P * rg[:, :, None, :, None, 2:] * 0.5
    lib = _hf(vg, shapes, sg, loc, wts).cpu()
    err_lib = float((lib.double() - want).abs().max())
    top = float(want.abs().max())
    bound = max(4.0 * err_lib, 1e-6 * top)
    rc, buf = _fused_launch(dev, value, shapes, start, ol, ref, L, P)
    assert rc == _lib.VLFM_OK
    got = buf[:B * Q].view(B, Q, HEADS * D)
    assert bool((buf[B * Q:] == SENTINEL).all())                                     # the row beyond the last query stays untouched
    assert torch.equal(det_ops.ms_deform_attn_fused(vg, shapes, sg, og, rg, L, P).cpu(), got)
    err = float((got.double() - want).abs().max())
    print(f"ms_deform_attn_fused coords={coords} L={L} P={P} B*Q={B * Q} {kw or ''}: err={err:.3e} library f32={err_lib:.3e} "
          f"bound={bound:.3e} max|ref|={top:.2f} outside={share:.2f}")
    assert not bool(torch.isnan(got).any())
    assert err <= bound, (err, err_lib, bound)
    # the plain kernel on the f64 locations and weights rounded to f32
    plain = det_ops.ms_deform_attn(vg, shapes, sg, loc64.float().to(dev), w64.float().to(dev)).cpu()
    assert torch.allclose(got, plain, atol=1e-5, rtol=1e-5), float((got - plain).abs().max())
    return w64


@pytest.mark.parametrize("B,Q", [(1, 1), (1, 5), (2, 101)])
@pytest.mark.parametrize("L,P", [(4, 4), (2, 3)])
@pytest.mark.parametrize("coords", [2, 4])
def test_fused_kernel_against_f64(gpu_device, coords, L, P, B, Q):
    """ms_deform_attn_fused_kernel against softmax -> locations -> four-tap gather in f64; B * Q = 1, 5, 202 (a workgroup holds four
    queries); at least a fifth of the taps outside.  The kernel forms its sampling coordinate in f32, so the bound is measured, not
    fixed: 4 x the error of the module's own f32 arithmetic (F.softmax, the location formula, transformers' unpatched
    MultiScaleDeformableAttention) on the same inputs on the GPU, floor 1e-6 * max|ref|.

    Measured on an MI355X, max |library f32 - f64| (the kernel's own error in brackets), B * Q = 1 / 5 / 202:
      points, L = 4, P = 4:  1.7e-7 / 7.9e-7 / 1.7e-6   (1.5e-7 / 6.7e-7 / 1.7e-6)     at max|ref| 0.4 / 1.0 / 1.6
      points, L = 2, P = 3:  4.3e-7 / 1.5e-6 / 2.2e-6   (4.3e-7 / 1.7e-6 / 2.3e-6)     at max|ref| 1.0 / 1.8 / 1.7
      boxes,  L = 4, P = 4:  1.5e-7 / 5.9e-7 / 1.5e-6   (1.1e-7 / 5.9e-7 / 1.5e-6)     at max|ref| 0.7 / 0.8 / 1.6
      boxes,  L = 2, P = 3:  2.2e-7 / 1.8e-6 / 1.7e-6   (1.4e-7 / 2.6e-6 / 1.4e-6)     at max|ref| 0.6 / 2.4 / 2.2
    logits x 30 (202 queries): points 7.1e-6 (7.7e-6), boxes 5.9e-6 (5.9e-6); equal logits (5 queries): 7.0e-7 (8.4e-7), 6.2e-7 (9.7e-7).
    Both are dominated by the f32 rounding of the sampling location (up to 27 pixels wide here), which is why they often coincide."""
    _fused_case(gpu_device, coords, L, P, B, Q, seed=coords * 100 + L * 10 + B * Q)


@pytest.mark.parametrize("coords", [2, 4])
def test_fused_kernel_large_logits(gpu_device, coords):
    """Logits of N(0, 30): the max-subtracted softmax neither overflows nor flattens (the weights are close to one-hot)."""
    w = _fused_case(gpu_device, coords, 4, 4, 2, 101, seed=7 + coords, logit_scale=30.0)
    assert float(w.max(-1).values.max(-1).values.median()) > 0.9


@pytest.mark.parametrize("coords", [2, 4])
def test_fused_kernel_equal_logits(gpu_device, coords):
    """All logits of head 2 equal: every weight of that head is 1 / (L * P)."""
    w = _fused_case(gpu_device, coords, 2, 3, 1, 5, seed=11 + coords, equal_head=2)
    assert torch.allclose(w[:, :, 2], torch.full_like(w[:, :, 2], 1.0 / 6.0), atol=1e-15)


def test_fused_kernel_refusals(gpu_device):
    """The fused kernel is written for 8 heads of width 32 and reference points with 2 or 4 coordinates; anything else is an error
    (the caller uses the plain kernel), never a quiet wrong answer."""
    from vlfm_amd import _lib

    shapes, start, S, value, ol, ref = _fused_inputs(2, 2, 3, 1, 5, seed=0)
    for kw in (dict(heads=4), dict(head_dim=64), dict(coords=3)):
        rc, buf = _fused_launch(gpu_device, value, shapes, start, ol, ref, 2, 3, **kw)
        assert rc == _lib.VLFM_ERR_INVALID and bool((buf == SENTINEL).all()), kw
