"""tests/detect_ref.py -- the f64 references the detector / segmenter kernel tests compare with -- pinned to the framework on the
CPU: attention to F.scaled_dot_product_attention in f64, the LayerNorm / window forms to F.layer_norm and transformers' Swin helpers,
the depthwise convolution to F.conv2d, the two deformable-attention references to transformers' MultiScaleDeformableAttention in f32
at atol = rtol = 1e-5 (the bar of test_ms_deform_attn_matches_hf_pytorch_path)."""
import pytest
import torch
import torch.nn.functional as F

import detect_ref as R

try:
    from transformers.models.swin.modeling_swin import window_partition, window_reverse
except Exception:   # the torch spelling of the same two helpers
    def window_partition(t, ws):
        b, h, w, c = t.shape
        return t.view(b, h // ws, ws, w // ws, ws, c).transpose(2, 3).contiguous().view(-1, ws, ws, c)

    def window_reverse(t, ws, h, w):
        c = t.shape[-1]
        return t.view(-1, h // ws, w // ws, ws, ws, c).transpose(2, 3).contiguous().view(-1, h, w, c)


@pytest.mark.parametrize("tokens,heads,masked", [(1, 1, False), (33, 3, True), (49, 2, True), (70, 1, False)])
def test_window_attention_reference(tokens, heads, masked):
    g = torch.Generator().manual_seed(tokens)
    nw, per_image = 6, 3
    qkv = torch.randn(nw, tokens, heads * 96, generator=g, dtype=torch.float64)
    bias = torch.randn(heads, tokens, tokens, generator=g, dtype=torch.float64) * 2
    mask = R.swin_like_mask(tokens, per_image, g).double() if masked else None
    got, scores = R.window_attention_f64(qkv, bias, mask, heads, 32 ** -0.5)
    q, k, v = (t.transpose(1, 2) for t in qkv.view(nw, tokens, heads, 96).split(32, dim=3))
    add = bias[None].expand(nw, -1, -1, -1)
    if masked:
        assert not torch.equal(mask, mask.transpose(1, 2)) and bool((mask.diagonal(dim1=1, dim2=2) == 0).all())
        add = add + mask.repeat(nw // per_image, 1, 1)[:, None]                  # window w uses mask[w mod per_image]
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=add, scale=32 ** -0.5).transpose(1, 2).reshape(nw, tokens, heads * 32)
    assert got.dtype == torch.float64 and torch.allclose(got, want, atol=1e-12, rtol=1e-12)
    assert scores.shape == (nw, heads, tokens, tokens)


@pytest.mark.parametrize("B,H,W,ws", [(2, 9, 13, 4), (1, 7, 7, 7), (1, 3, 5, 7)])
@pytest.mark.parametrize("pad_zero", [False, True])
def test_layernorm_windows_reference(B, H, W, ws, pad_zero):
    C = 12
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) + 50.0
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    assert torch.allclose(R.layernorm_windows_f64(x, gamma, beta, 1e-5, 0, 0, False), F.layer_norm(x, (C,), gamma, beta, 1e-5),
                          atol=1e-10, rtol=1e-10)
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    for shift in range(ws):
        if pad_zero:    # Swin: norm, pad with zeros, roll, partition
            t = F.pad(F.layer_norm(x, (C,), gamma, beta, 1e-5), (0, 0, 0, pw, 0, ph))
        else:           # TinyViT: pad with zeros, norm (LayerNorm(0) = beta), [roll,] partition
            t = F.layer_norm(F.pad(x, (0, 0, 0, pw, 0, ph)), (C,), gamma, beta, 1e-5)
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
        want = window_partition(t, ws).view(-1, ws * ws, C)
        got = R.layernorm_windows_f64(x, gamma, beta, 1e-5, ws, shift, pad_zero)
        assert got.shape == want.shape and torch.allclose(got, want, atol=1e-10, rtol=1e-10), shift


@pytest.mark.parametrize("B,H,W,ws", [(2, 9, 13, 4), (1, 7, 7, 7), (1, 3, 5, 7)])
def test_window_reverse_reference(B, H, W, ws):
    C = 8
    g = torch.Generator().manual_seed(H + W)
    hp, wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
    x = torch.randn(B, H, W, C, generator=g)
    a = torch.randn(B * (hp // ws) * (wp // ws), ws * ws, C, generator=g)
    for shift in range(ws):
        back = torch.roll(window_reverse(a.view(-1, ws, ws, C), ws, hp, wp), shifts=(shift, shift), dims=(1, 2))
        want = x + back[:, :H, :W]
        assert torch.equal(R.window_reverse_f64(x, a, ws, shift).float(), want), shift
        # the reverse of the partition is the identity on the real cells
        part = R.layernorm_windows_f64(x, torch.ones(C), torch.zeros(C), 1e-5, ws, shift, True)
        norm = F.layer_norm(x.double(), (C,), None, None, 1e-5)
        assert torch.allclose(R.window_reverse_f64(torch.zeros_like(x), part, ws, shift), norm, atol=1e-12)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 1, 6, 8), (2, 6, 1, 8), (1, 5, 7, 12)])
def test_dwconv3x3_nhwc_reference(B, H, W, C):
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    for bias in (b, None):
        want = F.conv2d(x.permute(0, 3, 1, 2), w, bias, padding=1, groups=C).permute(0, 2, 3, 1)
        assert torch.allclose(R.dwconv3x3_nhwc_f64(x, w, bias), want, atol=1e-12, rtol=1e-12)


SMALL_LEVELS = [(5, 7), (3, 4), (1, 3), (1, 1)]


def _hf_attn():
    from transformers.models.grounding_dino.modeling_grounding_dino import MultiScaleDeformableAttention

    return MultiScaleDeformableAttention()


def test_ms_deform_attn_reference_against_the_hf_module():
    g = torch.Generator().manual_seed(1)
    shapes = SMALL_LEVELS
    start, S = R.level_starts(shapes)
    B, Q, heads, D, L, P = 2, 37, 8, 32, 4, 3
    value = torch.randn(B, S, heads, D, generator=g)
    loc = torch.rand(B, Q, heads, L, P, 2, generator=g) * 1.6 - 0.3
    for l, (hl, wl) in enumerate(shapes):
        for q, (cx, cy) in enumerate(zip(R.exact_coordinates(wl), R.exact_coordinates(hl))):
            loc[:, q, :, l, 0, 0], loc[:, q, :, l, 0, 1] = cx, cy
    w = torch.softmax(torch.randn(B, Q, heads, L * P, generator=g), -1).view(B, Q, heads, L, P)
    want = _hf_attn()(value, torch.tensor(shapes), shapes, start, loc, w, 64)
    got, mag = R.ms_deform_attn_f64(value, shapes, start, loc, w)
    assert got.dtype == torch.float64 and got.shape == want.shape == mag.shape
    assert bool((mag >= got.abs() - 1e-12).all())
    err = float((got - want.double()).abs().max())
    print(f"ms_deform_attn_f64 vs the HF module in f32: max err {err:.2e} at max|ref| {float(got.abs().max()):.2f}")
    assert torch.allclose(got.float(), want, atol=1e-5, rtol=1e-5), err
    # every point outside every level: exactly 0
    far, _ = R.ms_deform_attn_f64(value, shapes, start, torch.full_like(loc, 5.0), w)
    assert bool((far == 0).all())


@pytest.mark.parametrize("coords", [2, 4])
@pytest.mark.parametrize("L,P", [(4, 4), (2, 3)])
def test_ms_deform_attn_fused_reference_against_the_hf_arithmetic(coords, L, P):
    """The fused reference against the module's own spelling: F.softmax over a head's L * P logits, the sampling-location formula of
    GroundingDinoMultiscaleDeformableAttention.forward [ext], then MultiScaleDeformableAttention, all in f32."""
    g = torch.Generator().manual_seed(coords * 10 + L)
    shapes = SMALL_LEVELS[:L]
    start, S = R.level_starts(shapes)
    B, Q, heads, D = 2, 11, 8, 32
    value = torch.randn(B, S, heads, D, generator=g)
    ol = torch.randn(B, Q, heads * L * P * 3, generator=g)
    ref = torch.rand(B, Q, L, coords, generator=g)
    offsets = ol[..., :heads * L * P * 2].view(B, Q, heads, L, P, 2)
    weights = F.softmax(ol[..., heads * L * P * 2:].view(B, Q, heads, L * P), -1).view(B, Q, heads, L, P)
    spatial = torch.tensor(shapes)
    if coords == 2:
        normalizer = torch.stack([spatial[..., 1], spatial[..., 0]], -1)
        loc = ref[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5
    want = _hf_attn()(value, spatial, shapes, start, loc, weights, 64)
    got, _ = R.ms_deform_attn_fused_f64(value, shapes, start, ol, ref, L, P)
    assert torch.allclose(got.float(), want, atol=1e-5, rtol=1e-5), float((got - want.double()).abs().max())
