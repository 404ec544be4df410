"""csrc/sam_ops.hip -- the NHWC-rows kernels of TinyViT's windowed-attention blocks (MobileSAM's image encoder behind
vlfm/vlm/sam.py:54; TinyViTBlock of mobile_sam/modeling/tiny_vit_sam.py [ext]) against the framework formulation the block used
before (which tests/test_sam_cpu.py pins to the oracle), in f32: |err| <= 2e-5 * max(1, |ref|) per kernel (different summation
orders of a 128-320-term mean / variance and of the 9 filter taps), and the whole encoder on the rows path against the NCHW path
and against the CPU (<= 2e-3 relative to the output's magnitude, the bound the other detector networks use).  The second half
holds the same kernels -- with Swin's shift / pad_zero forms -- to the f64 references of tests/detect_ref.py at the same bound, and
asserts what they refuse."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def close(a, b, tol=2e-5):
    return bool(((a - b).abs() <= tol * b.abs().clamp(min=1.0)).all())


@pytest.mark.parametrize("B,H,W,C,ws", [(2, 64, 64, 160, 14), (1, 128, 128, 128, 7), (2, 64, 64, 320, 7), (1, 9, 13, 8, 4),
                                        (1, 14, 14, 516, 7)])
def test_layernorm_rows_and_window_partition(gpu_device, B, H, W, C, ws):
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(C + ws)
    x = (torch.randn(B, H, W, C, generator=g) * 1.7 + 0.3).to(gpu_device)
    gamma, beta = torch.randn(C, generator=g).to(gpu_device), torch.randn(C, generator=g).to(gpu_device)
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    assert close(ops.layernorm_rows(x, gamma, beta, 1e-5), ref)
    # pad -> partition -> norm, exactly as the block spells it (the padding is normalised too: LayerNorm(0) = beta)
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    t = F.pad(x, (0, 0, 0, pw, 0, ph))
    hp, wp = H + ph, W + pw
    t = t.view(B, hp // ws, ws, wp // ws, ws, C).transpose(2, 3).reshape(-1, ws * ws, C)
    got = ops.layernorm_rows(x, gamma, beta, 1e-5, ws)
    assert got.shape == t.shape and close(got, F.layer_norm(t, (C,), gamma, beta, 1e-5))


@pytest.mark.parametrize("B,H,W,C,ws", [(2, 64, 64, 160, 14), (1, 128, 128, 128, 7), (1, 9, 13, 8, 4)])
def test_window_reverse_add(gpu_device, B, H, W, C, ws):
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(C * 3 + ws)
    x = torch.randn(B, H, W, C, generator=g).to(gpu_device)
    hp, wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
    a = torch.randn(B * (hp // ws) * (wp // ws), ws * ws, C, generator=g).to(gpu_device)
    ref = x + a.view(B, hp // ws, wp // ws, ws, ws, C).transpose(2, 3).reshape(B, hp, wp, C)[:, :H, :W]
    got = ops.window_reverse_add_(x.clone(), a, ws)
    assert torch.equal(got, ref)                 # one f32 addition per element: bit-identical


@pytest.mark.parametrize("B,H,W,C", [(2, 64, 64, 160), (1, 128, 128, 128), (2, 5, 7, 12), (1, 1, 1, 4)])
def test_depthwise_conv_on_nhwc_rows(gpu_device, B, H, W, C):
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, H, W, C, generator=g).to(gpu_device)
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).to(gpu_device)
    b = torch.randn(C, generator=g).to(gpu_device)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1, groups=C).permute(0, 2, 3, 1)
    got = ops.depthwise_conv3x3_nhwc(x, w.reshape(C, 9).t().contiguous(), b)
    assert close(got, ref)
    assert close(ops.depthwise_conv3x3_nhwc(x, w.reshape(C, 9).t().contiguous(), None), ref - b)


def test_tinyvit_encoder_rows_path_matches_the_nchw_path_and_the_cpu(gpu_device):
    from vlfm_amd.vlm import det_ops
    from vlfm_amd.vlm.sam import TinyViT, _TinyViTBlock

    torch.manual_seed(5)
    enc = TinyViT().eval()
    with torch.no_grad():
        for m in enc.modules():          # non-trivial BatchNorm statistics and attention biases, so that folding and the bias matter
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
        for m in enc.modules():
            if hasattr(m, "attention_biases"):
                m.attention_biases.normal_(0, 0.5)
    x = torch.randn(1, 3, 512, 512)      # 1/2 of SAM's side: 32 x 32 maps in the last stages (padded to 35 / 42 by the windows)
    with torch.no_grad():
        cpu = enc(x)[0]
    enc.to(gpu_device)
    det_ops.fold_batchnorm_(enc)
    xg = x.to(gpu_device)
    blocks = [m for m in enc.modules() if isinstance(m, _TinyViTBlock)]
    assert len(blocks) == 10
    with torch.inference_mode():
        assert all(b.rows_path(xg.new_zeros(1, 8, 8, b.local_conv.c.in_channels)) for b in blocks)
        rows = enc(xg)[0].float().cpu()
        for b in blocks:                 # force the NCHW formulation
            b.rows_path = lambda t: False
        nchw = enc(xg)[0].float().cpu()
    scale = float(cpu.abs().max())
    assert scale > 0.1
    assert float((rows - nchw).abs().max()) <= 2e-4 * scale
    assert float((rows - cpu).abs().max()) <= 2e-3 * scale


@pytest.mark.parametrize("nw,n,heads", [(37, 49, 4), (11, 196, 5), (5, 49, 10), (3, 1, 2), (2, 256, 1), (4, 70, 3)])
def test_window_attention(gpu_device, nw, n, heads):
    """vlfm_window_attention_f32 against the library's scaled_dot_product_attention with the additive bias as attn_mask (what the
    block called before), f32: |err| <= 2e-5 * max(1, |ref|) (online softmax over chunks of four keys vs the library's tiling)."""
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(nw * 100 + n + heads)
    qkv = (torch.randn(nw, n, heads * 96, generator=g) * 1.3).to(gpu_device)
    bias = (torch.randn(heads, n, n, generator=g) * 2.0).to(gpu_device)          # NOT symmetric: the transposition matters
    q, k, v = qkv.view(nw, n, heads, 96).split(32, dim=3)
    ref = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=bias.unsqueeze(0))
    ref = ref.transpose(1, 2).reshape(nw, n, heads * 32)
    got = ops.window_attention(qkv, bias.transpose(1, 2).contiguous(), heads, 32 ** -0.5)
    assert got.shape == ref.shape and close(got, ref)


# ------------------------------------------------------------------------------------------------ against f64 (tests/detect_ref.py)
SENTINEL = -777.25
LN_CHANNELS = [4, 256, 260, 512, 516, 1024]      # both sides of the template switch (C / 4 <= 64, <= 128, else), and its limit
GEOMETRIES = [(2, 9, 13, 4), (1, 7, 7, 7), (2, 15, 20, 7), (1, 3, 5, 7)]      # the last: a window larger than the map


def rel_err(got, ref):
    return float(((got.double().cpu() - ref).abs() / ref.abs().clamp(min=1.0)).max())


@pytest.mark.parametrize("B,H,W,ws", GEOMETRIES)
@pytest.mark.parametrize("C", LN_CHANNELS)
def test_layernorm_rows_shifted_against_f64(gpu_device, B, H, W, C, ws):
    """vlfm_layernorm_rows_shifted_f32 at every shift and both paddings against LayerNorm -> pad -> roll -> partition in f64, on rows
    with a large common offset (mean 50, deviation 1: a one-pass variance E[x^2] - E[x]^2 loses every digit there);
    |err| <= 2e-5 * max(1, |ref|); padded positions hold beta (or 0) exactly."""
    import detect_ref as R
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(C * 31 + H)
    x = torch.randn(B, H, W, C, generator=g) + 50.0
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xg, gg, bg = x.to(gpu_device), gamma.to(gpu_device), beta.to(gpu_device)
    ref = R.layernorm_windows_f64(x, gamma, beta, 1e-5, 0, 0, False)
    worst = rel_err(ops.layernorm_rows(xg, gg, bg, 1e-5), ref)
    lib = rel_err(F.layer_norm(xg, (C,), gg, bg, 1e-5), ref)
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    real = F.pad(torch.ones(B, H, W, 1), (0, 0, 0, pw, 0, ph))
    for shift in range(ws):
        live = torch.roll(real, shifts=(-shift, -shift), dims=(1, 2))
        live = live.view(B, (H + ph) // ws, ws, (W + pw) // ws, ws, 1).transpose(2, 3).reshape(-1, ws * ws) > 0
        assert int(live.sum()) == B * H * W
        for pad_zero in (False, True):
            ref = R.layernorm_windows_f64(x, gamma, beta, 1e-5, ws, shift, pad_zero)
            got = ops.layernorm_rows(xg, gg, bg, 1e-5, ws, shift, pad_zero).cpu()
            assert got.shape == ref.shape
            assert torch.equal(got[~live], (torch.zeros(C) if pad_zero else beta).expand(int((~live).sum()), C)), (shift, pad_zero)
            worst = max(worst, rel_err(got, ref))
    print(f"layernorm rows B={B} H={H} W={W} C={C} window={ws}: err={worst:.3e} library f32={lib:.3e} bound=2e-05")
    assert worst <= 2e-5, worst


@pytest.mark.parametrize("B,H,W,ws", GEOMETRIES)
@pytest.mark.parametrize("C", [4, 260])
def test_window_reverse_add_shifted(gpu_device, B, H, W, C, ws):
    """vlfm_window_reverse_add_shifted_f32 at every shift: merge the windows, roll back by +shift, crop, add -- one f32 addition per
    element, so bit-identical to the torch spelling; the window operand has a sentinel tail that must not be read."""
    import detect_ref as R
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(C * 3 + ws + H)
    hp, wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
    nwin = B * (hp // ws) * (wp // ws)
    x = torch.randn(B, H, W, C, generator=g)
    buf = torch.full((nwin + 1, ws * ws, C), SENTINEL)
    buf[:nwin] = torch.randn(nwin, ws * ws, C, generator=g)
    bufg = buf.to(gpu_device)
    for shift in range(ws):
        a = buf[:nwin].view(B, hp // ws, wp // ws, ws, ws, C).transpose(2, 3).reshape(B, hp, wp, C)
        want = x + torch.roll(a, shifts=(shift, shift), dims=(1, 2))[:, :H, :W]
        got = ops.window_reverse_add_(x.to(gpu_device), bufg[:nwin], ws, shift).cpu()
        assert torch.equal(got, want), shift
        assert torch.equal(got, R.window_reverse_f64(x, buf[:nwin], ws, shift).float()), shift
    assert torch.equal(bufg.cpu(), buf)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 1, 6, 8), (2, 6, 1, 8), (1, 2, 2, 1024)])
def test_depthwise_conv_on_nhwc_rows_against_f64(gpu_device, B, H, W, C):
    """vlfm_dwconv3x3_nhwc_f32 on maps where almost every tap is padding (one row, one column, one pixel) against nine shifted
    products in f64, with and without the bias: |err| <= 2e-5 * max(1, |ref|)."""
    import detect_ref as R
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(C + H * 7 + W)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    b = torch.randn(C, generator=g)
    w9c = w.reshape(C, 9).t().contiguous().to(gpu_device)
    for bias in (b, None):
        ref = R.dwconv3x3_nhwc_f64(x, w, bias)
        got = ops.depthwise_conv3x3_nhwc(x.to(gpu_device), w9c, bias.to(gpu_device) if bias is not None else None)
        lib = F.conv2d(x.to(gpu_device).permute(0, 3, 1, 2), w.to(gpu_device), bias.to(gpu_device) if bias is not None else None,
                       padding=1, groups=C).permute(0, 2, 3, 1)
        err = rel_err(got, ref)
        print(f"dwconv3x3 nhwc B={B} H={H} W={W} C={C} bias={bias is not None}: err={err:.3e} library f32={rel_err(lib, ref):.3e} "
              f"bound=2e-05")
        assert err <= 2e-5, err


def test_rows_kernels_refuse_what_they_cannot_do(gpu_device):
    """channels not a multiple of 4, channels > 1024 (LayerNorm), shift == window, a shift without a window: VLFM_ERR_INVALID, and
    nothing is written."""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    L = _lib.lib()
    x = torch.randn(1, 4, 4, 1028).to(gpu_device)
    gamma, beta = torch.ones(1028, device=gpu_device), torch.zeros(1028, device=gpu_device)
    out = torch.full((4 * 4 * 4 * 1028,), SENTINEL, device=gpu_device)
    p = [t.data_ptr() for t in (x, gamma, beta, out)]

    def layernorm(C, window, shift):
        return L.vlfm_layernorm_rows_shifted_f32(*p, 1, 4, 4, C, window, 1e-5, shift, 0, ops._stream())

    assert layernorm(6, 0, 0) == _lib.VLFM_ERR_INVALID                             # C % 4 != 0
    assert layernorm(1028, 0, 0) == _lib.VLFM_ERR_INVALID                          # C > 1024
    assert layernorm(8, 4, 4) == _lib.VLFM_ERR_INVALID                             # shift == window
    assert layernorm(8, 0, 1) == _lib.VLFM_ERR_INVALID                             # a shift without a window
    assert L.vlfm_window_reverse_add_shifted_f32(out.data_ptr(), x.data_ptr(), 1, 4, 4, 6, 4, 0, ops._stream()) == _lib.VLFM_ERR_INVALID
    assert L.vlfm_window_reverse_add_shifted_f32(out.data_ptr(), x.data_ptr(), 1, 4, 4, 8, 4, 4, ops._stream()) == _lib.VLFM_ERR_INVALID
    assert L.vlfm_dwconv3x3_nhwc_f32(x.data_ptr(), gamma.data_ptr(), None, out.data_ptr(), 1, 4, 4, 6, ops._stream()) == _lib.VLFM_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert layernorm(8, 4, 3) == _lib.VLFM_OK                                      # the same call with a legal shift goes through


@pytest.mark.parametrize("width,stride", [(30, 1), (12, 2), (4100, 1), (8, 3)])
def test_depthwise_conv_nchw_refusals(gpu_device, width, stride):
    """vlfm_dwconv3x3_f32 (csrc/detect_ops.hip) handles four outputs per thread: a width or an output width that is no multiple of 4
    (30; 12 at stride 2 -> 6), more than 1024 outputs per row (4100) and a stride other than 1 or 2 are refused, nothing written."""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    x = torch.randn(1, 2, 3, width).to(gpu_device)
    w = torch.randn(2, 1, 3, 3).to(gpu_device)
    y = torch.full((1, 2, 3, width), SENTINEL, device=gpu_device)
    rc = _lib.lib().vlfm_dwconv3x3_f32(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), 1, 2, 3, width, stride, 0, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.VLFM_ERR_INVALID and bool((y == SENTINEL).all())
