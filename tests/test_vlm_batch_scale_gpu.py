"""-m gpu: the BLIP-2 HIP kernels at the batch the benchmark runs (256 images per cosine_batch call, eager), where their schedules differ
from the small batches of tests/test_vlm_gpu.py: the preprocess kernel's band height, LayerNorm's rows per wavefront (the prefetch rotation),
the attention kernel's items per persistent workgroup, the fc1 / fc2 GEMM's 24 rounds plus n-half leftovers.  Every kernel is compared with
a float64 reference of the same operation, evaluated on the GPU in chunks, at the bound the kernel's small-batch test uses.  Outputs go
into NaN-filled buffers with a guard row / image behind them: a kernel that skips its last rows, or writes one row too many, cannot pass
on the caching allocator's leftovers of an earlier correct run."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref

pytestmark = pytest.mark.gpu

_BITS = {torch.float16: torch.int16, torch.float32: torch.int32}


def _nan_f16(*shape, device):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=device)


def _is_nan_bits(t):
    """every element of an f16 / f32 tensor still holds torch.full's NaN, bit for bit"""
    fill = torch.tensor(float("nan"), dtype=t.dtype).view(_BITS[t.dtype]).item()
    return bool((t.contiguous().view(_BITS[t.dtype]) == fill).all())


def _cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ preprocess
def _fused_bands(n, height, out_size, vksize):
    """vlfm_preprocess_rgb_batched's band choice for the one-launch kernel (csrc/vlm_ops.hip), restated: (bands, rows per band)."""
    op = (out_size + 3) & ~3
    span = lambda r: ((r - 1) * height + out_size - 1) // out_size + vksize + 2  # noqa: E731
    lds_of = lambda r: 3 * 256 * 4 + 2 * 3 * (4096 + 128) + 3 * span(r) * op  # noqa: E731
    r = min(out_size, 32)
    while r > 1 and lds_of(r) > 80 * 1024:
        r -= 1
    while r > 8 and ((out_size + r - 1) // r) * n < 512:
        r = (r + 1) // 2
    bands = (out_size + r - 1) // r
    return bands, (out_size + bands - 1) // bands


def _preprocess_fused_into(img, out, dtype, patch):
    """ops.preprocess_rgb's launch, into a caller's buffer"""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    n, H, W, _ = img.shape
    hb, hk, hks = ops._device_coeffs(img.device, W, 224)
    vb, vk, vks = ops._device_coeffs(img.device, H, 224)
    tmp = torch.empty((n, H, 224, 3), dtype=torch.uint8, device=img.device)
    m = (ctypes.c_float * 3)(*ops.CLIP_MEAN)
    s = (ctypes.c_float * 3)(*ops.CLIP_STD)
    _lib.check(_lib.lib().vlfm_preprocess_rgb_batched(img.data_ptr(), n, H, W, 224, hb.data_ptr(), hk.data_ptr(), hks, vb.data_ptr(),
                                                     vk.data_ptr(), vks, ctypes.addressof(m), ctypes.addressof(s), tmp.data_ptr(),
                                                     out.data_ptr(), ops._DTYPE_CODE[dtype], patch, ops._stream()), "preprocess_rgb")


@pytest.mark.parametrize("n,dtype,bands", [(48, torch.float16, 14), (63, torch.float16, 14), (64, torch.float16, 8),
                                           (256, torch.float16, 8), (256, torch.float32, 8)])
def test_preprocess_at_batch_equals_two_launch_and_pil(gpu_device, n, dtype, bands, monkeypatch):
    """480 x 640 -> 224 patches of 14: 63 and 64 frames sit either side of the switch from 14 bands of 16 rows to 8 bands of 28
    (11 vertical taps); the one-launch kernel against the two-launch form (identical bits) and, on 8 frames spread over the batch,
    against PIL's BICUBIC (bit-exact, as test_preprocess_matches_pil_bit_exact)."""
    from PIL import Image

    from vlfm_amd.vlm import ops

    H, W = 480, 640
    vks = ops.resample_coeffs(H, 224)[2]
    assert vks == 11 and _fused_bands(n, H, 224, vks)[0] == bands
    if n in (63, 64):
        assert _fused_bands(127 - n, H, 224, vks)[0] != bands            # the other side of the switch
    g = torch.Generator(device=gpu_device).manual_seed(1000 + n)
    img = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8, device=gpu_device)
    out = torch.full((n + 1, 256, 588), float("nan"), dtype=dtype, device=gpu_device)
    _preprocess_fused_into(img, out[:n], dtype, 14)
    assert _is_nan_bits(out[n]), "the guard frame behind the last one was written"
    got = out[:n]
    assert bool(torch.isfinite(got).all())
    monkeypatch.setenv("VLFM_PREPROCESS_TWO_PASS", "1")
    want = ops.preprocess_rgb(img, 224, dtype, patch_size=14)
    monkeypatch.delenv("VLFM_PREPROCESS_TWO_PASS")
    assert torch.equal(got, want)
    mean = torch.tensor(ops.CLIP_MEAN).view(3, 1, 1)
    std = torch.tensor(ops.CLIP_STD).view(3, 1, 1)
    picks = sorted({0, n - 1, *np.linspace(0, n - 1, 8).round().astype(int).tolist()})
    host = img[picks].cpu().numpy()
    for j, i in enumerate(picks):
        pil = np.asarray(Image.fromarray(host[j]).resize((224, 224), Image.BICUBIC))
        ref = (torch.from_numpy(pil.copy()).permute(2, 0, 1).float().div(255) - mean) / std     # ToTensor + Normalize
        ref = ref.reshape(3, 16, 14, 16, 14).permute(1, 3, 0, 2, 4).reshape(256, 588).to(dtype)
        assert torch.equal(got[i].cpu(), ref), i


# ------------------------------------------------------------------------------------------------ LayerNorm(x + c)
def _ln_rows_per_wave(rows):
    """vlfm_layernorm_bias_f16's launcher (csrc/vlm_ops.hip: rpw = rows / 8192 clamped to [1, LN_ROWS = 8]), restated"""
    return min(max(rows // 8192, 1), 8)


@pytest.mark.parametrize("rows,dim,rpw", [(16448, 1408, 2), (32896, 1408, 4), (65792, 1408, 8), (24581, 1408, 3), (73729, 1408, 8),
                                          (65792, 2048, 8)])
def test_layernorm_bias_at_batch_vs_f64(gpu_device, rows, dim, rpw):
    """vlfm_layernorm_bias_f16 at 64-256 images of 257 tokens: 2, 4 and 8 rows per wavefront (the two-row prefetch rotation), a
    partial last wavefront (24 581 rows at 3 per wave, 73 729 at the cap of 8), and D = 2048.  Bound: 4e-3, as the small-batch test."""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    assert _ln_rows_per_wave(rows) == rpw
    g = torch.Generator(device=gpu_device).manual_seed(rows + dim)
    x = (torch.randn(rows, dim, generator=g, device=gpu_device) * 3).half()
    c = torch.randn(dim, generator=g, device=gpu_device)
    w = (1 + 0.2 * torch.randn(dim, generator=g, device=gpu_device)).half()
    b = (0.3 * torch.randn(dim, generator=g, device=gpu_device)).half()
    L = _lib.lib()
    for cb in (c, None):
        y = _nan_f16(rows + 1, dim, device=gpu_device)
        _lib.check(L.vlfm_layernorm_bias_f16(x.data_ptr(), cb.data_ptr() if cb is not None else None, w.data_ptr(), b.data_ptr(),
                                             y.data_ptr(), rows, dim, 1e-6, ops._stream()), "layernorm_bias_f16")
        assert _is_nan_bits(y[rows]), "the guard row behind the last row was written"
        got = y[:rows]
        assert bool(torch.isfinite(got).all()), int((~torch.isfinite(got)).any(1).nonzero()[0])
        err_max, rel_max = 0.0, 0.0
        for r0 in range(0, rows, 16384):
            xs = x[r0:r0 + 16384].double() + (cb.double() if cb is not None else 0.0)
            ref = torch.nn.functional.layer_norm(xs, (dim,), w.double(), b.double(), 1e-6)
            err = (got[r0:r0 + 16384].double() - ref).abs()
            err_max = max(err_max, float(err.max()))
            rel_max = max(rel_max, float((err / (2.0 ** -11 * ref.abs() + 1e-4)).max()))
        assert err_max <= 4e-3, (cb is not None, err_max, f"max |err| / (2^-11 |ref| + 1e-4) = {rel_max:.2f}")


# ------------------------------------------------------------------------------------------------ ViT attention
S, HEADS, DH = 257, 16, 88


def _qkv(B, device, seed):
    """the input of test_vit_attention_kernel_vs_fp32_reference, built on the GPU: [B*257, 3*16*88] f16 with peaked rows"""
    g = torch.Generator(device=device).manual_seed(seed)
    qkv = torch.randn(B, S, 3, HEADS, DH, generator=g, device=device) * 1.5
    qkv[0, :, 0, 0] *= 4.0                                # a head with peaked softmax rows
    qkv[B - 1, :, 0, 5] *= 3.0
    qkv[B - 1, 0, 0, 7] *= 5.0                            # a peaked CLS query (the VALU path)
    return qkv.half().reshape(B * S, 3 * HEADS * DH).contiguous()


def _attention_into(x, out, B):
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    _lib.check(_lib.lib().vlfm_vit_attention_f16(x.data_ptr(), out.data_ptr(), B, S, HEADS, DH, DH ** -0.5, ops._stream()),
               "vit_attention_f16")


def _items_per_workgroup(B):
    """vlfm_vit_attention_f16's persistent grid, restated: the fewest (image, head) items any workgroup walks"""
    cus = _cu_count() & ~7
    per = min(cus // 8, (B + 7) // 8 * HEADS)
    return min(((B - xcd + 7) // 8) * HEADS // per for xcd in range(8))


@pytest.mark.parametrize("B", [64, 128, 255, 256])
def test_vit_attention_at_batch_vs_f64(gpu_device, B):
    """vlfm_vit_attention_f16 with 4-16 items per persistent workgroup (both LDS buffer parities many times over; 255 images give
    XCDs of 32 and 31 images) against softmax(q k^T / sqrt(88)) v in float64.  Bound: 6e-3, as the small-batch test; a second run
    is bitwise equal."""
    x = _qkv(B, gpu_device, 70 + B)
    if B == 256:
        assert _items_per_workgroup(B) >= 16
    outs = []
    for _ in range(2):
        out = _nan_f16((B + 1) * S, HEADS * DH, device=gpu_device)
        _attention_into(x, out, B)
        assert _is_nan_bits(out[B * S:]), "the guard image behind the last one was written"
        outs.append(out[:B * S])
    got = outs[0]
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(torch.int16), outs[1].view(torch.int16))        # bitwise reproducible
    err_max, where = 0.0, None
    for b0 in range(0, B, 16):
        xb = x[b0 * S:(b0 + 16) * S].view(-1, S, 3, HEADS, DH).double()
        q, k, v = [xb[:, :, i].permute(0, 2, 1, 3) for i in range(3)]         # [b, H, S, D]
        ref = torch.softmax(q @ k.transpose(-1, -2) * DH ** -0.5, dim=-1) @ v
        ref = ref.permute(0, 2, 1, 3).reshape(-1, HEADS * DH)
        err = (got[b0 * S:(b0 + 16) * S].double() - ref).abs()
        if float(err.max()) > err_max:
            err_max, where = float(err.max()), divmod(b0 * S * HEADS * DH + int(err.argmax()), S * HEADS * DH)   # (image, element)
    assert err_max <= 6e-3, (err_max, where)


def test_vit_attention_item_result_is_independent_of_the_schedule(gpu_device):
    """Images 0..39 of a 256-image call (16 items per workgroup) run as their own 40-image call (3 per workgroup, other workgroups,
    other LDS buffer parities): identical bits.  An item's maths must not depend on where or in which buffer it runs."""
    x = _qkv(256, gpu_device, 326)
    big = _nan_f16(256 * S, HEADS * DH, device=gpu_device)
    _attention_into(x, big, 256)
    small = _nan_f16(41 * S, HEADS * DH, device=gpu_device)
    _attention_into(x[:40 * S].contiguous(), small, 40)
    assert _is_nan_bits(small[40 * S:])
    assert bool(torch.isfinite(big).all())
    diff = (big[:40 * S].view(torch.int16) != small[:40 * S].view(torch.int16))
    assert not bool(diff.any()), int(diff.nonzero()[0, 0])


# ------------------------------------------------------------------------------------------------ fc1 / fc2 GEMM
def _check_gemm(got, x, w, b, r0, gelu):
    """|got - ref| <= 2e-3 * max(1, max|ref|) with ref = [gelu](x . w^T + b) [+ r0] in float64, 8192 rows at a time"""
    wd = w.double().t()
    err_max, ref_max = 0.0, 0.0
    for m0 in range(0, x.shape[0], 8192):
        ref = x[m0:m0 + 8192].double() @ wd
        if b is not None:
            ref += b.double()
        if gelu:
            ref = torch.nn.functional.gelu(ref)
        if r0 is not None:
            ref += r0[m0:m0 + 8192].double()
        err_max = max(err_max, float((got[m0:m0 + 8192].double() - ref).abs().max()))
        ref_max = max(ref_max, float(ref.abs().max()))
    assert err_max <= 2e-3 * max(1.0, ref_max), (err_max, ref_max)


@pytest.mark.parametrize("M", [16448, 65792])
def test_fc1_gelu_gemm_at_batch_vs_f64(gpu_device, M):
    """fc1 + exact GELU of 64 and 256 images (N = 6144, K = 1408): 24 rounds of whole tiles per workgroup at 256 images, then the
    ragged round as n-halves.  Tolerance as test_gemm_f16_epilogues_against_f64."""
    from vlfm_amd.vlm import ops

    N, K = 6144, 1408
    grid = min(_cu_count() & ~7, ((M + 255) // 256) * 24)           # the launcher's grid: one workgroup per CU
    items = gemm_ref.work_items(M, N, grid)
    assert (items[:, 1] >= 0).any()                                  # the leftover round runs as n-halves
    if M == 65792:
        whole = np.bincount(np.arange(len(items))[items[:, 1] < 0] % grid, minlength=grid)
        assert whole.min() >= 24
    g = torch.Generator(device=gpu_device).manual_seed(M + 11)
    x = (torch.randn(M, K, generator=g, device=gpu_device) * 0.5).half()
    w = (torch.randn(N, K, generator=g, device=gpu_device) * 0.05).half()
    b = torch.randn(N, generator=g, device=gpu_device).half()
    out = _nan_f16(M + 1, N, device=gpu_device)
    ops.linear_f16(x, w, b, "bias_gelu", out=out[:M])
    assert _is_nan_bits(out[M]), "the guard row was written"
    got = out[:M]
    assert bool(torch.isfinite(got).all())
    _check_gemm(got, x, w, b, None, gelu=True)


def test_fc2_accumulate_gemm_at_batch_vs_f64(gpu_device):
    """fc2 of 256 images, accumulated into the residual stream: 65 792 x 1408 x 6144 (96 K-tiles, the half-empty last n-tile of
    N = 1408, the ragged round as n-halves).  Tolerance as test_gemm_f16_epilogues_against_f64."""
    from vlfm_amd.vlm import ops

    M, N, K = 65792, 1408, 6144
    grid = min(_cu_count() & ~7, 257 * 6)
    assert (gemm_ref.work_items(M, N, grid)[:, 1] >= 0).any()
    g = torch.Generator(device=gpu_device).manual_seed(65)
    x = (torch.randn(M, K, generator=g, device=gpu_device) * 0.5).half()
    w = (torch.randn(N, K, generator=g, device=gpu_device) * 0.05).half()
    b = torch.randn(N, generator=g, device=gpu_device).half()
    r0 = torch.randn(M, N, generator=g, device=gpu_device).half()
    out = _nan_f16(M + 1, N, device=gpu_device)
    out[:M] = r0
    ops.linear_f16(x, w, b, "accumulate", out=out[:M])
    assert _is_nan_bits(out[M]), "the guard row was written"
    got = out[:M]
    assert bool(torch.isfinite(got).all())
    _check_gemm(got, x, w, b, r0, gelu=False)


# ------------------------------------------------------------------------------------------------ end to end
def test_blip2_cosine_at_the_benchmark_batch_vs_fp32(gpu_device):
    """BLIP2ITM.cosine_batch on 256 images in one eager call (what bench.py runs per step) at the real ViT-g + Q-Former geometry,
    random weights spread as in test_blip2_full_geometry_is_batch_size_independent_and_close_to_fp32, against the plain fp32 PyTorch
    graph of the same weights evaluated 16 images at a time.  Same bar: 5e-4."""
    from vlfm_amd.vlm import ops
    from vlfm_amd.vlm.blip2itm import BLIP2ITM, Blip2ITCModel, blip_caption

    fast = BLIP2ITM(device=gpu_device, allow_random_init=True, seed=7)
    g = torch.Generator(device=gpu_device).manual_seed(4)
    with torch.no_grad():
        for n, p in fast.model.named_parameters():
            if p.dim() > 1:
                p.mul_(2.5)
            elif "norm" not in n.lower():
                p.copy_((torch.randn(p.shape, generator=g, device=gpu_device) * 0.05).to(p.dtype))
    fast.model.weights_changed()
    for blk in fast.model.blocks:
        blk.pack_heads()
    fast._text_cache.clear()
    fast._proj_t = None
    with torch.device(gpu_device):
        ref = Blip2ITCModel(fast.cfg)
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(fast.model.named_parameters(), ref.named_parameters()):
            assert n1 == n2
            p2.copy_(p1.float())
    ref.eval()
    ref.deferred_bias = False
    ref.split_kv = False
    N = 256
    gi = torch.Generator(device=gpu_device).manual_seed(256)
    imgs = torch.randint(0, 256, (N, 480, 640, 3), generator=gi, dtype=torch.uint8, device=gpu_device)
    imgs[::3] = (imgs[::3].float() * 0.3 + 90).to(torch.uint8)
    txt = "Seems like there is a potted plant ahead."
    ids = torch.tensor([fast.tokenizer(blip_caption(txt))], device=gpu_device)
    want = []
    with torch.inference_mode():
        for i in range(0, N, 16):
            pix = ops.preprocess_rgb(imgs[i:i + 16], fast.cfg.image_size, torch.float32)
            want.append(ref.itc_reference_head(ref.query_features(ref.vision_tokens(pix)), ref.text_feature(ids)).float().cpu())
    want = torch.cat(want)
    del ref
    assert float(want.std()) > 1e-3
    ops.gemm_f32_overflow_flag(gpu_device, "blip2").zero_()
    got = fast.cosine_batch(imgs, [txt]).float().cpu()
    fast.check_numerics()
    assert fast.attention_path == "hip" and fast.mlp_path(N) == "hip"
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    assert float(err.max()) <= 5e-4, (float(err.max()), int(err.argmax()))


# ------------------------------------------------------------------------------------------------ value edges: LayerNorm, attention
def _layernorm_into(x, cb, w, b, y, rows, dim):
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    _lib.check(_lib.lib().vlfm_layernorm_bias_f16(x.data_ptr(), cb.data_ptr() if cb is not None else None, w.data_ptr(), b.data_ptr(),
                                                 y.data_ptr(), rows, dim, 1e-6, ops._stream()), "layernorm_bias_f16")


@pytest.mark.parametrize("pattern", ["massive_channels", "offset_1000", "near_60000"])
@pytest.mark.parametrize("dim", [1408, 136, 2048])
def test_layernorm_bias_value_edges_vs_f64(gpu_device, dim, pattern):
    """vlfm_layernorm_bias_f16 where EVA ViT-g's residual stream goes: two channels at +-400 in a row of 0.5-sigma noise (the massive
    activations), every channel offset by 1000 (the mean dwarfs the spread: a one-pass variance would cancel), values near +-60000 (the
    sum of squares near 5e12).  41 rows = one per wavefront; D = 1408, 136 (17 vectors: a partly filled wavefront) and 2048.
    Bound, measured against the library and not fixed: max|kernel - f64| <= 2 max|lib - f64| + 2^-11 max|f64|, lib = F.layer_norm in
    f32 on the same x.float() + c, rounded to f16 -- as good as the library's f32 path to within the order of the sums, plus one final
    rounding falling the other way at the largest output."""
    rows = 41
    assert _ln_rows_per_wave(rows) == 1 and (dim == 136) == ((dim // 8) % 64 == 17)
    g = torch.Generator(device=gpu_device).manual_seed(dim * 3 + len(pattern))
    x = torch.randn(rows, dim, generator=g, device=gpu_device) * 0.5
    if pattern == "massive_channels":
        x[:, 3], x[:, 700 if dim > 700 else 100] = 400.0, -400.0
    elif pattern == "offset_1000":
        x += 1000.0
    else:
        x = torch.where(torch.rand(rows, dim, generator=g, device=gpu_device) < 0.5, -1.0, 1.0) * (60000.0 + 200.0 * x)
    x = x.half()
    assert bool(torch.isfinite(x).all())
    c = torch.randn(dim, generator=g, device=gpu_device)
    w = (1 + 0.2 * torch.randn(dim, generator=g, device=gpu_device)).half()
    b = (0.3 * torch.randn(dim, generator=g, device=gpu_device)).half()
    for cb in (c, None):
        y = _nan_f16(rows + 1, dim, device=gpu_device)
        _layernorm_into(x, cb, w, b, y, rows, dim)
        assert _is_nan_bits(y[rows]), "the guard row behind the last row was written"
        got = y[:rows]
        assert bool(torch.isfinite(got).all())
        xs = x.float() + cb if cb is not None else x.float()
        ref = torch.nn.functional.layer_norm(x.double() + (cb.double() if cb is not None else 0.0), (dim,), w.double(), b.double(), 1e-6)
        lib = torch.nn.functional.layer_norm(xs, (dim,), w.float(), b.float(), 1e-6).half()
        err_k, err_l, top = float((got.double() - ref).abs().max()), float((lib.double() - ref).abs().max()), float(ref.abs().max())
        print(f"layernorm D={dim} {pattern} c={'yes' if cb is not None else 'no'}: kernel {err_k:.3e} library f32 {err_l:.3e} "
              f"max|ref| {top:.3f} bound {2 * err_l + 2.0 ** -11 * top:.3e}")
        assert err_k <= 2 * err_l + 2.0 ** -11 * top, (err_k, err_l, top)


@pytest.mark.parametrize("dim", [2048, 128])
def test_layernorm_bias_of_constant_rows_is_beta_bit_for_bit(gpu_device, dim):
    """1 / D is a power of two at D = 2048 and 128: a row of one dyadic value v has the exact sum D v, the exact mean v, deviations of
    exactly zero, and LayerNorm returns beta bit for bit whatever 1 / sqrt(eps) and gamma are -- row 20 is all zeros.  c = None."""
    rows = 41
    g = torch.Generator(device=gpu_device).manual_seed(dim)
    x = ((torch.arange(rows, device=gpu_device, dtype=torch.float32) - 20) / 8).half()[:, None].expand(rows, dim).contiguous()
    assert not bool(x[20].any()) and float(x.abs().max()) * dim < 2 ** 24 / 8
    w = (1 + 0.2 * torch.randn(dim, generator=g, device=gpu_device)).half()
    b = (0.3 * torch.randn(dim, generator=g, device=gpu_device)).half()
    assert bool((b != 0).all())
    y = _nan_f16(rows + 1, dim, device=gpu_device)
    _layernorm_into(x, None, w, b, y, rows, dim)
    assert _is_nan_bits(y[rows])
    diff = y[:rows].view(torch.int16) != b.view(torch.int16)[None, :]
    assert not bool(diff.any()), (int(diff.sum()), diff.nonzero()[0].tolist())


def test_vit_attention_value_edges(gpu_device):
    """vlfm_vit_attention_f16 on three images: 0 -- queries scaled until the scores reach about +-60 (the max-subtracted softmax must
    neither overflow nor go NaN); 1 -- a head whose CLS query (the VALU path) is won by the LAST key, 256 (the one-token tail tile);
    2 -- q = 0: every p_i is exactly 1, the softmax is uniform and the output is the key-mean of v, within one f16 ulp of its f16
    rounding (the only inexact steps are the f32 sum of 257 f16 values and the final scaling).  Bound for the first two: 6e-3 against
    f64, test_vit_attention_kernel_vs_fp32_reference's for the same distribution of v.  Finite, and identical bits over 3 runs."""
    import conv_ref as R

    B = 3
    g = torch.Generator(device=gpu_device).manual_seed(60)
    qkv = torch.randn(B, S, 3, HEADS, DH, generator=g, device=gpu_device) * 1.5
    raw = (qkv[0, :, 0].permute(1, 0, 2) @ qkv[0, :, 1].permute(1, 2, 0)) * DH ** -0.5       # [H, S, S]
    qkv[0, :, 0] *= 60.0 / float(raw.abs().max())
    qkv[1, 0, 0, 2] = 3.0 * qkv[1, 256, 1, 2]
    qkv[2, :, 0] = 0.0
    x = qkv.half().reshape(B * S, 3 * HEADS * DH).contiguous()
    xb = x.view(B, S, 3, HEADS, DH).double()
    q, k, v = [xb[:, :, i].permute(0, 2, 1, 3) for i in range(3)]            # [b, H, S, D]
    scores = q @ k.transpose(-1, -2) * DH ** -0.5
    prob = torch.softmax(scores, dim=-1)
    assert 58.0 <= float(scores[0].abs().max()) <= 62.0 and float(scores[0].max()) >= 45.0 and float(scores[0].min()) <= -45.0
    assert int(prob[1, 2, 0].argmax()) == 256 and float(prob[1, 2, 0, 256]) > 0.9
    assert not bool(scores[2].any())
    ref = (prob @ v).permute(0, 2, 1, 3).reshape(B * S, HEADS * DH)
    outs = []
    for _ in range(3):
        out = _nan_f16((B + 1) * S, HEADS * DH, device=gpu_device)
        _attention_into(x, out, B)
        assert _is_nan_bits(out[B * S:]), "the guard image behind the last one was written"
        outs.append(out[:B * S])
    got = outs[0]
    assert bool(torch.isfinite(got).all())
    assert all(torch.equal(got.view(torch.int16), o.view(torch.int16)) for o in outs[1:])
    err = (got.double() - ref).abs()
    per_image = [float(err[i * S:(i + 1) * S].max()) for i in range(B)]
    print(f"attention value edges: max |err| per image {per_image}, max|score| {float(scores.abs().max()):.1f}")
    assert max(per_image) <= 6e-3, (per_image, int(err.argmax()))
    mean = v[2].mean(dim=1)                                                   # [H, D]: what every query of image 2 returns
    want = R.f16_bits(mean.reshape(1, HEADS * DH).expand(S, HEADS * DH).cpu().numpy())
    ulps = R.ulp_distance(got[2 * S:].contiguous().view(torch.int16).cpu().numpy(), want)
    print(f"attention, uniform softmax: max {int(ulps.max())} f16 ulp from the key-mean, {int((ulps > 0).sum())} of {ulps.size} off")
    assert int(ulps.max()) <= 1
