"""-m gpu: VLM-side HIP kernels against the real PIL / plain PyTorch fp32, and the in-process BLIP-2 ITC path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(480, 640), (720, 1280), (100, 150)])
def test_preprocess_matches_pil_bit_exact(gpu_device, shape):
    from PIL import Image

    from vlfm_amd.vlm import ops

    rng = np.random.default_rng(1)
    H, W = shape
    imgs = rng.integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    out = ops.preprocess_rgb(torch.from_numpy(imgs).to(gpu_device), 224, torch.float32).cpu()
    mean = torch.tensor(ops.CLIP_MEAN).view(3, 1, 1)
    std = torch.tensor(ops.CLIP_STD).view(3, 1, 1)
    for i in range(3):
        pil = np.asarray(Image.fromarray(imgs[i]).resize((224, 224), Image.BICUBIC))
        want = (torch.from_numpy(pil.copy()).permute(2, 0, 1).float().div(255) - mean) / std  # ToTensor + Normalize
        assert torch.equal(out[i], want)  # bit-exact f32
    half = ops.preprocess_rgb(torch.from_numpy(imgs).to(gpu_device), 224, torch.float16).cpu()
    assert torch.equal(half, out.half())
    # im2col layout for the GEMM patch embedding: same values, [n, 256, 588] in conv-weight order (c, ky, kx)
    pat = ops.preprocess_rgb(torch.from_numpy(imgs).to(gpu_device), 224, torch.float32, patch_size=14).cpu()
    want_pat = out.reshape(3, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(3, 256, 588)
    assert torch.equal(pat, want_pat)


@pytest.mark.parametrize("case", [(9, 480, 640, 224, 14, torch.float16), (2, 720, 1280, 224, 14, torch.bfloat16),
                                  (5, 120, 160, 56, 0, torch.float32), (3, 96, 128, 224, 14, torch.float16),
                                  (70, 48, 64, 30, 0, torch.float32)])
def test_preprocess_one_launch_equals_two_launch(gpu_device, case, monkeypatch):
    """The fused resampler (u8 intermediate in LDS) against the two-launch form it replaced, on downscaling, upscaling,
    band counts from 1 to 28 and every output type: identical bits.  (PIL itself is the judge of both in the test above.)"""
    from vlfm_amd.vlm import ops

    n, H, W, out, patch, dt = case
    img = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    got = ops.preprocess_rgb(img, out, dt, patch_size=patch)
    monkeypatch.setenv("VLFM_PREPROCESS_TWO_PASS", "1")
    want = ops.preprocess_rgb(img, out, dt, patch_size=patch)
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", [(300, 264, 128), (1000, 776, 1408), (130, 8, 64), (2570, 6144, 1408)])
def test_linear_gelu_kernel_vs_fp32_reference(gpu_device, shape, monkeypatch):
    """vlfm_gemm_f16_nt (hand-written MFMA GEMM, exact-form GELU in the epilogue) against x @ w.T + b -> F.gelu in fp32:
    ragged M / N tails, one and many K-tiles, asymmetric data (a transposed operand or a swapped tile would show), both
    schedules.  Tolerance: f16 output rounding (2^-11 relative) plus the f32 accumulation order."""
    import torch.nn.functional as F

    from vlfm_amd.vlm import ops

    M, N, K = shape
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, K, generator=g) * 0.5).half().to(gpu_device)
    w = (torch.randn(N, K, generator=g) * 0.05).half().to(gpu_device)
    b = torch.randn(N, generator=g).half().to(gpu_device)
    want = F.gelu(x.float() @ w.float().t() + b.float())
    got = ops.linear_gelu(x, w, b).float()
    err = (got - want).abs()
    assert float((err - 1e-3 * want.abs()).max()) <= 1e-3, float(err.max())
    # the activation alone over its whole range (x = v e_0, w = e_0: the GEMM returns gelu(v) for every output column),
    # against float64 -- including the negative tail, where an f32 "1 + erf" would cancel
    v = torch.linspace(-11, 11, 2816).half()
    xe = torch.zeros(2816, 64, dtype=torch.float16)
    xe[:, 0] = v
    we = torch.zeros(8, 64, dtype=torch.float16)
    we[:, 0] = 1.0
    got = ops.linear_gelu(xe.to(gpu_device), we.to(gpu_device), None).cpu().double()
    ref = F.gelu(v.double())
    assert torch.equal(got[:, 0], got[:, 7])
    assert float(((got[:, 0] - ref).abs() - 2.0 ** -11 * ref.abs()).max()) <= 1e-7


def test_itc_head_vs_fp32_reference(gpu_device):
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(0)
    for (B, NQ, H, P) in [(5, 32, 768, 256), (2, 5, 24, 8), (1, 32, 768, 256), (256, 32, 768, 256), (257, 32, 768, 256)]:
        q = torch.randn(B, NQ, H, generator=g)
        w = torch.randn(P, H, generator=g) * 0.05
        b = torch.randn(P, generator=g) * 0.1
        t = torch.nn.functional.normalize(torch.randn(B, P, generator=g), dim=-1)
        want = torch.einsum("bqp,bp->bq", torch.nn.functional.normalize(q @ w.t() + b, dim=-1), t).max(1).values
        got = ops.itc_head(q.to(gpu_device), w.t().contiguous().to(gpu_device), b.to(gpu_device),
                           t.to(gpu_device)).cpu()
        assert torch.allclose(got, want, atol=2e-5, rtol=0), (got, want)


def test_blip2_cosine_fp16_gpu_vs_fp32_cpu(gpu_device):
    """Self-parity of the whole ITC path: fp16 ViT on the GPU vs the same random weights in
    fp32 on the CPU, small geometry.  Tolerance 2e-2 on a cosine (fp16 ViT activations)."""
    from vlfm_amd.vlm.blip2itm import BLIP2ITM, Blip2ITCConfig, Blip2ITCModel, blip_caption
    from vlfm_amd.vlm import ops

    cfg = Blip2ITCConfig(image_size=56, patch_size=14, v_hidden=128, v_layers=3, v_heads=4, v_mlp=256, q_hidden=64,
                         q_layers=4, q_heads=4, q_mlp=128, vocab_size=2000, max_position_embeddings=40,
                         num_query_tokens=8, proj_dim=32)
    gpu = BLIP2ITM(device=gpu_device, config=cfg, seed=5)
    cpu = Blip2ITCModel(cfg).init_random(5).eval()
    # random-init at 0.02 gives near-degenerate cosines; scale the weights up identically on both sides
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(gpu.model.named_parameters(), cpu.named_parameters()):
            if p2.dim() > 1:
                p2.mul_(6.0)
                p1.copy_(p2.to(p1.dtype))
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, size=(4, 120, 160, 3), dtype=np.uint8)
    txt = "Seems like there is a chair ahead."
    got = gpu.cosine_batch(torch.from_numpy(imgs).to(gpu_device), [txt]).cpu()
    pix = ops.preprocess_rgb(torch.from_numpy(imgs).to(gpu_device), 56, torch.float32).cpu()
    ids = torch.tensor([gpu.tokenizer(blip_caption(txt))])
    with torch.inference_mode():
        want = cpu.itc_reference_head(cpu.query_features(cpu.vision_tokens(pix)), cpu.text_feature(ids))
    assert torch.allclose(got, want, atol=2e-2, rtol=0), (got, want)
    one = gpu.cosine(imgs[2], txt)
    assert isinstance(one, float) and abs(one - float(got[2])) < 1e-3


def test_blip2_client_signature_and_full_geometry(gpu_device):
    """BLIP2ITMClient(port).cosine(image, txt) -> float at the real ViT-g/14 geometry (random weights)."""
    from vlfm_amd.vlm.blip2itm import BLIP2ITMClient

    client = BLIP2ITMClient(port=12182, device=gpu_device, allow_random_init=True)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    c = client.cosine(img, "Seems like there is a target_object ahead.".replace("target_object", "bed"))
    assert isinstance(c, float) and -1.0 <= c <= 1.0
    assert client._model.cfg.v_layers == 39 and client._model.weights == "random-init"


@pytest.mark.parametrize("rows,dim", [(257 * 3, 1408), (50, 128), (9, 2048), (17, 136)])
def test_layernorm_bias_kernel_vs_fp32_reference(gpu_device, rows, dim):
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(rows + dim)
    x = (torch.randn(rows, dim, generator=g) * 3).half()
    c = torch.randn(dim, generator=g)
    w, b = (1 + 0.2 * torch.randn(dim, generator=g)).half(), (0.3 * torch.randn(dim, generator=g)).half()
    for cb in (c, None):
        want = torch.nn.functional.layer_norm(x.float() + (cb if cb is not None else 0), (dim,), w.float(), b.float(), 1e-6)
        got = ops.layernorm_bias(x.to(gpu_device), cb.to(gpu_device) if cb is not None else None, w.to(gpu_device),
                                 b.to(gpu_device), 1e-6).cpu()
        assert got.dtype == torch.float16
        assert (got.float() - want).abs().max() <= 4e-3  # one f16 ulp at |y| <= 4


def test_vit_deferred_bias_path_equals_plain_path(gpu_device):
    """The ViT fast path (residual adds folded into the GEMMs, biases entering through LayerNorm(x + c)) against the
    plain block-by-block path on the same f16 weights, and both against fp32 on the CPU.  88-wide heads so that the
    packed-head path is the one in use, non-zero biases everywhere."""
    from vlfm_amd.vlm.blip2itm import Blip2ITCConfig, Blip2ITCModel

    cfg = Blip2ITCConfig(image_size=56, patch_size=14, v_hidden=176, v_layers=4, v_heads=2, v_mlp=352, q_hidden=64,
                         q_layers=2, q_heads=4, q_mlp=128, vocab_size=100, max_position_embeddings=40,
                         num_query_tokens=4, proj_dim=16)
    ref = Blip2ITCModel(cfg).init_random(3).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() > 1:
                p.mul_(4.0)
            elif "layer_norm" not in n and "LayerNorm" not in n and "layernorm" not in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    gpu = Blip2ITCModel(cfg).eval()
    gpu.load_state_dict(ref.state_dict())
    gpu.to(gpu_device).set_precision(torch.float16)
    for blk in gpu.blocks:
        blk.pack_heads()
    assert gpu.blocks[0]._packed is not None
    pix = torch.randn(5, 3, 56, 56, generator=g)
    with torch.inference_mode():
        want = ref.vision_tokens(pix)
        gpu.deferred_bias = True
        fast = gpu.vision_tokens(pix.to(gpu_device).half()).float().cpu()
        gpu.deferred_bias = False
        plain = gpu.vision_tokens(pix.to(gpu_device).half()).float().cpu()
    assert (plain - want).abs().max() <= 3e-2 and (fast - want).abs().max() <= 3e-2
    assert (fast - plain).abs().max() <= 2e-2
    assert (fast - want).abs().mean() <= 1.2 * (plain - want).abs().mean() + 1e-4  # not less accurate than the plain path


def test_vit_block_with_the_fc1_gelu_kernel(gpu_device):
    """The ViT fast path with fc1 + GELU through vlfm_gemm_f16_nt (forced on: the product switches to it at 32 images) against
    the same path with the library GEMM + GELU pass, and against fp32 on the CPU; a hidden width the kernel cannot tile
    (176) must silently stay on the library."""
    from vlfm_amd.vlm.blip2itm import Blip2ITCConfig, Blip2ITCModel

    g = torch.Generator().manual_seed(2)
    for hidden, uses_kernel in ((192, True), (176, False)):
        cfg = Blip2ITCConfig(image_size=56, patch_size=14, v_hidden=hidden, v_layers=3, v_heads=2, v_mlp=2 * hidden, q_hidden=64,
                             q_layers=2, q_heads=4, q_mlp=128, vocab_size=100, max_position_embeddings=40,
                             num_query_tokens=4, proj_dim=16)
        ref = Blip2ITCModel(cfg).init_random(4).eval()
        with torch.no_grad():
            for n, p in ref.named_parameters():
                if p.dim() > 1:
                    p.mul_(4.0)
                elif "layer_norm" not in n and "LayerNorm" not in n and "layernorm" not in n:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.5)
        gpu = Blip2ITCModel(cfg).eval()
        gpu.load_state_dict(ref.state_dict())
        gpu.to(gpu_device).set_precision(torch.float16)
        pix = torch.randn(6, 3, 56, 56, generator=g)
        calls = []
        from vlfm_amd.vlm import ops
        real = ops.linear_gelu
        ops.linear_gelu = lambda *a: (calls.append(1), real(*a))[1]
        try:
            with torch.inference_mode():
                want = ref.vision_tokens(pix)
                gpu.deferred_bias = True
                for blk in gpu.blocks:
                    blk.hip_mlp_min_rows = 1
                ours = gpu.vision_tokens(pix.to(gpu_device).half()).float().cpu()
                n_calls = len(calls)
                for blk in gpu.blocks:
                    blk.hip_mlp_min_rows = 0
                lib = gpu.vision_tokens(pix.to(gpu_device).half()).float().cpu()
        finally:
            ops.linear_gelu = real
        assert n_calls == (cfg.v_layers if uses_kernel else 0) and len(calls) == n_calls
        assert (ours - want).abs().max() <= 3e-2 and (lib - want).abs().max() <= 3e-2
        assert (ours - lib).abs().max() <= 2e-2
        assert (ours - want).abs().mean() <= 1.2 * (lib - want).abs().mean() + 1e-4


@pytest.mark.parametrize("B", [1, 3, 19, 40])
def test_vit_attention_kernel_vs_fp32_reference(gpu_device, B):
    """vlfm_vit_attention_f16 (257 tokens, 16 heads of 88) against softmax(q k^T / sqrt(88)) v in fp32.  B = 19 and 40 make the
    persistent workgroups walk 2 and 3 (image, head) items each (the LDS-DMA pipeline across items), B = 1 uses one XCD only; the
    run is repeated (a race between the DMA pieces, the staged rows and the barriers would not be deterministic)."""
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(7 + B)
    S, H, D = 257, 16, 88
    qkv = torch.randn(B, S, 3, H, D, generator=g) * 1.5
    qkv[0, :, 0, 0] *= 4.0                                # a head with peaked softmax rows
    qkv[B - 1, :, 0, 5] *= 3.0
    qkv[B - 1, 0, 0, 7] *= 5.0                            # a peaked CLS query (the VALU path)
    half = qkv.half()
    scale = 88 ** -0.5
    q, k, v = [half[:, :, i].float().permute(0, 2, 1, 3) for i in range(3)]          # [B,H,S,D]
    want = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v                 # [B,H,S,D]
    want = want.permute(0, 2, 1, 3).reshape(B * S, H * D)
    x = half.to(gpu_device).reshape(B * S, 3 * H * D).contiguous()
    first = None
    for _ in range(3):
        got = ops.vit_attention(x, B, S, H, D, scale)
        if first is None:
            first = got.clone()
        assert torch.equal(got, first)                    # bitwise reproducible
        err = (got.float().cpu() - want).abs()
        assert err.max() <= 6e-3, (float(err.max()), int(err.argmax()))


def test_vit_attention_rejects_other_shapes(gpu_device):
    """Anything but 257 tokens x heads of 88 is VLFM_ERR_INVALID (the caller then uses the library attention)."""
    from vlfm_amd import _lib

    x = torch.zeros(2 * 257 * 3 * 16 * 96, dtype=torch.float16, device=gpu_device)
    out = torch.zeros(2 * 257 * 16 * 96, dtype=torch.float16, device=gpu_device)
    L = _lib.lib()
    assert L.vlfm_vit_attention_f16(x.data_ptr(), out.data_ptr(), 2, 257, 16, 96, 0.1, None) == _lib.VLFM_ERR_INVALID
    assert L.vlfm_vit_attention_f16(x.data_ptr(), out.data_ptr(), 2, 256, 16, 88, 0.1, None) == _lib.VLFM_ERR_INVALID
    assert L.vlfm_vit_attention_f16(x.data_ptr(), out.data_ptr(), 0, 257, 16, 88, 0.1, None) == _lib.VLFM_OK


def test_vit_fast_path_full_geometry_vs_plain(gpu_device):
    """ViT-g/14 at the real geometry (random weights, non-zero biases): attention kernel + deferred-bias path vs the plain
    PyTorch path on the same f16 weights."""
    from vlfm_amd.vlm.blip2itm import BLIP2ITM

    m = BLIP2ITM(device=gpu_device, allow_random_init=True).model
    g = torch.Generator(device=gpu_device).manual_seed(2)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1 and "norm" not in n.lower():
                p.copy_(torch.randn(p.shape, generator=g, device=gpu_device, dtype=torch.float32).to(p.dtype) * 0.1)
        for blk in m.blocks:
            blk.pack_heads()
    m._deferred_c = None
    pat = torch.randn(3, 256, 588, generator=g, device=gpu_device, dtype=torch.float32).half()
    with torch.inference_mode():
        m.deferred_bias = True
        fast = m.vision_tokens(pat).float()
        for blk in m.blocks:
            blk.hip_attention = False
        mid = m.vision_tokens(pat).float()
        m.deferred_bias = False
        plain = m.vision_tokens(pat).float()
    assert (mid - plain).abs().max() <= 6e-2 and (fast - plain).abs().max() <= 6e-2   # 39 blocks of f16 rounding noise
    assert (fast - plain).abs().mean() <= 4e-3 and (fast - mid).abs().mean() <= 4e-3


def test_vit_all_four_gemms_on_the_8phase_kernel_full_geometry(gpu_device):
    """ViT-g/14 at the real geometry with qkv / projection / fc1 / fc2 of every block on csrc/gemm_f16.hip (bias, accumulate-into-the-
    stream and bias + GELU epilogues) against the same blocks on hipBLASLt, same f16 weights, 40 images (10 280 rows: a ragged last
    m-tile, the half-empty last n-tile of N = 1408 and 4224)."""
    from vlfm_amd.vlm.blip2itm import BLIP2ITM

    m = BLIP2ITM(device=gpu_device, allow_random_init=True).model
    g = torch.Generator(device=gpu_device).manual_seed(5)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1 and "norm" not in n.lower():
                p.copy_(torch.randn(p.shape, generator=g, device=gpu_device, dtype=torch.float32).to(p.dtype) * 0.1)
        for blk in m.blocks:
            blk.pack_heads()          # (the plain path runs on packed copies of the qkv / projection parameters)
    m._deferred_c = None
    pat = torch.randn(40, 256, 588, generator=g, device=gpu_device, dtype=torch.float32).half()
    with torch.inference_mode():
        m.deferred_bias = True
        for blk in m.blocks:
            blk.hip_gemms = frozenset(("qkv", "proj", "fc1", "fc2"))
            blk.hip_mlp_min_rows = 1
        assert m.blocks[0].hip_gemms_at(40 * 257) == frozenset(("qkv", "proj", "fc1", "fc2"))
        hip = m.vision_tokens(pat).float()
        for blk in m.blocks:
            blk.hip_gemms = frozenset()
        lib = m.vision_tokens(pat).float()
        m.deferred_bias = False
        plain = m.vision_tokens(pat[:4]).float()
    assert torch.isfinite(hip).all()
    assert (hip - lib).abs().max() <= 6e-2 and (hip - lib).abs().mean() <= 4e-3          # 39 blocks of f16 rounding noise
    assert (hip[:4] - plain).abs().max() <= 6e-2 and (hip[:4] - plain).abs().mean() <= 4e-3
    assert (hip[:4] - plain).abs().mean() <= 1.3 * (lib[:4] - plain).abs().mean() + 1e-4     # not noisier than the library path


def test_blip2_cosine_split_f16_qformer_equals_exact_f32_qformer_at_the_real_geometry(gpu_device):
    """the product's Q-Former runs its f32 Linears as split-f16 GEMMs (hi / lo planes, ~22 mantissa bits) and
    projects the cross-attention K / V from two weight pieces.  End to end, at the real ViT-g + Q-Former geometry and a batch that
    takes those paths (64 images: 2 048 query rows), the ITC cosine must equal the one computed with exact-f32 library GEMMs and
    three K / V pieces within 1e-5 (the reference's blip2itm.py:37-54 compares nothing tighter than its own f16 ViT allows: 5e-3)."""
    from vlfm_amd.vlm import blip2itm, ops
    from vlfm_amd.vlm.blip2itm import BLIP2ITM

    m = BLIP2ITM(device=gpu_device, allow_random_init=True)
    g = torch.Generator().manual_seed(9)
    imgs = torch.randint(0, 256, (64, 480, 640, 3), generator=g, dtype=torch.uint8).to(gpu_device)
    prompts = ["Seems like there is a chair ahead."]
    ops.gemm_f32_overflow_flag(gpu_device, "blip2").zero_()
    with torch.inference_mode():
        fast = m.cosine_batch(imgs, prompts).double().cpu()
        m.check_numerics()
        saved = (blip2itm.QFORMER_SPLIT_MIN_ROWS, blip2itm.KV_SPLIT_PIECES)
        blip2itm.QFORMER_SPLIT_MIN_ROWS, blip2itm.KV_SPLIT_PIECES = 1 << 60, 3
        try:
            for blk in m.model.modules():          # cached split / pieced weights belong to the other setting
                for name in ("_kv_pieces", "_kv_cache"):
                    if hasattr(blk, name):
                        setattr(blk, name, None)
            exact = m.cosine_batch(imgs, prompts).double().cpu()
        finally:
            blip2itm.QFORMER_SPLIT_MIN_ROWS, blip2itm.KV_SPLIT_PIECES = saved
    assert torch.isfinite(fast).all() and fast.abs().max() <= 1.0 + 1e-6
    assert float((fast - exact).abs().max()) <= 1e-5, float((fast - exact).abs().max())


def test_qformer_split_kv_projection_is_f32_grade(gpu_device):
    """Cross-attention K/V projection of f16 tokens through the split weights (f16 x f16 -> f32 GEMMs) against the plain f32 GEMM
    path and against f64, with three pieces (exact weights) and with two (the product default: 22-23 of 24 bits): not less
    accurate than the f32 GEMM, and within 1e-6 of the result's scale of the f32 result."""
    from vlfm_amd.vlm import blip2itm
    from vlfm_amd.vlm.blip2itm import Blip2ITCConfig, Blip2ITCModel

    cfg = Blip2ITCConfig(image_size=56, patch_size=14, v_hidden=176, v_layers=1, v_heads=2, v_mlp=352, q_hidden=64,
                         q_layers=4, q_heads=4, q_mlp=128, vocab_size=100, max_position_embeddings=40,
                         num_query_tokens=8, proj_dim=16)
    m = Blip2ITCModel(cfg).init_random(11).eval()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1) + (1.0 if "LayerNorm.weight" in n else 0.0))
    ref64 = Blip2ITCModel(cfg).eval().double()
    ref64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    m.to(gpu_device)
    m.split_kv_min_rows = 0
    tokens16 = (torch.randn(6, 17, 176, generator=g) * 2).half()
    default_pieces = blip2itm.KV_SPLIT_PIECES
    assert default_pieces == 2
    try:
        with torch.inference_mode():
            want = ref64.query_features(tokens16.double())
            m.split_kv = False
            plain = m.query_features(tokens16.to(gpu_device)).double().cpu()
            e_plain = (plain - want).abs().max()
            for pieces in (3, 2):
                blip2itm.KV_SPLIT_PIECES = pieces
                m.split_kv = True
                split = m.query_features(tokens16.to(gpu_device)).double().cpu()
                e_split = (split - want).abs().max()
                assert e_split <= 5e-5 and e_plain <= 5e-5, (pieces, float(e_split), float(e_plain))
                assert e_split <= 2.0 * e_plain + 1e-6, (pieces, float(e_split), float(e_plain))   # f32-grade
        cross = [l.crossattention for l in m.q_layers if l.crossattention is not None]
        w1t, w2t, w3t, _ = m._kv_all            # all cross-attention layers, [K_0 | V_0 | K_1 | V_1 ...]
        full = torch.cat([torch.cat([c.key.weight, c.value.weight]) for c in cross]).detach().double().t()
        rec3 = w1t.double() + w2t.double() / 2048 + w3t.double() / 2048 ** 2
        assert float((rec3 - full).abs().max()) <= 1e-12    # the three f16 pieces carry the f32 weights (2^-33 relative)
        rec2 = w1t.double() + w2t.double() / 2048
        # two pieces: one f32 rounding of the weight (plus f16's subnormal floor of the second piece, 2^-25 / 2048 absolute)
        assert bool(((rec2 - full).abs() <= 2.0 ** -22 * full.abs() + 2.0 ** -35).all())
        # the projection itself at the Q-Former's REAL contraction length (1408) against f64 and against the f32 GEMM
        x16 = (torch.randn(4096, 1408, generator=g) * 1.5).half().to(gpu_device)
        w = (torch.randn(1536, 1408, generator=g) * 0.05).to(gpu_device)
        b = torch.randn(1536, generator=g).to(gpu_device)
        want = torch.nn.functional.linear(x16.double(), w.double(), b.double())
        f32 = torch.nn.functional.linear(x16.float(), w, b).double()
        pieces3 = tuple(t.t() for t in blip2itm._exact_split3(w))
        scale = float(want.abs().max())
        for pieces in (3, 2):
            got = blip2itm._split_gemm(x16, pieces3, b, n_pieces=pieces).double()
            e_got, e_f32 = float((got - want).abs().max()), float((f32 - want).abs().max())
            assert e_got <= 2.0 * e_f32 + 1e-6 * scale, (pieces, e_got, e_f32, scale)
            assert float((got - f32).abs().max()) <= 1e-6 * scale + 2.0 * e_f32, (pieces, float((got - f32).abs().max()), scale)
        # the per-layer form of the same projection (used when a caller passes kv= directly)
        k, v = cross[0]._project_kv_f16(tokens16.to(gpu_device))
        want_k = torch.nn.functional.linear(tokens16.double(), cross[0].key.weight.detach().double().cpu(),
                                            cross[0].key.bias.detach().double().cpu())
        assert (k.double().cpu() - want_k).abs().max() <= 2e-5
    finally:
        blip2itm.KV_SPLIT_PIECES = default_pieces


def test_blip2_full_geometry_fp16_hip_path_vs_fp32_on_the_gpu(gpu_device):
    """ViT-g/14 + Q-Former at the REAL geometry, batch 2: the product path (f16 ViT with the HIP attention / LayerNorm
    kernels and deferred biases, f32 Q-Former with the split K/V projections, HIP ITC head) against the plain PyTorch graph
    of the same weights evaluated entirely in fp32 on the GPU.  Bar: |cosine difference| <= 5e-3."""
    from vlfm_amd.vlm import ops
    from vlfm_amd.vlm.blip2itm import BLIP2ITM, Blip2ITCModel, blip_caption

    fast = BLIP2ITM(device=gpu_device, allow_random_init=True, seed=7)
    fast.strict_hip_attention = True
    g = torch.Generator(device=gpu_device).manual_seed(4)
    with torch.no_grad():   # random-init at 0.02 gives near-degenerate cosines: spread the weights, add biases
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
            p2.copy_(p1.float())   # the f16 ViT weights are exactly representable: both sides hold the same numbers
    ref.eval()
    ref.deferred_bias = False
    ref.split_kv = False
    rng = np.random.default_rng(1)
    imgs = torch.from_numpy(rng.integers(0, 256, size=(2, 480, 640, 3), dtype=np.uint8)).to(gpu_device)
    txt = "Seems like there is a potted plant ahead."
    got = fast.cosine_batch(imgs, [txt]).float().cpu()
    assert fast.attention_path == "hip"
    pix = ops.preprocess_rgb(imgs, fast.cfg.image_size, torch.float32)
    ids = torch.tensor([fast.tokenizer(blip_caption(txt))], device=gpu_device)
    with torch.inference_mode():
        want = ref.itc_reference_head(ref.query_features(ref.vision_tokens(pix)), ref.text_feature(ids)).float().cpu()
    print(f"BLIP-2 full geometry: f16 HIP path {got.tolist()} vs fp32 {want.tolist()}")
    assert float(want.abs().max()) > 1e-3 and float((want[0] - want[1]).abs()) > 1e-4   # not a degenerate comparison
    assert torch.allclose(got, want, atol=5e-3, rtol=0), (got, want)


def test_blip2_full_geometry_is_batch_size_independent_and_close_to_fp32(gpu_device):
    """The product path switches kernels with the batch size (the fused fc1 + GELU kernel from 32 images on, several items per workgroup
    in the attention kernel, library GEMM solutions per shape): 33 images through it at batch sizes 1, 8 and 33 against the plain fp32
    PyTorch graph of the same weights.  Measured 8e-5 at every batch size from 1 to 64 (profiles/r06_random_parity_stress.txt); the
    bar here is 5e-4.  Graph replay equals the eager call bit for bit."""
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
            p2.copy_(p1.float())
    ref.eval()
    ref.deferred_bias = False
    ref.split_kv = False
    rng = np.random.default_rng(2)
    N = 33
    imgs = torch.from_numpy(rng.integers(0, 256, size=(N, 480, 640, 3), dtype=np.uint8)).to(gpu_device)
    imgs[::3] = (imgs[::3].float() * 0.3 + 90).to(torch.uint8)
    txt = "Seems like there is a potted plant ahead."
    ids = torch.tensor([fast.tokenizer(blip_caption(txt))], device=gpu_device)
    want = []
    with torch.inference_mode():
        for i in range(0, N, 11):
            pix = ops.preprocess_rgb(imgs[i:i + 11], fast.cfg.image_size, torch.float32)
            want.append(ref.itc_reference_head(ref.query_features(ref.vision_tokens(pix)), ref.text_feature(ids)).float().cpu())
    want = torch.cat(want)
    assert float(want.std()) > 1e-3
    for bs in (1, 8, 33):
        got = torch.cat([fast.cosine_batch(imgs[i:i + bs], [txt]).float().cpu() for i in range(0, N, bs)])
        assert float((got - want).abs().max()) <= 5e-4, (bs, float((got - want).abs().max()))
    eager = fast.cosine_batch(imgs[:8], [txt]).float().cpu()
    assert torch.equal(fast.cosine_batch_graphed(imgs[:8], [txt]).float().cpu(), eager)
    assert torch.equal(fast.cosine_batch_graphed(imgs[8:16], [txt]).float().cpu(), fast.cosine_batch(imgs[8:16], [txt]).float().cpu())
