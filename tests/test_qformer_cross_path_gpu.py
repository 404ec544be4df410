"""-m gpu: Blip2ITCModel.query_features through the one-pass K/V projection and csrc/qformer_attention.hip (``fused_cross_kv``)
against the two-launch projection + library attention it replaces and against the f64 model, at the Q-Former's real sizes (768
hidden, 12 heads of 64, 12 layers, 32 queries, 1408-wide image tokens, 257 tokens per image); and the fallback: a geometry the
kernels do not take (heads of 16, 17 tokens) runs exactly the code it ran before."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _randomise(m, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (std if p.dim() > 1 else 0.1) + (1.0 if "LayerNorm.weight" in n else 0.0))
    m.weights_changed()
    return g


def test_fused_cross_path_matches_split_path_and_f64(gpu_device):
    from vlfm_amd.vlm import blip2itm
    from vlfm_amd.vlm.blip2itm import Blip2ITCConfig, Blip2ITCModel

    assert blip2itm.KV_SPLIT_PIECES == 2
    cfg = Blip2ITCConfig(v_layers=1, v_mlp=64, vocab_size=100, max_position_embeddings=40)
    assert (cfg.q_hidden, cfg.q_heads, cfg.q_layers, cfg.num_query_tokens, cfg.v_hidden) == (768, 12, 12, 32, 1408)
    m = Blip2ITCModel(cfg).eval()
    g = _randomise(m, 21, 0.03)       # (0.03: scores of order 1 at 768 / 1408 inputs -- a softmax that is neither flat nor one-hot)
    ref64 = Blip2ITCModel(cfg).eval().double()
    ref64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    m.to(gpu_device)
    m.split_kv_min_rows = 0
    tokens16 = torch.randn(4, 257, 1408, generator=g).half()
    with torch.inference_mode():
        want = ref64.query_features(tokens16.double())
        assert m.fused_cross_kv and m._fused_cross_ok(tokens16.to(gpu_device))
        on = m.query_features(tokens16.to(gpu_device)).double().cpu()
        assert m._kv_pair is not None                      # the new path ran
        m.fused_cross_kv = False
        off = m.query_features(tokens16.to(gpu_device)).double().cpu()
    scale = float(off.abs().max())
    d, e_on, e_off = float((on - off).abs().max()), float((on - want).abs().max()), float((off - want).abs().max())
    print(f"fused cross path: |on - off|={d:.3e} (max|off|={scale:.3e}) |on - f64|={e_on:.3e} |off - f64|={e_off:.3e}")
    assert not bool(torch.isnan(on).any())
    assert d <= 1e-5 * scale, (d, scale)
    assert e_on <= 5e-5 and e_off <= 5e-5, (e_on, e_off)
    m.weights_changed()
    assert m._kv_pair is None and m._kv_all is None        # derived weights are dropped with the rest


def test_fused_cross_path_at_a_product_batch_matches_split_path_and_f64(gpu_device):
    """64 images with the DEFAULT thresholds -- what the product sends down this path: 780 GEMM tiles (three per workgroup) and 768
    attention items, and 2048 query rows, which also take _qlinear to the split f32 GEMM.  The yardstick for the f64 comparison is the
    two-launch projection + library attention on the same inputs, not a figure observed at another batch."""
    from vlfm_amd.vlm import blip2itm, ops
    from vlfm_amd.vlm.blip2itm import Blip2ITCConfig, Blip2ITCModel

    n_img = 64
    assert blip2itm.KV_SPLIT_PIECES == 2
    cfg = Blip2ITCConfig(v_layers=1, v_mlp=64, vocab_size=100, max_position_embeddings=40)
    m = Blip2ITCModel(cfg).eval()
    _randomise(m, 21, 0.03)
    ref64 = Blip2ITCModel(cfg).eval().double()
    ref64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    m.to(gpu_device)
    ref64.to(gpu_device)
    assert m.split_kv_min_rows == 32 * 257 <= n_img * 257                                   # the defaults, untouched
    assert blip2itm.QFORMER_SPLIT_MIN_ROWS == 2048 <= n_img * cfg.num_query_tokens
    g = torch.Generator(device=gpu_device).manual_seed(64)
    tokens16 = torch.randn(n_img, 257, 1408, generator=g, device=gpu_device).half()
    flag = ops.gemm_f32_overflow_flag(gpu_device, "blip2")
    with torch.inference_mode():
        want = torch.cat([ref64.query_features(tokens16[i:i + 16].double()) for i in range(0, n_img, 16)])
        del ref64
        assert m.fused_cross_kv and m._fused_cross_ok(tokens16)
        flag.zero_()
        on = m.query_features(tokens16).double()
        assert int(flag.item()) == 0
        assert m._kv_pair is not None                      # the new path ran
        m.fused_cross_kv = False
        off = m.query_features(tokens16).double()
        assert int(flag.item()) == 0
    scale, want_max = float(off.abs().max()), float(want.abs().max())
    d, e_on, e_off = float((on - off).abs().max()), float((on - want).abs().max()), float((off - want).abs().max())
    print(f"fused cross path, {n_img} images: |on - off|={d:.3e} (max|off|={scale:.3e}) |on - f64|={e_on:.3e} |off - f64|={e_off:.3e} "
          f"max|f64|={want_max:.3e}")
    assert not bool(torch.isnan(on).any())
    assert d <= 1e-5 * scale, (d, scale)
    assert e_on <= 2.0 * e_off + 1e-7 * want_max, (e_on, e_off, want_max)


def test_refused_geometry_runs_the_old_code(gpu_device):
    from vlfm_amd.vlm.blip2itm import Blip2ITCConfig, Blip2ITCModel

    cfg = Blip2ITCConfig(image_size=56, patch_size=14, v_hidden=176, v_layers=1, v_heads=2, v_mlp=352, q_hidden=64,
                         q_layers=4, q_heads=4, q_mlp=128, vocab_size=100, max_position_embeddings=40,
                         num_query_tokens=8, proj_dim=16)
    m = Blip2ITCModel(cfg).eval()
    g = _randomise(m, 4, 0.3)
    m.to(gpu_device)
    m.split_kv_min_rows = 0
    tokens16 = (torch.randn(6, 17, 176, generator=g) * 2).half().to(gpu_device)
    with torch.inference_mode():
        m.fused_cross_kv = True
        assert not m._fused_cross_ok(tokens16)
        on = m.query_features(tokens16)
        assert m._kv_pair is None and m._kv_all is not None
        m.fused_cross_kv = False
        off = m.query_features(tokens16)
    assert torch.equal(on, off)
