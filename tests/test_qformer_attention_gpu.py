"""-m gpu: csrc/qformer_attention.hip (the Q-Former's cross-attention in f32, K / V read from the pair GEMM's block-major tensor)
against an f64 softmax attention on the host.  Bound: twice the error of F.scaled_dot_product_attention in f32 on the same tensors
plus 1e-7 max|ref|.  B = 9 puts two images on one XCD's share of the items, T = 1 / 33 / 257 are "no full key tile", "one tile + one
key" and the real shape (8 tiles + one key), T = 50 / 64 a longer vector-ALU remainder and none at all."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HEADS = 12
SENTINEL = 12345.5


def _case(B, T, Q, seed, q_scale=1.0):
    """q [B, Q, H * 64] and a block-major K/V tensor [2 H + 4, B * T, 64] with the K heads at blocks [2, 2 + H), the V heads at
    [3 + H, 3 + 2 H) and unrelated blocks around them; image b is rows [b T, (b + 1) T) of every block."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Q, HEADS * 64, generator=g) * q_scale
    blocks = torch.randn(2 * HEADS + 4, B * T, 64, generator=g)
    k0, v0 = 2, 3 + HEADS
    k = blocks[k0:k0 + HEADS].reshape(HEADS, B, T, 64).permute(1, 0, 2, 3)      # [B, H, T, 64]
    v = blocks[v0:v0 + HEADS].reshape(HEADS, B, T, 64).permute(1, 0, 2, 3)
    return q, blocks, k0, v0, k, v


def _check(gpu_device, B, T, Q, seed, q_scale=1.0):
    from vlfm_amd.vlm import ops

    q, blocks, k0, v0, k, v = _case(B, T, Q, seed, q_scale)
    scale = 0.125
    qh = q.view(B, Q, HEADS, 64).transpose(1, 2)                                 # [B, H, Q, 64]
    s64 = (qh.double() @ k.double().transpose(-1, -2)) * scale
    ref = (torch.softmax(s64, dim=-1) @ v.double()).transpose(1, 2).reshape(B, Q, HEADS * 64)
    sdpa = F.scaled_dot_product_attention(qh.to(gpu_device), k.to(gpu_device), v.to(gpu_device), scale=scale)
    sdpa = sdpa.transpose(1, 2).reshape(B, Q, HEADS * 64).double().cpu()
    out = torch.full((B + 2, Q, HEADS * 64), SENTINEL, dtype=torch.float32, device=gpu_device)
    got = ops.qformer_cross_attention(q.to(gpu_device), blocks.to(gpu_device), T, HEADS, k0, v0, scale, out=out)
    torch.cuda.synchronize()
    got = got.cpu()
    assert not bool(torch.isnan(got).any())
    assert bool((got[B:] == SENTINEL).all())                                      # rows beyond B are untouched
    err, err_lib = float((got[:B].double() - ref).abs().max()), float((sdpa - ref).abs().max())
    print(f"cross-attention B={B} T={T} Q={Q} q_scale={q_scale}: err={err:.3e} sdpa={err_lib:.3e} max|ref|={float(ref.abs().max()):.3e} "
          f"max|score|={float(s64.abs().max()):.1f}")
    assert err <= 2.0 * err_lib + 1e-7 * float(ref.abs().max()), (B, T, Q, err, err_lib)
    return float(s64.abs().max())


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("T", [1, 33, 257])
@pytest.mark.parametrize("Q", [1, 32])
def test_cross_attention_against_f64(gpu_device, B, T, Q):
    _check(gpu_device, B, T, Q, seed=B * 1000 + T * 10 + Q)


@pytest.mark.parametrize("T", [50, 64])
def test_cross_attention_key_remainders(gpu_device, T):
    _check(gpu_device, 3, T, 7, seed=T)


def test_cross_attention_large_scores(gpu_device):
    """Scores of about +-30 (queries scaled up): the max-subtracted softmax neither overflows nor loses the small terms."""
    top = _check(gpu_device, 9, 257, 32, seed=5, q_scale=6.0)
    assert 25.0 <= top <= 60.0, top


def test_cross_attention_rejects_other_geometries(gpu_device):
    from vlfm_amd import _lib

    q = torch.zeros(1, 40, 64, dtype=torch.float32, device=gpu_device)
    kv = torch.zeros(2, 300, 64, dtype=torch.float32, device=gpu_device)
    L = _lib.lib()
    args = (q.data_ptr(), kv.data_ptr(), q.data_ptr())
    assert L.vlfm_qformer_cross_attention_f32(*args, 1, 257, 33, 1, 0, 1, 300, 0.125, None) == _lib.VLFM_ERR_INVALID   # 33 queries
    assert L.vlfm_qformer_cross_attention_f32(*args, 1, 258, 32, 1, 0, 1, 300, 0.125, None) == _lib.VLFM_ERR_INVALID   # 258 tokens
    assert L.vlfm_qformer_cross_attention_f32(*args, 2, 257, 32, 1, 0, 1, 300, 0.125, None) == _lib.VLFM_ERR_INVALID   # rows beyond m_total
