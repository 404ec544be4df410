"""-m gpu: vlfm_window_attention_masked_f32 (csrc/sam_ops.hip; TinyViT's and Swin's window attention) against the f64 reference of
tests/detect_ref.py, with and without the shifted-window mask, at every instantiation the dispatch has -- the vector kernel with 64 /
128 / 256 threads, the MFMA kernel with 2 (33-64 tokens) and 7 (193-224 tokens) key tiles -- and on both sides of every dispatch edge.
Bound: |err| <= 2e-5 * max(1, |ref|) per element, the bar tests/test_sam_ops_gpu.py grants the kernel against the library, here
against f64; the library's own f32 attention on the same inputs is printed next to it."""
import pytest
import torch
import torch.nn.functional as F

import detect_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
TOL = 2e-5
PER_IMAGE = 3
WINDOWS = 6            # two images of three window positions: win % windows_per_image matters


def _launch(qkv, bias_t, mask_t, per_image, heads, scale, windows=None, tokens=None):
    """The C entry point on an output over-allocated by one window of SENTINEL.  Returns (status, whole buffer)."""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    nw, n, _ = qkv.shape
    out = torch.full((nw + 1, n, heads * 32), SENTINEL, dtype=torch.float32, device=qkv.device)
    rc = _lib.lib().vlfm_window_attention_masked_f32(qkv.data_ptr(), bias_t.data_ptr(), mask_t.data_ptr() if mask_t is not None else None,
                                                     per_image, out.data_ptr(), nw if windows is None else windows,
                                                     n if tokens is None else tokens, heads, float(scale), ops._stream())
    torch.cuda.synchronize()
    return rc, out


def _check(dev, tokens, heads, seed, masked, q_scale=1.0):
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(seed)
    scale = 32 ** -0.5
    qkv = torch.randn(WINDOWS, tokens, heads * 96, generator=g) * 1.3
    qkv.view(WINDOWS, tokens, heads, 3, 32)[:, :, :, 0] *= q_scale
    bias = torch.randn(heads, tokens, tokens, generator=g) * 2.0                     # NOT symmetric: the transposition matters
    mask = R.swin_like_mask(tokens, PER_IMAGE, g) if masked else None
    if masked and tokens > 2:
        assert not torch.equal(mask, mask.transpose(1, 2))                           # a transposition error cannot hide
        assert bool((mask.diagonal(dim1=1, dim2=2) == 0).all())                      # Swin's guarantee: own key visible
    ref, scores = R.window_attention_f64(qkv, bias, mask, heads, scale)
    q, k, v = (t.transpose(1, 2).to(dev) for t in qkv.view(WINDOWS, tokens, heads, 96).split(32, dim=3))
    add = bias[None].expand(WINDOWS, -1, -1, -1)
    if masked:
        add = add + mask.repeat(WINDOWS // PER_IMAGE, 1, 1)[:, None]
    lib = F.scaled_dot_product_attention(q, k, v, attn_mask=add.contiguous().to(dev), scale=scale)
    lib = lib.transpose(1, 2).reshape(WINDOWS, tokens, heads * 32).double().cpu()
    bias_t = bias.transpose(1, 2).contiguous().to(dev)
    mask_t = mask.transpose(1, 2).contiguous().to(dev) if masked else None
    got = ops.window_attention(qkv.to(dev), bias_t, heads, scale, mask_t)
    rc, buf = _launch(qkv.to(dev), bias_t, mask_t, PER_IMAGE if masked else 1, heads, scale)
    assert rc == _lib.VLFM_OK
    assert torch.equal(buf[:WINDOWS], got) and bool((buf[WINDOWS:] == SENTINEL).all())   # the rows beyond stay untouched
    got = got.double().cpu()
    assert not bool(torch.isnan(got).any())
    denom = ref.abs().clamp(min=1.0)
    err, err_lib = float(((got - ref).abs() / denom).max()), float(((lib - ref).abs() / denom).max())
    top = float((scores if mask is None else scores - mask.double().repeat(WINDOWS // PER_IMAGE, 1, 1)[:, None]).abs().max())
    print(f"window attention tokens={tokens} heads={heads} masked={masked} q_scale={q_scale}: err={err:.3e} library f32={err_lib:.3e} "
          f"bound={TOL:.0e} max|ref|={float(ref.abs().max()):.2f} max|score|={top:.1f}")
    assert err <= TOL, (tokens, heads, masked, err, err_lib)
    return top


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("tokens", [1, 32, 33, 49, 64, 65, 128, 129, 192, 193, 196, 224, 225, 256])
def test_window_attention_against_f64(gpu_device, tokens, heads):
    _check(gpu_device, tokens, heads, seed=tokens * 10 + heads, masked=False)
    _check(gpu_device, tokens, heads, seed=tokens * 10 + heads + 5, masked=True)


@pytest.mark.parametrize("tokens", [49, 70, 196])
def test_window_attention_large_scores(gpu_device, tokens):
    """Scores of about +-40 (queries scaled up), one case per kernel family (MFMA with 2 key tiles, vector, MFMA with 7): the
    max-subtracted online softmax neither overflows nor loses the small terms; the same with the mask on top."""
    top = _check(gpu_device, tokens, 3, seed=tokens, masked=False, q_scale=5.0)
    assert 25.0 <= top <= 60.0, top
    top = _check(gpu_device, tokens, 3, seed=tokens + 1, masked=True, q_scale=5.0)
    assert 25.0 <= top <= 60.0, top


def test_window_attention_refusals(gpu_device):
    from vlfm_amd import _lib

    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(2, 256, 96, generator=g).to(gpu_device)
    bias_t = torch.zeros(1, 256, 256, device=gpu_device)
    for kw in (dict(tokens=0), dict(tokens=257)):
        rc, buf = _launch(qkv, bias_t, None, 1, 1, 0.1, **kw)
        assert rc == _lib.VLFM_ERR_INVALID and bool((buf == SENTINEL).all()), kw
    rc, buf = _launch(qkv, bias_t, bias_t, 0, 1, 0.1)                               # windows_per_image = 0
    assert rc == _lib.VLFM_ERR_INVALID and bool((buf == SENTINEL).all())
    rc, buf = _launch(qkv, bias_t, None, 1, 1, 0.1, windows=0)                      # nothing to do: OK, nothing touched
    assert rc == _lib.VLFM_OK and bool((buf == SENTINEL).all())
