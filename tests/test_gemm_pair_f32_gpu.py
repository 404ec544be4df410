"""-m gpu: the one-pass two-piece K/V projection (csrc/gemm_f16.hip, epilogue EPI_PAIR_F32; ops.linear_pair_f32) against f64, with the
two-launch path it replaces (blip2itm._split_gemm, n_pieces=2) as the yardstick for "f32-grade": err_new <= 2 err_old + 1e-6 max|ref|
on the same inputs.  The block-major layout is checked exactly by re-indexing (through ops.linear_pair_f32's own description of it),
guard values around the result must survive, and the 30-repeat bitwise screen of tests/test_gemm_f16_gpu.py covers the counted waits
around the new epilogue."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N_out, K): one block + one K-tile + M tail | odd block count: a half-filled last tile | two images at the real K, rows cross a
# tile boundary | four images, five blocks
SHAPES = [(130, 64, 64), (257, 192, 128), (514, 1536, 1408), (1028, 320, 1408)]
GUARD = 4096
SENTINEL = -777.25


def _problem(shape, device):
    from vlfm_amd.vlm import blip2itm

    M, N, K = shape
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x16 = (torch.randn(M, K, generator=g) * 1.5).half().to(device)
    w = (torch.randn(N, K, generator=g) * 0.05).to(device)
    bias = torch.randn(N, generator=g).to(device)
    w1, w2, w3 = blip2itm._exact_split3(w)
    return x16, (w1, w2, w3), bias


def _guarded(nblk, M, device):
    flat = torch.full((2 * GUARD + nblk * M * 64,), SENTINEL, dtype=torch.float32, device=device)
    return flat, flat[GUARD:GUARD + nblk * M * 64].view(nblk, M, 64)


@pytest.mark.parametrize("shape", SHAPES)
def test_pair_gemm_is_f32_grade_and_block_major(gpu_device, shape):
    from vlfm_amd.vlm import blip2itm, ops

    M, N, K = shape
    x16, (w1, w2, w3), bias = _problem(shape, gpu_device)
    ref = x16.double() @ (w1.double() + w2.double() / 2048).t() + bias.double()
    old = blip2itm._split_gemm(x16, (w1.t(), w2.t(), w3.t()), bias, n_pieces=2).double()
    flat, out = _guarded(N // 64, M, gpu_device)
    got = ops.linear_pair_f32(x16, ops.interleave_pair_weights(w1, w2), bias, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == (N // 64, M, 64)
    assert not bool(torch.isnan(got).any())
    # block-major -> row-major by re-indexing: element (m, c) lives at [c // 64, m, c % 64]
    rows = got.permute(1, 0, 2).reshape(M, N)
    m_idx = torch.arange(M, device=gpu_device)[:, None].expand(M, N)
    c_idx = torch.arange(N, device=gpu_device)[None, :].expand(M, N)
    assert torch.equal(got[c_idx // 64, m_idx, c_idx % 64], rows)
    scale = float(ref.abs().max())
    err_new, err_old = float((rows.double() - ref).abs().max()), float((old - ref).abs().max())
    print(f"pair GEMM {shape}: err_new={err_new:.3e} err_old={err_old:.3e} max|ref|={scale:.3e}")
    assert err_new <= 2.0 * err_old + 1e-6 * scale, (shape, err_new, err_old, scale)
    # nothing outside [N / 64][M][64] is written
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + (N // 64) * M * 64:] == SENTINEL).all())


def test_pair_gemm_without_bias_and_fresh_output(gpu_device):
    from vlfm_amd.vlm import ops

    shape = (257, 192, 128)
    x16, (w1, w2, _), _ = _problem(shape, gpu_device)
    got = ops.linear_pair_f32(x16, ops.interleave_pair_weights(w1, w2)).permute(1, 0, 2).reshape(shape[0], shape[1])
    ref = x16.double() @ (w1.double() + w2.double() / 2048).t()
    assert float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())   # f32 accumulation of 128 exact products


def test_pair_gemm_rejects_unsupported_shapes(gpu_device):
    from vlfm_amd import _lib

    x = torch.zeros(64, 96, dtype=torch.float16, device=gpu_device)
    w = torch.zeros(128, 96, dtype=torch.float16, device=gpu_device)
    o = torch.zeros(1, 64, 64, dtype=torch.float32, device=gpu_device)
    L = _lib.lib()
    assert L.vlfm_gemm_f16_pair_f32_nt(x.data_ptr(), w.data_ptr(), None, o.data_ptr(), 64, 64, 96, None) == _lib.VLFM_ERR_INVALID    # K % 64
    assert L.vlfm_gemm_f16_pair_f32_nt(x.data_ptr(), w.data_ptr(), None, o.data_ptr(), 64, 32, 64, None) == _lib.VLFM_ERR_INVALID    # N_out % 64


def test_pair_gemm_is_deterministic_under_repetition(gpu_device):
    """Race screen (the convention of tests/test_gemm_f16_gpu.py) at ONE tile per workgroup: (1028, 1536, 1408) is 5 x 12 = 60 tiles on
    a grid of 60, so it covers the counted waits of one tile's K loop and the epilogue's re-request of its own K-tile 0 -- 30 launches,
    bitwise equal to the first.  No workgroup has a next tile here: the prefetch that is read and the stores that drain under the next
    tile's first phases are screened on a 780-tile schedule in tests/test_qformer_batch_scale_gpu.py."""
    from vlfm_amd.vlm import ops

    shape = (1028, 1536, 1408)
    x16, (w1, w2, _), bias = _problem(shape, gpu_device)
    wp = ops.interleave_pair_weights(w1, w2)
    first = ops.linear_pair_f32(x16, wp, bias).clone()
    ref = x16.double() @ (w1.double() + w2.double() / 2048).t() + bias.double()
    rows = first.permute(1, 0, 2).reshape(shape[0], shape[1]).double()
    assert float((rows - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    out = torch.empty_like(first)
    for rep in range(30):
        out.fill_(float("nan"))
        ops.linear_pair_f32(x16, wp, bias, out=out)
        assert torch.equal(out, first), rep
