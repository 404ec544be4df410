"""-m gpu: the Q-Former's two persistent kernels on the schedules the product runs them on -- Blip2ITCModel.query_features takes the
fused cross path from 32 images, i.e. about 9 GEMM tiles and 2-12 attention items per workgroup -- where tests/test_gemm_pair_f32_gpu.py
and tests/test_qformer_attention_gpu.py stay at one work item per workgroup:
  * csrc/gemm_f16.hip, epilogue EPI_PAIR_F32 (ops.linear_pair_f32): a next tile behind the epilogue (its K-tile 0 requested before
    the stores, the stores draining under its first phases), the n-half items of a ragged last round, the half item of the half-empty
    last n-tile in which no wavefront is active, a plain second round on part of the grid, three rounds at the real K;
  * csrc/qformer_attention.hip: the ``if (more)`` half of the kernel -- a tile of the next item overwriting the tile just consumed, the
    query row reloaded under the current item, the merge area reused behind one barrier -- with both outcomes of ``more``, fewer than
    32 queries, every kind of key remainder and chains of three items.
The conventions are those of tests/test_vlm_batch_scale_gpu.py: inputs built on the GPU from a seeded generator, float64 references
evaluated on the GPU in chunks, results written into sentinel- / NaN-filled buffers with guard space around them.  Every test first
ASSERTS the schedule it is about, from the library's own description of the GEMM's walk (vlfm_gemm_f16_work_items /
vlfm_gemm_f16_tile_order) and from a restatement of the attention launcher's, with shapes derived from the device's CU count (the
figures in the comments are those of 256 CUs).  Bounds: those of the two one-item test files, relative to a yardstick evaluated on
the same inputs.  A result must also not depend on the schedule at all: the same rows / images computed alone, one item per workgroup,
give identical bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 4096


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7      # the launchers' grid: a multiple of 8 workgroups


def _ceil_div(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ pair GEMM
N_OUT_REAL, K_REAL, M_STEADY = 1536, 1408, 64 * 257


def _pair_shape(case, cus):
    """(M, N_out, K) of a schedule case: the M at which a grid of ``cus`` workgroups gets that schedule (256 CUs: the figure in the
    comment).  M is never a multiple of the tile: the last m-tile has a row tail."""
    if case in ("split", "split_one_ktile"):      # one round + cus / 8 leftover tiles, run as n-halves: (6000, 1536, 128 | 64)
        return _ceil_div(cus + cus // 8, 12) * 256 - 144, 1536, 128 if case == "split" else 64
    if case == "odd_blocks":                      # 25 blocks: a half-filled last n-tile, whose tiles end the list: (5200, 1600, 128)
        return _ceil_div(cus + cus // 16, 13) * 256 - 176, 1600, 128
    if case == "no_split":                        # more than half a round left over: (8224, 1536, 128)
        return (_ceil_div(3 * cus // 2, 12) + 1) * 256 - 224, 1536, 128
    assert case == "steady"                       # 64 images at the real sizes: (16448, 1536, 1408)
    return M_STEADY, N_OUT_REAL, K_REAL


PAIR_CASES = ["split", "split_one_ktile", "odd_blocks", "no_split", "steady"]


def _walk(m, n, grid):
    """(items [n, 2] = (list position, n-half or -1), order [tiles, 2] = (m-tile, n-tile) of a list position) for ``grid`` workgroups;
    workgroup w runs items w, w + grid, ..."""
    assert grid == min(grid, _ceil_div(m, 256) * _ceil_div(n, 256))
    return gemm_ref.work_items(m, n, grid), gemm_ref.tile_order(m, n)


def _assert_pair_schedule(case, shape, cus):
    """The schedule the case is named after holds on this device; returns the m-tiles whose item in the LAST n-tile is an n-half
    item (odd_blocks; empty otherwise)."""
    M, n_out, K = shape
    N = 2 * n_out
    tiles_m, tiles_n = _ceil_div(M, 256), _ceil_div(N, 256)
    tiles = tiles_m * tiles_n
    grid = min(cus, tiles)
    items, order = _walk(M, N, grid)
    per_wg = np.bincount(np.arange(len(items)) % grid, minlength=grid)
    half = items[:, 1]
    assert tiles > grid == cus, (tiles, grid)                       # somebody has a next tile behind its epilogue
    assert per_wg.max() >= 2
    if cus == 256:
        assert (M, n_out, K) == {"split": (6000, 1536, 128), "split_one_ktile": (6000, 1536, 64), "odd_blocks": (5200, 1600, 128),
                                 "no_split": (8224, 1536, 128), "steady": (16448, 1536, 1408)}[case]
    split_m = np.zeros(0, np.int64)
    if case in ("split", "split_one_ktile"):
        assert (half == 0).any() and (half == 1).any()              # the leftover tiles run as n-half items ...
        assert (half[:grid] < 0).all()                              # ... behind a round of whole tiles
        assert K // 64 == (2 if case == "split" else 1)             # (one K-tile: the NT == 1 branch of the prologue)
        if cus == 256:
            assert tiles == 288 and int((half >= 0).sum()) == 64
    elif case == "odd_blocks":
        assert n_out // 64 % 2 == 1 and N - (tiles_n - 1) * 256 == 128          # the last n-tile holds ONE block
        in_last = order[items[:, 0], 1] == tiles_n - 1
        dead = in_last & (half == 1)                                # n-columns [128, 256) of that tile: beyond N, nobody is active
        live = in_last & (half == 0)
        assert dead.any() and int(dead.sum()) == int(live.sum())
        split_m = np.sort(order[items[live, 0], 0]).astype(np.int64)
        assert np.array_equal(split_m, np.sort(order[items[dead, 0], 0]))
        if cus == 256:
            assert tiles == 273 and int((half >= 0).sum()) == 34
    elif case == "no_split":
        assert (half < 0).all() and len(items) == tiles             # no half items: a plain second round ...
        assert per_wg.max() == 2 and per_wg.min() == 1              # ... on only part of the grid
        assert 2 * (tiles - grid) > grid
        if cus == 256:
            assert tiles == 396
    else:
        assert per_wg.max() >= 3                                    # three epilogues with a next tile behind them
        if cus == 256:
            assert tiles == 780 and int((half >= 0).sum()) == 24 and per_wg.min() == 3
    return split_m


def _pair_problem(shape, device):
    """tests/test_gemm_pair_f32_gpu.py's _problem, built on the GPU: nothing in it is symmetric, so a transpose cannot hide"""
    from vlfm_amd.vlm import blip2itm

    M, N, K = shape
    g = torch.Generator(device=device).manual_seed(M * 7 + N * 3 + K)
    x16 = (torch.randn(M, K, generator=g, device=device) * 1.5).half()
    w = torch.randn(N, K, generator=g, device=device) * 0.05
    bias = torch.randn(N, generator=g, device=device)
    w1, w2, w3 = blip2itm._exact_split3(w)
    return x16, (w1, w2, w3), bias


def _pair_ref(x16, w1, w2, bias):
    """x (W1 + 2^-11 W2)^T + bias in float64, 4096 rows at a time"""
    wd = (w1.double() + w2.double() / 2048).t().contiguous()
    ref = torch.empty(x16.shape[0], w1.shape[0], dtype=torch.float64, device=x16.device)
    for m0 in range(0, x16.shape[0], 4096):
        torch.matmul(x16[m0:m0 + 4096].double(), wd, out=ref[m0:m0 + 4096])
    if bias is not None:
        ref += bias.double()
    return ref


def _pair_guarded(nblk, M, device):
    """[nblk][M][64] inside a sentinel-filled buffer: GUARD floats in front, one whole BLOCK behind (where an item of the empty half
    of the last n-tile would put its rows, whichever m-tile it has)"""
    size = nblk * M * 64
    flat = torch.full((GUARD + size + M * 64 + GUARD,), SENTINEL, dtype=torch.float32, device=device)
    return flat, flat[GUARD:GUARD + size].view(nblk, M, 64)


def _pair_run_and_check(shape, x16, pieces, bias, ref, label):
    """one launch into a guarded buffer: layout, guards, no fill value left, and the bound of tests/test_gemm_pair_f32_gpu.py
    (err_new <= 2 err_old + 1e-6 max|ref|, err_old from the two-launch path on the same inputs); returns the block-major result"""
    from vlfm_amd.vlm import blip2itm, ops

    M, N, K = shape
    w1, w2, w3 = pieces
    device = x16.device
    zero = torch.zeros(N, dtype=torch.float32, device=device)
    old = blip2itm._split_gemm(x16, (w1.t(), w2.t(), w3.t()), bias if bias is not None else zero, n_pieces=2)
    err_old = float((old.double() - ref).abs().max())
    del old
    flat, out = _pair_guarded(N // 64, M, device)
    got = ops.linear_pair_f32(x16, ops.interleave_pair_weights(w1, w2), bias, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == (N // 64, M, 64)
    # nothing outside [N / 64][M][64] is written, and nothing inside it is left out
    assert bool((flat[:GUARD] == SENTINEL).all()), "the guard in front of the result was written"
    assert bool((flat[GUARD + out.numel():] == SENTINEL).all()), "the guard block behind the result was written"
    left = got == SENTINEL
    assert not bool(left.any()), ("never written (block, row, channel)", left.nonzero()[0].tolist())
    assert not bool(torch.isnan(got).any())
    # block-major -> row-major by re-indexing: element (m, c) lives at [c // 64, m, c % 64]
    rows = got.permute(1, 0, 2).reshape(M, N)
    c_idx = torch.arange(N, device=device)[None, :]
    for m0 in range(0, M, 4096):
        m_idx = torch.arange(m0, min(m0 + 4096, M), device=device)[:, None]
        assert torch.equal(got[(c_idx // 64).expand(len(m_idx), N), m_idx.expand(len(m_idx), N), (c_idx % 64).expand(len(m_idx), N)],
                           rows[m0:m0 + 4096])
    scale = float(ref.abs().max())
    diff = (rows.double() - ref).abs()
    err_new = float(diff.max())
    print(f"pair GEMM {label} {shape}: err_new={err_new:.3e} err_old={err_old:.3e} max|ref|={scale:.3e}")
    m_bad, c_bad = divmod(int(diff.argmax()), N)
    assert err_new <= 2.0 * err_old + 1e-6 * scale, (shape, err_new, err_old, scale, "worst (row, channel)", (m_bad, c_bad),
                                                      "(m-tile, n-tile)", (m_bad // 256, 2 * c_bad // 256))
    return got


@pytest.fixture(scope="module")
def steady_pair(gpu_device):
    """the 64-image problem at the real sizes, its float64 reference and its first result: shared by the three tests that use it"""
    shape = (M_STEADY, N_OUT_REAL, K_REAL)
    x16, (w1, w2, w3), bias = _pair_problem(shape, gpu_device)
    hold = {"shape": shape, "x16": x16, "pieces": (w1, w2, w3), "bias": bias, "ref": _pair_ref(x16, w1, w2, bias), "first": None}
    yield hold
    hold.clear()


def _steady_first(hold):
    """the checked first result of the steady problem (read-only for every user)"""
    if hold["first"] is None:
        _assert_pair_schedule("steady", hold["shape"], _cus())
        got = _pair_run_and_check(hold["shape"], hold["x16"], hold["pieces"], hold["bias"], hold["ref"], "steady")
        hold["first"] = got.clone()
    return hold["first"]


@pytest.mark.parametrize("case", PAIR_CASES)
def test_pair_gemm_multi_round_schedules_against_f64(gpu_device, case, request):
    """288 tiles = a round + 32 tiles as 64 n-half items | the same with one K-tile | 273 tiles of which the last 17, all in the
    half-filled last n-tile, are split: 17 items with nobody active | 396 tiles: no split, a second round on 140 workgroups | 780
    tiles at K = 1408: three rounds + 12 split tiles."""
    cus = _cus()
    if case == "steady":
        _steady_first(request.getfixturevalue("steady_pair"))
        return
    shape = _pair_shape(case, cus)
    split_m = _assert_pair_schedule(case, shape, cus)
    x16, (w1, w2, w3), bias = _pair_problem(shape, gpu_device)
    ref = _pair_ref(x16, w1, w2, bias)
    got = _pair_run_and_check(shape, x16, (w1, w2, w3), bias, ref, case)
    if case == "odd_blocks":
        # the rows of the last block that only an n-half item (half 0; its half 1 has nobody active) can have written
        M, last = shape[0], shape[1] // 64 - 1
        rows = (split_m[:, None] * 256 + np.arange(256)[None, :]).reshape(-1)
        rows = torch.from_numpy(rows[rows < M]).to(gpu_device)
        assert len(rows) > 0
        blk = got[last][rows]
        assert not bool((blk == SENTINEL).any()) and bool(torch.isfinite(blk).all())
        err_rows = float((blk.double() - ref[rows][:, last * 64:]).abs().max())
        print(f"pair GEMM {case}: last block, the {len(rows)} rows of its n-half items: err={err_rows:.3e}")


def test_pair_gemm_multi_round_without_bias(gpu_device):
    """the split schedule (288 tiles) with a null bias pointer: the epilogue's zero bias must hold for every tile of a workgroup"""
    cus = _cus()
    shape = _pair_shape("split", cus)
    _assert_pair_schedule("split", shape, cus)
    x16, (w1, w2, w3), _ = _pair_problem(shape, gpu_device)
    _pair_run_and_check(shape, x16, (w1, w2, w3), None, _pair_ref(x16, w1, w2, None), "split, no bias")


def test_pair_gemm_result_is_independent_of_the_schedule(gpu_device, steady_pair):
    """Rows [0, 1028) of the 780-tile call against the same rows computed alone -- 60 tiles, one per workgroup: identical bits.  An
    output element is one k-ordered accumulation; where its tile runs and what ran before it in that workgroup must not show."""
    from vlfm_amd.vlm import ops

    cus = _cus()
    first = _steady_first(steady_pair)
    M, n_out, K = steady_pair["shape"]
    rows = 4 * 257
    small_tiles = _ceil_div(rows, 256) * _ceil_div(2 * n_out, 256)
    assert small_tiles <= cus                                        # one tile per workgroup ...
    items, _ = _walk(rows, 2 * n_out, small_tiles)
    assert len(items) == small_tiles and (items[:, 1] < 0).all()     # ... whole
    w1, w2, _ = steady_pair["pieces"]
    flat, out = _pair_guarded(n_out // 64, rows, gpu_device)
    ops.linear_pair_f32(steady_pair["x16"][:rows].contiguous(), ops.interleave_pair_weights(w1, w2), steady_pair["bias"], out=out)
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + out.numel():] == SENTINEL).all())
    diff = first[:, :rows].contiguous().view(torch.int32) != out.view(torch.int32)
    print(f"pair GEMM schedule independence: {int(diff.sum())} of {diff.numel()} elements differ between the {M}-row and the {rows}-row call")
    assert not bool(diff.any()), ("first differing (block, row, channel)", diff.nonzero()[0].tolist())


def test_pair_gemm_multi_round_is_deterministic_under_repetition(gpu_device, steady_pair):
    """Race screen (the convention of tests/test_gemm_f16_gpu.py) on a schedule that HAS a next tile: 780 tiles, three per workgroup,
    the next tile's K-tile 0 in flight across every epilogue and its stores draining under the next tile's first phases.  A wrong
    wait count is a RARE wrong tile -- 30 launches, bitwise equal to the first."""
    from vlfm_amd.vlm import ops

    first = _steady_first(steady_pair)
    M, n_out, K = steady_pair["shape"]
    ref = steady_pair["ref"]
    err = float((first.permute(1, 0, 2).reshape(M, n_out).double() - ref).abs().max())
    print(f"pair GEMM race screen {steady_pair['shape']}: err={err:.3e} max|ref|={float(ref.abs().max()):.3e}")
    assert err <= 1e-5 * float(ref.abs().max())
    w1, w2, _ = steady_pair["pieces"]
    wp = ops.interleave_pair_weights(w1, w2)
    out = torch.empty_like(first)
    for rep in range(30):
        out.fill_(float("nan"))
        ops.linear_pair_f32(steady_pair["x16"], wp, steady_pair["bias"], out=out)
        assert torch.equal(out, first), rep


# ------------------------------------------------------------------------------------------------ cross-attention
HEADS = 12
ATT_SENTINEL = 12345.5
K0, V0 = 2, 3 + HEADS          # K heads at blocks [2, 14), V heads at [15, 27), unrelated blocks around them


def _attention_walks(B, cus):
    """vlfm_qformer_cross_attention_f32's persistent walk, restated: (items, grid, per workgroup the list of (item, more)), where
    item w is head (w >> 3) % heads of image ((w >> 3) // heads) * 8 + (w & 7) and ``more`` says whether the kernel found a real item
    behind it.  A workgroup whose first item is an image beyond B returns at once: an empty list."""
    items = _ceil_div(B, 8) * 8 * HEADS
    grid = min(items, cus)
    image = lambda w: ((w >> 3) // HEADS) * 8 + (w & 7)  # noqa: E731
    walks = []
    for wg in range(grid):
        walk, w = [], wg
        while image(w) < B:
            more = image(w + grid) < B
            walk.append((w, more))
            if not more:
                break
            w += grid
        walks.append(walk)
    assert sorted(w for walk in walks for w, _ in walk) == [w for w in range(items) if image(w) < B]      # every real item once
    return items, grid, walks


def _attention_batch(case, cus):
    """B of a schedule case for ``cus`` workgroups, cus / 8 per XCD (256 CUs: the figure in the comment)"""
    full = (cus // 8) // HEADS                    # images whose heads fit one round of an XCD's workgroups: 2
    if case == "second_item":                     # XCD 0 alone has one image more than a round holds: 17
        return 8 * full + 1
    if case == "ragged_batch":                    # XCDs 0-3 have that image, XCDs 4-7 do not: 20
        return 8 * full + 4
    if case == "few_queries":                     # every XCD has a second-round image, XCD 0 two: 25
        return 8 * (full + 1) + 1
    assert case == "three_items"                  # three items for every workgroup: 64
    return 8 * _ceil_div(3 * (cus // 8), HEADS)


def _assert_attention_schedule(case, B, cus):
    items, grid, walks = _attention_walks(B, cus)
    per = np.array([len(w) for w in walks])
    first_more = [w[0][1] for w in walks if w]
    assert grid == cus < items, (grid, items)
    assert per.max() >= 2 and any(first_more)                       # somebody runs ``if (more)``
    if case == "second_item":
        assert per.max() == 2
        if cus == 256:
            assert (B, items) == (17, 288) and int((per == 2).sum()) == 4 and all(wg & 7 == 0 for wg in np.nonzero(per == 2)[0])
    elif case == "ragged_batch":
        assert B % 8 != 0
        # both outcomes of ``more`` on a workgroup that has walked one item, the false one on an item INSIDE the list (nb >= B)
        assert any(w[0][1] for w in walks if w)
        assert any(not w[0][1] and w[0][0] + grid < items for w in walks if w)
        if cus == 256:
            assert (B, items) == (20, 288)
            assert {wg & 7 for wg in np.nonzero(per == 2)[0]} == {0, 1, 2, 3} and int((per == 2).sum()) == 16
    elif case == "few_queries":
        if cus == 256:
            assert (B, items) == (25, 384) and int((per == 2).sum()) == 16 + 7 * 4
    else:
        assert per.min() >= 3                                       # a prefetch issued during an item that was itself prefetched
        if cus == 256:
            assert (B, items) == (64, 768) and (per == 3).all()
    return items


def _attention_case(B, T, Q, seed, device, q_scale=1.0):
    """tests/test_qformer_attention_gpu.py's _case on the GPU: q [B, Q, H * 64] and the block-major K / V tensor [2 H + 4, B * T, 64];
    image b is rows [b T, (b + 1) T) of every block"""
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randn(B, Q, HEADS * 64, generator=g, device=device) * q_scale
    blocks = torch.randn(2 * HEADS + 4, B * T, 64, generator=g, device=device)
    return q, blocks


def _heads_of(blocks, block0, B, T, b0, b1):
    return blocks[block0:block0 + HEADS].view(HEADS, B, T, 64)[:, b0:b1].permute(1, 0, 2, 3)      # [b, H, T, 64]


def _attention_into(q, blocks, T, n_guard=2):
    from vlfm_amd.vlm import ops

    B, Q, _ = q.shape
    out = torch.full((B + n_guard, Q, HEADS * 64), ATT_SENTINEL, dtype=torch.float32, device=q.device)
    got = ops.qformer_cross_attention(q, blocks, T, HEADS, K0, V0, 0.125, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((out[B:] == ATT_SENTINEL).all()), "the guard images behind the last one were written"
    return out[:B]


def _attention_check(device, B, T, Q, seed, q_scale=1.0):
    """the yardstick and bound of tests/test_qformer_attention_gpu.py: err <= 2 err_sdpa + 1e-7 max|ref| against an f64 softmax
    attention (on the GPU, 16 images at a time), err_sdpa = F.scaled_dot_product_attention in f32 on the same tensors"""
    q, blocks = _attention_case(B, T, Q, seed, device, q_scale)
    got = _attention_into(q, blocks, T)
    assert not bool(torch.isnan(got).any())
    left = got == ATT_SENTINEL
    assert not bool(left.any()), ("never written (image, query, channel)", left.nonzero()[0].tolist())
    err, err_lib, ref_max, top, where = 0.0, 0.0, 0.0, 0.0, None
    for b0 in range(0, B, 16):
        b1 = min(b0 + 16, B)
        k, v = _heads_of(blocks, K0, B, T, b0, b1), _heads_of(blocks, V0, B, T, b0, b1)
        qh = q[b0:b1].view(b1 - b0, Q, HEADS, 64).transpose(1, 2)                       # [b, H, Q, 64]
        s64 = (qh.double() @ k.double().transpose(-1, -2)) * 0.125
        ref = (torch.softmax(s64, dim=-1) @ v.double()).transpose(1, 2).reshape(b1 - b0, Q, HEADS * 64)
        sdpa = F.scaled_dot_product_attention(qh, k, v, scale=0.125).transpose(1, 2).reshape(b1 - b0, Q, HEADS * 64)
        diff = (got[b0:b1].double() - ref).abs()
        if float(diff.max()) > err:
            i, rest = divmod(int(diff.argmax()), Q * HEADS * 64)
            err, where = float(diff.max()), (b0 + i, rest % (HEADS * 64) // 64)           # (image, head)
        err_lib = max(err_lib, float((sdpa.double() - ref).abs().max()))
        ref_max, top = max(ref_max, float(ref.abs().max())), max(top, float(s64.abs().max()))
    print(f"cross-attention B={B} T={T} Q={Q} q_scale={q_scale}: err={err:.3e} sdpa={err_lib:.3e} max|ref|={ref_max:.3e} "
          f"max|score|={top:.1f}")
    assert err <= 2.0 * err_lib + 1e-7 * ref_max, (B, T, Q, err, err_lib, "worst (image, head)", where)
    return top


@pytest.mark.parametrize("case,T,Q", [("second_item", 257, 32), ("ragged_batch", 257, 32), ("few_queries", 257, 7),
                                      ("three_items", 257, 32)])
def test_cross_attention_several_items_per_workgroup(gpu_device, case, T, Q):
    """B = 17: 288 items, the workgroups of XCD 0 that hold image 16's heads walk two -- the first ``if (more)`` | B = 20: in the
    second round XCDs 0-3 have a real next image, XCDs 4-7 have nb >= B | B = 25, 7 queries: min(col, Q - 1) in load_q and
    col < Q at the store while qn is reloaded for the next item | B = 64: 768 items, three per workgroup."""
    cus = _cus()
    B = _attention_batch(case, cus)
    _assert_attention_schedule(case, B, cus)
    _attention_check(gpu_device, B, T, Q, seed=B * 1000 + T * 10 + Q)


@pytest.mark.parametrize("T", [1, 33, 50, 64])
def test_cross_attention_key_remainders_on_a_multi_item_walk(gpu_device, T):
    """The key remainders with a next item behind them (issue_rows(..., left_ins) re-requests the remainder rows): no full tile --
    only wavefront 0 works, the others merge m = -inf --, one tile + one key on wavefront 1, an 18-key vector-ALU remainder, none."""
    cus = _cus()
    B = _attention_batch("ragged_batch", cus)
    _assert_attention_schedule("ragged_batch", B, cus)
    assert (T >> 5, T & 31) == {1: (0, 1), 33: (1, 1), 50: (1, 18), 64: (2, 0)}[T]
    _attention_check(gpu_device, B, T, 32, seed=7000 + T)


def test_cross_attention_large_scores_on_a_multi_item_walk(gpu_device):
    """test_cross_attention_large_scores (scores of about +-30) with second items: the running maximum and sum start afresh per item"""
    cus = _cus()
    B = _attention_batch("ragged_batch", cus)
    _assert_attention_schedule("ragged_batch", B, cus)
    top = _attention_check(gpu_device, B, 257, 32, seed=5, q_scale=6.0)
    assert 25.0 <= top <= 60.0, top


def test_cross_attention_item_result_is_independent_of_the_schedule(gpu_device):
    """Images 0-7 of the three-items-per-workgroup call against the same eight images as a call of their own (their rows copied out of
    every block: m_total = 8 * 257; 96 items, one per workgroup): identical bits; and the large call twice: identical bits."""
    cus = _cus()
    T, Q = 257, 32
    B = _attention_batch("three_items", cus)
    _assert_attention_schedule("three_items", B, cus)
    items8, grid8, walks8 = _attention_walks(8, cus)
    assert items8 == grid8 == 8 * HEADS and all(len(w) == 1 and not w[0][1] for w in walks8)      # one item per workgroup
    q, blocks = _attention_case(B, T, Q, 64257, gpu_device)
    big = [_attention_into(q, blocks, T) for _ in range(2)]
    assert not bool(torch.isnan(big[0]).any()) and not bool((big[0] == ATT_SENTINEL).any())
    diff = big[0].view(torch.int32) != big[1].view(torch.int32)
    assert not bool(diff.any()), ("two runs differ at (image, query, channel)", diff.nonzero()[0].tolist())
    blocks8 = blocks.view(-1, B, T, 64)[:, :8].reshape(-1, 8 * T, 64).contiguous()
    assert blocks8.shape[1] == 8 * T
    small = _attention_into(q[:8].contiguous(), blocks8, T)
    diff = big[0][:8].view(torch.int32) != small.view(torch.int32)
    print(f"cross-attention schedule independence: {int(diff.sum())} of {diff.numel()} elements differ between B={B} and B=8")
    assert not bool(diff.any()), ("first differing (image, query, channel)", diff.nonzero()[0].tolist())
