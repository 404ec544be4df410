"""vlfm_gemm_f16_nt / vlfm_gemm_f16_pair_f32_nt (csrc/gemm_f16.hip) against f64, bit for bit, on every path of the persistent schedule.

The operands are dyadic (tests/gemm_ref.py): every product and partial sum is exact in f32 in any order, so the f64 pre-activation is
the ONLY value a correct accumulator can hold and each epilogue has one right answer -- f16(pre) for bias / no bias,
f16(f16(pre) + r0) for accumulate (the kernel rounds the product before it adds the stream: pinned here), fl32(acc1 + fl32(bias +
2^-11 acc2)) for the pair epilogue -- compared as integers, -0 == +0.  A conversion that truncates, a second rounding, a bias added
behind the rounding, a K-slot dropped or read twice, a bias quad shifted by a lane, an addition in the other order: all show, which
the max-norm bounds of tests/test_gemm_f16_gpu.py cannot see.  bias + GELU must land between f16(gelu64(pre) - A) and
f16(gelu64(pre) + A) for |pre| <= 12, on f16(pre) above and on +-0 below; A is measured by tests/test_gemm_ref_cpu.py (3.14e-7).
Cases: one to four tiles with every kind of ragged edge and 1 - 96 K-tiles (prologue and tail wait counts); the persistent walk with
G = the launcher's grid: a leftover tile run as two n-halves, whole rounds, a leftover of exactly half a round (split) and one tile more
(a ragged round of whole tiles), three n-tiles with the half-empty ones listed last; each asserts through vlfm_gemm_f16_work_items /
vlfm_gemm_f16_tile_order that it has the structure it is named for.  Every output buffer holds a NaN pattern and a guard row.
Around them: f16 saturation, subnormal results, ties and NaN confinement on hand-made operands, a 10-launch repeat screen, and the
refusal of pointers that are not 16-byte aligned.  Subnormal f16 INPUTS are out of scope: what the matrix cores do with them is not
established."""
import numpy as np
import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

PATTERN = 0x7E5A                 # an f16 NaN: what output buffers hold before a launch
CHUNK = 16384                    # rows per f64 evaluation on the device
# (epilogue, with bias, operand set)
RUNS = [("bias", True, "wide"), ("bias", False, "wide"), ("bias_gelu", True, "wide"), ("bias_gelu", True, "narrow"),
        ("accumulate", True, "wide"), ("accumulate", False, "wide")]


def _grid(tiles):
    return min(torch.cuda.get_device_properties(0).multi_processor_count & ~7, tiles)       # the launcher's: one workgroup per CU


def _tiles(M, N):
    return (M + 255) // 256, (N + 255) // 256


def _launch(x, w, b, epi, r0):
    """One launch into a NaN-patterned buffer with a guard row behind it -> the [M, N] f16 view of the result."""
    from vlfm_amd.vlm import ops

    M, N = x.shape[0], w.shape[0]
    buf = torch.full((M + 1, N), PATTERN, dtype=torch.int16, device=x.device)
    out = buf.view(torch.float16)[:M]
    if epi == "accumulate":
        out.copy_(r0)
    got = ops.linear_f16(x, w, b, epi, out=out)
    assert got.data_ptr() == buf.data_ptr()
    assert bool((buf[M] == PATTERN).all()), "the guard row behind the last row was written"
    return out


def _check_on_device(got, x, w, b, r0, epi, A, what, shares_of=None):
    """The large cases: f64 on the device, CHUNK rows at a time (exact for these operands, as on the CPU); a chunk with a flagged
    element goes to the numpy check, which reports it.  ``shares_of`` (gemm_ref.shares_t or gelu_shares_t): the two shares of the
    whole pre-activation, from the reference alone, are returned."""
    wd = w.double().t()
    n_first = n_second = 0.0
    for m0 in range(0, x.shape[0], CHUNK):
        m1 = min(m0 + CHUNK, x.shape[0])
        pre = x[m0:m1].double() @ wd
        if b is not None:
            pre += b.double()
        assert bool((pre.float().double() == pre).all()) and float(pre.abs().max()) < 2 ** 15
        if shares_of is not None:
            i, t = shares_of(pre)
            n_first, n_second = n_first + i * (m1 - m0), n_second + t * (m1 - m0)
        if epi == "bias_gelu":
            bad = G.bad_gelu_t(got[m0:m1], pre, A)
        else:
            bad = G.bad_exact_t(got[m0:m1], G.rn16(pre) + r0[m0:m1].double() if epi == "accumulate" else pre)
        if bool(bad.any()):
            bits, p = got[m0:m1].contiguous().view(torch.int16).cpu().numpy(), pre.cpu().numpy()
            if epi == "bias_gelu":
                G.check_gelu(bits, p, A, what, row0=m0)
            else:
                G.check_exact(bits, G.want_accumulate(p, r0[m0:m1].cpu()) if epi == "accumulate" else p, what, row0=m0)
            raise AssertionError(f"{what}: {int(bad.sum())} outputs flagged on the device in rows from {m0}, none by the numpy check")
    print(f"{what}: all {got.numel()} outputs as expected (f64 on the device)")
    return n_first / x.shape[0], n_second / x.shape[0]


def run_case(M, N, K, dev, repeats=1, runs=RUNS):
    """Every epilogue of ``runs`` on the dyadic operands of (M, N, K): ``repeats`` launches each, bit-identical, the first one checked."""
    A = G.gelu_tolerance()[0]
    large = M * N > G.CPU_LIMIT
    sets = {}
    for name in ("wide", "narrow"):
        c = G.operands(M, N, K, narrow=name == "narrow")
        sets[name] = (c, [t.to(dev) if t is not None else None for t in (c.x, c.w, c.b, c.r0)])
    shares = gelu_shares = None
    for epi, with_bias, name in runs:
        c, (x, w, b, r0) = sets[name]
        what = f"({M}, {N}, {K}) {name} {epi}{'' if with_bias else ', no bias'}"
        outs = [_launch(x, w, b if with_bias else None, epi, r0) for _ in range(repeats)]
        for i, o in enumerate(outs[1:], 1):
            assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{what}: launch {i} differs from launch 0"
        got = outs[0]
        plain, narrow_gelu = (epi, with_bias) == ("bias", True), (epi, name) == ("bias_gelu", "narrow")
        if large:
            s = _check_on_device(got, x, w, b if with_bias else None, r0, epi, A, what,
                                 shares_of=G.shares_t if plain else G.gelu_shares_t if narrow_gelu else None)
            shares, gelu_shares = (s if plain else shares), (s if narrow_gelu else gelu_shares)
            continue
        pre = G.pre_cpu(c.x, c.w, c.b if with_bias else None)
        assert float(np.abs(pre).max()) < 2 ** 15
        bits = got.contiguous().view(torch.int16).cpu().numpy()
        if epi == "bias_gelu":
            gelu_shares = G.gelu_shares(pre) if narrow_gelu else gelu_shares
            G.check_gelu(bits, pre, A, what)
        elif epi == "accumulate":
            G.check_exact(bits, G.want_accumulate(pre, c.r0), what)
        else:
            shares = G.shares(pre) if plain else shares
            G.check_exact(bits, pre, what)
    # from the reference alone, on the CPU and on the device path alike (shares of the eight outputs of (1, 8, 64) say nothing)
    if shares is not None:
        print(f"({M}, {N}, {K}): {shares[0]:.1%} of the outputs need the f16 rounding, {shares[1]:.1%} are exact ties")
        assert M * N < 1024 or (shares[0] >= 0.05 and shares[1] >= 0.02)
    if gelu_shares is not None:
        print(f"({M}, {N}, {K}) narrow: {gelu_shares[0]:.1%} of the pre-activations in [-6, 6], {gelu_shares[1]:.1%} in [-6, -1]")
        assert M * N < 1024 or K > 192 or (gelu_shares[0] >= 0.30 and gelu_shares[1] >= 0.05)


# ------------------------------------------------------------------------------------------------ one to a few tiles
def _few_tiles(M, N, K):
    tm, tn = _tiles(M, N)
    assert tm * tn <= _grid(1 << 30)
    items = G.work_items(M, N, _grid(tm * tn))
    assert len(items) == tm * tn and (items[:, 1] == -1).all()          # one whole tile per workgroup
    return tm, tn, K // 64


def _s_smallest(M, N, K):
    assert _few_tiles(M, N, K) == (1, 1, 1)


def _s_one_ktile(M, N, K):
    assert _few_tiles(M, N, K) == (1, 1, 1) and (M, N) == (256, 256)


def _s_two_ktiles(M, N, K):
    assert _few_tiles(M, N, K) == (1, 1, 2) and M % 256 == 255 and N == 248


def _s_four_ragged(M, N, K):
    assert _few_tiles(M, N, K) == (2, 2, 3) and M % 256 == 1 and N % 256 == 8
    assert sorted(map(tuple, G.tile_order(M, N))) == [(0, 0), (0, 1), (1, 0), (1, 1)]


def _s_second_group_8(M, N, K):
    assert _few_tiles(M, N, K) == (2, 1, 4) and N - 128 == 8                # wavefronts 4-7 own columns 128..135 only


def _s_half_empty(M, N, K):
    assert _few_tiles(M, N, K) == (1, 2, 5) and N - 256 == 128              # wavefronts 4-7 of the last n-tile are inactive
    assert tuple(G.tile_order(M, N)[-1]) == (0, 1)


def _s_vit_half_tile(M, N, K):
    assert _few_tiles(M, N, K) == (2, 6, 22) and N - 5 * 256 == 128
    order = G.tile_order(M, N)
    assert (order[:, 1] == 5).sum() == 2 and set(order[-2:, 1]) == {5}       # the half tiles close the list of their XCDs


def _s_long_k(M, N, K):
    assert _few_tiles(M, N, K) == (1, 2, 96) and N - 256 == 8


FEW = [((1, 8, 64), _s_smallest), ((256, 256, 64), _s_one_ktile), ((255, 248, 128), _s_two_ktiles), ((257, 264, 192), _s_four_ragged),
       ((300, 136, 256), _s_second_group_8), ((130, 384, 320), _s_half_empty), ((257, 1408, 1408), _s_vit_half_tile),
       ((130, 264, 6144), _s_long_k)]


@pytest.mark.parametrize("shape,structure", FEW, ids=[f"{m}x{n}x{k}" for (m, n, k), _ in FEW])
def test_gemm_is_exact_on_few_tiles(gpu_device, shape, structure):
    structure(*shape)
    run_case(*shape, gpu_device)


# ------------------------------------------------------------------------------------------------ the persistent walk
def _walk_shape(name):
    """(M, N) of a persistent-walk case for this device's grid G, after asserting the structure it is named for."""
    g = _grid(1 << 30)
    assert g >= 16 and g % 8 == 0
    if name == "one_leftover_tile_as_two_halves":
        M, N = 256 * g + 1, 200
        items = G.work_items(M, N, g)
        assert len(items) == g + 2 and (items[:g, 1] == -1).all()
        assert [tuple(i) for i in items[g:]] == [(g, 0), (g, 1)]
    elif name == "three_whole_rounds":
        M, N = 256 * 3 * g, 256
        items = G.work_items(M, N, g)
        assert len(items) == 3 * g and (items[:, 1] == -1).all()
    elif name == "leftover_half_a_round_is_split":
        M, N = 256 * (2 * g + g // 2), 256
        items = G.work_items(M, N, g)
        assert len(items) == 3 * g and (items[:2 * g, 1] == -1).all() and sorted(items[2 * g:, 1]) == [0] * (g // 2) + [1] * (g // 2)
    elif name == "leftover_above_half_a_round_is_not":
        M, N = 256 * (2 * g + g // 2 + 1), 256
        items = G.work_items(M, N, g)
        assert len(items) == 2 * g + g // 2 + 1 and (items[:, 1] == -1).all()
    else:
        assert name == "three_n_tiles_ragged_groups"
        tm = (g + 17 + 2) // 3
        M, N = 256 * tm - 5, 520
        assert _tiles(M, N) == (tm, 3) and tm % 4 != 0 and 3 * tm > g and N - 512 == 8
        order = G.tile_order(M, N)
        assert sorted(map(tuple, order)) == [(m, n) for m in range(tm) for n in range(3)]
        for xcd in range(8):                                                # the 8-column tiles close every XCD's share of the list
            tn = order[xcd::8, 1]
            assert (tn[:int((tn < 2).sum())] < 2).all()
        assert len(G.work_items(M, N, g)) >= 3 * tm
    return M, N


WALK = ["one_leftover_tile_as_two_halves", "three_whole_rounds", "leftover_half_a_round_is_split", "leftover_above_half_a_round_is_not",
        "three_n_tiles_ragged_groups"]


@pytest.mark.parametrize("name", WALK)
def test_gemm_is_exact_on_the_persistent_walk(gpu_device, name):
    M, N = _walk_shape(name)
    run_case(M, N, 64, gpu_device)


def test_gemm_repeats_bit_for_bit(gpu_device):
    """The G + 1 tile case ten times per epilogue: workgroup 0 walks on to the split leftover tile while every other one is done --
    the prefetch that is read, the stores that drain under the next item.  The ten launches are compared with each other;
    test_gemm_is_exact_on_the_persistent_walk has checked this case against f64, so only the first run is checked here again, which
    ties the ten identical results of the others to the launch that test checked."""
    M, N = _walk_shape(WALK[0])
    run_case(M, N, 64, gpu_device, repeats=10, runs=RUNS[:1])
    for run in RUNS[1:]:
        c = G.operands(M, N, 64, narrow=run[2] == "narrow")
        x, w, b, r0 = (t.to(gpu_device) if t is not None else None for t in (c.x, c.w, c.b, c.r0))
        outs = [_launch(x, w, b if run[1] else None, run[0], r0) for _ in range(10)]
        for i, o in enumerate(outs[1:], 1):
            assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{run}: launch {i} differs from launch 0"


# ------------------------------------------------------------------------------------------------ pair-f32
GUARD, SENTINEL = 4096, -777.25


def _pair_shape(which):
    return (256 * _grid(1 << 30) + 1, 64, 64) if which == "walk" else which


PAIR = [(130, 64, 64), (257, 192, 128), (300, 320, 192), "walk"]


@pytest.mark.parametrize("which", PAIR, ids=[w if isinstance(w, str) else "x".join(map(str, w)) for w in PAIR])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_pair_gemm_is_exact(gpu_device, which, with_bias):
    """fl32(acc1 + fl32(bias + 2^-11 acc2)) bit for bit at [c // 64, m, c % 64]: dyadic w1, w2 (acc1, acc2 exact), a random f32 bias
    (the two additions round, in THIS order).  (130, 64, 64): a.N = 128, the second wavefront group idle; (257, 192, 128): three
    blocks, a half-filled last tile; the walk: G + 1 tiles, the leftover one as two items of one block each."""
    from vlfm_amd.vlm import ops

    M, N, K = _pair_shape(which)
    tm, tn = _tiles(M, 2 * N)
    if which == (130, 64, 64):
        assert 2 * N == 128
    if which == (257, 192, 128):
        assert (N // 64) % 2 == 1 and 2 * N - 256 == 128
    if which == "walk":
        g = _grid(1 << 30)
        items = G.work_items(M, 2 * N, g)
        assert len(items) == g + 2 and [tuple(i) for i in items[g:]] == [(g, 0), (g, 1)]
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x, w1, w2 = G._dyadic(g, (M, K), G.WIDE.x), G._dyadic(g, (N, K), G.WIDE.w), G._dyadic(g, (N, K), G.WIDE.w)
    # f32 bias, not dyadic, over 13 binades: both additions of the epilogue round, at different places in different columns
    bias = torch.randn(N, generator=g) * torch.exp2(torch.randint(-6, 7, (N,), generator=g).float())
    G.assert_budget(x, w1)
    G.assert_budget(x, w2)
    acc1, acc2 = G.pre_cpu(x, w1), G.pre_cpu(x, w2)
    want = G.want_pair_bits(acc1, acc2, bias.numpy() if with_bias else None)
    if with_bias:      # from the reference alone: these operands tell the kernel's order of the two additions from the other two
        a1, low, bf = acc1.astype(np.float32), acc2.astype(np.float32) * np.float32(2.0 ** -11), bias.numpy()[None, :]
        others = [int((((a1 + bf) + low).view(np.int32) != want).sum()), int((((a1 + low) + bf).view(np.int32) != want).sum())]
        print(f"pair {M, N, K}: (acc1 + bias) + low / (acc1 + low) + bias differ from the kernel's order at {others} of {want.size} outputs")
        assert min(others) >= 8
    nblk = N // 64
    flat = torch.full((2 * GUARD + nblk * M * 64,), SENTINEL, dtype=torch.float32, device=gpu_device)
    out = flat[GUARD:GUARD + nblk * M * 64].view(nblk, M, 64)
    out.view(torch.int32).fill_(0x7FC00000 | PATTERN)
    got = ops.linear_pair_f32(x.to(gpu_device), ops.interleave_pair_weights(w1, w2).to(gpu_device),
                              bias.to(gpu_device) if with_bias else None, out=out)
    assert got.data_ptr() == out.data_ptr()
    whole = flat.cpu().numpy()
    assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + nblk * M * 64:] == SENTINEL).all()
    bits = whole[GUARD:GUARD + nblk * M * 64].view(np.int32).reshape(nblk, M, 64).transpose(1, 0, 2).reshape(M, N)   # [m, c]
    bad = bits != want
    print(f"pair {M, N, K} {'bias' if with_bias else 'no bias'}: {int(bad.sum())} of {bad.size} outputs differ")
    if bad.any():
        m, c = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{int(bad.sum())} of {bad.size} differ; first at [block, m, c % 64] = {[c // 64, m, c % 64]}: got "
                             f"{bits[m, c].view(np.float32)!r}, want {want[m, c].view(np.float32)!r}")


# ------------------------------------------------------------------------------------------------ value edges
def test_gemm_value_edges(gpu_device):
    """f16 saturation (65504 + 15.99 stays, the tie 65520 goes to inf, with the bias tipping it, through accumulate and through GELU),
    results in the subnormal range (2^-24 comes back; the ties 2^-25 and 3 * 2^-25 go to even) and NaN confinement: a NaN in the last
    row of x and one in the last row of w make exactly row M - 1 and column N - 1 NaN; everything else stays bit-exact."""
    c = G.edge_case()
    A = G.gelu_tolerance()[0]
    M, N, K = G.EDGE_SHAPE
    assert _tiles(M, N) == (1, 2)
    x, w, b, r0 = (t.to(gpu_device) for t in (c.x, c.w, c.b, c.r0))
    nan = np.zeros((M, N), bool)
    nan[M - 1, :] = True
    nan[:, N - 1] = True
    for epi, with_bias in (("bias", True), ("bias", False), ("bias_gelu", True), ("accumulate", True), ("accumulate", False)):
        what = f"edges, {epi}{'' if with_bias else ', no bias'}"
        pre = c.pre if with_bias else c.pre_nobias
        assert np.array_equal(np.isnan(pre), nan)
        bits = _launch(x, w, b if with_bias else None, epi, r0).contiguous().view(torch.int16).cpu().numpy()
        assert np.array_equal((bits & 0x7FFF) > 0x7C00, nan), f"{what}: NaN is not confined to row {M - 1} and column {N - 1}"
        if epi == "bias_gelu":
            G.check_gelu(bits, pre, A, what)
        else:
            G.check_exact(bits, G.want_accumulate(pre, c.r0) if epi == "accumulate" else pre, what)
        got = bits.view(np.float16).astype(np.float64)
        for name, (m, n, _, _, _) in G.EDGE_COLUMNS.items():
            print(f"  {what}: {name}: pre {pre[m, n]!r}, r0 {float(c.r0[m, n])!r} -> {got[m, n]!r}")
        # the named outcomes, spelled out (they follow from the checks above; tests/test_gemm_ref_cpu.py has the same table)
        for (e, wb), (m, n), value in G.EDGE_OUTCOMES:
            if (e, wb) == (epi, with_bias):
                assert got[m, n] == value, (what, m, n, got[m, n], value)


# ------------------------------------------------------------------------------------------------ alignment
def test_gemm_refuses_misaligned_pointers(gpu_device):
    """The kernels move 16-byte pieces (LDS-DMA, half8 / floatx4): a contiguous view with a storage offset of 1 or 4 elements is
    refused on the host -- VLFM_ERR_INVALID from the entries, an AssertionError from the wrappers.  Nothing is launched here."""
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    L = _lib.lib()
    M, N, K = 64, 64, 64

    def zeros(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=gpu_device)

    for off in (1, 4):
        def shifted(shape, dtype):
            n = int(np.prod(shape))
            return torch.full((n + 8,), 3.0, dtype=dtype, device=gpu_device)[off:off + n].view(shape)

        h, f = torch.float16, torch.float32
        good = dict(x=zeros((M, K), h), w=zeros((N, K), h), b=zeros((N,), h), c=zeros((M, N), h))
        odd = dict(x=shifted((M, K), h), w=shifted((N, K), h), b=shifted((N,), h), c=shifted((M, N), h))
        assert all(t.is_contiguous() and t.data_ptr() % 16 == 2 * off for t in odd.values())
        assert all(t.data_ptr() % 16 == 0 for t in good.values())
        for which in ("x", "w", "b", "c"):
            a = dict(good, **{which: odd[which]})
            for epi in (0, 1, 2):
                rc = L.vlfm_gemm_f16_nt(a["x"].data_ptr(), a["w"].data_ptr(), a["b"].data_ptr(), a["c"].data_ptr(), M, N, K, epi, None)
                assert rc == _lib.VLFM_ERR_INVALID and "16-byte aligned" in _lib.last_error(), (which, off, epi)
            with pytest.raises(AssertionError):
                ops.linear_f16(a["x"], a["w"], a["b"], "bias", out=a["c"])
        # pair-f32: x [M, K] and w_pair [2 N, K] f16, bias [N] and out [N / 64, M, 64] f32 (four f32 are 16 bytes: only offset 1 is odd)
        good = dict(x=good["x"], w=zeros((2 * N, K), h), b=zeros((N,), f), c=zeros((1, M, 64), f))
        odd = dict(x=odd["x"], w=shifted((2 * N, K), h), b=shifted((N,), f), c=shifted((1, M, 64), f))
        for which in ("x", "w", "b", "c"):
            a = dict(good, **{which: odd[which]})
            if a[which].data_ptr() % 16 == 0:
                assert off == 4 and which in ("b", "c")
                continue
            rc = L.vlfm_gemm_f16_pair_f32_nt(a["x"].data_ptr(), a["w"].data_ptr(), a["b"].data_ptr(), a["c"].data_ptr(), M, N, K, None)
            assert rc == _lib.VLFM_ERR_INVALID and "16-byte aligned" in _lib.last_error(), (which, off)
            with pytest.raises(AssertionError):
                ops.linear_pair_f32(a["x"], a["w"], a["b"], out=a["c"])
