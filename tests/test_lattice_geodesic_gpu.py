"""-m gpu: the lattice geodesic on the device (vlfm_lattice_free / vlfm_lattice_fields / vlfm_lattice_query, through the raw entry
points and through RoomsRenderer.lattice_fields_worlds / lattice_distances) against the host statement of vlfm_amd/synthetic.py,
with == on free planes, uint16 fields and f64 answers; BatchedEpisodes(..., geodesic="lattice")."""
import numpy as np
import pytest

import lattice_cases as C
from vlfm_amd import synthetic as S
from test_grid_worlds_cpu import _two_plans
from test_grid_worlds_gpu import _objects, _table, _worlds
from world_object_cases import objects_array

pytestmark = pytest.mark.gpu

NONE = S.LATTICE_NONE


def _pack(free, max_nb, words):
    """uint32 [max_nb, words]: the free plane of one field, every bit beyond its dims SET (a free node everywhere, were it read)."""
    nb, na = free.shape
    bits = np.ones((max_nb, words * 32), np.uint8)
    bits[:nb, :na] = free
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(max_nb, words)


def _fields(device, masks, sources, max_cost=S.LATTICE_MAX_COST, origins=None, max_sources=None):
    """vlfm_lattice_fields over the free masks ``masks`` (bool [nb, na] each, mixed dims) around the GLOBAL source nodes
    ``sources`` -> (dist uint16 [n, max_nb, max_na] on the host, the status, dims)."""
    import torch

    from vlfm_amd import _lib as L

    n = len(masks)
    max_nb, max_na = max(m.shape[0] for m in masks), max(m.shape[1] for m in masks)
    words = (max_na + 31) // 32
    origins = [(0, 0)] * n if origins is None else origins
    max_sources = max([1] + [len(s) for s in sources]) if max_sources is None else max_sources
    dims = np.array([(a0, b0, m.shape[1], m.shape[0]) for (a0, b0), m in zip(origins, masks)], np.int32)
    src = np.full((n, max_sources, 2), 7777, np.int32)
    cnt = np.zeros(n, np.int32)
    for i, s in enumerate(sources):
        s = np.asarray(s, np.int32).reshape(-1, 2)
        src[i, :len(s)], cnt[i] = s, len(s)
    planes = np.stack([_pack(m, max_nb, words) for m in masks])
    lib = L.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    d_planes, d_dims, d_src, d_cnt = dev(planes.view(np.int32)), dev(dims), dev(src), dev(cnt)
    dist = torch.zeros((n, max_nb, max_na), dtype=torch.int16, device=device)
    need = lib.vlfm_lattice_scratch_bytes(n, max_nb, max_na)
    scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=device)
    rc = lib.vlfm_lattice_fields(d_planes.data_ptr(), d_dims.data_ptr(), n, max_nb, max_na, d_src.data_ptr(), d_cnt.data_ptr(),
                                 max_sources, max_cost, dist.data_ptr(), scratch.data_ptr(), need,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc >= 0, L.last_error()
    assert (rc == L.LATTICE_IN_LDS) == (need == 0)
    return dist.cpu().numpy().view(np.uint16), rc, dims


def _want(masks, sources, max_cost=S.LATTICE_MAX_COST, origins=None):
    max_nb, max_na = max(m.shape[0] for m in masks), max(m.shape[1] for m in masks)
    out = np.full((len(masks), max_nb, max_na), NONE, np.uint16)
    for i, m in enumerate(masks):
        o = (0, 0) if origins is None else origins[i]
        out[i, :m.shape[0], :m.shape[1]] = S.lattice_field_numpy(m, np.asarray(sources[i], np.int64).reshape(-1, 2), o, max_cost)
    return out


def _check(device, masks, sources, max_cost=S.LATTICE_MAX_COST, origins=None):
    got, rc, _ = _fields(device, masks, sources, max_cost, origins)
    want = _want(masks, sources, max_cost, origins)
    assert np.array_equal(got, want), int((got != want).sum())
    return want, rc


@pytest.mark.parametrize("nb,na", [(1, 1), (1, 40), (40, 1), (17, 31), (17, 32), (17, 33), (17, 64), (17, 65)])
def test_small_lattices_and_word_seams(gpu_device, nb, na):
    """Obstacles and sources on the columns either side of every 32-bit word seam, in the first and in the last column."""
    rng = np.random.default_rng(100 * nb + na)
    masks, sources = [np.ones((nb, na), bool)], [[(na - 1, nb - 1)]]
    for density in (0.15, 0.35):
        m = C.random_mask(rng, nb, na, density)
        for seam in (31, 32, 63, 64):
            if seam < na:
                m[rng.integers(0, nb, 3), seam] = False
        src = [(c, int(rng.integers(0, nb))) for c in (0, 30, 31, 32, 33, 62, 63, 64, na - 1) if c < na]
        for (a, b) in src[::2]:
            m[b, a] = True
        masks.append(m)
        sources.append(src)
    want, _ = _check(gpu_device, masks, [[(a - 3, b + 5) for (a, b) in s] for s in sources], origins=[(-3, 5)] * 3)
    assert want[0, 0, 0] == (0 if nb * na == 1 else want[0].max()) and (want[1] != NONE).any()


def test_a_spiral_a_comb_and_a_capped_serpentine(gpu_device):
    """Many levels, long runs of levels that touch a few rows, and levels that are empty for a while (a comb's teeth end)."""
    spiral, comb, snake = C.spiral(40), C.comb(40), C.serpentine(41)
    want, _ = _check(gpu_device, [spiral, comb, snake], [[(0, 0)], [(0, 0)], [(0, 0)]])
    assert want[0][want[0] != NONE].max() > 1500 and (want[0] != NONE).sum() == spiral.sum()       # the whole corridor, far
    assert want[1, 39, 38] == 5 * (38 + 39) and want[2, 40, 40] == 5 * (41 * 21 + 20 - 1)
    # a cap about half way: the far end lies beyond it from both sides, the middle of the corridor stays unsettled
    capped, _ = _check(gpu_device, [snake], [[(0, 0), (40, 40)]], max_cost=2000)
    assert capped.max() == NONE and capped[capped != NONE].max() == 2000 and (capped[0][snake] == NONE).sum() > 40
    assert capped[0, 0, 0] == 0 and capped[0, 40, 40] == 0


def test_random_masks_and_degenerate_fields(gpu_device):
    rng = np.random.default_rng(7)
    masks = [C.random_mask(rng, int(rng.integers(2, 90)), int(rng.integers(2, 130)), d) for d in (0.1, 0.3, 0.3, 0.45, 0.2, 0.6)]
    sources = [[(int(rng.integers(0, m.shape[1])), int(rng.integers(0, m.shape[0]))) for _ in range(4)] for m in masks]
    blocked = np.ones((9, 40), bool)
    blocked[4, 20] = False
    masks += [np.ones((12, 35), bool), blocked, np.ones((5, 5), bool), np.zeros((6, 33), bool)]
    sources += [[], [(20, 4)], [(-1, 0), (5, 2), (2, 5), (2, -1)], [(1, 1)]]      # none; on a blocked node; outside; nothing free
    want, rc = _check(gpu_device, masks, sources)
    from vlfm_amd import _lib as L

    assert rc == L.LATTICE_IN_LDS
    assert all((want[i] == NONE).all() for i in (6, 7, 8, 9)) and all((want[i] != NONE).any() for i in range(6))
    # the same source twice, and sources of one field that settle each other's neighbourhoods
    _check(gpu_device, [np.ones((8, 70), bool)], [[(31, 3), (31, 3), (32, 3), (33, 4)]])


def test_max_cost_at_11_and_at_65534(gpu_device):
    free = np.ones((9, 9), bool)
    full, _ = _check(gpu_device, [free], [[(4, 4)]], max_cost=65534)
    cut, _ = _check(gpu_device, [free], [[(4, 4)]], max_cost=11)
    assert full.max() == 28 and (cut == 11).sum() == 8 and np.array_equal(cut, np.where(full <= 11, full, NONE))
    zero, _ = _check(gpu_device, [free], [[(4, 4)]], max_cost=0)
    assert (zero != NONE).sum() == 1


@pytest.mark.parametrize("n", [1, 3, 67])
def test_batches_of_mixed_dims_with_tails_of_ones(gpu_device, n):
    rng = np.random.default_rng(n)
    masks = [C.random_mask(rng, int(rng.integers(1, 50)), int(rng.integers(1, 100)), 0.25) for _ in range(n)]
    origins = [(int(rng.integers(-500, 500)), int(rng.integers(-500, 500))) for _ in range(n)]
    sources = [[(a0 + int(rng.integers(0, m.shape[1])), b0 + int(rng.integers(0, m.shape[0]))) for _ in range(3)]
               for m, (a0, b0) in zip(masks, origins)]
    want, _ = _check(gpu_device, masks, sources, origins=origins)
    assert sum(int((w != NONE).any()) for w in want) >= (n + 1) // 2


def test_a_300_x_300_field_lives_in_scratch(gpu_device):
    from vlfm_amd import _lib as L

    rng = np.random.default_rng(300)
    free = C.random_mask(rng, 300, 300, 0.2)
    free[150, 150] = free[0, 299] = True
    want, rc = _check(gpu_device, [free, free[:40, :50]], [[(150, 150), (299, 0)], [(3, 3), (4, 3), (3, 4), (4, 4)]])
    assert rc == L.LATTICE_IN_SCRATCH and (want[0] != NONE).sum() > 60000 and want[0][want[0] != NONE].max() > 1000
    lib = L.lib()           # the twelve level planes of 12 x 304 words; free and open stay in LDS
    assert lib.vlfm_lattice_scratch_bytes(2, 300, 300) == 2 * 12 * 12 * 304 * 4 and lib.vlfm_lattice_scratch_bytes(9, 256, 256) == 0


def test_an_800_x_790_field_lives_wholly_in_scratch(gpu_device):
    """Two planes of this bound no longer fit 160 KB of LDS: all fourteen go to the scratch."""
    from vlfm_amd import _lib as L

    rng = np.random.default_rng(800)
    free = C.random_mask(rng, 790, 800, 0.15)
    free[400, 400] = True
    want, rc = _check(gpu_device, [free, C.comb(40)], [[(400, 400)], [(0, 0)]], max_cost=1500)
    assert rc == L.LATTICE_ALL_IN_SCRATCH and (want[0] != NONE).sum() > 200000 and want[0][want[0] != NONE].max() == 1500
    assert L.lib().vlfm_lattice_scratch_bytes(2, 790, 800) == 2 * 14 * 27 * 794 * 4


def test_a_side_stream(gpu_device):
    import torch

    side = torch.cuda.Stream(gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    masks, sources = [C.spiral(40), C.comb(40)], [[(0, 0)], [(39, 0)]]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            big.mul_(1.0001)                    # work queued in front of the memset and the kernel on the same stream
        got, _, _ = _fields(gpu_device, masks, sources)
    side.synchronize()
    assert np.array_equal(got, _want(masks, sources))


def _renderer(device):
    from vlfm_amd.harness import RoomsRenderer

    return RoomsRenderer([0], 500, 36, 64, device)


def _host_fields(worlds, world_of, objects, targets, n=20, pad_m=1.0, max_cost=S.LATTICE_MAX_COST):
    """Per field (extent, free mask, field) by the host statement, the way lattice_fields_worlds states it."""
    out = []
    for w, rec, box in zip(world_of, objects, targets):
        boxes, grid = worlds[w]
        ext = S.lattice_extent(boxes, grid, rec, n, pad_m)
        free = S.lattice_free_numpy(ext, boxes, grid, rec, n)
        src = np.zeros((0, 2), np.int64)
        if np.all(np.isfinite(box)):
            src = S.lattice_sources(S.goal_viewpoints(box, S.inflated_rects(rec, S.STEP_MARGIN, boxes), 1.0, grid=grid), n)
        out.append((ext, free, S.lattice_field_numpy(free, src, ext[:2], max_cost)))
    return out


def test_free_planes_and_fields_of_a_world_table(gpu_device):
    """Boxes only (the rooms world), grids only (1 x 1, 3 x 5, 33 x 70 cells), boxes and a grid, an empty grid; with objects;
    the table's tails set to ones behind the wrapper's back."""
    worlds = _worlds()
    table = _table(gpu_device, worlds, "ones")
    world_of = [0, 1, 2, 3, 4, 5, 3]
    objects = objects_array([_objects()[i] for i in (0, 3, 3, 1, 2, 0, 3)])
    objects[2, 5, :4], objects[2, 5, 6] = (-9.0, -9.0, 9.0, 9.0), 0.0             # an invalid slot's numbers mean nothing
    targets = [objects[0, 0, :4], objects[1, 0, :4], (np.nan,) * 4, objects[3, 0, :4], objects[4, 0, :4], objects[5, 1, :4],
               objects[6, 1, :4]]
    h = _renderer(gpu_device).lattice_fields_worlds(table, world_of, objects, targets, 1.0)
    want = _host_fields(worlds, world_of, objects, targets)
    assert h.n == 7 and h.has_target.tolist() == [True, True, False, True, True, True, True] and h.cells_per_metre == 20
    assert h.dims_host.tolist() == [list(e) for e, _, _ in want] and np.array_equal(h.dims.cpu().numpy(), h.dims_host)
    assert tuple(h.dist.shape[1:]) == (449, 449)
    for i, (ext, free, field) in enumerate(want):
        assert np.array_equal(h.free(i), free), (i, int((h.free(i) != free).sum()))
        assert np.array_equal(h.costs(i), field), (i, int((h.costs(i) != field).sum()))
        assert 0 < free.sum() < free.size
    assert (want[2][2] == NONE).all() and all((f != NONE).any() for k, (_, _, f) in enumerate(want) if k != 2)
    # beyond a field's dims: free planes hold zeros, fields 0xFFFF
    bits, dist = h.bits.cpu().numpy(), h.dist.cpu().numpy().view(np.uint16)
    _, _, na, nb = want[1][0]
    assert not bits[1, nb:].any() and not bits[1, :, (na + 31) // 32:].any() and (dist[1, nb:] == NONE).all() and (dist[1, :, na:] == NONE).all()
    # another spacing and pad, a cap
    h8 = _renderer(gpu_device).lattice_fields_worlds(table, world_of[3:5], objects[3:5], targets[3:5], 1.0, cells_per_metre=8,
                                                      pad_m=0.5, max_cost=300)
    for i, (ext, free, field) in enumerate(_host_fields(worlds, world_of[3:5], objects[3:5], targets[3:5], 8, 0.5, 300)):
        assert h8.dims_host[i].tolist() == list(ext) and np.array_equal(h8.free(i), free) and np.array_equal(h8.costs(i), field)
        assert field[field != NONE].max() <= 300


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_queries_and_assign(gpu_device):
    worlds = _worlds()
    table = _table(gpu_device, worlds)
    r = _renderer(gpu_device)
    objects = objects_array([_objects()[1], _objects()[2]])
    targets = [objects[0, 0, :4], objects[1, 1, :4]]
    h = r.lattice_fields_worlds(table, [3, 4], objects, targets, 1.0)
    want = _host_fields(worlds, [3, 4], objects, targets)
    rng = np.random.default_rng(11)
    pts = np.concatenate([0.05 * rng.integers(-80, 80, size=(40, 2)),                   # on nodes
                          0.05 * rng.integers(-80, 80, size=(40, 2)) + (0.025, 0.0),     # on cell edges
                          rng.uniform(-4.5, 4.5, size=(80, 2)),                          # anywhere, beyond the lattices too
                          [(1e9, 0.0), (0.0, -1e300), (np.nan, 0.0), (np.inf, 0.0), (100.0, 100.0)],
                          0.25 * rng.integers(-12, 12, size=(30, 2)) + 0.25 * np.array(S.HEADINGS)[rng.integers(0, 12, 30)]])
    for f in (0, 1):
        ext, _, field = want[f]
        host = S.lattice_query_numpy(field, ext[:2], pts, 20)
        got = r.lattice_distances(h, np.full(len(pts), f), pts)
        assert got.dtype.is_floating_point and got.device.type == "cuda" and _same_bits(got.cpu().numpy(), host), f
        assert 20 < np.isfinite(host).sum() < len(host)
    mixed = r.lattice_distances(h, [0, -1, 1, -1], [(0.0, 0.0)] * 4).cpu().numpy()
    assert np.isnan(mixed[[1, 3]]).all() and not np.isnan(mixed[[0, 2]]).any()
    with pytest.raises(ValueError):
        r.lattice_distances(h, [2], [(0.0, 0.0)])
    assert r.lattice_distances(h, [], np.zeros((0, 2))).shape == (0,)
    assert r.lattice_fields_worlds(table, [], objects[:0], np.zeros((0, 4)), 1.0).n == 0
    # assign: row 0 becomes the rooms world's field (larger planes: the handle grows), and answers like it
    lay = S.object_layout(0, 0, (0.0, 0.0))
    rec = objects_array([[b for _, b in lay]])
    rooms = r.lattice_fields_worlds(table, [0], rec, [lay[0][1][:4]], 1.0)
    (ext0, free0, field0), = _host_fields(worlds, [0], rec, [lay[0][1][:4]])
    h.assign([0], rooms)
    assert h.has_target.tolist() == [True, True] and h.dims_host[0].tolist() == list(ext0) and tuple(h.dist.shape[1:]) == (449, 449)
    assert np.array_equal(h.costs(0), field0) and np.array_equal(h.free(0), free0) and np.array_equal(h.costs(1), want[1][2])
    far = 0.25 * rng.integers(-38, 39, size=(40, 2))
    assert _same_bits(r.lattice_distances(h, np.zeros(40, np.int32), far).cpu().numpy(), S.lattice_query_numpy(field0, ext0[:2], far, 20))
    assert _same_bits(r.lattice_distances(h, np.ones(len(pts), np.int32), pts).cpu().numpy(),
                      S.lattice_query_numpy(want[1][2], want[1][0][:2], pts, 20))
    with pytest.raises(ValueError):
        h.assign([0, 1], rooms)
    with pytest.raises(ValueError):
        h.assign([2], rooms)


def test_refusals_launch_nothing(gpu_device):
    import torch

    from vlfm_amd import _lib as L

    lib = L.lib()
    assert lib.vlfm_abi_version() >= 26
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device=gpu_device)
    planes, dims = torch.full((1, 8, 1), -1, **i32), torch.tensor([[0, 0, 8, 8]], **i32)
    src, cnt = torch.tensor([[[4, 4]]], **i32), torch.ones(1, **i32)
    dist = torch.full((1, 8, 8), 77, dtype=torch.int16, device=gpu_device)
    out = torch.full((1,), -3.0, dtype=torch.float64, device=gpu_device)
    pts, fof = torch.zeros((1, 2), dtype=torch.float64, device=gpu_device), torch.zeros(1, **i32)

    def fields(n=1, max_nb=8, max_na=8, max_sources=1, max_cost=100, d_dist=dist.data_ptr(), d_dims=dims.data_ptr()):
        return lib.vlfm_lattice_fields(planes.data_ptr(), d_dims, n, max_nb, max_na, src.data_ptr(), cnt.data_ptr(), max_sources,
                                       max_cost, d_dist, None, 0, st)

    for kw in (dict(max_na=1025), dict(max_nb=1025), dict(max_na=0), dict(max_nb=0), dict(n=-1), dict(max_sources=-1),
               dict(max_cost=-1), dict(max_cost=65535), dict(d_dist=None), dict(d_dims=None)):
        assert fields(**kw) == L.VLFM_ERR_INVALID, kw
    assert lib.vlfm_lattice_fields(planes.data_ptr(), dims.data_ptr(), 1, 300, 300, src.data_ptr(), cnt.data_ptr(), 1, 100,
                                   dist.data_ptr(), None, 0, st) == L.VLFM_ERR_CAPACITY
    table = _table(gpu_device, _worlds())
    wof, rec = torch.zeros(1, **i32), torch.zeros((1, 8, 8), dtype=torch.float64, device=gpu_device)

    def free(n=1, cpm=20, max_nb=8, max_na=8, bits=table.d_grid_bits.data_ptr(), max_nx=70, margin=0.2):
        return lib.vlfm_lattice_free(table.d_boxes.data_ptr(), table.d_counts.data_ptr(), table.n_worlds, table.max_boxes, bits,
                                     table.d_grid_edges.data_ptr(), table.d_grid_dims.data_ptr(), max_nx, 64, wof.data_ptr(), margin,
                                     rec.data_ptr(), dims.data_ptr(), n, cpm, max_nb, max_na, planes.data_ptr(), st)

    for kw in (dict(max_na=1025), dict(max_nb=0), dict(cpm=10), dict(cpm=0), dict(bits=None), dict(max_nx=1025), dict(n=65536),
               dict(margin=float("nan"))):
        assert free(**kw) == L.VLFM_ERR_INVALID, kw

    def query(m=1, n_fields=1, max_nb=8, max_na=8, cpm=20, d_out=out.data_ptr()):
        return lib.vlfm_lattice_query(pts.data_ptr(), fof.data_ptr(), m, n_fields, dist.data_ptr(), dims.data_ptr(), max_nb, max_na,
                                      cpm, d_out, st)

    for kw in (dict(m=-1), dict(n_fields=-1), dict(max_na=2000), dict(cpm=6), dict(d_out=None)):
        assert query(**kw) == L.VLFM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((dist == 77).all()) and bool((planes == -1).all()) and bool((out == -3.0).all())              # nothing written
    assert fields(n=0) == L.VLFM_OK and free(n=0) == L.VLFM_OK and query(m=0) == L.VLFM_OK
    # the same calls unrefused run: a source in the middle of an open 8 x 8 lattice
    assert fields() == L.LATTICE_IN_LDS, L.last_error()
    assert np.array_equal(dist.cpu().numpy().view(np.uint16)[0], S.lattice_field_numpy(np.ones((8, 8), bool), [(4, 4)], max_cost=100))
    assert query() == L.VLFM_OK and float(out.cpu()[0]) == S.lattice_query_numpy(dist.cpu().numpy().view(np.uint16)[0], (0, 0), [(0.0, 0.0)])[0]
    # a field wider than 1024 nodes is refused on the host, before any device is touched
    wide = np.zeros((1, 8, 8))
    wide[0, 0, :7] = (-30.0, 0.0, 30.0, 1.0, 0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="1024"):
        _renderer(gpu_device).lattice_fields_worlds(table, [5], wide, [(np.nan,) * 4], 1.0)
    with pytest.raises(ValueError, match="multiple of 4"):
        _renderer(gpu_device).lattice_fields_worlds(table, [], wide[:0], np.zeros((0, 4)), 1.0, cells_per_metre=10)


# ------------------------------------------------------------------------------------------------------------------- harness
E, STEPS = 4, 30


def _harness(device, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    return BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, closed_loop=True,
                           world_objects=WorldObjects(max_episode_steps=12), **kw)


def _bits(t):
    import torch

    return t.contiguous().view({torch.float32: torch.int32}.get(t.dtype, t.dtype)).cpu().numpy()


def _host_field_of(live, e):
    """(origin, field) of environment e's running episode by the host statement; None: its layout has no target."""
    k = int(live.target_slot[e])
    if k < 0:
        return None
    w = int(live.world_of[e])
    walls, grid, rec = live.table.world(w), live.table.grids[w], live.objects[e]
    ext = S.lattice_extent(walls, grid, rec, 20)
    pts = S.goal_viewpoints(rec[k, :4], S.inflated_rects(rec, S.STEP_MARGIN, walls), live.world_objects.success_distance, grid=grid)
    free = S.lattice_free_numpy(ext, walls, grid, rec, 20)
    return ext[:2], S.lattice_field_numpy(free, S.lattice_sources(pts, 20), ext[:2])


def _host_distance(field, xy) -> float:
    return float("nan") if field is None else float(S.lattice_query_numpy(field[1], field[0], [xy], 20)[0])


def test_harness_in_grid_worlds_scores_spl(gpu_device):
    """30 steps at 4 environments over two drawn plans: every distance_to_goal and every episode_geodesic is the host
    statement's; frames, modes, goals, actions and poses are those of the same harness without the metrics."""
    import torch

    worlds = lambda: S.GridWorlds(_two_plans(), seed=3)      # noqa: E731
    on = _harness(gpu_device, worlds=worlds(), objectnav_metrics=True, geodesic="lattice")
    off = _harness(gpu_device, worlds=worlds())
    live = on.live
    assert on.geodesic_backend == "lattice" and type(live.geodesic).__name__ == "LatticeFields"
    fields = [_host_field_of(live, e) for e in range(E)]
    running = [_host_distance(fields[e], live.xy[e]) for e in range(E)]          # the running episodes' start distances
    assert np.array_equal(live.ep_geodesic, running, equal_nan=True) and np.array_equal(live.distance_to_goal, running, equal_nan=True)
    scored, finite = [], 0
    for t in range(STEPS):
        episode = live.world_episode.copy()
        on.step()
        off.step()
        assert on.last_modes == off.last_modes and np.array_equal(on.last_goals, off.last_goals, equal_nan=True), t
        assert np.array_equal(on.last_world_actions, off.last_world_actions) and np.array_equal(on.last_poses, off.last_poses), t
        if t % 6 == 0 or t == STEPS - 1:
            torch.cuda.synchronize()
            assert np.array_equal(_bits(on.live.frames), _bits(off.live.frames)) and np.array_equal(_bits(on.live.ids), _bits(off.live.ids)), t
        for e in range(E):
            if live.world_episode[e] != episode[e]:                            # scored with this step; the next episode runs
                scored.append(running[e])
                fields[e] = _host_field_of(live, e)
                running[e] = _host_distance(fields[e], live.xy[e])
                assert live.ep_geodesic[e] == running[e] or (np.isnan(running[e]) and np.isnan(live.ep_geodesic[e])), (t, e)
            want = _host_distance(fields[e], live.xy[e])
            got = float(live.distance_to_goal[e])
            assert got == want or (np.isnan(want) and np.isnan(got)), (t, e, got, want)
            finite += int(np.isfinite(want))
    st = live.objectnav_stats
    assert np.array_equal(st["episode_geodesic"], scored, equal_nan=True) and len(scored) >= 2 * E
    assert finite > STEPS * E // 2 and np.isfinite(scored).sum() >= E
    for key in off.live.objectnav_stats:
        assert np.array_equal(np.asarray(st[key]), np.asarray(off.live.objectnav_stats[key])), key
    assert np.array_equal(live.xy, off.live.xy) and np.array_equal(live.k, off.live.k)
    summary = live.objectnav_summary()
    assert set(summary) == {"episodes", "scored", "excluded_no_target", "excluded_unreachable", "success_rate", "spl", "soft_spl",
                            "distance_to_goal"} and summary["episodes"] == len(scored)
    print("grid worlds, lattice metrics after 30 steps:", summary)


def test_rooms_world_lattice_beside_graph(gpu_device):
    """The same episodes scored by both backends: identical poses and actions, the same keys, and every start distance l of the
    lattice inside the band the CPU test asserts against the visibility graph."""
    kw = dict(objectnav_metrics=True, object_maps=True)
    lat, gra = _harness(gpu_device, geodesic="lattice", **kw), _harness(gpu_device, geodesic="graph", **kw)
    assert gra.geodesic_backend == "graph" and type(gra.live.geodesic).__name__ == "GeodesicFields"
    for t in range(STEPS):
        lat.step()
        gra.step()
        assert np.array_equal(lat.last_world_actions, gra.last_world_actions) and np.array_equal(lat.last_poses, gra.last_poses), t
        assert lat.last_modes == gra.last_modes, t
    a, b = lat.live.objectnav_stats, gra.live.objectnav_stats
    assert set(a) == set(b) and a["episode_outcome"] == b["episode_outcome"] and a["episode_path_length"] == b["episode_path_length"]
    l, g = np.array(a["episode_geodesic"] + list(lat.live.ep_geodesic)), np.array(b["episode_geodesic"] + list(gra.live.ep_geodesic))
    assert len(l) >= 3 * E and np.array_equal(np.isfinite(l), np.isfinite(g)) and np.array_equal(np.isnan(l), np.isnan(g))
    far = np.isfinite(g) & (g > 1.0)
    ratio = l[far] / g[far]
    print("rooms world, l lattice / l graph:", ratio.round(4).tolist())
    assert far.sum() >= E and C.BAND_LO <= ratio.min() and ratio.max() <= C.BAND_HI
    assert set(lat.live.objectnav_summary()) == set(gra.live.objectnav_summary())
