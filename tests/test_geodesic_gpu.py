"""-m gpu: vlfm_geodesic_fields / vlfm_geodesic_query (csrc/geodesic.hip) against the host statement in vlfm_amd/synthetic.py:
rectangles, node tables, dist and the queried distances are bit-equal (compared as int64), inf patterns included."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S

pytestmark = pytest.mark.gpu

MAX_SRC = 16


def _lib():
    from vlfm_amd import _lib as L

    return L


def _records(boxes_per_env, slots_per_env=None) -> np.ndarray:
    """[n,8,8] object records with the footprints ``boxes_per_env[e]`` in the slots ``slots_per_env[e]`` (default: 0, 1, ...)."""
    out = np.zeros((len(boxes_per_env), 8, 8))
    for e, boxes in enumerate(boxes_per_env):
        slots = range(len(boxes)) if slots_per_env is None else slots_per_env[e]
        for k, b in zip(slots, boxes):
            out[e, k, :4], out[e, k, 5], out[e, k, 6] = b[:4], 1.0, 1.0
    return out


def _fields(device, walls, margin, records, sources_per_env, max_sources=MAX_SRC):
    """Raw call of vlfm_geodesic_fields, the shared ``walls`` as a table of one world that every field stands in -> dict of
    device tensors (the strides of include/vlfm_amd.h)."""
    import torch

    L = _lib()
    n, B = len(records), len(walls)
    R = B + 8
    f64 = dict(dtype=torch.float64, device=device)
    src = np.zeros((n, max_sources, 2))
    cnt = np.zeros(n, np.int32)
    for e, s in enumerate(sources_per_env):
        s = np.asarray(s, np.float64).reshape(-1, 2)
        src[e, :len(s)], cnt[e] = s, len(s)
    t = {"walls": torch.tensor(np.asarray(walls, np.float64).reshape(-1, 4), **f64), "records": torch.tensor(records, **f64),
         "sources": torch.tensor(src, **f64), "source_counts": torch.tensor(cnt, dtype=torch.int32, device=device),
         "rects": torch.full((n, R, 4), -7.0, **f64), "nodes": torch.full((n, 4 * R, 2), -7.0, **f64),
         "dist": torch.full((n, 4 * R), -7.0, **f64), "counts": torch.full((n, 2), -7, dtype=torch.int32, device=device),
         "box_counts": torch.tensor([B], dtype=torch.int32, device=device),
         "world_of": torch.zeros(n, dtype=torch.int32, device=device), "n": n, "B": B, "max_sources": max_sources}
    rc = L.lib().vlfm_geodesic_fields(t["walls"].data_ptr() if B else None, t["box_counts"].data_ptr(), 1, B,
                                      t["world_of"].data_ptr(), float(margin), t["records"].data_ptr(),
                                      t["sources"].data_ptr(), t["source_counts"].data_ptr(), n, max_sources,
                                      t["rects"].data_ptr(), t["nodes"].data_ptr(), t["dist"].data_ptr(), t["counts"].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == L.VLFM_OK, L.last_error()
    torch.cuda.synchronize()
    return t


def _query(device, t, field_of, points) -> np.ndarray:
    import torch

    L = _lib()
    pts = torch.tensor(np.asarray(points, np.float64).reshape(-1, 2), dtype=torch.float64, device=device)
    fo = torch.tensor(np.asarray(field_of, np.int32), dtype=torch.int32, device=device)
    out = torch.full((len(pts),), -7.0, dtype=torch.float64, device=device)
    rc = L.lib().vlfm_geodesic_query(pts.data_ptr(), fo.data_ptr(), len(pts), t["n"], t["B"], t["rects"].data_ptr(),
                                     t["nodes"].data_ptr(), t["dist"].data_ptr(), t["counts"].data_ptr(), t["sources"].data_ptr(),
                                     t["source_counts"].data_ptr(), t["max_sources"], out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == L.VLFM_OK, L.last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check_field(t, e, walls, margin, records, sources):
    """Field ``e`` of the device tables against the host statement; returns the host's (rects, nodes, dist)."""
    rects = S.inflated_rects(records[e], margin, boxes=np.asarray(walls, np.float64).reshape(-1, 4))
    nodes, dist = S.geodesic_field_numpy(rects, sources)
    counts = t["counts"][e].cpu().numpy()
    assert counts.tolist() == [len(rects), len(nodes)], (e, counts, len(rects), len(nodes))
    g_rects, g_nodes, g_dist = (t[k][e].cpu().numpy() for k in ("rects", "nodes", "dist"))
    assert _same_bits(g_rects[:len(rects)], rects), e
    assert _same_bits(g_nodes[:len(nodes)], nodes), e
    assert np.array_equal(np.isinf(g_dist[:len(nodes)]), np.isinf(dist)), e
    assert _same_bits(g_dist[:len(nodes)], dist), (e, np.abs(g_dist[:len(nodes)] - dist).max())
    assert not g_rects[len(rects):].any() and not g_nodes[len(nodes):].any() and np.isinf(g_dist[len(nodes):]).all(), e
    return rects, nodes, dist


UNIT = (-1.0, -1.0, 1.0, 1.0)
RING = [(-3.0, -3.0, 3.0, -2.0), (-3.0, 2.0, 3.0, 3.0), (-3.0, -3.0, -2.0, 3.0), (2.0, -3.0, 3.0, 3.0)]


def test_tiny_cases(gpu_device):
    """The cases of tests/test_geodesic_cpu.py in one batch: no rectangle; one box to walk around, along and inside; sources
    inside the box; a walled-in source; no source."""
    boxes = [[], [UNIT], [UNIT], RING, [UNIT]]
    sources = [[(3.0, 4.0), (1.0, 1.0), (-2.0, 0.5)], [(2.0, 0.0)], [(0.0, 0.0), (0.5, 0.5)], [(0.0, 0.0)], []]
    points = [[(0.0, 0.0), (3.0, 4.0), (-5.0, 0.5)],
              [(-2.0, 0.0), (0.0, 0.0), (0.5, -0.99), (-3.0, 1.0), (-2.0, 0.0), (1.0, -1.0), (2.0, 0.0), (0.0, -2.0)],
              [(-2.0, 0.0), (5.0, 5.0)], [(5.0, 0.0), (1.0, 1.0), (2.0, 2.0)], [(-2.0, 0.0)]]
    rec = _records(boxes)
    t = _fields(gpu_device, [], 0.0, rec, sources)
    field_of, pts, want = [], [], []
    for e in range(len(boxes)):
        rects, nodes, dist = _check_field(t, e, [], 0.0, rec, sources[e])
        field_of += [e] * len(points[e])
        pts += points[e]
        want.append(S.geodesic_query_numpy(rects, sources[e], nodes, dist, points[e]))
    got = _query(gpu_device, t, field_of, pts)
    want = np.concatenate(want)
    assert _same_bits(got, want), (got, want)
    s2 = float(np.sqrt(2.0))
    assert got[3] == (s2 + 2.0) + s2 and np.isinf(got[4]) and np.isinf(got[5]) and got[0] == s2       # walk around; inside
    assert np.isinf(got[11:13]).all() and np.isinf(got[13]) and got[14] == s2 and np.isinf(got[16])


def _random_batch(seed=20260):
    rng = np.random.default_rng(seed)
    n = 8
    boxes, slots, sources, points = [], [], [], []
    for e in range(n):
        k = [0, 6, 1, 3, 5, 2, 4, 6][e]
        bs = []
        for _ in range(k):          # corners on a 0.25 lattice: shared edges, touching corners, collinear sides do occur
            x0, y0 = 0.25 * rng.integers(-16, 12), 0.25 * rng.integers(-16, 12)
            bs.append((x0, y0, x0 + 0.25 * rng.integers(1, 9), y0 + 0.25 * rng.integers(1, 9)))
        boxes.append(bs)
        slots.append(sorted(rng.choice(8, size=k, replace=False).tolist()))
        ns = int(rng.integers(0 if e == 3 else 1, 9))
        lattice = 0.25 * rng.integers(-20, 21, size=(ns, 2))
        sources.append(np.where(rng.random((ns, 1)) < 0.5, lattice, rng.uniform(-5.0, 5.0, size=(ns, 2))))
        lattice = 0.25 * rng.integers(-20, 21, size=(16, 2))
        points.append(np.where(rng.random((16, 1)) < 0.5, lattice, rng.uniform(-5.0, 5.0, size=(16, 2))))
    return boxes, slots, sources, points


def test_random_batch_is_bit_equal(gpu_device):
    boxes, slots, sources, points = _random_batch()
    margin = 0.125
    rec = _records(boxes, slots)
    t = _fields(gpu_device, [], margin, rec, sources)
    want, reach = [], 0
    for e in range(8):
        rects, nodes, dist = _check_field(t, e, [], margin, rec, sources[e])
        want.append(S.geodesic_query_numpy(rects, sources[e], nodes, dist, points[e]))
        reach += int(np.isfinite(dist).sum())
    got = _query(gpu_device, t, np.repeat(np.arange(8), 16), np.concatenate(points))
    want = np.concatenate(want)
    print("random batch: finite node distances", reach, "finite queries", int(np.isfinite(want).sum()), "of", len(want))
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert _same_bits(got, want), np.abs(got - want)[np.isfinite(want)].max()
    assert reach > 20 and 0 < int(np.isinf(want).sum()) < len(want)          # the batch has both kinds


def test_shared_walls_and_objects_with_gaps_in_the_slots(gpu_device):
    """Shared walls AND per-environment objects, valid slots interleaved with invalid ones; environment 2: all slots invalid."""
    walls = [(-4.0, -0.5, -1.0, 0.5), (1.0, -0.5, 4.0, 0.5), (-0.25, 2.0, 0.25, 3.0)]
    boxes = [[(-0.5, -1.5, 0.5, -1.0), (2.0, 1.0, 2.5, 1.5)], [(-1.0, -0.5, 1.0, 0.5)], []]      # (1: closes the doorway)
    slots = [[2, 7], [5], []]
    sources = [[(0.0, 4.0), (0.25, 4.0)]] * 3
    rec = _records(boxes, slots)
    rec[0, 4, :4], rec[0, 4, 6] = (-9.0, -9.0, 9.0, 9.0), 0.0                     # an invalid slot's numbers mean nothing
    t = _fields(gpu_device, walls, S.STEP_MARGIN, rec, sources)
    pts = [(0.0, -4.0), (0.0, 0.0), (3.0, -2.0)]
    for e in range(3):
        rects, nodes, dist = _check_field(t, e, walls, S.STEP_MARGIN, rec, sources[e])
        assert len(rects) == 3 + len(boxes[e])
        want = S.geodesic_query_numpy(rects, sources[e], nodes, dist, pts)
        assert _same_bits(_query(gpu_device, t, [e] * 3, pts), want), e
        assert np.isfinite(want[0]) and (np.isinf(want[1]) == (e == 1))          # (0, 0) lies inside the closing object


@functools.lru_cache(maxsize=None)
def _rooms_reference():
    lay = S.object_layout(0, 0, (0.0, 0.0))
    rec = _records([[b for _, b in lay]])
    rects = S.inflated_rects(rec[0])
    src = S.goal_viewpoints(lay[0][1], rects, 1.0)
    nodes, dist = S.geodesic_field_numpy(rects, src)
    for a in (rects, src, nodes, dist):
        a.setflags(write=False)
    return lay, rec, rects, src, nodes, dist


def test_rooms_world_field_through_the_renderer(gpu_device):
    """One full rooms-world field -- the walls and the two objects of object_layout(0, 0) -- through
    RoomsRenderer.geodesic_fields / geodesic_distances; a second environment without a target."""
    from vlfm_amd.harness import RoomsRenderer

    lay, rec, rects, src, nodes, dist = _rooms_reference()
    rooms = RoomsRenderer([0], 500, 48, 64, gpu_device)
    two = np.concatenate([rec, rec])
    h = rooms.geodesic_fields(two, [lay[0][1][:4], (np.nan,) * 4], 1.0)
    assert h.n == 2 and h.has_target.tolist() == [True, False]
    assert h.counts.cpu().numpy().tolist() == [[len(rects), len(nodes)]] * 2
    assert h.source_counts.cpu().numpy().tolist() == [len(src), 0]
    assert _same_bits(h.sources[0, :len(src)].cpu().numpy(), src)
    assert _same_bits(h.rects[0, :len(rects)].cpu().numpy(), rects) and _same_bits(h.nodes[0, :len(nodes)].cpu().numpy(), nodes)
    got = h.dist[0, :len(nodes)].cpu().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(dist)) and _same_bits(got, dist), np.abs(got - dist).max()
    assert np.isinf(h.dist[1].cpu().numpy()).all()                               # no source: nothing is reachable
    rng = np.random.default_rng(5)
    pts = np.concatenate([[(0.0, 0.0), (9.9, 9.9), (-8.6, 8.6)], 0.25 * rng.integers(-38, 39, size=(29, 2))])
    want = S.geodesic_query_numpy(rects, src, nodes, dist, pts)
    d = rooms.geodesic_distances(h, np.zeros(len(pts), np.int32), pts)           # all points in ONE field
    assert d.dtype.is_floating_point and d.shape == (len(pts),) and d.device.type == "cuda"
    assert _same_bits(d.cpu().numpy(), want) and np.isinf(want[1]) and np.isfinite(want[0])
    mixed = rooms.geodesic_distances(h, [0, 1, -1, 0], [(0.0, 0.0)] * 4).cpu().numpy()
    assert mixed[0] == want[0] and np.isinf(mixed[1]) and np.isnan(mixed[2]) and mixed[3] == want[0]
    # a handle row replaced on the device answers like the field it was replaced with
    h.assign([1], rooms.geodesic_fields(rec, [lay[0][1][:4]], 1.0))
    assert h.has_target.tolist() == [True, True]
    assert _same_bits(rooms.geodesic_distances(h, np.ones(len(pts), np.int32), pts).cpu().numpy(), want)
    with pytest.raises(ValueError):
        rooms.geodesic_distances(h, [2], [(0.0, 0.0)])
    assert rooms.geodesic_fields(rec[:0], np.zeros((0, 4)), 1.0).n == 0
    assert rooms.geodesic_distances(h, [], np.zeros((0, 2))).shape == (0,)


def test_empty_calls_and_refusals(gpu_device):
    import torch

    L = _lib()
    lib = L.lib()
    assert lib.vlfm_abi_version() >= 24
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vlfm_geodesic_fields(None, None, 0, 0, None, 0.2, None, None, None, 0, 8, None, None, None, None,
                                    st) == L.VLFM_OK                                                                   # n == 0
    assert lib.vlfm_geodesic_query(None, None, 0, 0, 0, None, None, None, None, None, None, 8, None, st) == L.VLFM_OK  # m == 0
    # tables that do not fit 64 KB of LDS are refused by status, before any launch: 134 walls + 8 slots = 142 rectangles
    B = 134
    walls = [(3.0 * i, 0.0, 3.0 * i + 1.0, 1.0) for i in range(B)]
    R = B + 8
    f64 = dict(dtype=torch.float64, device=gpu_device)
    bufs = dict(walls=torch.tensor(walls, **f64), rec=torch.zeros((1, 8, 8), **f64), src=torch.zeros((1, 8, 2), **f64),
                cnt=torch.zeros(1, dtype=torch.int32, device=gpu_device), rects=torch.full((1, R, 4), -7.0, **f64),
                nodes=torch.full((1, 4 * R, 2), -7.0, **f64), dist=torch.full((1, 4 * R), -7.0, **f64),
                counts=torch.full((1, 2), -7, dtype=torch.int32, device=gpu_device),
                nb=torch.tensor([B], dtype=torch.int32, device=gpu_device), wof=torch.zeros(1, dtype=torch.int32, device=gpu_device))
    p = {k: v.data_ptr() for k, v in bufs.items()}
    rc = lib.vlfm_geodesic_fields(p["walls"], p["nb"], 1, B, p["wof"], 0.2, p["rec"], p["src"], p["cnt"], 1, 8, p["rects"],
                                  p["nodes"], p["dist"], p["counts"], st)
    assert rc == L.VLFM_ERR_INVALID and "LDS" in L.last_error()
    torch.cuda.synchronize()
    assert bool((bufs["dist"] == -7.0).all()) and bool((bufs["counts"] == -7).all())                 # nothing written
    assert lib.vlfm_geodesic_fields(p["walls"], p["nb"], 1, -1, p["wof"], 0.2, p["rec"], p["src"], p["cnt"], 1, 8, p["rects"],
                                    p["nodes"], p["dist"], p["counts"], st) == L.VLFM_ERR_INVALID
    assert lib.vlfm_geodesic_fields(p["walls"], p["nb"], 1, 4, p["wof"], float("nan"), p["rec"], p["src"], p["cnt"], 1, 8,
                                    p["rects"], p["nodes"], p["dist"], p["counts"], st) == L.VLFM_ERR_INVALID
    assert lib.vlfm_geodesic_query(None, None, 3, 1, 4, p["rects"], p["nodes"], p["dist"], p["counts"], p["src"], p["cnt"], 8,
                                   None, st) == L.VLFM_ERR_INVALID
    # the largest wall count that fits does run (133 walls: 141 rectangles, 564 candidate nodes over 256 lanes)
    t = _fields(gpu_device, walls[:133], 0.25, np.zeros((1, 8, 8)), [[(-1.0, 0.5)]], max_sources=8)
    rects, nodes, dist = _check_field(t, 0, walls[:133], 0.25, np.zeros((1, 8, 8)), [(-1.0, 0.5)])
    assert len(nodes) == 4 * 133 and np.isfinite(dist).all()
    want = S.geodesic_query_numpy(rects, [(-1.0, 0.5)], nodes, dist, [(3.0 * 132 + 2.0, 0.5)])
    assert _same_bits(_query(gpu_device, t, [0], [(3.0 * 132 + 2.0, 0.5)]), want) and np.isfinite(want[0])
