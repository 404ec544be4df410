"""The host statement of the lattice geodesic (vlfm_amd/synthetic.py, section "Lattice geodesic": lattice_extent,
lattice_free_numpy, lattice_field_numpy, lattice_query_numpy, goal_viewpoints' grid test) and the refusals around it.  No device."""
import functools

import numpy as np
import pytest

import lattice_cases as C
from vlfm_amd import synthetic as S

NONE = S.LATTICE_NONE


def _allowed(free, a, b, dx, dy) -> bool:
    """The move rule, node by node: may a robot at (a, b) take the move (dx, dy)."""
    nb, na = free.shape
    at = lambda u, v: 0 <= u < na and 0 <= v < nb and bool(free[v, u])      # noqa: E731
    if not (at(a, b) and at(a + dx, b + dy)):
        return False
    if abs(dx) == 1 and abs(dy) == 1:
        return at(a + dx, b) and at(a, b + dy)
    if abs(dx) == 2:
        return at(a + dx // 2, b) and at(a + dx // 2, b + dy)
    if abs(dy) == 2:
        return at(a, b + dy // 2) and at(a + dx, b + dy // 2)
    return True


def _scipy_field(free, sources, max_cost=S.LATTICE_MAX_COST):
    """The same field by scipy's Dijkstra over a graph built edge by edge."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    nb, na = free.shape
    rows, cols, costs = [], [], []
    for b in range(nb):
        for a in range(na):
            for (dx, dy, c) in S.LATTICE_MOVES:
                if _allowed(free, a, b, dx, dy):
                    rows.append(b * na + a)
                    cols.append((b + dy) * na + a + dx)
                    costs.append(c)
    src = sorted({b * na + a for (a, b) in sources if 0 <= a < na and 0 <= b < nb and free[b, a]})
    out = np.full(nb * na, NONE, np.uint16)
    if src:
        g = csr_matrix((costs, (rows, cols)), shape=(nb * na, nb * na))
        d = dijkstra(g, directed=True, indices=src, min_only=True)
        ok = np.isfinite(d) & (d <= max_cost)
        out[ok] = d[ok].astype(np.uint16)
    return out.reshape(nb, na)


def test_the_host_field_is_scipys_dijkstra_on_random_lattices():
    rng = np.random.default_rng(20260)
    for case in range(100):
        nb, na = int(rng.integers(1, 34)), int(rng.integers(1, 41))
        if case < 4:
            nb, na = [(33, 40), (1, 40), (33, 1), (1, 1)][case]
        free = C.random_mask(rng, nb, na, 0.1 if case % 2 == 0 else 0.3)
        sources = np.stack([rng.integers(-1, na + 1, 3), rng.integers(-1, nb + 1, 3)], axis=1)
        cap = S.LATTICE_MAX_COST if case % 3 else 60
        got = S.lattice_field_numpy(free, sources + (7, -5), origin=(7, -5), max_cost=cap)
        assert got.dtype == np.uint16 and np.array_equal(got, _scipy_field(free, sources.tolist(), cap)), case


def _costs(rows, source=(0, 0)):
    free = np.array([[ch == "." for ch in row] for row in rows])
    return S.lattice_field_numpy(free, [source])


def test_corner_rules_on_hand_drawn_masks():
    open5 = _costs(["....."] * 5, (2, 2))
    assert open5[2].tolist() == [10, 5, 0, 5, 10] and open5[3, 3] == 7 and open5[4, 4] == 14
    assert open5[3, 4] == 11 and open5[4, 3] == 11 and open5[1, 0] == 11 and open5[0, 1] == 11 and open5[4, 0] == 14
    # a diagonal needs BOTH nodes beside it: one wall node at (1, 0) forbids (0, 0) -> (1, 1); the way round is (0, 1), (1, 1)
    d = _costs([".#...", ".....", ".....", ".....", "....."])
    assert d[1, 1] == 10 and d[0, 1] == NONE and d[1, 0] == 5
    # a knight move (2, 1) out of (0, 0) needs (1, 0) and (1, 1)
    assert _costs(["...", "..."])[1, 2] == 11
    assert _costs([".#.", "..."])[1, 2] == 5 + 5 + 5              # (1, 0) blocked: down, right, right
    assert _costs(["...", ".#."])[1, 2] == 5 + 5 + 5              # (1, 1) blocked: right, right, down
    assert _costs(["...", "#.."])[1, 2] == 11                     # (0, 1) is not on its way
    # (1, 2) out of (0, 0) needs (0, 1) and (1, 1)
    assert _costs(["..", "..", ".."])[2, 1] == 11
    assert _costs(["..", "#.", ".."])[2, 1] == 5 + 5 + 5
    assert _costs(["..", ".#", ".."])[2, 1] == 5 + 5 + 5
    assert _costs([".#", "..", ".."])[2, 1] == 11
    # no move leaves the lattice and comes back: a wall across a 3-wide lattice is final
    assert (_costs(["...", "###", "..."])[2] == NONE).all()
    # symmetric: the field from s at t is the field from t at s
    rng = np.random.default_rng(5)
    free = C.random_mask(rng, 12, 13, 0.25)
    free[0, 0] = free[11, 12] = True
    assert S.lattice_field_numpy(free, [(0, 0)])[11, 12] == S.lattice_field_numpy(free, [(12, 11)])[0, 0]


def test_max_cost_at_11_and_at_65534():
    free = np.ones((9, 9), bool)
    full = S.lattice_field_numpy(free, [(4, 4)], max_cost=65534)
    cut = S.lattice_field_numpy(free, [(4, 4)], max_cost=11)
    assert full.max() == 28 and np.array_equal(cut, np.where(full <= 11, full, NONE)) and (cut == 11).sum() == 8
    assert (S.lattice_field_numpy(free, [(4, 4)], max_cost=0) != NONE).sum() == 1
    for bad in (-1, 65535):
        with pytest.raises(ValueError):
            S.lattice_field_numpy(free, [(4, 4)], max_cost=bad)


def test_the_free_mask_of_a_plan_is_the_mask_of_its_cell_boxes():
    rng = np.random.default_rng(77)
    for case in range(6):
        plan = C.random_plan(rng, 40, 48, [0.05, 0.3, 0.6][case % 3], uniform=case >= 4)
        none = np.zeros((0, 4))
        ext = S.lattice_extent(none, plan, None, 20, 0.25)
        from_plan = S.lattice_free_numpy(ext, none, plan, None, 20)
        from_boxes = S.lattice_free_numpy(ext, S.grid_boxes(plan), None, None, 20)
        assert np.array_equal(from_plan, from_boxes) and 0 < from_plan.sum() < from_plan.size, case
    # an empty plan blocks nothing; a full one everything strictly inside its inflated extent
    full = S.GridPlan.uniform(np.ones((4, 4), bool), 4, 0, 0)                         # [0, 1]^2
    free = S.lattice_free_numpy((-8, -8, 37, 37), np.zeros((0, 4)), full, None, 20)    # nodes -0.4 .. 1.4
    x = np.arange(-8, 29) / 20.0
    inside = (0.0 - S.STEP_MARGIN < x) & (x < 1.0 + S.STEP_MARGIN)
    assert np.array_equal(~free, inside[:, None] & inside[None, :])
    assert not inside[4] and x[4] == -0.2 and inside[5]                                # OPEN: the node ON the inflated edge is free


def test_grid_plans_of_procedural_worlds_give_their_box_worlds_masks_and_fields():
    worlds = S.ProceduralWorlds(seed=3)
    for (env, ep) in ((0, 0), (5, 2)):
        w = worlds.world(env, ep)
        plan = S.GridPlan.from_boxes(w.boxes, 20)
        ext = S.lattice_extent(w.boxes, None, None, 20)
        assert ext == S.lattice_extent(np.zeros((0, 4)), plan, None, 20)
        free = S.lattice_free_numpy(ext, w.boxes, None, None, 20)
        assert np.array_equal(free, S.lattice_free_numpy(ext, np.zeros((0, 4)), plan, None, 20))
        src = S.lattice_sources([w.start_xy], 20)
        field = S.lattice_field_numpy(free, src, ext[:2])
        assert field[tuple((src[0] - ext[:2])[::-1])] == 0 and (field != NONE).sum() > 1000


@functools.lru_cache(maxsize=None)
def _band(env, ep):
    """(graph distance, lattice distance) of every 0.25 m point of the rooms world the inflated obstacles do not hold, for the
    layout's first object as the target."""
    objs = np.zeros((S.WORLD_MAX_OBJECTS, 8))
    for k, (_, box) in enumerate(S.object_layout(env, ep, np.zeros(2))):
        objs[k, :6], objs[k, 6] = box, 1.0
    rects = S.inflated_rects(objs, S.STEP_MARGIN)
    src = S.goal_viewpoints(objs[0, :4], rects, 1.0)
    nodes, dist = S.geodesic_field_numpy(rects, src)
    ext = S.lattice_extent(None, None, objs, 20)
    field = S.lattice_field_numpy(S.lattice_free_numpy(ext, None, None, objs, 20), S.lattice_sources(src, 20), ext[:2])
    a = 0.25 * np.arange(-40, 41)
    pts = np.stack(np.meshgrid(a, a, indexing="ij"), axis=-1).reshape(-1, 2)
    pts = pts[~S._within(pts[:, 0], pts[:, 1], rects, 0.0)]
    return S.geodesic_query_numpy(rects, src, nodes, dist, pts), S.lattice_query_numpy(field, ext[:2], pts, 20), field


@pytest.mark.parametrize("env,ep", C.BAND_LAYOUTS)
def test_the_band_against_the_visibility_graph_in_the_rooms_world(env, ep):
    g, l, field = _band(env, ep)
    assert np.array_equal(np.isfinite(g), np.isfinite(l))                  # finite / inf agree at every point
    far = np.isfinite(g) & (g > 1.0)
    ratio = l[far] / g[far]
    print(f"layout ({env}, {ep}): {far.sum()} points, l / g in [{ratio.min():.5f}, {ratio.max():.5f}], mean {ratio.mean():.5f}, "
          f"largest cost {field[field != NONE].max()}")
    assert far.sum() > 4000 and C.BAND_LO <= ratio.min() and ratio.max() <= C.BAND_HI
    assert (l[np.isfinite(g) & (g == 0.0)] == 0.0).all()                   # a view point is a source of both


def test_goal_viewpoints_against_a_plan_is_the_brute_force_over_its_cell_boxes():
    rng = np.random.default_rng(9)
    none = np.zeros((0, 4))
    for case in range(4):
        plan = C.random_plan(rng, 40, 48, 0.02, uniform=case % 2 == 0)
        box = (0.1, -0.2, 0.4, 0.3)
        got = S.goal_viewpoints(box, none, 0.75, grid=plan)
        cells = S.grid_boxes(plan)
        want = S.goal_viewpoints(box, none, 0.75, boxes=cells)
        m = S.STEP_MARGIN
        brute = S.goal_viewpoints(box, np.stack([cells[:, 0] - m, cells[:, 1] - m, cells[:, 2] + m, cells[:, 3] + m], axis=1), 0.75)
        assert np.array_equal(got, want) and np.array_equal(got, brute) and 0 < len(got) < len(S.goal_viewpoints(box, none, 0.75))
    # without the keywords: what it returned before they existed
    rects = S.inflated_rects(None, S.STEP_MARGIN)
    assert np.array_equal(S.goal_viewpoints((0.0, 2.4, 0.5, 2.9), rects, 1.0), S.goal_viewpoints((0.0, 2.4, 0.5, 2.9), rects, 1.0, boxes=none))


def test_every_view_point_is_a_free_node():
    for (env, ep) in C.BAND_LAYOUTS[:2]:
        objs = np.zeros((S.WORLD_MAX_OBJECTS, 8))
        for k, (_, box) in enumerate(S.object_layout(env, ep, np.zeros(2))):
            objs[k, :6], objs[k, 6] = box, 1.0
        src = S.goal_viewpoints(objs[0, :4], S.inflated_rects(objs, S.STEP_MARGIN), 1.0)
        ext = S.lattice_extent(None, None, objs, 20)
        nodes = S.lattice_sources(src, 20)
        assert np.array_equal(nodes / 20.0, src)                           # 5 k / 20 is exactly 0.25 k
        local = nodes - ext[:2]
        assert S.lattice_free_numpy(ext, None, None, objs, 20)[local[:, 1], local[:, 0]].all()


def test_the_query_rule():
    field = np.full((3, 4), NONE, np.uint16)
    field[1, 1], field[1, 2] = 10, 5
    q = lambda *p: S.lattice_query_numpy(field, (8, -4), [p], 4).tolist()[0]         # noqa: E731  nodes 2.0 .. 2.75 by -1.0 .. -0.5
    assert q(2.25, -0.75) == 10 / 20.0 and q(2.5, -0.75) == 5 / 20.0                 # on a node: dx = dy = 0
    assert q(2.375, -0.75) == min(0.125 + 10 / 20.0, 0.125 + 5 / 20.0)               # on a cell edge
    assert q(2.3, -0.8) == min(np.sqrt((2.3 - 2.25) ** 2 + (-0.8 + 0.75) ** 2) + 0.5, np.sqrt((2.3 - 2.5) ** 2 + (-0.8 + 0.75) ** 2) + 0.25)
    assert q(2.0, -1.0) == float(np.sqrt(0.25 * 0.25 + 0.25 * 0.25) + 0.5)            # only (1, 1) of its four nodes holds a cost
    assert q(1.9, -0.75) == np.inf and q(3.0, -0.75) == np.inf and q(2.25, 5.0) == np.inf and q(np.nan, 0.0) == np.inf
    assert q(2.74, -0.51) == float(np.sqrt((2.74 - 2.5) ** 2 + (-0.51 + 0.75) ** 2) + 0.25)   # nodes beyond the lattice do not exist


def test_refusals():
    for bad in (0, 2, 10, 20.5, -4):
        with pytest.raises(ValueError, match="multiple of 4"):
            S.lattice_extent(None, None, None, bad)
    with pytest.raises(ValueError, match="1024"):
        S.lattice_extent([(-30.0, 0.0, 30.0, 1.0)], None, None, 20)                  # 62.4 m at 20 per metre
    # STEP_MARGIN + 0.8 is exactly 1: nodes -512 .. 511 are 1024 and fit, -512 .. 512 do not
    assert S.lattice_extent([(-127.0, 0.0, 126.75, 1.0)], None, None, 4, 0.8) == (-512, -4, 1024, 13)
    with pytest.raises(ValueError, match="1024"):
        S.lattice_extent([(-127.0, 0.0, 127.0, 1.0)], None, None, 4, 0.8)
    with pytest.raises(ValueError):
        S.lattice_extent(None, None, None, 20, pad_m=-1.0)
    with pytest.raises(ValueError, match="view points"):                             # more than GEODESIC_MAX_SOURCES, as today
        S.goal_viewpoints((0.0, 0.0, 0.5, 0.5), np.zeros((0, 4)), 3.0, grid=C.drawn_plans()[0])


def test_the_harness_checks_the_backend_before_any_device_is_touched():
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    worlds = S.GridWorlds(C.drawn_plans())
    kw = dict(device="cuda:0", use_blip2=False, select_frontiers=True, closed_loop=True, world_objects=WorldObjects(),
              objectnav_metrics=True)
    with pytest.raises(ValueError, match='geodesic="lattice"'):                       # "graph" with grid worlds still raises
        BatchedEpisodes(2, worlds=worlds, **kw)
    with pytest.raises(ValueError, match='geodesic="lattice"'):
        BatchedEpisodes(2, worlds=worlds, geodesic="graph", **kw)
    with pytest.raises(ValueError, match="geodesic"):
        BatchedEpisodes(2, geodesic="navmesh", **kw)
    with pytest.raises(ValueError, match="objectnav_metrics"):                        # a backend without the metrics it serves
        BatchedEpisodes(2, device="cuda:0", use_blip2=False, select_frontiers=True, closed_loop=True, geodesic="lattice")
