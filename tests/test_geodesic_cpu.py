"""The host statement of the geodesic rule behind the ObjectNav metrics (vlfm_amd/synthetic.py: inflated_rects, goal_viewpoints,
geodesic_field_numpy, geodesic_query_numpy, spl, soft_spl).  No device."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S

SQRT2 = float(np.sqrt(2.0))
UNIT = np.array([[-1.0, -1.0, 1.0, 1.0]])          # one box, margin 0
# (environment, episode) of the built-in layouts the rooms-world checks use, robot at (0, 0)
LAYOUTS = [(0, 0), (1, 3), (4, 0), (6, 2)]


def _d(rects, sources, points):
    nodes, dist = S.geodesic_field_numpy(rects, sources)
    return S.geodesic_query_numpy(rects, sources, nodes, dist, points)


def test_no_rectangles_nearest_source():
    src = [(3.0, 4.0), (1.0, 1.0), (-2.0, 0.5)]
    nodes, dist = S.geodesic_field_numpy(np.zeros((0, 4)), src)
    assert nodes.shape == (0, 2) and dist.shape == (0,)
    got = _d(np.zeros((0, 4)), src, [(0.0, 0.0), (3.0, 4.0), (-5.0, 0.5)])
    assert got.tolist() == [float(np.sqrt(1.0 * 1.0 + 1.0 * 1.0)), 0.0, 3.0]


def test_one_box_around():
    src = [(2.0, 0.0)]
    nodes, dist = S.geodesic_field_numpy(UNIT, src)
    assert nodes.tolist() == [[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]]
    assert dist.tolist() == [SQRT2 + 2.0, SQRT2, SQRT2, SQRT2 + 2.0]
    d = float(_d(UNIT, src, [(-2.0, 0.0)])[0])
    assert d == (SQRT2 + 2.0) + SQRT2                  # w(p, c) + dist[c], dist[c] = dist[u] + w(u, c): the rule's order
    assert abs(d - (2.0 + 2.0 * np.sqrt(2.0))) <= 1e-12


def test_edges_and_corners_are_free_interiors_are_not():
    blocked = lambda p, q: bool(S.segments_blocked_numpy([p], [q], UNIT)[0, 0])      # noqa: E731
    assert not blocked((-1.0, -1.0), (1.0, -1.0)) and not blocked((-3.0, 1.0), (3.0, 1.0))        # along an edge
    assert not blocked((-2.0, 0.0), (0.0, -2.0)) and not blocked((0.0, 2.0), (2.0, 0.0))          # through a corner
    assert blocked((-1.0, -1.0), (1.0, 1.0)) and blocked((-2.0, 0.0), (2.0, 0.0))                 # the diagonal, straight through
    assert blocked((-2.0, 0.5), (0.0, 0.5)) and blocked((0.0, 0.5), (-2.0, 0.5))                  # ends inside / starts inside
    assert not blocked((-3.0, 0.0), (-1.0, 0.0))                                                  # stops AT the boundary
    assert not blocked((2.0, 2.0), (2.0, 2.0)) and blocked((0.0, 0.0), (0.0, 0.0))                # a point
    # along an edge to a source: the straight distance
    assert _d(UNIT, [(3.0, 1.0)], [(-3.0, 1.0)]).tolist() == [6.0]


def test_inside_a_rectangle_and_enclosed_sources_are_unreachable():
    assert np.isinf(_d(UNIT, [(2.0, 0.0)], [(0.0, 0.0), (0.5, -0.99)])).all()
    # sources inside the box: nobody reaches them, no corner either
    nodes, dist = S.geodesic_field_numpy(UNIT, [(0.0, 0.0), (0.5, 0.5)])
    assert np.isinf(dist).all() and len(nodes) == 4
    assert np.isinf(_d(UNIT, [(0.0, 0.0), (0.5, 0.5)], [(-2.0, 0.0), (5.0, 5.0)])).all()
    # a source walled in by four overlapping boxes (a ring around the origin)
    ring = np.array([[-3.0, -3.0, 3.0, -2.0], [-3.0, 2.0, 3.0, 3.0], [-3.0, -3.0, -2.0, 3.0], [2.0, -3.0, 3.0, 3.0]])
    got = _d(ring, [(0.0, 0.0)], [(5.0, 0.0), (1.0, 1.0)])
    assert np.isinf(got[0]) and got[1] == SQRT2
    # no source at all
    assert np.isinf(_d(UNIT, np.zeros((0, 2)), [(-2.0, 0.0)])).all()


def test_nodes_inside_another_rectangle_are_dropped():
    two = np.array([[0.0, 0.0, 2.0, 2.0], [1.0, 1.0, 3.0, 3.0]])
    assert S.geodesic_nodes_numpy(two).tolist() == [[0.0, 0.0], [2.0, 0.0], [0.0, 2.0], [3.0, 1.0], [3.0, 3.0], [1.0, 3.0]]
    # a corner ON another rectangle's boundary stays
    touch = np.array([[0.0, 0.0, 2.0, 2.0], [2.0, 1.0, 3.0, 3.0]])
    assert len(S.geodesic_nodes_numpy(touch)) == 8


def test_inflated_rects_are_the_kinematics_doubles():
    objs = np.zeros((8, 8))
    objs[0, :6], objs[0, 6] = S.object_box("chair", 3.2, 0.4), 1.0
    objs[3, :6], objs[3, 6] = S.object_box("tv", -0.4, -1.8), 1.0
    objs[5, :6] = S.object_box("bed", 0.0, 2.6)                        # valid == 0: not an obstacle
    r = S.inflated_rects(objs)
    m = S.STEP_MARGIN
    assert len(r) == len(S.BOXES) + 2
    assert np.array_equal(r[:len(S.BOXES), 0], S.BOXES[:, 0] - m) and np.array_equal(r[:len(S.BOXES), 3], S.BOXES[:, 3] + m)
    assert r[-2].tolist() == [objs[0, 0] - m, objs[0, 1] - m, objs[0, 2] + m, objs[0, 3] + m]
    assert r[-1].tolist() == [objs[3, 0] - m, objs[3, 1] - m, objs[3, 2] + m, objs[3, 3] + m]
    assert np.array_equal(S.inflated_rects(objs[[0, 3], :6]), r) and len(S.inflated_rects()) == len(S.BOXES)
    assert S.inflated_rects([(0.0, 0.0, 1.0, 1.0)], margin=0.0, boxes=np.zeros((0, 4))).tolist() == [[0.0, 0.0, 1.0, 1.0]]


def test_goal_viewpoints_on_one_box():
    box = (0.0, 0.0, 0.5, 0.5)
    rects = S.inflated_rects([box], margin=0.2, boxes=np.zeros((0, 4)))
    pts = S.goal_viewpoints(box, rects, 0.5)
    # by hand: lattice points within 0.5 of the footprint and outside the closed [-0.2, 0.7]^2
    want = []
    for i in range(-4, 8):
        for j in range(-4, 8):
            x, y = 0.25 * i, 0.25 * j
            dx, dy = max(0.0 - x, 0.0, x - 0.5), max(0.0 - y, 0.0, y - 0.5)
            if dx * dx + dy * dy <= 0.25 and not (-0.2 <= x <= 0.7 and -0.2 <= y <= 0.7):
                want.append([x, y])
    assert pts.tolist() == want and len(want) == 28
    assert [-0.5, 0.0] in want and [-0.25, -0.25] in want and [-0.5, -0.25] not in want and [0.75, 0.25] in want
    assert [0.0, 0.0] not in want and [-0.25, 0.0] in want
    for p in pts:
        assert S.rect_distance(p, box) <= 0.5
    # another obstacle over some of them takes those away
    fewer = S.goal_viewpoints(box, np.concatenate([rects, [[-1.0, -1.0, -0.25, 2.0]]]), 0.5)
    assert len(fewer) < len(pts) and all(p[0] > -0.25 for p in fewer)
    with pytest.raises(ValueError, match="view points"):
        S.goal_viewpoints((0.0, 0.0, 4.0, 4.0), np.zeros((0, 4)), 1.0)            # 25 x 25 lattice points and more
    with pytest.raises(ValueError, match="view points"):
        S.goal_viewpoints(box, rects, 0.5, max_points=27)
    assert len(S.goal_viewpoints(box, rects, 0.5, max_points=28)) == 28


def test_spl_and_soft_spl_by_hand():
    assert S.spl(True, 4.0, 8.0) == 0.5 and S.spl(True, 4.0, 4.0) == 1.0
    assert S.spl(True, 4.0, 3.0) == 1.0                                  # p < l: max(p, l) = l
    assert S.spl(False, 4.0, 8.0) == 0.0
    assert S.spl(True, 0.0, 0.0) == 1.0 and S.spl(True, 0.0, 2.0) == 1.0   # l == 0: the ratio is 1
    assert S.spl(True, float("inf"), 3.0) == 0.0 and S.spl(True, float("nan"), 3.0) == 0.0
    assert S.soft_spl(1.0, 4.0, 8.0) == 0.75 * 0.5
    assert S.soft_spl(0.0, 4.0, 4.0) == 1.0 and S.soft_spl(0.0, 4.0, 3.0) == 1.0
    assert S.soft_spl(6.0, 4.0, 8.0) == 0.0                              # farther than at the start: clamped
    assert S.soft_spl(4.0, 4.0, 0.0) == 0.0                              # a failure that never moved
    assert S.soft_spl(0.0, 0.0, 0.0) == 1.0 and S.soft_spl(0.5, 0.0, 1.0) == 0.0
    assert S.soft_spl(float("inf"), 4.0, 1.0) == 0.0 and S.soft_spl(1.0, float("nan"), 1.0) == 0.0


@functools.lru_cache(maxsize=None)
def _rooms_case(e: int, ep: int):
    lay = S.object_layout(e, ep, (0.0, 0.0))
    rects = S.inflated_rects(np.array([b for _, b in lay]))
    src = S.goal_viewpoints(lay[0][1], rects, 1.0)
    nodes, dist = S.geodesic_field_numpy(rects, src)
    return lay, rects, src, nodes, dist


def _grid_distance(rects, sources, start, h=0.05):
    """8-connected Dijkstra distance on the h-grid over [-10, 10]^2 from the grid points nearest to ``sources`` to ``start``:
    a cell is free iff `step_poses`' CLOSED test does not block it; a diagonal move may not cut a blocked cell's corner."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra

    n = int(round(20.0 / h)) + 1
    xs = -10.0 + np.arange(n) * h
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    free = ~np.any((rects[:, 0] <= gx[..., None]) & (gx[..., None] <= rects[:, 2]) &
                   (rects[:, 1] <= gy[..., None]) & (gy[..., None] <= rects[:, 3]), axis=2)
    idx = np.arange(n * n).reshape(n, n)
    rows, cols, wts = [], [], []
    for di, dj in ((1, 0), (0, 1), (1, 1), (1, -1)):
        a = (slice(0, n - di), slice(max(0, -dj), n - max(0, dj)))
        b = (slice(di, n), slice(max(0, dj), n - max(0, -dj)))
        ok = free[a] & free[b]
        if di and dj:                                     # both cells beside the diagonal must be free
            ok &= free[(a[0], b[1])] & free[(b[0], a[1])]
        rows.append(idx[a][ok])
        cols.append(idx[b][ok])
        wts.append(np.full(int(ok.sum()), h * (np.sqrt(2.0) if di and dj else 1.0)))
    g = coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n)).tocsr()
    cell = lambda p: int(idx[int(round((p[0] + 10.0) / h)), int(round((p[1] + 10.0) / h))])       # noqa: E731
    src = sorted({cell(p) for p in sources if free.reshape(-1)[cell(p)]})
    return float(dijkstra(g, directed=False, indices=src, min_only=True)[cell(start)])


@pytest.mark.parametrize("e,ep", LAYOUTS)
def test_rooms_world_distance_between_its_bounds(e, ep):
    lay, rects, src, nodes, dist = _rooms_case(e, ep)
    assert len(rects) == len(S.BOXES) + 2 and 0 < len(src) <= S.GEODESIC_MAX_SOURCES
    d = float(S.geodesic_query_numpy(rects, src, nodes, dist, [(0.0, 0.0)])[0])
    straight = S.rect_distance((0.0, 0.0), lay[0][1])
    grid = _grid_distance(rects, src, (0.0, 0.0))
    print(f"layout ({e}, {ep}): nodes {len(nodes)}, view points {len(src)}, d {d:.6f}, through the walls {straight:.6f}, "
          f"grid {grid:.6f}, grid / d {grid / d:.4f}")
    assert np.isfinite(d)
    assert d >= straight - 1.0                           # no path beats the straight line to the success disc
    assert d <= grid + 1e-9                              # every grid path is a path
    assert np.isfinite(dist).any()
    # every view point itself is at distance 0, and the field agrees with the query at its own nodes
    assert S.geodesic_query_numpy(rects, src, nodes, dist, src[:3]).tolist() == [0.0] * min(3, len(src))
    at_nodes = S.geodesic_query_numpy(rects, src, nodes, dist, nodes)
    assert np.array_equal(at_nodes <= dist, np.ones(len(nodes), bool))


def test_the_known_slits():
    """Two inflated rectangles that exactly abut leave a zero-width slit the open-set rule lets a path through (it can only
    shorten l): among the built-in (class, spot) pairs that is a bed or a couch on two spots, against a pillar or the east wall."""
    walls = S.inflated_rects()
    hits = []
    for cls in S.OBJECT_SIZES:
        for spot in S.OBJECT_SPOTS:
            o = S.inflated_rects([S.object_box(cls, *spot)], boxes=np.zeros((0, 4)))[0]
            for w in walls:
                ox, oy = min(o[2], w[2]) - max(o[0], w[0]), min(o[3], w[3]) - max(o[1], w[1])
                if ((o[2] == w[0] or o[0] == w[2]) and oy > 0) or ((o[3] == w[1] or o[1] == w[3]) and ox > 0):
                    hits.append((cls, spot))
    assert hits == [("bed", (3.2, -3.2)), ("bed", (8.8, 8.6)), ("couch", (3.2, -3.2)), ("couch", (8.8, 8.6))]
