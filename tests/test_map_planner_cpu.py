"""The host statement of the map planner (synthetic.plan_paths_numpy) against code that shares nothing with it --
scipy.sparse.csgraph.dijkstra over a graph built edge by edge from the move rule -- its descent and statuses on hand-made
cases, and MapPlannerController over a stub ``obstacles`` that plans on the host."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from vlfm_amd.synthetic import (ACTION_FORWARD, ACTION_STOP, ACTION_TURN_LEFT, PLAN_INVALID, PLAN_NONE, PLAN_OK, PLAN_TOO_LONG,
                                PLAN_UNREACHABLE, BangBangController, MapPlannerController, plan_paths_numpy)

DX = (1, 1, 0, -1, -1, -1, 0, 1)        # chain codes E NE N NW W SW S SE, y grows downwards (csrc/bitmap.h)
DY = (0, -1, -1, -1, 0, 1, 1, 1)


def _free_of(plane, job):
    """The free cells of the job's window, cell by cell, from the rule's words."""
    _, y0, y1, x0, x1, sx, sy, rs, gx, gy, rg = job
    free = np.zeros((y1 - y0 + 1, x1 - x0 + 1), bool)
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            free[y - y0, x - x0] = bool(plane[y, x]) or (x - sx) ** 2 + (y - sy) ** 2 <= rs * rs or \
                (x - gx) ** 2 + (y - gy) ** 2 <= rg * rg
    return free


def _allowed(free, x, y, s):
    h, w = free.shape
    inside = lambda a, b: 0 <= a < w and 0 <= b < h and free[b, a]   # noqa: E731
    nx, ny = x + DX[s], y + DY[s]
    if not (inside(x, y) and inside(nx, ny)):
        return False
    if DX[s] and DY[s]:
        return bool(inside(nx, y) and inside(x, ny))
    return True


def _scipy_field(free, gx, gy, max_cost):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    h, w = free.shape
    rows, cols, wts = [], [], []
    for y in range(h):
        for x in range(w):
            for s in range(8):
                if _allowed(free, x, y, s):
                    rows.append(y * w + x)
                    cols.append((y + DY[s]) * w + x + DX[s])
                    wts.append(3.0 if s & 1 else 2.0)
    g = csr_matrix((wts, (rows, cols)), shape=(h * w, h * w))
    d = dijkstra(g, directed=True, indices=gy * w + gx).reshape(h, w)
    return np.where(np.isfinite(d) & (d <= max_cost), d, PLAN_NONE).astype(np.uint16), d


def _random_case(rng):
    n = int(rng.integers(5, 41))
    plane = rng.random((n, n)) >= rng.uniform(0.1, 0.45)
    y0, y1 = sorted(int(v) for v in rng.integers(0, n, 2))
    x0, x1 = sorted(int(v) for v in rng.integers(0, n, 2))
    sx, gx = (int(v) for v in rng.integers(x0, x1 + 1, 2))
    sy, gy = (int(v) for v in rng.integers(y0, y1 + 1, 2))
    job = (0, y0, y1, x0, x1, sx, sy, int(rng.integers(0, 4)), gx, gy, int(rng.integers(0, 4)))
    return plane, job


def test_fields_equal_scipy_on_random_planes():
    rng = np.random.default_rng(20260)
    seen = {PLAN_OK: 0, PLAN_UNREACHABLE: 0, PLAN_TOO_LONG: 0}
    for case in range(200):
        plane, job = _random_case(rng)
        max_cost = int(rng.choice([65534, 65534, 30, 9]))
        lookahead = int(rng.integers(0, 12))
        res, fields = plan_paths_numpy(plane, [job], lookahead, max_cost)
        _, y0, y1, x0, x1, sx, sy, rs, gx, gy, rg = job
        free = _free_of(plane, job)
        want, exact = _scipy_field(free, gx - x0, gy - y0, max_cost)
        assert fields[0].dtype == np.uint16 and np.array_equal(fields[0], want), (case, job)
        status, cost, wx, wy, steps = (int(v) for v in res[0])
        d_start = exact[sy - y0, sx - x0]
        if np.isfinite(d_start) and d_start <= max_cost:
            assert status == PLAN_OK and cost == int(d_start), (case, job)
            # the descent: at most `lookahead` allowed steps, each dropping the cost by exactly its own
            assert steps <= lookahead and (steps == lookahead or (wx, wy) == (gx, gy))
            assert int(want[wy - y0, wx - x0]) <= cost
            cx, cy = sx - x0, sy - y0
            for _ in range(steps):
                for s in range(8):
                    if _allowed(free, cx, cy, s) and int(want[cy + DY[s], cx + DX[s]]) + (3 if s & 1 else 2) == int(want[cy, cx]):
                        cx, cy = cx + DX[s], cy + DY[s]
                        break
                else:
                    raise AssertionError("no descending step")
            assert (cx + x0, cy + y0) == (wx, wy), (case, job)
        else:
            beyond = bool((np.isfinite(exact) & (exact > max_cost)).any())
            assert status == (PLAN_TOO_LONG if beyond else PLAN_UNREACHABLE), (case, job)
            assert (cost, wx, wy, steps) == (PLAN_NONE, sx, sy, 0)
        seen[status] += 1
    assert min(seen.values()) >= 5, seen


def test_first_code_breaks_ties():
    # a pillar in the middle of an open 5 x 5 room, start below it, goal above it: left and right are mirror images, cost 10
    # either way (diagonal, straight, straight, diagonal); NE is chain code 1, NW is 3: the path goes round the RIGHT side
    plane = np.ones((5, 5), bool)
    plane[2, 2] = False
    job = (0, 0, 4, 0, 4, 2, 4, 0, 2, 0, 0)
    for lookahead, want in ((1, (3, 3)), (2, (3, 2)), (3, (3, 1)), (4, (2, 0)), (9, (2, 0))):
        res, fields = plan_paths_numpy(plane, [job], lookahead)
        assert tuple(res[0]) == (PLAN_OK, 10, *want, min(lookahead, 4))
    assert fields[0][4, 2] == 10 and fields[0][3, 1] == fields[0][3, 3] == 7 and fields[0][2, 2] == PLAN_NONE
    # no ties about E before N: two steps east and one north-east in some order, E (code 0) goes first
    res, _ = plan_paths_numpy(np.ones((6, 6), bool), [(0, 0, 3, 0, 5, 0, 2, 0, 3, 1, 0)], 1)
    assert tuple(res[0]) == (PLAN_OK, 7, 1, 2, 1)


def test_a_diagonal_gap_is_not_passable():
    plane = np.array([[1, 0], [0, 1]], bool)             # two obstacles touching at a corner, seen from the free cells
    res, fields = plan_paths_numpy(plane, [(0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 0)])
    assert res[0, 0] == PLAN_UNREACHABLE and fields[0][0, 0] == PLAN_NONE
    plane = np.array([[1, 1], [0, 1]], bool)             # one of the two cells opened: still no diagonal (corner cutting) ...
    res, _ = plan_paths_numpy(plane, [(0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 0)])
    assert tuple(res[0, :2]) == (PLAN_OK, 4)             # ... but the way round: E, S
    res, _ = plan_paths_numpy(np.ones((2, 2), bool), [(0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 0)])
    assert tuple(res[0, :2]) == (PLAN_OK, 3)


def test_every_status_on_a_hand_made_case():
    corridor = np.zeros((12, 12), bool)                  # (maps are square; the jobs' windows are rows 0-2)
    corridor[1, :] = True
    ok = (0, 0, 2, 0, 11, 0, 1, 0, 11, 1, 0)
    res, fields = plan_paths_numpy(corridor, [ok], 4)
    assert tuple(res[0]) == (PLAN_OK, 22, 4, 1, 4)
    # max_cost cuts a reachable path: cells beyond it are still to expand
    res, fields = plan_paths_numpy(corridor, [ok], 4, max_cost=20)
    assert tuple(res[0]) == (PLAN_TOO_LONG, PLAN_NONE, 0, 1, 0)
    assert fields[0][1].tolist() == [PLAN_NONE] + list(range(20, -1, -2))
    res, _ = plan_paths_numpy(corridor, [ok], 4, max_cost=22)
    assert res[0, 0] == PLAN_OK
    # a walled-in start: the start cell itself is free (radius 0), its neighbours are not
    walled = corridor.copy()
    walled[1, 0:3] = False
    res, _ = plan_paths_numpy(walled, [ok], 4)
    assert tuple(res[0]) == (PLAN_UNREACHABLE, PLAN_NONE, 0, 1, 0)
    res, _ = plan_paths_numpy(walled, [(0, 0, 2, 0, 11, 0, 1, 3, 11, 1, 0)], 4)      # ... a free radius of 3 opens the way
    assert tuple(res[0, :2]) == (PLAN_OK, 22)
    # walled in and max_cost never reached: UNREACHABLE, not TOO_LONG
    res, _ = plan_paths_numpy(walled, [ok], 4, max_cost=40)
    assert res[0, 0] == PLAN_UNREACHABLE
    bad = [(1, 0, 2, 0, 11, 0, 1, 0, 11, 1, 0),          # slot out of range
           (0, 2, 0, 0, 11, 0, 1, 0, 11, 1, 0),          # empty window
           (0, 0, 12, 0, 11, 0, 1, 0, 11, 1, 0),         # window outside the map
           (0, 0, 2, -1, 11, 0, 1, 0, 11, 1, 0),
           (0, 0, 2, 1, 11, 0, 1, 0, 11, 1, 0),          # start outside the window
           (0, 0, 2, 0, 10, 0, 1, 0, 11, 1, 0),          # goal outside the window
           (0, 0, 2, 0, 11, 0, 1, -1, 11, 1, 0)]         # a negative radius
    res, fields = plan_paths_numpy(corridor, bad + [ok], 4)
    assert (res[:-1, 0] == PLAN_INVALID).all() and all(f is None for f in fields[:-1])
    assert all(tuple(r[1:]) == (PLAN_NONE, b[5], b[6], 0) for r, b in zip(res[:-1], bad))
    assert tuple(res[-1]) == (PLAN_OK, 22, 4, 1, 4)      # the valid job beside them is unaffected
    # start == goal, and neighbours
    res, _ = plan_paths_numpy(corridor, [(0, 0, 2, 0, 11, 5, 1, 0, 5, 1, 0), (0, 0, 2, 0, 11, 5, 1, 0, 6, 1, 0)], 4)
    assert tuple(res[0]) == (PLAN_OK, 0, 5, 1, 0) and tuple(res[1]) == (PLAN_OK, 2, 6, 1, 1)
    # the window blocks what lies outside it
    room = np.ones((9, 9), bool)
    room[4, 1:] = False                                  # a wall with its gap at column 0
    res, _ = plan_paths_numpy(room, [(0, 0, 8, 0, 8, 4, 0, 0, 4, 8, 0), (0, 0, 8, 1, 8, 4, 0, 0, 4, 8, 0)])
    assert res[0, 0] == PLAN_OK and res[1, 0] == PLAN_UNREACHABLE


# ---------------------------------------------------------------------------------------------- the controller
class HostObstacles:
    """What MapPlannerController asks of an ObstacleMapBatch, answered on the host: the conversions of the map classes and
    plan_paths_numpy over ``planes`` [n,S,S]."""

    def __init__(self, planes, pixels_per_meter=20, kernel_size=7, status=None):
        self.planes = np.asarray(planes, bool)
        self.size, self.pixels_per_meter, self.kernel_size = self.planes.shape[1], pixels_per_meter, kernel_size
        self.force_status = status
        self.calls = []

    def cells_of(self, xy):
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        px = np.rint(xy[:, ::-1] * self.pixels_per_meter) + self.size // 2
        px[:, 0] = self.size - px[:, 0]
        return px.astype(np.int64)

    def px_to_xy(self, px):
        q = np.array(px, np.float64)
        q[:, 0] = self.size - q[:, 0]
        return ((q - self.size // 2) / self.pixels_per_meter)[:, ::-1]

    def plan_paths(self, starts_xy, goals_xy, env_ids=None, start_free_m=None, goal_free_m=None, lookahead_m=0.75):
        s, g = self.cells_of(starts_xy), self.cells_of(goals_xy)
        n = len(s)
        self.calls.append((np.array(starts_xy), np.array(goals_xy), np.array(env_ids), goal_free_m))
        rg = np.full(n, self.kernel_size // 2, np.int64)
        if goal_free_m is not None:
            gf = np.asarray(goal_free_m, np.float64)
            rg = np.where(np.isfinite(gf), np.rint(np.nan_to_num(gf) * self.pixels_per_meter), rg).astype(np.int64)
        jobs = [(int(env_ids[i]), 0, self.size - 1, 0, self.size - 1, s[i, 0], s[i, 1], self.kernel_size // 2, g[i, 0], g[i, 1],
                 rg[i]) for i in range(n)]
        res, _ = plan_paths_numpy(self.planes, jobs, max(1, int(round(lookahead_m * self.pixels_per_meter))))
        if self.force_status is not None:
            res[:, 0] = self.force_status
        ok = res[:, 0] == PLAN_OK
        return {"status": res[:, 0], "cost": res[:, 1], "path_m": np.where(ok, res[:, 1] * 0.5 / self.pixels_per_meter, np.inf),
                "waypoints": self.px_to_xy(res[:, 2:4]), "waypoints_px": res[:, 2:4], "steps": res[:, 4],
                "at_goal": ok & (res[:, 2] == g[:, 0]) & (res[:, 3] == g[:, 1])}


def _door_world():
    """A 200-cell map at 20 cells a metre: a wall 1 m ahead of the robot (rows 120-122: x forward is the row), with one door
    1.5 m to its left (columns 66-74: y left is the mirrored column), the goal 2 m straight ahead, behind the wall."""
    plane = np.ones((1, 200, 200), bool)
    plane[0, 120:123, :] = False
    plane[0, 120:123, 66:75] = True
    poses = np.array([[0.0, 0.0, 0.0]])
    goals = np.array([[2.0, 0.0]])
    return plane, poses, goals


def _rho_theta(poses, goals):
    d = goals - poses[:, :2]
    c, s = np.cos(-poses[:, 2]), np.sin(-poses[:, 2])
    lx, ly = c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]
    return np.stack([np.hypot(lx, ly), np.arctan2(ly, lx)], axis=1)


def test_controller_turns_towards_the_door():
    plane, poses, goals = _door_world()
    rt = _rho_theta(poses, goals)
    args = (["explore"], rt, np.zeros(1, bool), np.zeros(1, bool))
    assert BangBangController().act(*args)[0] == ACTION_FORWARD               # straight at the wall
    om = HostObstacles(plane)
    ctl = MapPlannerController(lookahead_m=0.75)
    assert ctl.act_on_map(om, poses, goals, [None], *args)[0] == ACTION_TURN_LEFT
    assert ctl.last_status.tolist() == [PLAN_OK]
    # the door lies ahead and to the left: every step of a shortest path is W or SW (chain codes 4, 5), so the waypoint is 15
    # columns (0.75 m) to the left and at most as far ahead: a bearing of 45 degrees or more
    start = om.cells_of(poses[:, :2])[0]
    res, _ = plan_paths_numpy(plane, [(0, 0, 199, 0, 199, start[0], start[1], 3, *om.cells_of(goals)[0], 3)], 15)
    assert res[0, 0] == PLAN_OK and res[0, 2] == start[0] - 15 and start[1] <= res[0, 3] <= start[1] + 15 and res[0, 4] == 15
    wp = om.px_to_xy(res[:, 2:4].astype(float))[0]
    assert wp[1] == 0.75 and 0.0 <= wp[0] <= 0.75
    assert ctl.last_cost_m[0] == res[0, 1] * 0.5 / 20 and ctl.last_cost_m[0] > 2.0
    assert rt[0, 1] == 0.0                                                    # the caller's array is not written
    # without maps it is the inner rule on the goal's bearing
    assert ctl.act(*args)[0] == ACTION_FORWARD


def test_controller_delegates():
    plane, poses, goals = _door_world()
    E = 5
    poses = np.repeat(poses, E, axis=0)
    goals = np.repeat(goals, E, axis=0)
    goals[1] = np.nan                                                          # no goal
    modes = ["explore", "explore", "initialize", "navigate", "explore"]
    stops = np.array([False, False, False, False, True])
    rt = np.where(np.isfinite(goals[:, :1]), _rho_theta(poses, np.nan_to_num(goals)), np.nan)
    collided = np.zeros(E, bool)
    om = HostObstacles(np.repeat(plane, E, axis=0))
    ctl = MapPlannerController()
    acts = ctl.act_on_map(om, poses, goals, [None, None, None, 0.9, None], modes, rt, stops, collided)
    # only the environments with a finite goal that neither stop nor initialise plan: ONE call for all of them
    assert len(om.calls) == 1 and om.calls[0][2].tolist() == [0, 3]
    assert np.isnan(om.calls[0][3][0]) and om.calls[0][3][1] == 0.9
    assert ctl.last_status.tolist() == [PLAN_OK, -1, -1, PLAN_OK, -1]
    assert acts.tolist() == [ACTION_TURN_LEFT, ACTION_STOP, ACTION_TURN_LEFT, ACTION_TURN_LEFT, ACTION_STOP]
    # a status other than PLAN_OK leaves (rho, theta) alone: the inner rule on the goal's bearing
    for status in (PLAN_UNREACHABLE, PLAN_TOO_LONG, PLAN_INVALID):
        om = HostObstacles(np.repeat(plane, E, axis=0), status=status)
        ctl, ref = MapPlannerController(), BangBangController()
        assert np.array_equal(ctl.act_on_map(om, poses, goals, None, modes, rt, stops, collided),
                              ref.act(modes, rt, stops, collided))
        assert ctl.last_status.tolist() == [status, -1, -1, status, -1] and np.isnan(ctl.last_cost_m).all()
    # the detour after a refused move is the inner rule's, whatever the plan says; reset reaches it
    om = HostObstacles(np.repeat(plane, E, axis=0))
    ctl, ref = MapPlannerController(), BangBangController()
    hit = np.array([True, False, False, False, False])
    for c in (hit, collided, collided, collided, collided, collided):
        a = ctl.act_on_map(om, poses, goals, None, modes, rt, stops, c)
        b = ref.act(modes, np.where(np.isnan(rt), rt, [[1.0, 1.0]]), stops, c)    # (theta = 1 rad: a left turn, like the plan's)
        assert a[0] == b[0]
    ctl.reset()
    assert ctl.inner.turns is None
    # a goal in the robot's own cell: the descent takes no step and the goal's own bearing stays
    near = poses.copy()
    near[:, :2] = goals[0] + [0.01, -0.02]
    rt2 = _rho_theta(near, np.repeat(goals[:1], E, axis=0))
    a = MapPlannerController().act_on_map(om, near, np.repeat(goals[:1], E, axis=0), None, ["explore"] * E, rt2, ~hit & False,
                                          collided)
    assert np.array_equal(a, BangBangController().act(["explore"] * E, rt2, ~hit & False, collided))
    with pytest.raises(ValueError):
        plan_paths_numpy(plane, [], 15, 65535)
