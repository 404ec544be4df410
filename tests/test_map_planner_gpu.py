"""-m gpu: the map planner's kernel (csrc/map_planner.hip through ObstacleMapBatch.plan_paths) against its host statement
(synthetic.plan_paths_numpy), == on results and fields, over hand-set navigable planes at the smallest shapes that can still
go wrong; MapPlannerController in the closed-loop harness."""
import numpy as np
import pytest

from vlfm_amd.synthetic import (PLAN_INVALID, PLAN_NONE, PLAN_OK, PLAN_TOO_LONG, PLAN_UNREACHABLE, BangBangController,
                                MapPlannerController, plan_paths_numpy)

pytestmark = pytest.mark.gpu
PPM = 20


def _batch(device, n_envs, size):
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    return ObstacleMapBatch(n_envs, min_height=0.61, max_height=0.88, agent_radius=0.18, size=size, pixels_per_meter=PPM,
                            device=device)


def _set_planes(om, planes):
    """navigable_bits <- ``planes`` [n_envs,S,S] of truth values (bit x of row y in word x >> 5 at position x & 31)."""
    import torch

    planes = np.asarray(planes, bool)
    padded = np.zeros(planes.shape[:2] + (om.stride * 32,), bool)
    padded[:, :, :om.size] = planes
    words = np.packbits(padded, axis=2, bitorder="little").view(np.uint32).view(np.int32)
    om.navigable_bits.copy_(torch.from_numpy(np.ascontiguousarray(words)).to(om.device))


def _metres(om, cells):
    """Metres whose ``cells_of`` are the cells (x, y)."""
    c = np.asarray(cells, np.float64).reshape(-1, 2)
    return np.stack([(c[:, 1] - om.size // 2) / om.pixels_per_meter, (om.size - c[:, 0] - om.size // 2) / om.pixels_per_meter],
                    axis=1)


def _plan(om, jobs, lookahead=15, max_cost=65534, return_fields=True):
    jobs = np.asarray(jobs, np.int64).reshape(-1, 11)
    assert np.array_equal(om.cells_of(_metres(om, jobs[:, 5:7])), jobs[:, 5:7])
    return om.plan_paths(_metres(om, jobs[:, 5:7]), _metres(om, jobs[:, 8:10]), env_ids=jobs[:, 0],
                         start_free_m=jobs[:, 7] / om.pixels_per_meter, goal_free_m=jobs[:, 10] / om.pixels_per_meter,
                         lookahead_m=lookahead / om.pixels_per_meter, max_cost=max_cost, windows=jobs[:, 1:5],
                         return_fields=return_fields)


def _results(out):
    return np.concatenate([np.stack([out["status"], out["cost"]], axis=1), out["waypoints_px"], out["steps"][:, None]], axis=1)


def _check(om, planes, jobs, lookahead=15, max_cost=65534, want=None):
    """Plans ``jobs`` with and without fields and compares both with the host statement; returns (results, device output)."""
    jobs = np.asarray(jobs, np.int64).reshape(-1, 11)
    res, fields = want if want is not None else plan_paths_numpy(planes, jobs, lookahead, max_cost)
    out = _plan(om, jobs, lookahead, max_cost, return_fields=True)
    assert np.array_equal(_results(out), res), (np.flatnonzero((_results(out) != res).any(axis=1)), _results(out), res)
    for n, f in enumerate(fields):
        got = out["fields"][n]
        if f is None:
            assert (got == PLAN_NONE).all(), n
            continue
        h, w = f.shape
        assert np.array_equal(got[:h, :w], f), (n, np.argwhere(got[:h, :w] != f)[:5])
        assert (got[h:] == PLAN_NONE).all() and (got[:, w:] == PLAN_NONE).all(), n
    early = _plan(om, jobs, lookahead, max_cost, return_fields=False)          # the early exit: the same results
    assert np.array_equal(_results(early), res) and "fields" not in early
    assert np.array_equal(early["path_m"], np.where(res[:, 0] == PLAN_OK, res[:, 1] * 0.5 / PPM, np.inf))
    return res, out


@pytest.fixture(scope="module", autouse=True)
def _host_waits_first(gpu_device):
    """The harness tests at the end share the process with the map fixtures: set the device's host-wait mode before the
    device's first allocation, as BatchedEpisodes and bench.py do first thing (the runtime fixes a queue's wait policy when it
    creates the queue; _lib.host_wait_blocking).  Set by the first harness AFTER the maps' allocations, the flag left the
    interpreter of one run unable to exit: 400 s after the last test had passed it was still there."""
    from vlfm_amd import _lib

    _lib.try_host_wait_blocking(gpu_device)


@pytest.fixture(scope="module")
def om70(gpu_device):
    return _batch(gpu_device, 2, 70)


@pytest.fixture(scope="module")
def om96(gpu_device):
    return _batch(gpu_device, 3, 96)


@pytest.fixture(scope="module")
def om1000(gpu_device):
    return _batch(gpu_device, 1, 1000)


def _random_planes(seed, n, size, fill):
    return np.random.default_rng(seed).random((n, size, size)) >= fill


# ---------------------------------------------------------------------------------------------- window shapes
@pytest.mark.parametrize("fill", [0.2, 0.4])
def test_random_planes_and_window_shapes(om70, fill):
    planes = _random_planes(70 + int(fill * 10), 2, 70, fill)
    _set_planes(om70, planes)
    S = 70
    jobs = [(0, 0, S - 1, 0, S - 1, 1, 1, 1, 66, 67, 1),          # the whole map: stride 3, the last word partial
            (1, 0, S - 1, 0, S - 1, 69, 0, 2, 0, 69, 2),          # corner to corner
            (0, 5, 5, 7, 7, 7, 5, 0, 7, 5, 0),                    # 1 x 1
            (0, 9, 9, 3, 42, 3, 9, 0, 42, 9, 0),                  # 1 x 40
            (1, 3, 42, 33, 33, 33, 3, 0, 33, 42, 0),              # 40 x 1
            (0, 2, 30, 4, 31, 4, 2, 1, 31, 30, 1),                # ends on bit 31
            (0, 2, 30, 4, 32, 4, 2, 1, 32, 30, 1),                # ... 32
            (1, 2, 30, 4, 33, 4, 30, 1, 33, 2, 1),                # ... 33
            (1, 10, 60, 17, 50, 20, 12, 1, 49, 58, 1),            # starts mid-word
            (0, 40, 66, 37, 63, 38, 41, 3, 62, 65, 0),            # starts and ends mid-word, in the second word
            (0, 0, 20, 0, 20, 0, 0, 1, 20, 20, 1),                # the four map corners
            (1, 0, 20, S - 21, S - 1, S - 1, 0, 1, S - 21, 20, 1),
            (0, S - 21, S - 1, 0, 20, 0, S - 1, 1, 20, S - 21, 1),
            (1, S - 21, S - 1, S - 21, S - 1, S - 1, S - 1, 1, S - 21, S - 21, 1)]
    res, _ = _check(om70, planes, jobs, lookahead=6)
    assert (res[:, 0] != PLAN_INVALID).all() and (res[:, 0] == PLAN_OK).sum() >= 4


@pytest.mark.parametrize("n_jobs", [1, 3, 67])
def test_batches_of_random_jobs(om96, n_jobs):
    rng = np.random.default_rng(960 + n_jobs)
    planes = rng.random((3, 96, 96)) >= rng.uniform(0.1, 0.4, (3, 1, 1))
    _set_planes(om96, planes)
    jobs = []
    for _ in range(n_jobs):
        y0, y1 = sorted(int(v) for v in rng.integers(0, 96, 2))
        x0, x1 = sorted(int(v) for v in rng.integers(0, 96, 2))
        sx, gx = (int(v) for v in rng.integers(x0, x1 + 1, 2))
        sy, gy = (int(v) for v in rng.integers(y0, y1 + 1, 2))
        jobs.append((int(rng.integers(0, 3)), y0, y1, x0, x1, sx, sy, int(rng.integers(0, 5)), gx, gy, int(rng.integers(0, 5))))
    res, out = _check(om96, planes, jobs, lookahead=int(rng.integers(1, 20)))
    assert out["residence"] == "lds"
    if n_jobs == 67:
        assert len(set(j[0] for j in jobs)) == 3 and (res[:, 0] == PLAN_OK).sum() >= 10      # several jobs on every slot


def test_two_jobs_on_one_slot_and_path_lengths(om96):
    planes = np.ones((3, 96, 96), bool)
    _set_planes(om96, planes)
    whole = (0, 95, 0, 95)
    jobs = [(1, *whole, 10, 10, 0, 10, 10, 0),                    # start == goal
            (1, *whole, 10, 10, 0, 11, 10, 0),                    # adjacent, straight
            (1, *whole, 10, 10, 0, 11, 11, 0),                    # adjacent, diagonal
            (1, *whole, 0, 0, 0, 95, 95, 0),                      # two jobs on slot 1 ... and 2
            (2, *whole, 95, 0, 0, 0, 40, 0),
            (2, *whole, 3, 90, 0, 80, 2, 0)]
    res, out = _check(om96, planes, jobs, lookahead=4)
    assert res[:5].tolist() == [[PLAN_OK, 0, 10, 10, 0], [PLAN_OK, 2, 11, 10, 1], [PLAN_OK, 3, 11, 11, 1],
                                [PLAN_OK, 95 * 3, 4, 4, 4], [PLAN_OK, 40 * 3 + 55 * 2, 91, 0, 4]]
    assert out["at_goal"].tolist() == [True, True, True, False, False, False]
    assert np.allclose(out["path_m"][3], 95 * 3 * 0.5 / PPM)      # (1.5 a diagonal cell against sqrt 2: 6 % long)


# ---------------------------------------------------------------------------------------------- path shapes
def _spiral(n=60):
    """(plane, inner end): a one-cell-wide corridor spiralling clockwise from the corner (1, 1) into the middle of an n x n
    plane, the walls between its turns one cell thick."""
    plane = np.zeros((n, n), bool)
    x, y, dx, dy = 1, 1, 1, 0
    plane[y, x] = True

    def can_move(dx, dy):
        nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if not (1 <= nx <= n - 2 and 1 <= ny <= n - 2) or plane[ny, nx]:
            return False
        return not (0 <= ax < n and 0 <= ay < n and plane[ay, ax])          # keep a wall to the turn walked before

    while True:
        if not can_move(dx, dy):
            dx, dy = -dy, dx                                                # turn right (y grows downwards)
            if not can_move(dx, dy):
                return plane, (x, y)
        x, y = x + dx, y + dy
        plane[y, x] = True


def test_spiral_corridor_and_comb(om70):
    spiral, end = _spiral(60)
    comb = np.zeros((70, 70), bool)
    comb[2, 1:69] = True                                           # a spine with dead-end teeth of growing length
    for k, x in enumerate(range(2, 68, 3)):
        comb[2:4 + 2 * k, x] = True
    planes = np.zeros((2, 70, 70), bool)
    planes[0, :60, :60] = spiral
    planes[1] = comb
    _set_planes(om70, planes)
    jobs = [(0, 0, 59, 0, 59, 1, 1, 0, end[0], end[1], 0),
            (0, 0, 69, 0, 69, end[0], end[1], 0, 1, 1, 0),
            (1, 0, 69, 0, 69, 1, 2, 0, 65, 3 + 2 * 21, 0),         # from the spine's end into the longest tooth
            (1, 0, 69, 0, 69, 65, 3 + 2 * 21, 0, 2, 3, 0)]         # from tooth to tooth
    res, _ = _check(om70, planes, jobs, lookahead=15)
    assert (res[:, 0] == PLAN_OK).all()
    # thousands of levels in a band that moves: straight steps all the way but for the U-turn in the middle
    assert res[0, 1] == res[1, 1] and 2 * (int(spiral.sum()) - 3) <= res[0, 1] <= 2 * (int(spiral.sum()) - 1) and res[0, 1] > 3000
    assert res[2, 1] == res[3, 1] == 2 * (64 + 43)


def test_free_discs(om70):
    planes = np.ones((2, 70, 70), bool)
    planes[0, 20:41, 20:41] = False                                # a block
    planes[1] = planes[0]
    _set_planes(om70, planes)
    whole = (0, 69, 0, 69)
    jobs = [(0, *whole, 22, 30, 0, 5, 5, 0),                       # a start inside the obstacle: walled in ...
            (0, *whole, 22, 30, 1, 5, 5, 0),                       # ... a radius that does not reach the edge cells ...
            (0, *whole, 22, 30, 2, 5, 5, 0),                       # ... and one that does
            (1, *whole, 5, 5, 0, 30, 30, 0),                       # a goal inside the block
            (1, *whole, 5, 5, 0, 30, 30, 9),
            (1, *whole, 5, 5, 0, 30, 30, 10),
            (1, *whole, 30, 32, 0, 30, 30, 0)]                     # both inside: only their own cells are free
    res, _ = _check(om70, planes, jobs)
    assert res[:, 0].tolist() == [PLAN_UNREACHABLE, PLAN_UNREACHABLE, PLAN_OK, PLAN_UNREACHABLE, PLAN_UNREACHABLE,
                                  PLAN_OK, PLAN_UNREACHABLE]


def test_equal_fields_where_one_window_contains_the_others_reachable_set(om96):
    planes = np.ones((3, 96, 96), bool)
    planes[0, 30, 20:71] = planes[0, 70, 20:71] = planes[0, 30:71, 20] = planes[0, 30:71, 70] = False     # a closed room
    planes[0, 40:45, 40:60] = False
    _set_planes(om96, planes)
    inner, outer, whole = (31, 69, 21, 69), (17, 90, 3, 88), (0, 95, 0, 95)
    jobs = [(0, *w, 25, 35, 0, 65, 65, 0) for w in (inner, outer, whole)]
    res, out = _check(om96, planes, jobs)
    assert (res[:, 0] == PLAN_OK).all() and (res == res[0]).all()
    a = out["fields"][0][:39, :49]
    assert np.array_equal(a, out["fields"][1][31 - 17:31 - 17 + 39, 21 - 3:21 - 3 + 49])
    assert np.array_equal(a, out["fields"][2][31:70, 21:70]) and (a != PLAN_NONE).sum() == 39 * 49 - 5 * 20
    # the walls and everything beyond them: never reached
    f = out["fields"][2]
    assert (f[:30] == PLAN_NONE).all() and (f[71:] == PLAN_NONE).all() and (f[:, :20] == PLAN_NONE).all()


# ---------------------------------------------------------------------------------------------- statuses, max_cost
@pytest.mark.parametrize("max_cost", [7, 65534])
def test_every_status_in_one_batch(om96, max_cost):
    planes = np.ones((3, 96, 96), bool)
    planes[1, 50, :] = False                                       # slot 1: two halves
    _set_planes(om96, planes)
    whole = (0, 95, 0, 95)
    valid = [(0, *whole, 10, 10, 0, 13, 11, 0),                    # cost 7: OK at either max_cost
             (0, *whole, 10, 10, 0, 14, 11, 0),                    # cost 9
             (1, *whole, 10, 10, 0, 10, 80, 0),                    # the other half: never
             (2, *whole, 0, 0, 0, 95, 95, 0)]
    bad = [(3, *whole, 10, 10, 0, 12, 11, 0), (-1, *whole, 10, 10, 0, 12, 11, 0),          # slot out of range
           (0, 9, 8, 0, 95, 10, 9, 0, 12, 9, 0), (0, 0, 95, 40, 39, 40, 9, 0, 40, 9, 0),   # empty windows
           (0, 0, 96, 0, 95, 10, 10, 0, 12, 11, 0), (0, -1, 95, 0, 95, 10, 10, 0, 12, 11, 0),           # outside the map
           (0, 0, 95, 0, 2000, 10, 10, 0, 12, 11, 0), (0, 0, 95, -5, 95, 10, 10, 0, 12, 11, 0),
           (0, 20, 95, 0, 95, 10, 10, 0, 12, 30, 0), (0, 0, 95, 0, 11, 10, 10, 0, 12, 11, 0),           # start / goal outside
           (0, *whole, 10, 10, -1, 12, 11, 0), (0, *whole, 10, 10, 0, 12, 11, 4097)]                    # radii
    jobs = [bad[0], valid[0], bad[1], bad[2], valid[1], bad[3], bad[4], bad[5], valid[2], bad[6], bad[7], bad[8], valid[3],
            bad[9], bad[10], bad[11]]
    res, out = _check(om96, planes, jobs, max_cost=max_cost)
    is_valid = np.array([j in valid for j in jobs])
    assert (res[~is_valid, 0] == PLAN_INVALID).all() and (res[~is_valid, 1] == PLAN_NONE).all()
    want = [PLAN_OK, PLAN_TOO_LONG, PLAN_TOO_LONG, PLAN_TOO_LONG] if max_cost == 7 else \
        [PLAN_OK, PLAN_OK, PLAN_UNREACHABLE, PLAN_OK]
    assert res[is_valid, 0].tolist() == want
    # the valid jobs are what they are alone
    alone, _ = _check(om96, planes, valid, max_cost=max_cost)
    assert np.array_equal(alone, res[is_valid])
    if max_cost == 7:                                              # nothing beyond the bound is written
        f = out["fields"][1].astype(np.int64)
        assert set(np.unique(f)) == {0, 2, 3, 4, 5, 6, 7, PLAN_NONE}
    # a small closed component and a bound it never reaches: UNREACHABLE, not TOO_LONG
    planes[2, 0:5, 4] = planes[2, 4, 0:5] = False
    _set_planes(om96, planes)
    res, _ = _check(om96, planes, [(2, *whole, 50, 50, 0, 1, 1, 0)], max_cost=max(max_cost, 20))
    assert res[0, 0] == PLAN_UNREACHABLE


# ---------------------------------------------------------------------------------------------- both residences
def _lattice(size=1000, seed=5):
    """A sparse plane: three-cell corridors every 64 cells with 4 % of their cells knocked out, and free speckle."""
    rng = np.random.default_rng(seed)
    plane = np.zeros((size, size), bool)
    for k in range(4, size, 64):
        plane[k:k + 3, :] = True
        plane[:, k:k + 3] = True
    plane &= rng.random((size, size)) >= 0.04
    plane |= rng.random((size, size)) < 0.03
    return plane


@pytest.fixture(scope="module")
def lattice(om1000):
    plane = _lattice()
    # (the second job of each pair starts in a corner off the corridors: a speckle's few cells, then the search runs dry)
    whole = [(0, 0, 999, 0, 999, 5, 5, 2, 965, 965, 2), (0, 0, 999, 0, 999, 999, 0, 1, 0, 999, 1)]
    centre = [(0, 350, 649, 350, 649, 389, 390, 2, 645, 646, 2), (0, 350, 649, 350, 649, 649, 350, 1, 350, 649, 1)]
    return plane, whole, plan_paths_numpy(plane, whole, 15), centre, plan_paths_numpy(plane, centre, 15)


def test_whole_map_in_global_scratch(om1000, lattice):
    plane, whole, want, _, _ = lattice
    _set_planes(om1000, plane[None])
    res, out = _check(om1000, plane, whole, want=want)
    assert out["residence"] == "scratch" and out["fields"].shape == (2, 1000, 1000)
    assert res[0, 0] == PLAN_OK and res[0, 1] > 3000               # thousands of levels, bands over the whole map


def test_centre_window_in_lds(om1000, lattice):
    plane, _, _, centre, want = lattice
    _set_planes(om1000, plane[None])
    res, out = _check(om1000, plane, centre, want=want)
    assert out["residence"] == "lds" and out["fields"].shape == (2, 300, 300)
    assert res[0, 0] == PLAN_OK and res[0, 1] > 1000 and res[1, 0] == PLAN_UNREACHABLE


def test_default_windows_and_radii(om1000):
    plane = np.ones((1000, 1000), bool)
    plane[480:520, 530] = False
    _set_planes(om1000, plane[None])
    om1000.reset()                                                 # (clears the planes too)
    _set_planes(om1000, plane[None])
    starts, goals = np.array([[0.0, 0.0], [0.5, -1.0]]), np.array([[1.0, -2.5], [-3.0, 2.0]])
    out = om1000.plan_paths(starts, goals, env_ids=[0, 0], return_fields=True)
    s, g = om1000.cells_of(starts), om1000.cells_of(goals)
    assert s.tolist() == [[500, 500], [520, 510]] and g.tolist() == [[550, 520], [460, 440]]
    pad, r = 2 * om1000.kernel_size, om1000.kernel_size // 2
    win = [[min(a[1], b[1]) - pad, max(a[1], b[1]) + pad, min(a[0], b[0]) - pad, max(a[0], b[0]) + pad] for a, b in zip(s, g)]
    assert out["windows"].tolist() == win                          # nothing revealed yet: start and goal, padded
    jobs = [(0, *w, *a, r, *b, r) for w, a, b in zip(win, s, g)]
    res, fields = plan_paths_numpy(plane, jobs, 15)
    assert np.array_equal(_results(out), res) and (res[:, 0] == PLAN_OK).all()
    for n, f in enumerate(fields):
        assert np.array_equal(out["fields"][n][:f.shape[0], :f.shape[1]], f)
    assert np.allclose(out["waypoints"], om1000.px_to_xy(res[:, 2:4].astype(np.float64)))
    # the revealed box joins the window
    om1000._bbox_host[0] = (300, 700, 380, 640)
    out = om1000.plan_paths(starts[:1], goals[:1], env_ids=[0])
    assert out["windows"].tolist() == [[300 - pad, 700 + pad, 380 - pad, 640 + pad]]
    om1000._bbox_host[0] = (0, -1, 0, -1)
    # a goal off the map: answered by status
    out = om1000.plan_paths(starts[:1], np.array([[40.0, 0.0]]), env_ids=[0])
    assert out["status"].tolist() == [PLAN_INVALID] and np.isinf(out["path_m"][0])
    assert om1000.plan_paths(np.zeros((0, 2)), np.zeros((0, 2)))["status"].shape == (0,)


# ---------------------------------------------------------------------------------------------- streams, reset
def test_other_stream_and_reset_of_one_slot(om96):
    import torch

    planes = _random_planes(11, 3, 96, 0.15)
    _set_planes(om96, planes)
    whole = (0, 95, 0, 95)
    jobs = [(e, *whole, 3 + e, 4, 2, 90, 88 - e, 2) for e in range(3)]
    want = plan_paths_numpy(planes, jobs, 15)
    side = torch.cuda.Stream(om96.device)
    side.wait_stream(torch.cuda.current_stream(om96.device))       # the planes were written on the current stream
    with torch.cuda.stream(side):
        _check(om96, planes, jobs, want=want)
    torch.cuda.current_stream(om96.device).wait_stream(side)
    om96.reset([1])                                                # slot 1 is empty again: nothing navigable
    planes[1] = False
    res, _ = _check(om96, planes, jobs)
    assert res[1, 0] == PLAN_UNREACHABLE and np.array_equal(res[[0, 2]], want[0][[0, 2]])


# ---------------------------------------------------------------------------------------------- the harness
class _Recorder:
    """An ObstacleMapBatch whose plan_paths calls are written down with the navigable bits they saw."""

    def __init__(self, om):
        self.om, self.calls = om, []

    def plan_paths(self, starts_xy, goals_xy, **kw):
        out = self.om.plan_paths(starts_xy, goals_xy, **kw)
        env = np.asarray(kw["env_ids"])
        bits = self.om._unpack(self.om.navigable_bits)[env].cpu().numpy().astype(bool)
        gf = np.broadcast_to(np.asarray(kw["goal_free_m"] if kw.get("goal_free_m") is not None else np.nan, np.float64), env.shape)
        r = self.om.kernel_size // 2
        rg = np.where(np.isfinite(gf), np.rint(np.nan_to_num(gf) * PPM), r).astype(np.int64)
        s, g = self.om.cells_of(starts_xy), self.om.cells_of(goals_xy)
        jobs = [(k, *out["windows"][k], *s[k], r, *g[k], rg[k]) for k in range(len(env))]
        self.calls.append((bits, jobs, _results(out)))
        return out


class _RecordingPlanner(MapPlannerController):
    def __init__(self):
        super().__init__()
        self.recorders = {}
        self.statuses = []

    def act_on_map(self, obstacles, *args):
        rec = self.recorders.setdefault(id(obstacles), _Recorder(obstacles))
        acts = super().act_on_map(rec, *args)
        self.statuses.append(self.last_status.copy())
        return acts


def _run(device, controller, steps=40, E=4):
    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True,
                          controller=controller)
    poses, actions = [], []
    for _ in range(steps):
        sim.step()
        poses.append(sim.last_poses.copy())
        actions.append(sim.last_world_actions.copy())
    return sim, np.array(poses), np.array(actions)


def test_harness_with_the_map_planner(gpu_device):
    ctl = _RecordingPlanner()
    sim, poses, actions = _run(gpu_device, ctl)
    _, poses2, actions2 = _run(gpu_device, MapPlannerController())
    assert np.array_equal(poses, poses2) and np.array_equal(actions, actions2)              # reproducible
    # the book-keeping adds up
    ps, status = sim.planner_stats, np.array(ctl.statuses)
    assert status.shape == actions.shape
    assert np.array_equal(ps["plans"], (status >= 0).sum(axis=0)) and ps["plans"].sum() > 0
    assert np.array_equal(ps["ok"], (status == PLAN_OK).sum(axis=0)) and ps["ok"].sum() > 0
    assert np.array_equal(ps["plans"], ps["ok"] + ps["unreachable"] + ps["too_long"] + ps["invalid"])
    assert set(sim.live.stats) == {"path_length", "collisions", "forward_steps", "turn_steps", "stops"}
    # every plan, recomputed on the host from the bits of its step.  The full search for the last call; for the
    # others the search is bounded by the reported cost, which leaves a PLAN_OK result as it is (and turns a cost that is too
    # small into PLAN_TOO_LONG)
    (rec,) = ctl.recorders.values()
    assert len(rec.calls) >= 10
    n_ok = 0
    for k, (bits, jobs, got) in enumerate(rec.calls):
        for n, job in enumerate(jobs):
            full = k == len(rec.calls) - 1 or got[n, 0] != PLAN_OK
            want, _ = plan_paths_numpy(bits[n], [(0, *job[1:])], 15, 65534 if full else int(got[n, 1]))
            assert np.array_equal(want[0], got[n]), (k, n, job, want[0], got[n])
            n_ok += got[n, 0] == PLAN_OK
    assert n_ok == ps["ok"].sum()


def test_harness_with_bang_bang_is_the_parents_path(gpu_device):
    _, poses, actions = _run(gpu_device, BangBangController())
    sim, poses0, actions0 = _run(gpu_device, None)
    assert np.array_equal(poses, poses0) and np.array_equal(actions, actions0)
    assert all((v == 0).all() for v in sim.planner_stats.values())
