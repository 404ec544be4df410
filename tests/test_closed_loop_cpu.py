"""Closed-loop episodes, host half: the world's kinematics (synthetic.step_poses), the controllers that turn the policy's
decision into an action id, and the argument checks of BatchedEpisodes(closed_loop=True), which come before the device is
touched.  No GPU needed."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from vlfm_amd.policy_step import ACTION_FORWARD, ACTION_STOP, ACTION_TURN_LEFT, ACTION_TURN_RIGHT

TO_ID = {S.LEFT: ACTION_TURN_LEFT, S.RIGHT: ACTION_TURN_RIGHT, S.FORWARD: ACTION_FORWARD}


def test_action_ids_are_the_policys():
    assert (S.ACTION_STOP, S.ACTION_FORWARD, S.ACTION_TURN_LEFT, S.ACTION_TURN_RIGHT) == \
        (ACTION_STOP, ACTION_FORWARD, ACTION_TURN_LEFT, ACTION_TURN_RIGHT) == (0, 1, 2, 3)


def test_tour_replay_reproduces_integrate_exactly():
    """The 500 actions of the planned tour through step_poses: x, y, k equal integrate()'s with ==, and no move is refused.
    Three robots at once, the second and third starting 37 and 74 steps into the tour (how the harness staggers them)."""
    plan = S.plan_actions(2 * S.ROOMS_STEPS)
    want = S.integrate(plan)
    offs = [0, 37, 74]
    xy = np.array([want[o][:2] for o in offs], np.float64)
    k = np.array([want[o][2] for o in offs], np.int64)
    for t in range(S.ROOMS_STEPS):
        for e, o in enumerate(offs):
            assert (xy[e, 0], xy[e, 1], int(k[e])) == want[o + t], (t, e)
        xy, k, hit = S.step_poses(xy, k, [TO_ID[int(plan[o + t])] for o in offs])
        assert not hit.any(), t


def test_refused_move_and_stop():
    # (0, 3.6) facing north: the hall's north wall starts at y = 4.0, so y = 3.85 is within the 0.2 m margin
    assert not S._blocked(0.0, 3.6, 0.2) and S._blocked(0.0, 3.85, 0.2)
    xy0, k0 = np.array([[0.0, 3.6], [0.0, 0.0], [0.0, 3.6]]), np.array([3, 3, 3])
    xy, k, hit = S.step_poses(xy0, k0, [ACTION_FORWARD, ACTION_FORWARD, ACTION_STOP])
    assert hit.tolist() == [True, False, False]
    assert np.array_equal(xy[0], xy0[0]) and np.array_equal(xy[1], [0.0, 0.25]) and np.array_equal(xy[2], xy0[2])
    assert k.tolist() == [3, 3, 3]
    assert np.array_equal(xy0, [[0.0, 3.6], [0.0, 0.0], [0.0, 3.6]])        # the inputs are not written to
    # turns wrap mod 12 and never move or collide, even facing the wall
    xy, k, hit = S.step_poses(xy0, [11, 0, 3], [ACTION_TURN_LEFT, ACTION_TURN_RIGHT, ACTION_TURN_LEFT])
    assert k.tolist() == [0, 11, 4] and not hit.any() and np.array_equal(xy, xy0)
    with pytest.raises(ValueError):
        S.step_poses(xy0, k0, [0, 1, 4])


def test_bang_bang_rule_table():
    d15 = float(np.deg2rad(15.0))
    nan = float("nan")
    c = S.BangBangController()
    modes = ["initialize", "explore", "explore", "explore", "explore", "explore", "navigate", "explore", "navigate"]
    theta = [0.0, d15, np.nextafter(d15, 1.0), -d15, np.nextafter(-d15, -1.0), nan, 0.3, float("inf"), 0.0]
    stops = np.array([False] * 6 + [True, False, False])
    rt = np.stack([np.ones(len(theta)), np.array(theta)], axis=1)
    got = c.act(modes, rt, stops, np.zeros(len(modes), bool))
    assert got.dtype == np.int64
    assert got.tolist() == [ACTION_TURN_LEFT, ACTION_FORWARD, ACTION_TURN_LEFT, ACTION_FORWARD, ACTION_TURN_RIGHT, ACTION_STOP,
                            ACTION_STOP, ACTION_STOP, ACTION_FORWARD]


def test_bang_bang_detour_after_a_refused_forward():
    c = S.BangBangController()
    ahead = np.array([[2.0, 0.0], [2.0, 0.0]])
    no, modes, stops = np.zeros(2, bool), ["explore", "explore"], np.zeros(2, bool)
    assert c.act(modes, ahead, stops, no).tolist() == [ACTION_FORWARD, ACTION_FORWARD]
    # environment 0's FORWARD was refused: 60 degrees to the left (two turns), three steps FORWARD whatever theta says, then the rule
    right = np.array([[2.0, -1.0], [2.0, 0.0]])
    seq = [c.act(modes, right, stops, np.array([True, False]))] + [c.act(modes, right, stops, no) for _ in range(5)]
    assert [int(a[0]) for a in seq] == [ACTION_TURN_LEFT] * 2 + [ACTION_FORWARD] * 3 + [ACTION_TURN_RIGHT]
    assert all(int(a[1]) == ACTION_FORWARD for a in seq)
    # a refused detour step costs one more turn, and the detour goes on
    c = S.BangBangController()
    seq = [c.act(modes, ahead, stops, np.array([True, False])), c.act(modes, ahead, stops, no), c.act(modes, ahead, stops, no),
           c.act(modes, ahead, stops, np.array([True, False])), c.act(modes, ahead, stops, no), c.act(modes, ahead, stops, no),
           c.act(modes, right, stops, no)]
    assert [int(a[0]) for a in seq] == [ACTION_TURN_LEFT, ACTION_TURN_LEFT, ACTION_FORWARD, ACTION_TURN_LEFT, ACTION_FORWARD,
                                        ACTION_FORWARD, ACTION_TURN_RIGHT]
    # a stop wins over a pending detour; reset() forgets it
    c = S.BangBangController()
    assert c.act(modes, ahead, np.array([True, False]), np.array([True, False])).tolist() == [ACTION_STOP, ACTION_FORWARD]
    c.reset()
    assert c.act(modes, ahead, stops, no).tolist() == [ACTION_FORWARD, ACTION_FORWARD]


def test_replay_controller_returns_its_rows():
    table = np.array([[1, 2], [3, 0], [2, 2]])
    c = S.ReplayController(table)
    rows = [c.act(None, None, None, None) for _ in range(4)]
    assert [r.tolist() for r in rows] == [[1, 2], [3, 0], [2, 2], [1, 2]] and rows[0].dtype == np.int64
    rows[0][:] = 9
    assert c.actions[0].tolist() == [1, 2]
    c.reset()
    assert c.act(None, None, None, None).tolist() == [1, 2]
    with pytest.raises(ValueError):
        S.ReplayController(np.zeros(3))


class _Continuous:
    discrete = False


@pytest.mark.parametrize("kw", [
    dict(world="random"),
    dict(host_inputs=True),
    dict(obstacle=False),
    dict(select_frontiers=False),
    dict(pointnav=_Continuous()),
], ids=["world", "host_inputs", "no_obstacle_map", "no_frontier_selection", "continuous_pointnav"])
def test_closed_loop_argument_checks_come_before_the_device(kw, monkeypatch):
    """Each invalid combination is a ValueError, raised before the device is asked for: a harness that passes the checks gets as
    far as require_gpu (stubbed here to a sentinel exception, so the test says the same thing on a machine with a GPU)."""
    from vlfm_amd import harness

    class Reached(Exception):
        pass

    def stop(_device):
        raise Reached

    monkeypatch.setattr(harness, "require_gpu", stop)
    good = dict(closed_loop=True, use_blip2=False, select_frontiers=True)
    with pytest.raises(Reached):
        harness.BatchedEpisodes(2, **good)
    with pytest.raises(ValueError, match="closed_loop"):
        harness.BatchedEpisodes(2, **{**good, **kw})


def test_controller_without_closed_loop_is_refused():
    from vlfm_amd.harness import BatchedEpisodes

    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, use_blip2=False, controller=S.BangBangController())
