"""The host side of the device-resident object clouds (vlfm_amd/mapping/object_point_cloud_map.py: the slot table a map keeps per
cloud, the merge of the device's flags with the host's own evaluation of the uncertain band, the refusals the batched queries make
before they touch a device, the hysteresis shared by get_best_object and get_best_objects_batch).  No GPU: the package has no CPU
path for the queries themselves (tests/test_object_clouds_device_gpu.py)."""
import types

import numpy as np
import pytest

from vlfm_amd.mapping import object_point_cloud_map as opm


class _Scripted:
    """A generator whose rand() returns the scripted values."""

    def __init__(self, values):
        self.values = list(values)

    def rand(self):
        return self.values.pop(0)


def _bare_map(rng):
    """An ObjectPointCloudMap without a device: the constructor refuses to build one on a machine without a GPU, the host
    bookkeeping under test needs none."""
    m = opm.ObjectPointCloudMap.__new__(opm.ObjectPointCloudMap)
    m._erosion_size, m._rng, m.last_target_coord, m.device = 1, rng, None, None
    m.clouds, m._bufs, m._near_only, m._mirrors = {}, None, {}, {}
    return m


def _tf(x, y, yaw, z=0.0):
    tf = np.eye(4)
    tf[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    tf[:3, 3] = x, y, z
    return tf


def _check_mirror(m, name):
    cloud = m.clouds[name]
    mirror = m._mirror_for(name, cloud)
    assert mirror is not None, "the mirror lost track of the array"
    tags, slots, table = cloud[:, -1], mirror.slots, np.array(mirror.table + [np.nan])
    assert slots.dtype == np.int32 and slots.shape == (len(cloud),)
    assert np.array_equal(slots == -1, tags == 1)
    assert np.array_equal(table[slots[slots >= 0]], tags[slots >= 0])
    assert len(set(mirror.table)) == len(mirror.table)
    assert sorted({mirror.table[s] for s in slots[slots >= 0]}) == np.unique(tags[tags != 1]).tolist()
    # an array nothing is known about gets the same partition, numbered by first appearance
    fresh, fresh_table = opm.slots_of_array(tags)
    assert np.array_equal(np.array(fresh_table + [np.nan])[fresh], table[slots], equal_nan=True)
    firsts = [int(np.argmax(fresh == s)) for s in range(len(fresh_table))]
    assert firsts == sorted(firsts)
    return mirror


def _frame(rng, n, lo, hi):
    """n camera-frame points, `lo`..`hi` metres ahead."""
    return np.stack([rng.uniform(lo, hi, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], axis=1)


def test_slot_table_over_commits_and_drops():
    rng = np.random.default_rng(0)
    almost_one = 1.0 - 1e-9                       # np.float32 rounds it to exactly 1.0
    m = _bare_map(_Scripted([0.25, 0.5, 0.5, almost_one, almost_one, 0.75, 0.125]))
    here = _tf(0.0, 0.0, 0.0)
    m._commit("chair", _frame(rng, 40, 2.0, 3.0), lambda: False, here, 5.0)          # near only: tags 1.0
    assert m._all_near("chair") and _check_mirror(m, "chair").table == []
    m._commit("chair", _frame(rng, 50, 4.0, 4.99), lambda: False, here, 5.0)         # 1.0 and f32(0.5)
    assert not m._all_near("chair") and _check_mirror(m, "chair").table == [0.5]
    m._commit("chair", _frame(rng, 30, 2.0, 3.0), lambda: True, here, 5.0)           # too offset: the SAME value again
    assert _check_mirror(m, "chair").table == [0.5]
    m._commit("chair", _frame(rng, 30, 4.0, 4.99), lambda: False, here, 5.0)         # f32(1 - 1e-9) = 1.0: trusted
    assert _check_mirror(m, "chair").table == [0.5]
    m._commit("chair", _frame(rng, 20, 2.0, 3.0), lambda: True, _tf(0.0, 0.0, np.pi / 2), 5.0)   # f64 1 - 1e-9: far, to the left
    assert _check_mirror(m, "chair").table == [0.5, almost_one]
    m._commit("chair", _frame(rng, 25, 2.0, 3.0), lambda: True, _tf(0.0, 0.0, np.pi), 5.0)       # 0.75, behind
    mirror = _check_mirror(m, "chair")
    assert mirror.table == [0.5, almost_one, 0.75] and len(m.clouds["chair"]) == 195
    mirror.on_device = len(m.clouds["chair"])     # as if a query had uploaded it
    # look left from the origin: the host path drops the 20 points tagged 1 - 1e-9 and nothing else
    m.update_explored(_tf(0.0, 0.0, np.pi / 2), 10.0, 0.5)
    mirror = _check_mirror(m, "chair")
    assert len(m.clouds["chair"]) == 175 and mirror.on_device == 0          # stale on the device: uploaded in full next time
    assert almost_one not in m.clouds["chair"][:, -1]
    # look ahead: f32(0.5) of the second commit and 0.5 of the third go together
    m.update_explored(_tf(0.0, 0.0, 0.0), 10.0, 0.5)
    _check_mirror(m, "chair")
    assert set(m.clouds["chair"][:, -1].tolist()) == {1.0, 0.75}
    # nothing in view: same array, same mirror
    before = m.clouds["chair"]
    m.update_explored(_tf(50.0, 50.0, 0.0), 10.0, 0.5)
    assert m.clouds["chair"] is before and _check_mirror(m, "chair").key == (id(before), len(before))
    m._commit("chair", _frame(rng, 10, 4.8, 4.99), lambda: False, here, 5.0)         # a commit after the drops: 0.125
    assert _check_mirror(m, "chair").table == [0.5, almost_one, 0.75, np.float32(0.125)]
    # an array the map did not build is not recognised; a commit on top of it drops the mirror instead of guessing
    m.clouds["chair"] = m.clouds["chair"].copy()
    assert m._mirror_for("chair", m.clouds["chair"]) is None
    m._rng = _Scripted([0.3])
    m._commit("chair", _frame(rng, 10, 2.0, 3.0), lambda: True, here, 5.0)
    assert "chair" not in m._mirrors
    m.reset()
    assert m._mirrors == {} and m.clouds == {}


def test_block_slots_and_unknown_arrays():
    table = []

    def slot_of(v):
        if v not in table:
            table.append(v)
        return table.index(v)

    assert opm.block_slots(np.array([1.0, 1.0]), slot_of).tolist() == [-1, -1] and table == []
    assert opm.block_slots(np.array([1.0, 0.5, 0.5, 1.0]), slot_of).tolist() == [-1, 0, 0, -1]
    assert opm.block_slots(np.array([0.25]), slot_of).tolist() == [1]
    assert opm.block_slots(np.array([0.5, 0.5]), slot_of).tolist() == [0, 0] and table == [0.5, 0.25]
    slots, tab = opm.slots_of_array(np.array([0.75, 1.0, 0.25, 0.75, 0.5, 0.25, 1.0]))
    assert slots.tolist() == [0, -1, 1, 0, 2, 1, -1] and tab == [0.75, 0.25, 0.5]
    slots, tab = opm.slots_of_array(np.ones(5))
    assert slots.tolist() == [-1] * 5 and tab == []
    slots, tab = opm.slots_of_array(np.zeros(0))
    assert slots.shape == (0,) and tab == []


def test_merge_of_device_flags_and_band_points():
    asked = []

    def decide(answers):
        def f(slot):
            asked.append(slot)
            return answers[slot]
        return f

    # inside wins without asking; uncertain slots are asked; the others are left alone
    assert opm.merge_cone_flags([1, 0, 0, 1, 0], [0, 1, 1, 1, 0], decide({1: True, 2: False})) == [0, 1, 3]
    assert asked == [1, 2]
    del asked[:]
    assert opm.merge_cone_flags([0, 0], [0, 0], decide({})) == [] and asked == []
    assert opm.merge_cone_flags(np.zeros(0, np.int32), np.zeros(0, np.int32), decide({})) == []
    assert opm.merge_cone_flags(np.array([0, 7], np.int32), np.array([5, 0], np.int32), decide({0: True})) == [0, 1]
    with pytest.raises(ValueError, match="per slot"):
        opm.merge_cone_flags([1, 0], [0], decide({}))


def test_band_is_narrower_than_the_wrap_margin():
    assert opm.CONE_BAND == 1e-9
    assert opm.QUERY_DTYPE.itemsize == 80


# ---------------------------------------------------------------------------------------------- refusals before the device
def _stand_in(device):
    return types.SimpleNamespace(device=device, clouds={})


def test_lengths_that_disagree_are_refused():
    maps = [_stand_in("cuda:0"), _stand_in("cuda:0")]
    with pytest.raises(ValueError, match="one entry per map"):
        opm.update_explored_batch(maps, [np.eye(4)], 5.0, 1.0)
    with pytest.raises(ValueError, match="one entry per map"):
        opm.get_best_objects_batch(maps, ["chair"], [np.zeros(2), np.zeros(2)])
    with pytest.raises(ValueError, match="one entry per map"):
        opm.get_best_objects_batch(maps, ["chair", "bed"], [np.zeros(2)])


def test_maps_on_different_devices_are_refused():
    maps = [_stand_in("cuda:0"), _stand_in("cuda:1")]
    with pytest.raises(ValueError, match="one device"):
        opm.update_explored_batch(maps, [np.eye(4)] * 2, 5.0, 1.0)
    with pytest.raises(ValueError, match="one device"):
        opm.get_best_objects_batch(maps, ["chair", "bed"], [np.zeros(2)] * 2)


def test_no_maps_is_a_no_op():
    assert opm.update_explored_batch([], [], 5.0, 1.0) == []
    assert opm.get_best_objects_batch([], [], []) == []


# ---------------------------------------------------------------------------------------------- hysteresis
def _reference_lines(previous, candidate, position):
    """object_point_cloud_map.py:82-100 of the reference, restated: (returned goal, last_target_coord afterwards)."""
    if previous is None:
        return candidate, candidate
    delta = np.linalg.norm(candidate - previous)
    if delta < 0.1:
        return previous, previous
    if delta < 0.5 and np.linalg.norm(position - candidate) > 2.0:
        return previous, previous
    return candidate, candidate


def _random_walk(rng, n):
    """(candidates, positions): steps of every size class around the two thresholds, robot nearer and farther than 2 m."""
    c, out = rng.uniform(-1, 1, 2), []
    for _ in range(n):
        step = rng.choice([0.0, 0.05, 0.0999, 0.1001, 0.3, 0.4999, 0.5001, 1.5])
        ang = rng.uniform(0, 2 * np.pi)
        c = c + step * np.array([np.cos(ang), np.sin(ang)])
        out.append((c.copy(), c + rng.choice([0.5, 1.9, 2.1, 4.0]) * np.array([np.cos(ang + 1), np.sin(ang + 1)])))
    return out


def test_factored_hysteresis_follows_the_rule():
    p = np.zeros(2)
    goal, new = opm.apply_hysteresis(None, np.array([3.0, 0.0]), p)
    assert new and goal.tolist() == [3.0, 0.0]
    prev = np.array([3.0, 0.0])
    goal, new = opm.apply_hysteresis(prev, np.array([3.05, 0.0]), p)
    assert not new and goal is prev                                   # moved < 0.1
    goal, new = opm.apply_hysteresis(prev, np.array([3.3, 0.0]), p)
    assert not new and goal is prev                                   # moved < 0.5, robot 3.3 m away
    goal, new = opm.apply_hysteresis(prev, np.array([3.3, 0.0]), np.array([2.0, 0.0]))
    assert new and goal.tolist() == [3.3, 0.0]                        # moved < 0.5, robot 1.3 m away
    goal, new = opm.apply_hysteresis(prev, np.array([3.6, 0.0]), p)
    assert new and goal.tolist() == [3.6, 0.0]                        # moved >= 0.5
    rng = np.random.default_rng(3)
    kept = taken = 0
    for _ in range(20):
        m = _bare_map(None)
        prev = None
        for cand, pos in _random_walk(rng, 40):
            want, prev = _reference_lines(prev, cand, pos)
            got = m._goal_with_hysteresis(cand, pos)
            assert np.array_equal(got, want) and np.array_equal(m.last_target_coord, prev)
            kept += got is not cand
            taken += got is cand
    assert kept > 50 and taken > 50


def test_factored_hysteresis_against_the_reference_class():
    """The reference's own get_best_object on one-point clouds (the closest point IS the candidate), where the reference is
    present; the restated lines above are the pin elsewhere."""
    from oracle import ref_shim

    if not ref_shim.available():
        return
    ref = ref_shim.reference_object_map()
    rng = np.random.default_rng(4)
    for _ in range(10):
        theirs = ref.ObjectPointCloudMap(erosion_size=1)
        theirs.reset()
        ours = _bare_map(None)
        for cand, pos in _random_walk(rng, 40):
            theirs.clouds = {"chair": np.array([[cand[0], cand[1], 0.3, 1.0]])}
            ours.clouds = {"chair": theirs.clouds["chair"].copy()}
            want = theirs.get_best_object("chair", pos)
            got = ours.get_best_object("chair", pos)
            assert np.array_equal(got, want) and np.array_equal(ours.last_target_coord, theirs.last_target_coord)
            assert np.array_equal(ours._goal_with_hysteresis(cand, pos), want)       # idempotent at the same candidate
