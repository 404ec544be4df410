"""-m gpu: object clouds on the device (object_point_cloud_map.update_explored_batch / get_best_objects_batch over device mirrors of
the clouds, csrc/cloud_query.hip).  Everything is compared BIT FOR BIT (bytes, shape, dtype) with the per-map host methods
(ObjectPointCloudMap.update_explored / get_best_object) run on a twin map fed identically, and the three recorded sessions with the
reference's own recordings (tests/golden/object_map_rand*.npz)."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

from golden_util import load
from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

FOV = camera_intrinsics(640)[2]


def _opm():
    from vlfm_amd.mapping import object_point_cloud_map as opm

    return opm


def _launches():
    from vlfm_amd import _lib

    return _lib.lib().vlfm_cloud_query_launch_count()


def _chunk():
    from vlfm_amd import _lib

    return _lib.lib().vlfm_cloud_query_chunk()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _same(a, b) -> bool:
    """Bit for bit, shape and dtype included; None equals None only."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_clouds(a, b) -> bool:
    return list(a.clouds.keys()) == list(b.clouds.keys()) and all(_same(a.clouds[k], b.clouds[k]) for k in a.clouds)


def _tf(x, y, yaw, z=0.0):
    tf = np.eye(4)
    tf[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    tf[:3, 3] = x, y, z
    return tf


def _twins(device, clouds=None, n=1):
    """n pairs (host twin, device twin) holding copies of ``clouds`` (name -> (N, 4) array)."""
    opm = _opm()
    pairs = []
    for _ in range(n):
        pair = []
        for _ in range(2):
            m = opm.ObjectPointCloudMap(erosion_size=1, device=device, rng=np.random.RandomState(5))
            m.clouds = {k: v.copy() for k, v in (clouds or {}).items()}
            pair.append(m)
        pairs.append(tuple(pair))
    return pairs if n > 1 else pairs[0]


def _explore(host, dev, tf, max_depth=MAX_DEPTH, fov=FOV):
    """update_explored on the host twin, update_explored_batch on the device twin; the clouds must agree.  Returns whether the
    device twin dropped something."""
    opm = _opm()
    before = sum(len(c) for c in host.clouds.values())
    host.update_explored(tf, max_depth, fov)
    dropped = opm.update_explored_batch([dev], [tf], max_depth, fov)
    assert _same_clouds(host, dev)
    assert dropped == [sum(len(c) for c in host.clouds.values()) != before]
    return dropped[0]


def _best(hosts, devs, names, positions):
    opm = _opm()
    want = [m.get_best_object(n, p) if m.has_object(n) else None for m, n, p in zip(hosts, names, positions)]
    got = opm.get_best_objects_batch(devs, names, positions)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (i, g, w)
    for a, b in zip(hosts, devs):
        assert _same(a.last_target_coord, b.last_target_coord)
    return got


# ---------------------------------------------------------------------------------------------- 1. the reference's sessions
@functools.lru_cache(maxsize=None)
def _random_sessions():
    from make_golden import object_map_random_script

    return [object_map_random_script(seed) for seed in (0, 1, 2)]


def test_three_reference_sessions_in_lockstep(gpu_device):
    """The three random sessions recorded from the reference's ObjectPointCloudMap as three maps in lockstep: every "explored"
    index is ONE update_explored_batch, every "best" index ONE get_best_objects_batch."""
    opm = _opm()
    sessions = _random_sessions()
    golden = [load(f"object_map_rand{seed}") for seed in (0, 1, 2)]
    assert len({len(s) for s in sessions}) == 1 and all(len({s[i][0] for s in sessions}) == 1 for i in range(len(sessions[0])))
    fx, fy, fov = camera_intrinsics(640)
    maps = [opm.ObjectPointCloudMap(erosion_size=(3, 5, 2)[seed], device=gpu_device, rng=np.random.RandomState(4321 + seed))
            for seed in (0, 1, 2)]
    n_best = n_explored = 0
    launches = _launches()
    for i in range(len(sessions[0])):
        ops = [s[i] for s in sessions]
        if ops[0][0] == "update":
            opm.update_maps_batch(maps, [op[1] for op in ops], np.stack([op[2] for op in ops]), [0, 1, 2],
                                  np.stack([op[3] for op in ops]), [op[4] for op in ops], MIN_DEPTH, MAX_DEPTH, fx, fy)
        elif ops[0][0] == "best":
            for m, g in zip(maps, golden):
                assert [int(m.has_object(n)) for n in ("chair", "bed", "tv")] == list(g[f"has_{i}"]), i
            goals = opm.get_best_objects_batch(maps, [op[1] for op in ops], [op[2] for op in ops])
            for goal, g in zip(goals, golden):
                assert (goal is not None) == (f"best_{i}" in g), i
                if goal is not None:
                    assert _same(np.asarray(goal, np.float64), g[f"best_{i}"]), i
                    n_best += 1
        else:
            opm.update_explored_batch(maps, [op[1] for op in ops], MAX_DEPTH, fov)
            n_explored += 1
        for m, g in zip(maps, golden):
            for name in ("chair", "bed", "tv"):
                assert (name in m.clouds) == (f"sig_{i}_{name}" in g), (i, name)
                if name in m.clouds:
                    c = np.asarray(m.clouds[name], np.float64)
                    assert [str(c.shape[0]), _sha(c)] == list(g[f"sig_{i}_{name}"]), (i, name, c.shape)
    assert n_best >= 15 and n_explored >= 3 and _launches() > launches
    for m, g in zip(maps, golden):
        for name in ("chair", "bed", "tv"):
            if f"final_{name}" in g:
                assert _same(np.asarray(m.clouds[name], np.float64), g[f"final_{name}"])


# ---------------------------------------------------------------------------------------------- 2. closest point at the edges
def _random_cloud(rng, n, trusted=0.5, centre=(4.0, -3.0, 0.5)):
    c = np.concatenate([rng.normal(0.0, 1.0, (n, 3)) + np.array(centre), np.ones((n, 1))], axis=1)
    c[rng.random(n) >= trusted, 3] = 0.375
    return c


@pytest.mark.parametrize("k", [2, 3])
def test_closest_point_over_cloud_sizes(gpu_device, k):
    """1, 63, 64, 65, 257 points, one workgroup chunk - 1 / exactly / + 1, and 20 011 points (5 chunks, the last one partial), each
    with mixed tags and with far tags only, all in ONE call; with k = 2 every map is asked twice in the call (its hysteresis sees
    both), with k = 3 once (the reference's hysteresis cannot subtract a 2-D goal from a 3-D position)."""
    chunk = _chunk()
    assert chunk >= 256
    rng = np.random.default_rng(20 + k)
    sizes = [1, 63, 64, 65, 257, chunk - 1, chunk, chunk + 1, 20011]
    pairs = [_twins(gpu_device, {"chair": _random_cloud(rng, n, trusted)}) for n in sizes for trusted in (0.5, 0.0)]
    hosts, devs = [p[0] for p in pairs], [p[1] for p in pairs]
    positions = [np.array([4.0, -3.0, 0.5])[:k] + rng.normal(0, 0.5, k) for _ in pairs]
    launches, syncs = _launches(), _opm().SYNCS[0]
    if k == 2:
        second = [p + np.array([0.3, 0.1]) for p in positions]
        _best(hosts + hosts, devs + devs, ["chair"] * (2 * len(pairs)), positions + second)
    else:
        _best(hosts, devs, ["chair"] * len(pairs), positions)
    assert (_launches() - launches, _opm().SYNCS[0] - syncs) == (2, 1)


def test_closest_point_special_clouds(gpu_device):
    chunk = _chunk()
    rng = np.random.default_rng(7)
    origin = np.zeros(2)
    # (a) no trusted point; (b) the trusted minimum lies later than the overall minimum
    far_only = _random_cloud(rng, 300, trusted=0.0)
    later = _random_cloud(rng, 300, trusted=0.0, centre=(5.0, 5.0, 0.0))
    later[3, :3], later[3, 3] = (0.1, 0.0, 0.0), 0.375           # the closest point of all, far-tagged
    later[200, :3], later[200, 3] = (0.0, 1.0, 0.0), 1.0         # the only trusted points: this one and a farther one before it
    later[150, :3], later[150, 3] = (0.0, 2.0, 0.0), 1.0
    # (c) exact ties in different chunks: (3,4), (4,3), (-3,4), (5,0) are all exactly 5 from the origin, the cloud is farther
    ties = _random_cloud(rng, 3 * chunk, trusted=1.0, centre=(40.0, 40.0, 0.0))
    for i, xy in ((2 * chunk + 3, (3.0, 4.0)), (chunk + 7, (4.0, 3.0)), (chunk + 900, (-3.0, 4.0)), (2 * chunk + 1, (5.0, 0.0)),
                  (2 * chunk + 2, (4.0, 3.0))):                   # ... and an exact duplicate of the winner
        ties[i, :2] = xy
    # (d) two points with DIFFERENT sums of squares whose rounded roots are equal; the first one has the larger sum
    a = rng.uniform(0.5, 3.0, (4000, 2))
    b = a.copy()
    b[:, 0] = np.nextafter(a[:, 0], 9.0)
    sa, sb = (a * a).sum(1), (b * b).sum(1)
    hit = np.flatnonzero((sa != sb) & (np.linalg.norm(a, axis=1) == np.linalg.norm(b, axis=1)))
    assert len(hit) > 0, "no pair with equal rounded roots among 4000"
    j = int(hit[0])
    roots = np.array([[b[j, 0], b[j, 1], 0.0, 1.0], [a[j, 0], a[j, 1], 0.0, 1.0], [9.0, 9.0, 0.0, 1.0]])
    assert sb[j] > sa[j] and np.argmin(np.linalg.norm(roots[:, :2], axis=1)) == 0 and np.argmin((roots[:, :2] ** 2).sum(1)) == 1
    cases = [far_only, later, ties, roots]
    pairs = [_twins(gpu_device, {"chair": c}) for c in cases]
    hosts, devs = [p[0] for p in pairs], [p[1] for p in pairs]
    got = _best(hosts, devs, ["chair"] * 4, [origin] * 4)
    assert got[1].tolist() == [0.0, 1.0]
    assert got[2].tolist() == [4.0, 3.0]                          # index chunk + 7, the lowest of the five
    assert got[3].tolist() == [b[j, 0], b[j, 1]]
    # a class the map lacks, and an empty cloud under the name
    devs[0].clouds["bed"] = np.zeros((0, 4))
    hosts[0].clouds["bed"] = np.zeros((0, 4))
    assert _best(hosts[:2], devs[:2], ["bed", "tv"], [origin] * 2) == [None, None]


def test_hysteresis_over_several_calls(gpu_device):
    """One trusted point that moves between the calls: < 0.1 (kept), < 0.5 with the robot farther than 2 m (kept), < 0.5 with the
    robot nearer (taken), >= 0.5 (taken), each compared with the host twin, ``last_target_coord`` included."""
    rng = np.random.default_rng(9)
    base = _random_cloud(rng, 500, trusted=0.3, centre=(30.0, 30.0, 0.0))
    host, dev = _twins(gpu_device)
    script = [((3.0, 0.0), (0.0, 0.0)), ((3.05, 0.0), (0.0, 0.0)), ((3.3, 0.0), (0.0, 0.0)), ((3.3, 0.0), (2.0, 0.0)),
              ((3.35, 0.0), (2.0, 0.0)), ((4.0, 0.0), (0.0, 0.0)), ((4.0, 0.45), (0.0, 0.0)), ((4.0, 0.45), (3.5, 0.0))]
    goals = []
    for point, robot in script:
        cloud = base.copy()
        cloud[77] = (point[0], point[1], 0.2, 1.0)
        host.clouds["tv"], dev.clouds["tv"] = cloud.copy(), cloud.copy()
        goals.append(_best([host], [dev], ["tv"], [np.array(robot)])[0].tolist())
    assert goals == [[3.0, 0.0], [3.0, 0.0], [3.0, 0.0], [3.3, 0.0], [3.3, 0.0], [4.0, 0.0], [4.0, 0.0], [4.0, 0.45]]


# ---------------------------------------------------------------------------------------------- 3. the cone at the edges
def _tagged(points, tag):
    points = np.asarray(points, np.float64).reshape(-1, 3)
    return np.concatenate([points, np.full((len(points), 1), tag)], axis=1)


def test_cone_range_is_inclusive_and_exact(gpu_device):
    """Origin 0, heading at the point (1.5, 2.0, 0): its distance is exactly 2.5 = max_depth / 2 and it is inside; with y one ulp
    larger the distance is the next f64 above 2.5 and the point is outside."""
    yaw = float(np.arctan2(2.0, 1.5))
    above = np.nextafter(2.0, 3.0)
    assert np.linalg.norm([1.5, 2.0, 0.0]) == 2.5 and np.linalg.norm([1.5, above, 0.0]) == np.nextafter(2.5, 3.0)
    cloud = np.concatenate([_tagged([[9.0, 9.0, 0.0]], 1.0), _tagged([[1.5, 2.0, 0.0]], 0.25), _tagged([[1.5, above, 0.0]], 0.5),
                            _tagged([[7.0, 7.0, 0.0], [7.0, 7.5, 0.0]], 0.25), _tagged([[6.0, 6.0, 0.0]], 0.5)])
    host, dev = _twins(gpu_device, {"chair": cloud})
    assert _explore(host, dev, _tf(0.0, 0.0, yaw), max_depth=5.0)
    assert sorted(set(dev.clouds["chair"][:, 3].tolist())) == [0.5, 1.0] and len(dev.clouds["chair"]) == 3


@pytest.mark.parametrize("heading", [np.pi - 1e-3, -np.pi + 1e-3, np.pi, -np.pi + 1e-12])
def test_cone_across_the_wrap(gpu_device, heading):
    """Headings next to +-pi with points on both sides of the wrap: one tag per direction, directions from just inside to just
    outside both edges of the cone."""
    half = FOV / 2
    offsets = [-half - 0.01, -half + 0.01, -0.02, 0.0, 0.02, half - 0.01, half + 0.01, np.pi - 0.5]
    rows = [_tagged([[9.0, 0.0, 0.0]], 1.0)]
    for s, off in enumerate(offsets):
        ang = heading + off
        rows.append(_tagged([[r * np.cos(ang), r * np.sin(ang), 0.1] for r in (0.5, 1.7, 2.6)], 0.1 + 0.05 * s))
    host, dev = _twins(gpu_device, {"chair": np.concatenate(rows)})
    assert _explore(host, dev, _tf(0.0, 0.0, heading))
    left = sorted(set(dev.clouds["chair"][:, 3].tolist()))
    assert left == sorted([1.0, 0.1, 0.1 + 0.05 * 6, 0.1 + 0.05 * 7])


def test_cone_tags_across_commits_and_rounding(gpu_device):
    """Through ``_commit``: a far tag that appears in two separate commits goes as a whole; a tag that np.float32 rounds to exactly
    1.0 is trusted; a slot whose only point inside the cone is the cloud's last row is found."""
    class Scripted:
        def __init__(self, values):
            self.values = list(values)

        def rand(self):
            return self.values.pop(0)

    opm = _opm()
    rng = np.random.default_rng(3)
    almost_one = 1.0 - 1e-9

    def frame(n, lo, hi):
        return np.stack([rng.uniform(lo, hi, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)], axis=1)

    blocks = [(frame(40, 4.0, 4.99), False, _tf(0, 0, 0.0)),             # 1.0 and f32(0.5), ahead
              (frame(30, 2.0, 3.0), True, _tf(0, 0, 2.0)),               # 0.5 again, elsewhere (too offset)
              (frame(30, 4.8, 4.99), False, _tf(0, 0, 0.0)),             # f32(1 - 1e-9) = 1.0: trusted although "far"
              (frame(20, 2.0, 3.0), True, _tf(0, 0, 0.0)),               # f64 1 - 1e-9: far
              (frame(25, 2.0, 3.0), True, _tf(0, 0, -2.0)),              # 0.75, elsewhere
              (np.array([[2.0, 0.0, 0.0]]), True, _tf(0, 0, 3.0))]       # 0.125: ONE point, the last row
    maps = []
    for _ in range(2):
        m = opm.ObjectPointCloudMap(erosion_size=1, device=gpu_device, rng=Scripted([0.5, 0.5, almost_one, almost_one, 0.75, 0.125]))
        for cam, off, tf in blocks:
            m._commit("bed", cam, lambda off=off: off, tf, 5.0)
        maps.append(m)
    host, dev = maps
    assert len(dev.clouds["bed"]) == 146 and _same_clouds(host, dev)
    assert _explore(host, dev, _tf(0, 0, 3.0), max_depth=5.0)            # sees the last row only
    assert len(dev.clouds["bed"]) == 145
    assert not _explore(host, dev, _tf(0, 0, 1.0), max_depth=5.0)        # sees nothing
    assert _explore(host, dev, _tf(0, 0, 0.0), max_depth=10.0)           # ahead: 0.5 (both commits) and 1 - 1e-9 go, f32's 1.0 stays
    assert sorted(set(dev.clouds["bed"][:, 3].tolist())) == [0.75, 1.0]
    assert int((dev.clouds["bed"][:, 3] == 1.0).sum()) >= 31 and len(dev.clouds["bed"]) < 145 - 30 - 20 + 1


def test_all_near_cloud_is_not_queried(gpu_device):
    opm = _opm()
    rng = np.random.default_rng(4)
    maps = _twins(gpu_device)
    cam = np.stack([rng.uniform(2.0, 3.0, 50), rng.uniform(-0.2, 0.2, 50), rng.uniform(-0.2, 0.2, 50)], axis=1)
    for m in maps:
        m._commit("chair", cam, lambda: False, _tf(0, 0, 0.0), 5.0)
        assert m._all_near("chair")
    launches, syncs, up = _launches(), opm.SYNCS[0], opm.UPLOADED_BYTES[0]
    assert not _explore(*maps, _tf(0, 0, 0.0))
    assert (_launches(), opm.SYNCS[0], opm.UPLOADED_BYTES[0]) == (launches, syncs, up)
    # an unrecognised array of trusted points only: uploaded and looked at once, but nothing to ask
    for m in maps:
        m.clouds["chair"] = m.clouds["chair"].copy()
    assert not _explore(*maps, _tf(0, 0, 0.0))
    assert _launches() == launches and opm.UPLOADED_BYTES[0] == up + 50 * 36


def test_points_on_the_edge_of_the_cone_go_to_the_host(gpu_device):
    """Points built AT heading +- fov / 2: the device leaves their slots uncertain, the host decides them (BAND_POINTS rises), and
    the result is the host method's."""
    opm = _opm()
    heading, half = 0.7, FOV / 2
    rows = [_tagged([[9.0, 0.0, 0.0]], 1.0)]
    for s, sign in enumerate((1.0, -1.0)):
        ang = heading + sign * half
        rows.append(_tagged([[r * np.cos(ang), r * np.sin(ang), 0.0] for r in (0.3, 0.9, 1.3, 1.9, 2.4)], 0.25 + 0.25 * s))
    rows.append(_tagged([[2.0 * np.cos(heading + 2.0), 2.0 * np.sin(heading + 2.0), 0.0]], 0.875))      # clearly outside
    host, dev = _twins(gpu_device, {"chair": np.concatenate(rows)})
    band = opm.BAND_POINTS[0]
    _explore(host, dev, _tf(0.0, 0.0, heading))
    assert opm.BAND_POINTS[0] >= band + 5
    assert 0.875 in dev.clouds["chair"][:, 3]


def test_random_points_never_fall_in_the_band(gpu_device):
    """200 000 uniformly random points under 64 far tags: no point may need the host (the band must not hide a wrong kernel), and
    the tags dropped are the host's."""
    opm = _opm()
    rng = np.random.default_rng(11)
    n = 200000
    cloud = np.concatenate([rng.uniform(-4.0, 4.0, (n, 2)), rng.uniform(-1.0, 1.0, (n, 1)),
                            (0.001 + rng.integers(0, 64, (n, 1))) / 80.0], axis=1)
    # tags 0..31 are far away from the origin (none may be dropped from there), 32..63 are everywhere
    low = cloud[:, 3] < 0.4
    cloud[low, :2] += 20.0
    host, dev = _twins(gpu_device, {"chair": cloud})
    band = opm.BAND_POINTS[0]
    assert _explore(host, dev, _tf(0.1, -0.2, 2.5, z=0.3))
    assert opm.BAND_POINTS[0] == band
    assert len(set(dev.clouds["chair"][:, 3].tolist())) == 32
    band = opm.BAND_POINTS[0]
    assert _explore(host, dev, _tf(20.5, 19.0, -1.0, z=0.0))
    assert opm.BAND_POINTS[0] == band and dev.clouds["chair"].shape == (0, 4)        # every tag had a point in view
    assert not _explore(host, dev, _tf(0.0, 0.0, 0.0))                               # an empty cloud is not asked


def test_full_circle_cone_takes_the_host_path(gpu_device):
    opm = _opm()
    rng = np.random.default_rng(12)
    cloud = _random_cloud(rng, 400, trusted=0.5, centre=(1.0, 1.0, 0.0))
    for fov, device_path in ((2 * np.pi, False), (2 * (np.pi - 5e-10), False), (2 * (np.pi - 1e-6), True)):
        host, dev = _twins(gpu_device, {"chair": cloud})
        launches = _launches()
        assert _explore(host, dev, _tf(0.0, 0.0, 0.3), fov=fov)
        assert (_launches() > launches) == device_path, fov
        assert set(dev.clouds["chair"][:, 3].tolist()) == {1.0}


# ---------------------------------------------------------------------------------------------- 4. mirror bookkeeping
def test_uploads_follow_commits_drops_and_assignments(gpu_device):
    opm = _opm()
    rng = np.random.default_rng(13)

    def frame(n, lo, hi):
        return np.stack([rng.uniform(lo, hi, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)], axis=1)

    host, dev = _twins(gpu_device)
    here, p = _tf(0, 0, 0.0), np.array([0.0, 0.0])

    def commit(cam, off, tf=here):
        for m in (host, dev):
            m._commit("chair", cam, lambda: off, tf, 5.0)

    def uploaded(action):
        before = opm.UPLOADED_BYTES[0]
        action()
        return opm.UPLOADED_BYTES[0] - before

    commit(frame(1500, 2.0, 3.0), False)                           # more rows than the mirror's first capacity
    assert uploaded(lambda: _best([host], [dev], ["chair"], [p])) == 1500 * 36
    assert uploaded(lambda: _best([host], [dev], ["chair"], [p])) == 0
    commit(frame(700, 4.0, 4.99), False)                           # mixed tags; the capacity doubles (2048 < 2200)
    assert uploaded(lambda: _explore(host, dev, _tf(0, 0, 2.0))) == 700 * 36       # the appended rows only; nothing in view
    commit(frame(100, 2.0, 3.0), True, _tf(0, 0, 3.0))
    assert uploaded(lambda: _best([host], [dev], ["chair"], [p])) == 100 * 36
    n = len(dev.clouds["chair"])
    assert n == 2300
    assert _explore(host, dev, _tf(0, 0, 3.0), max_depth=8.0)      # drops the 100
    assert len(dev.clouds["chair"]) == 2200
    assert uploaded(lambda: _best([host], [dev], ["chair"], [p])) == 2200 * 36     # after a drop: the whole cloud
    for m in (host, dev):
        m.clouds["chair"] = m.clouds["chair"][::-1].copy()         # a fresh array under the name
    assert uploaded(lambda: _best([host], [dev], ["chair"], [np.array([1.0, 1.0])])) == 2200 * 36
    assert _explore(host, dev, _tf(0, 0, 0.0), max_depth=10.0)     # and its far tag is still found
    # reset: nothing stale answers -- a different cloud of the SAME length under the same name
    stale = dev.clouds["chair"]
    for m in (host, dev):
        m.reset()
    assert _best([host], [dev], ["chair"], [p]) == [None]
    fresh = _random_cloud(rng, len(stale), trusted=0.5)
    for m in (host, dev):
        m.clouds["chair"] = fresh.copy()
    assert uploaded(lambda: _best([host], [dev], ["chair"], [p])) == len(stale) * 36


def test_cloud_with_a_nan_takes_the_host_path(gpu_device):
    opm = _opm()
    rng = np.random.default_rng(14)
    cloud = _random_cloud(rng, 300, trusted=0.5, centre=(1.0, 0.5, 0.0))
    cloud[17, 1] = np.nan
    other = _random_cloud(rng, 300, trusted=0.5, centre=(1.0, 0.5, 0.0))
    other[5, 2] = np.inf
    host, dev = _twins(gpu_device, {"chair": cloud, "bed": other})
    launches, up = _launches(), opm.UPLOADED_BYTES[0]
    _best([host, host], [dev, dev], ["chair", "bed"], [np.zeros(2), np.ones(2)])
    _explore(host, dev, _tf(0.0, 0.0, 0.4))
    assert _launches() == launches and opm.UPLOADED_BYTES[0] == up and dev._mirrors == {}


# ---------------------------------------------------------------------------------------------- 5. launches and read-backs
def test_launches_and_read_backs_do_not_grow_with_the_maps(gpu_device):
    opm = _opm()
    rng = np.random.default_rng(15)
    cost = {}
    for E in (2, 32):
        maps = []
        for e in range(E):
            m = opm.ObjectPointCloudMap(erosion_size=1, device=gpu_device)
            m.clouds = {"chair": _random_cloud(rng, 100 + 37 * e, trusted=0.5, centre=(1.0, 0.0, 0.0)),
                        "bed": _random_cloud(rng, 50 + e, trusted=0.0, centre=(0.0, 1.0, 0.0))}
            maps.append(m)
        before = (_launches(), opm.SYNCS[0])
        dropped = opm.update_explored_batch(maps, [_tf(0.0, 0.0, 0.1 * e) for e in range(E)], MAX_DEPTH, FOV)
        mid = (_launches(), opm.SYNCS[0])
        goals = opm.get_best_objects_batch(maps, ["chair"] * E, [np.zeros(2)] * E)
        after = (_launches(), opm.SYNCS[0])
        assert any(dropped) and all(g is not None for g in goals)
        cost[E] = (mid[0] - before[0], mid[1] - before[1], after[0] - mid[0], after[1] - mid[1])
    assert cost[2] == cost[32] == (1, 1, 2, 1), cost


# ---------------------------------------------------------------------------------------------- 6. the harness
def test_harness_device_clouds_equal_host_clouds(gpu_device):
    """Two closed-loop ObjectNav harnesses of 8 environments as in tests/test_object_map_batch_gpu.py, one with
    device_object_clouds=False, equal step for step."""
    import torch

    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from world_object_cases import A

    opm = _opm()
    bed = (2.95, 1.42, 3.95, 2.32, 0.0, 0.7)

    def layout(env_id, episode, robot_xy):
        if episode == 0 and env_id in (0, 1):
            return [("chair", A)] if env_id == 0 else [("bed", bed)]
        return S.object_layout(env_id, episode, robot_xy)

    sims = [BatchedEpisodes(8, device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True,
                            world_objects=WorldObjects(layout=layout, max_episode_steps=100), object_maps=True,
                            device_object_clouds=on) for on in (False, True)]
    a, b = sims
    assert b.device_object_clouds and not a.device_object_clouds
    device_drops = object_goals = 0
    for t in range(20):
        a.step()
        launches, b.last_explored_drops = _launches(), None
        b.step()
        queried = _launches() > launches
        assert np.array_equal(a.last_goals, b.last_goals, equal_nan=True), t
        assert a.last_modes == b.last_modes, t
        assert np.array_equal(a.last_world_actions, b.last_world_actions), t
        for ma, mb in zip(a.object_maps, b.object_maps):
            assert _same_clouds(ma, mb), t
            assert _same(ma.last_target_coord, mb.last_target_coord), t
            sa, sb = ma._rng.get_state(), mb._rng.get_state()
            assert len(sa) == len(sb) and all(np.array_equal(x, y) for x, y in zip(sa, sb)), t
        device_drops += bool(queried and b.last_explored_drops and any(b.last_explored_drops.values()))
        object_goals += any(m == "navigate" for m in b.last_modes)
    torch.cuda.synchronize()
    print("harness: steps with a device query that dropped a tag: %d, steps with an object goal: %d" % (device_drops, object_goals))
    assert device_drops >= 1
    assert object_goals >= 1
    assert a.object_stats.keys() == b.object_stats.keys()
    for key in a.object_stats:
        assert np.array_equal(np.asarray(a.object_stats[key]), np.asarray(b.object_stats[key])), key
    assert a.live.objectnav_stats.keys() == b.live.objectnav_stats.keys()
    for key in a.live.objectnav_stats:
        assert np.array_equal(np.asarray(a.live.objectnav_stats[key]), np.asarray(b.live.objectnav_stats[key])), key
