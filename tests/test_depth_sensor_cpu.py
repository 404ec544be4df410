"""The depth sensor's host statement (vlfm_amd/synthetic.py: DepthSensor, depth_sensor_numpy).  No GPU."""
import functools

import numpy as np
import pytest

import vlfm_amd.synthetic as S

LO, HI = np.float32(S.MIN_DEPTH), np.float32(S.MAX_DEPTH)
F = np.float32


@functools.lru_cache(maxsize=None)
def prototype_frame(H=48, W=64):
    """The rooms world seen from (0.6, 2.0) heading +x with a chair at (2.0, 2.0): walls, floor, a doorway and a silhouette."""
    d = S.render_objects_numpy(0.6, 2.0, 1.0, 0.0, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH, H, W,
                               [S.object_box("chair", 2.0, 2.0)])[0]
    d.setflags(write=False)
    return d


ALL_ON = S.DepthSensor(seed=5, sigma0_m=0.004, sigma2_per_m=0.003, disparity_k=35.0, dropout=0.08, patch_dropout=0.1, edge_m=0.4,
                       min_range_m=0.55, max_range_m=4.6)


def test_every_stage_off_returns_its_input():
    d = prototype_frame()
    assert len(np.unique(d)) > 30
    out, n = S.depth_sensor_numpy(d, LO, HI, S.DepthSensor(), 3, 7)
    assert out.dtype == np.float32 and out.tobytes() == d.tobytes() and n == 0
    odd = d.copy()
    odd[0, :3], odd[5, 5], odd[47, 63] = (1e-3, 1.0, np.nan), np.nan, 1e-3
    out, n = S.depth_sensor_numpy(odd, LO, HI, S.DepthSensor(seed=9), 0, 0)
    assert out.tobytes() == odd.tobytes() and n == 0
    # holes alone leave every valid pixel the input value, bit for bit: the trip through metres is not made
    out, n = S.depth_sensor_numpy(d, LO, HI, S.DepthSensor(dropout=0.3, patch_dropout=0.1, edge_m=0.3, max_range_m=4.0), 3, 7)
    assert 0 < n == int((out == 0).sum()) < d.size and out[out != 0].tobytes() == d[out != 0].tobytes()


def test_hand_computed_frame():
    """lo = 0, hi = 8, d = z / 8 with every z a multiple of 0.5: span = 8 and z = 0 + d * 8 are exact.  The sensor: range
    [1.0, 3.75] m, edge_m = 1.0, disparity_k = 5, no noise, no dropout (no hash).  Metres:

        0.5  1.5  2.5  3.5
        1.5  2.0  3.5  3.5
        1.5  2.0  3.0  4.0
        3.0  2.0  3.0  5.0

    invalid  (0,0): 0.5 < 1.0.  (2,3): 4.0 > 3.75; its neighbours differ by 1.0, 0.5 and 1.0: no edge.  (3,3): 5.0 > 3.75.
             Interior step: |2.0 - 3.5| = 1.5 > 1 between (1,1) and (1,2): both.  Steps at the border: |1.5 - 3.0| = 1.5 down
             the left column between (2,0) and (3,0): both; |3.0 - 5.0| = 2 along the bottom row between (3,2) and (3,3): both.
             Every other difference between neighbours is 0, 0.5 or exactly 1.0 (e.g. 0.5 | 1.5 | 2.5 | 3.5 along the top row,
             2.0 | 3.0 in rows 2 and 3, 4.0 over 5.0): exactly edge_m is NOT invalid.  Eight pixels invalid.
    valid    m = rint(5 / z), z1 = 5 / m, out = z1 / 8 (a power of two: exact):
             z = 1.5 at (0,1), (1,0): 5 / 1.5 = 3.33 -> 3, z1 = f32(5 / 3), out = f32(5 / 3) / 8
             z = 2.0 at (2,1), (3,1): 5 / 2 = 2.5 -> 2 (half to even; half up would give 3), z1 = 2.5, out = 0.3125
             z = 2.5 at (0,2): 2 -> 2.5 -> 0.3125;  z = 3.0 at (2,2): 1.67 -> 2 -> 2.5 -> 0.3125
             z = 3.5 at (0,3), (1,3): 1.43 -> 1, z1 = 5, out = 0.625"""
    z = np.array([[0.5, 1.5, 2.5, 3.5], [1.5, 2.0, 3.5, 3.5], [1.5, 2.0, 3.0, 4.0], [3.0, 2.0, 3.0, 5.0]], np.float32)
    sensor = S.DepthSensor(disparity_k=5.0, edge_m=1.0, min_range_m=1.0, max_range_m=3.75)
    t = F(5) / F(3) / F(8)
    want = np.array([[0, t, 0.3125, 0.625], [t, 0, 0, 0.625], [0, 0.3125, 0.3125, 0], [0, 0.3125, 0, 0]], np.float32)
    out, n = S.depth_sensor_numpy(z / F(8), 0.0, 8.0, sensor, 1, 2)
    assert out.tobytes() == want.tobytes() and n == 8
    # the same frame in another environment at another clock: nothing here is hashed
    assert S.depth_sensor_numpy(z / F(8), 0.0, 8.0, sensor, 7, 9)[0].tobytes() == want.tobytes()
    # quantisation floors: z1 below 1e-3 is lifted to it (m = 5000), a disparity below one step is one step (z1 = k)
    q = S.DepthSensor(disparity_k=5.0)
    out, n = S.depth_sensor_numpy(np.array([[0.0, 1.0]], np.float32), 0.0, 16.0, q, 0, 0)
    assert n == 0 and out.tobytes() == np.array([[1e-3, 0.3125]], np.float32).tobytes()     # 5 / rint(5 / 1e-3f) / 16 < 1e-3; 5 / 16


def loop_statement(d, lo, hi, s, env_id, clock):
    """The rule again, one pixel at a time over synthetic._mix32 and f32 scalars; it shares nothing with the vectorised statement."""
    H, W = d.shape
    lo, hi = F(lo), F(hi)
    span = F(hi - lo)
    kf = S._mix32(S._mix32(s.seed, env_id, 51), clock, 52)
    t_drop = min(int(s.dropout * 2 ** 32), 2 ** 32 - 1)
    t_patch = min(int(s.patch_dropout * 2 ** 32), 2 ** 32 - 1)
    z = [[F(lo + F(d[r, u] * span)) for u in range(W)] for r in range(H)]
    out, count = np.empty((H, W), np.float32), 0
    with np.errstate(all="ignore"):
        for r in range(H):
            for u in range(W):
                p, zz = r * W + u, z[r][u]
                bad = (s.min_range_m > 0 or s.max_range_m < np.inf) and not (zz >= F(s.min_range_m) and zz <= F(s.max_range_m))
                if s.edge_m > 0:
                    for rn, un in ((r - 1, u), (r + 1, u), (r, u - 1), (r, u + 1)):
                        if 0 <= rn < H and 0 <= un < W and abs(F(z[rn][un] - zz)) > F(s.edge_m):
                            bad = True
                bad = bad or S._mix32(kf, p, 55) < t_drop or S._mix32(kf, (r >> 3) * ((W + 7) >> 3) + (u >> 3), 56) < t_patch
                if bad:
                    out[r, u] = 0.0
                    count += 1
                    continue
                if s.sigma0_m == s.sigma2_per_m == s.disparity_k == 0:
                    out[r, u] = d[r, u]
                    continue
                h1, h2 = S._mix32(kf, p, 53), S._mix32(kf, p, 54)
                n = (h1 & 0xFFFF) + (h1 >> 16) + (h2 & 0xFFFF) + (h2 >> 16) - 131070
                nf = F(F(n) * F(1.0 / np.sqrt(1431655765.0)))
                z1 = F(zz + F(F(F(s.sigma0_m) + F(F(s.sigma2_per_m) * F(zz * zz))) * nf))
                if s.disparity_k > 0:
                    z1 = max(z1, F(1e-3))
                    m = max(F(np.rint(F(F(s.disparity_k) / z1))), F(1.0))
                    z1 = F(F(s.disparity_k) / m)
                out[r, u] = min(max(F(F(z1 - lo) / span), F(1e-3)), F(1.0))
    return out, count


@pytest.mark.parametrize("sensor", [ALL_ON, S.DepthSensor(seed=2, dropout=0.2, patch_dropout=0.2),
                                    S.DepthSensor(seed=3, sigma0_m=0.01, sigma2_per_m=0.01)])
def test_against_a_per_pixel_restatement(sensor):
    d = prototype_frame(9, 18)
    for env_id, clock, lo, hi in ((0, 0, LO, HI), (3, 11, 0.3, 6.0)):
        got, want = S.depth_sensor_numpy(d, lo, hi, sensor, env_id, clock), loop_statement(d, lo, hi, sensor, env_id, clock)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
        assert (0 < got[1] < d.size) if sensor.dropout else got[1] == 0


def test_determinism():
    d = prototype_frame()
    args = (d, LO, HI, ALL_ON, 3, 7)
    first = S.depth_sensor_numpy(*args)
    for other in ((d, LO, HI, ALL_ON, 4, 7), (d, LO, HI, ALL_ON, 3, 8),
                  (d, LO, HI, S.DepthSensor(**{**vars(ALL_ON), "seed": 6}), 3, 7)):
        assert not np.array_equal(S.depth_sensor_numpy(*other)[0] == 0, first[0] == 0)          # another hole pattern
    again = S.depth_sensor_numpy(*args)                       # after other frames were sensed: no generator state
    assert again[0].tobytes() == first[0].tobytes() and again[1] == first[1]
    assert S.DepthSensor(seed=1).frame_keys([3, 2 ** 32 + 3], [7, 7]).tolist() == [S._mix32(S._mix32(1, 3, 51), 7, 52)] * 2


def test_statistics():
    d = prototype_frame()
    H, W = d.shape
    n = S.depth_sensor_numpy(d, LO, HI, S.DepthSensor(dropout=0.1), 0, 0)[1]
    assert abs(n - 0.1 * H * W) <= 6 * np.sqrt(H * W * 0.1 * 0.9), n / (H * W)
    # nf of 4 environments x 4 clocks
    keys = S.DepthSensor(seed=1).frame_keys(np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4))
    nf = np.concatenate([S.depth_sensor_noise(int(k), H, W).astype(np.float64).ravel() for k in keys])
    assert len(nf) == 49152 and len(set(keys.tolist())) == 16
    assert abs(nf.mean()) <= 6 / np.sqrt(len(nf)), nf.mean()
    assert abs(nf.std() - 1) <= 0.03, nf.std()
    # the edge stage: only pixels with such a neighbour, and at least one
    out, n = S.depth_sensor_numpy(d, LO, HI, S.DepthSensor(edge_m=0.3), 0, 0)
    z = (LO + d * (HI - LO)).astype(np.float32)
    big = np.zeros((H, W), bool)
    dv, dh = np.abs(np.diff(z, axis=0)) > F(0.3), np.abs(np.diff(z, axis=1)) > F(0.3)
    big[1:] |= dv
    big[:-1] |= dv
    big[:, 1:] |= dh
    big[:, :-1] |= dh
    assert n == int(big.sum()) >= 1 and np.array_equal(out == 0, big)


@pytest.mark.parametrize("bad", [dict(seed=-1), dict(seed=1.5), dict(seed=2 ** 32), dict(sigma0_m=-0.1), dict(sigma0_m=np.nan),
                                 dict(sigma2_per_m=np.inf), dict(sigma2_per_m=-1), dict(disparity_k=-1.0), dict(disparity_k=np.inf),
                                 dict(dropout=-0.01), dict(dropout=0.51), dict(dropout=np.nan), dict(patch_dropout=0.6),
                                 dict(patch_dropout=-1), dict(edge_m=-0.3), dict(edge_m=np.inf), dict(min_range_m=-1),
                                 dict(min_range_m=np.inf), dict(max_range_m=-1), dict(max_range_m=np.nan), dict(sigma0_m="1")])
def test_refusals(bad):
    with pytest.raises(ValueError):
        S.DepthSensor(**bad)


def test_what_is_accepted():
    s = S.DepthSensor(dropout=0.5, patch_dropout=0.5, max_range_m=np.inf)
    assert s.thresholds() == (2 ** 31, 2 ** 31) and S.DepthSensor().thresholds() == (0, 0)
    with pytest.raises(Exception):
        s.seed = 1                                             # frozen
