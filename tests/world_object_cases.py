"""Scenes shared by tests/test_world_objects_cpu.py and tests/test_world_objects_gpu.py: camera poses (x, y, heading index) and
objects (x0, y0, x1, y1, z0, z1) of the rooms world that exercise one edge of the rendering contract each, and the NumPy
reference frames of a pose / object set, rendered once per process."""
import functools

import numpy as np

from vlfm_amd import synthetic as S

# the issue's pinned scene: seen from (0, 0)
A = (2.25, -0.25, 2.75, 0.25, 0.0, 0.9)
B = (3.2, 0.6, 3.6, 1.0, 0.0, 1.3)

# name -> ((x, y, k), [box6])
EDGES = {
    # the hall's north wall segment (-1.4, 4.0)-(1.4, 4.3) stands between the camera and the object
    "behind_wall": ((0.0, 2.0, 3), [(0.5, 4.8, 1.0, 5.3, 0.0, 1.2)]),
    # the pillar (1.3, 0.9)-(1.9, 1.5) in front of a wider object
    "behind_pillar": ((0.0, 1.2, 0), [(3.0, -0.2, 3.4, 2.6, 0.0, 1.2)]),
    "camera_inside": ((0.0, 0.0, 0), [(-0.3, -0.3, 0.3, 0.3, 0.0, 1.5)]),
    # seen through the hall's east doorway, 5.6 m away: beyond the 5 m range, like the boundary wall behind it
    "beyond_range": ((-1.0, 2.0, 0), [(4.6, 1.8, 5.0, 2.2, 0.0, 1.4)]),
    "low_before_tall": ((0.0, 0.0, 0), [(2.5, -0.3, 2.9, 0.3, 0.0, 1.4), (1.5, -0.2, 1.8, 0.2, 0.0, 0.5)]),
    "hanging": ((0.0, 0.0, 0), [(2.0, -0.3, 2.4, 0.3, 1.0, 1.5)]),
    "identical": ((0.0, 0.0, 0), [A, A]),
}
# a full set of 8 in one environment, in a ring around (0, 0) (some behind the hall's pillars, some overlapping in the image)
RING8 = [S.object_box(cls, 2.6 * np.cos(a), 2.6 * np.sin(a))
         for cls, a in zip(list(S.OBJECT_SIZES) + ["chair", "tv"], np.linspace(0.2, 0.2 + 2 * np.pi, 8, endpoint=False))]
# five environments with different objects (environment 4 has none)
ENV_OBJECTS = [[A, B], EDGES["low_before_tall"][1] + EDGES["hanging"][1], RING8,
               EDGES["identical"][1] + EDGES["camera_inside"][1] + EDGES["behind_pillar"][1], []]


@functools.lru_cache(maxsize=None)
def tour():
    return S.integrate(S.plan_actions(S.ROOMS_STEPS))


@functools.lru_cache(maxsize=None)
def poses():
    """Every 25th pose of the tour and its 11 turns on the spot: all 12 headings, the exact-zero dx / dy columns."""
    return tour()[::25] + tour()[1:12]


def objects_array(env_objects) -> np.ndarray:
    """[n_envs, 8, 8] f64 records (x0 y0 x1 y1 z0 z1 valid pad) of per-environment lists of box6."""
    out = np.zeros((len(env_objects), S.WORLD_MAX_OBJECTS, 8))
    for e, boxes in enumerate(env_objects):
        for k, b in enumerate(boxes):
            out[e, k, :6], out[e, k, 6] = b, 1.0
    return out


def render(pose, boxes, H, W, hfov_fx=None, height=S.CAMERA_HEIGHT, lo=S.MIN_DEPTH, hi=S.MAX_DEPTH):
    x, y, k = pose
    c, s = S.HEADINGS[k]
    fx = S.camera_intrinsics(W)[0] if hfov_fx is None else hfov_fx
    return S.render_objects_numpy(x, y, c, s, height, fx, lo, hi, H, W, boxes)


@functools.lru_cache(maxsize=None)
def reference(pose_index: int, env: int, H: int, W: int):
    """(depth, ids, stats) of pose ``poses()[pose_index]`` looking at ``ENV_OBJECTS[env]``; read-only."""
    d, i = render(poses()[pose_index], ENV_OBJECTS[env], H, W)
    st = S.object_stats_numpy(i)
    for a in (d, i, st):
        a.setflags(write=False)
    return d, i, st
