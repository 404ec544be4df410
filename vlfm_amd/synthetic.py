"""Synthetic RGB-D episodes of SURVEY.md section 8(d): deterministic (PCG64, seed = 1234 + env_id) depth frames,
scripted trajectories and stub values.  Used by bench.py, the harness and the parity tests (both the HIP path and the
oracle are fed from here, so they see identical inputs)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

HFOV_DEG = 79.0
MIN_DEPTH, MAX_DEPTH = 0.5, 5.0
CAMERA_HEIGHT = 0.88


def camera_intrinsics(width: int, hfov_deg: float = HFOV_DEG):
    """fx = fy = W / (2 tan(hfov/2))  (/root/reference/vlfm/policy/habitat_policies.py:91)."""
    hfov = np.deg2rad(hfov_deg)
    fx = width / (2 * np.tan(hfov / 2))
    return float(fx), float(fx), float(hfov)


def depth_frame(rng: np.random.Generator, height: int = 480, width: int = 640, holes: bool = False) -> np.ndarray:
    """Piecewise-smooth wall profile + floor plane, normalised to (0,1] (no exact zeros unless holes=True)."""
    wall = rng.uniform(1.0, 5.0, size=width + 30)
    d = depth_from_profile(np.convolve(wall, np.ones(31) / 31.0, mode="valid")[:width], height)
    if holes:
        for _ in range(5):
            r0, c0 = rng.integers(0, height - 40), rng.integers(0, width - 40)
            d[r0:r0 + rng.integers(5, 40), c0:c0 + rng.integers(5, 40)] = 0.0
    return d


def rgb_frame(rng: np.random.Generator, height: int = 480, width: int = 640) -> np.ndarray:
    return rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8)


def pose_to_tf(x: float, y: float, yaw: float, z: float = CAMERA_HEIGHT) -> np.ndarray:
    """geometry_utils.py:162-180 (xyz_yaw_to_tf_matrix)."""
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, z], [0, 0, 0, 1]])


class Trajectory:
    """Steps 0-11 turn 30 deg (habitat_policies.py:150-153), then forward 0.25 m w.p. 0.7 / turn +-30 deg."""

    def __init__(self, env_id: int, limit: float = 20.0) -> None:
        self.rng = np.random.Generator(np.random.PCG64(1234 + env_id))
        self.x = self.y = self.yaw = 0.0
        self.t = 0
        self.limit = limit

    def step(self):
        if self.t > 0:
            if self.t <= 11:
                self.yaw += np.deg2rad(30)
            else:
                u = self.rng.uniform()
                if u < 0.7:
                    nx, ny = self.x + 0.25 * np.cos(self.yaw), self.y + 0.25 * np.sin(self.yaw)
                    if abs(nx) <= self.limit and abs(ny) <= self.limit:
                        self.x, self.y = nx, ny
                    else:
                        self.yaw += np.deg2rad(30)
                elif u < 0.85:
                    self.yaw += np.deg2rad(30)
                else:
                    self.yaw -= np.deg2rad(30)
        self.t += 1
        yaw = (self.yaw + np.pi) % (2 * np.pi) - np.pi
        return self.x, self.y, yaw


class SyntheticEnv:
    def __init__(self, env_id: int, height: int = 480, width: int = 640, holes: bool = False, channels: int = 1):
        self.traj = Trajectory(env_id)
        self.rng = np.random.Generator(np.random.PCG64(99991 + env_id))
        self.height, self.width, self.holes, self.channels = height, width, holes, channels

    def observe(self):
        x, y, yaw = self.traj.step()
        depth = depth_frame(self.rng, self.height, self.width, self.holes)
        values = self.rng.uniform(0.15, 0.45, size=self.channels)
        return depth, pose_to_tf(x, y, yaw), values


# ---------------------------------------------------------------------------------------------- a consistent world
# Rooms, doorways, free-standing pillars, an L-shaped block and a U-shaped alcove, rendered by per-column ray casting.
# Everything that produces an observation uses only IEEE-exact operations (+ - * / sqrt, comparisons): headings are
# multiples of 30 degrees whose cosines / sines come from a sqrt(3)/2 table, a ray through image column u has the
# camera-frame direction (1, -(u - W/2)/fx) -- so the ray parameter IS the depth along the optical axis -- and poses are
# integrated from an action string (turn 30 degrees / forward 0.25 m: the reference's simulator step sizes,
# vlfm/policy/action_replay_policy.py:41-42).  Used by the 500-step golden episode (tests/golden/world500.py), the
# config-5 parity test and the batched-episode harness (frontier-rich maps instead of the per-frame random walls above).
ROOMS_H, ROOMS_W = 480, 640
ROOMS_STEPS = 500
_S3 = float(np.sqrt(3.0) / 2.0)
# (cos, sin) of k * 30 degrees, k = 0..11 -- sqrt is correctly rounded everywhere
HEADINGS = [(1.0, 0.0), (_S3, 0.5), (0.5, _S3), (0.0, 1.0), (-0.5, _S3), (-_S3, 0.5),
            (-1.0, 0.0), (-_S3, -0.5), (-0.5, -_S3), (0.0, -1.0), (0.5, -_S3), (_S3, -0.5)]
YAWS = [k * np.pi / 6 if k <= 6 else (k - 12) * np.pi / 6 for k in range(12)]  # reported to the policy layer only
LEFT, RIGHT, FORWARD = 0, 1, 2


def _walls():
    t = 0.3
    b = [(-10, -10, 10, -10 + t), (-10, 10 - t, 10, 10), (-10, -10, -10 + t, 10), (10 - t, -10, 10, 10)]  # boundary
    # central hall 8.6 m x 8.6 m, two 1.2 m doorways per side
    for y0, y1 in ((4.0, 4.3), (-4.3, -4.0)):
        for x0, x1 in ((-4.3, -2.6), (-1.4, 1.4), (2.6, 4.3)):
            b.append((x0, y0, x1, y1))                      # north / south wall segments
            b.append((y0, x0, y1, x1))                      # west / east wall segments (transposed)
    # partition walls of the ring around the hall, each leaving a gap
    b += [(4.3, 5.5, 7.8, 5.8), (-0.15, 4.3, 0.15, 7.5), (-9.7, 5.0, -6.2, 5.3), (-7.5, -4.3, -7.2, -0.5),
          (-5.5, -9.7, -5.2, -6.0), (1.0, -7.0, 4.5, -6.7), (6.5, -9.7, 6.8, -6.5)]
    # free-standing pillars (the explored area closes around them)
    for cx, cy, r in ((1.6, 1.2, 0.3), (-1.8, 2.0, 0.35), (-2.2, -1.5, 0.3), (1.9, -2.1, 0.4), (7.6, 2.6, 0.45),
                      (-6.0, 8.0, 0.5), (4.0, 8.2, 0.4), (-8.5, -7.5, 0.5), (8.3, -4.5, 0.4)):
        b.append((cx - r, cy - r, cx + r, cy + r))
    b += [(6.0, -1.5, 8.5, -1.0), (6.0, -1.5, 6.5, 0.8)]                                   # L-shaped block (non-convex)
    b += [(-3.6, 6.3, -3.3, 8.6), (-3.6, 8.3, -1.6, 8.6), (-1.9, 6.3, -1.6, 8.6)]          # U-shaped alcove
    return np.array(b, np.float64)


BOXES = _walls()
# tour: hall -> east door -> north-east room -> north room (around the alcove) -> west rooms -> back through the west door ->
# south door -> south-east rooms
WAYPOINTS = [(0.6, 2.0), (3.4, 2.0), (5.4, 2.0), (6.9, 3.9), (8.9, 4.2), (8.9, 7.0), (6.0, 7.3), (2.2, 7.0), (1.0, 8.6), (-0.9, 8.7),
             (-0.9, 5.4), (-2.7, 5.3), (-4.9, 5.6), (-5.3, 4.6), (-8.6, 3.6), (-8.6, 0.5), (-5.6, 0.6), (-5.6, -2.0),
             (-3.4, -2.0), (-3.2, -3.0), (0.0, -3.0), (2.0, -3.3), (2.0, -5.6), (5.4, -5.8), (8.6, -5.9), (8.6, -8.5),
             (8.6, -5.9), (9.2, -5.7), (9.2, -2.2), (5.4, -2.0), (3.4, -2.0), (3.0, -0.6), (0.0, 0.0)]


def _walls_of(boxes) -> np.ndarray:
    """[B,4] f64: the walls a host statement works on -- ``boxes``, or the rooms world's BOXES for None."""
    return BOXES if boxes is None else np.asarray(boxes, np.float64).reshape(-1, 4)


def _column_rays(c, s, fx, W: int):
    """(dx, dy) f64 [W]: the world direction of the ray through each image column u of a camera heading (c, s) = (cos, sin)
    with the focal length ``fx`` pixels -- (1, m) in the camera frame, m = -(u - W//2) / fx (geometry_utils.py:216-236: y_cam =
    -(u - W//2) z / fx), so the ray parameter t == z -- with a component of |d| < 1e-12 replaced by 1e-12."""
    m = -(np.arange(W, dtype=np.float64) - W // 2) / fx
    dx, dy = c - s * m, s + c * m
    return np.where(np.abs(dx) < 1e-12, 1e-12, dx), np.where(np.abs(dy) < 1e-12, 1e-12, dy)


def _slab(b, x, y, dx, dy):
    """The slab test of the rays (dx, dy) [W] out of (x, y) against the boxes ``b`` [B,>=4]: ([W,B] f64 tmin, the ray parameter
    at which the column enters the box, inf where it misses it or starts inside; [W,B] bool: it enters through a y-face, i.e.
    min(ty0, ty1) > min(tx0, tx1) -- ties: an x-face)."""
    dx, dy = dx[:, None], dy[:, None]
    tx0, tx1 = (b[None, :, 0] - x) / dx, (b[None, :, 2] - x) / dx
    ty0, ty1 = (b[None, :, 1] - y) / dy, (b[None, :, 3] - y) / dy
    ex, ey = np.minimum(tx0, tx1), np.minimum(ty0, ty1)
    tmin = np.maximum(ex, ey)
    tmax = np.minimum(np.maximum(tx0, tx1), np.maximum(ty0, ty1))
    return np.where((tmax >= np.maximum(tmin, 0.0)) & (tmin > 0.0), tmin, np.inf), ey > ex


def _within(px, py, boxes, m) -> np.ndarray:
    """bool [...]: does the point (px, py) [...] lie within ``m`` of one of ITS boxes ``boxes`` [...,B,4] (or [B,4]: the same for
    every point) -- the CLOSED test x0 - m <= x <= x1 + m, y0 - m <= y <= y1 + m.  Every comparison with a NaN row is False:
    such a row blocks nothing."""
    px, py = np.asarray(px, np.float64)[..., None], np.asarray(py, np.float64)[..., None]
    return np.any((boxes[..., 0] - m <= px) & (px <= boxes[..., 2] + m) & (boxes[..., 1] - m <= py) & (py <= boxes[..., 3] + m),
                  axis=-1)


def wall_profile(x: float, y: float, k: int, width: int = ROOMS_W, boxes=None, grid=None) -> np.ndarray:
    """(width,) f32 depth along the optical axis of the nearest box face per image column (inf where nothing is hit).
    ``boxes`` [B,4]: the walls of the world (None: BOXES).  ``grid``: a GridPlan whose occupied cells are walls as well (the
    f64 minimum of the two, then rounded; grid worlds section below)."""
    fx = camera_intrinsics(width)[0]
    c, s = HEADINGS[k]
    dx, dy = _column_rays(c, s, fx, width)
    best = _slab(_walls_of(boxes), x, y, dx, dy)[0].min(axis=1, initial=np.inf)            # (initial: a world without boxes)
    if grid is not None:
        best = np.minimum(best, grid_profile_numpy(x, y, c, s, fx, width, grid))
    return best.astype(np.float32)


def _normalise(d, lo, hi):
    return np.clip((d - lo) / (hi - lo), 1e-3, 1.0).astype(np.float32)


def depth_from_profile(wall: np.ndarray, height: int = ROOMS_H) -> np.ndarray:
    fy = camera_intrinsics(len(wall))[1]
    rows = np.arange(height)[:, None] - height // 2
    floor = np.where(rows > 0, CAMERA_HEIGHT * fy / np.maximum(rows, 1e-9), np.inf)
    return _normalise(np.minimum(wall.astype(np.float64)[None, :], floor), MIN_DEPTH, MAX_DEPTH)


def tf_of(x: float, y: float, k: int) -> np.ndarray:
    """xyz_yaw_to_tf_matrix (geometry_utils.py:162-180) with the exact (cos, sin) of the heading table."""
    c, s = HEADINGS[k]
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, CAMERA_HEIGHT], [0.0, 0.0, 0.0, 1.0]])


def _blocked(x: float, y: float, margin: float = 0.3, boxes=None, grid=None) -> bool:
    return bool(_within(x, y, _walls_of(boxes), margin)) or (grid is not None and grid_blocked(grid, x, y, margin))


def integrate(actions):
    """Poses (x, y, k) BEFORE each action: the observation of step i is taken at poses[i]."""
    x = y = 0.0
    k = 0
    poses = []
    for a in actions:
        poses.append((x, y, k))
        if a == LEFT:
            k = (k + 1) % 12
        elif a == RIGHT:
            k = (k - 1) % 12
        else:
            c, s = HEADINGS[k]
            x, y = x + 0.25 * c, y + 0.25 * s
    return poses


def plan_actions(steps: int = ROOMS_STEPS) -> np.ndarray:
    """12 initial left turns (habitat_policies.py:150-153), then a waypoint follower: face the heading of the 30-degree
    set that is best aligned with the next waypoint, step forward.  Deterministic, but only run by the generator --
    replayers integrate the stored action string."""
    for p, q in zip([(0.0, 0.0)] + WAYPOINTS[:-1], WAYPOINTS):  # the hand-placed legs must be collision-free
        for u in np.linspace(0.0, 1.0, int(np.hypot(q[0] - p[0], q[1] - p[1]) / 0.05) + 2):
            assert not _blocked(p[0] + u * (q[0] - p[0]), p[1] + u * (q[1] - p[1]), 0.4), (p, q)
    x = y = 0.0
    k = 0
    acts = []
    wp = 0
    while len(acts) < steps:
        if len(acts) < 12:
            a = LEFT
        else:
            tx, ty = WAYPOINTS[wp % len(WAYPOINTS)]
            if (tx - x) ** 2 + (ty - y) ** 2 < 0.3 ** 2:
                wp += 1
                continue
            best = max(range(12), key=lambda j: (HEADINGS[j][0] * (tx - x) + HEADINGS[j][1] * (ty - y), -j))
            turn = (best - k) % 12
            a = FORWARD if turn == 0 else (LEFT if turn <= 6 else RIGHT)
        acts.append(a)
        if a == LEFT:
            k = (k + 1) % 12
        elif a == RIGHT:
            k = (k - 1) % 12
        else:
            c, s = HEADINGS[k]
            x, y = x + 0.25 * c, y + 0.25 * s
            assert not _blocked(x, y, 0.2), (len(acts), x, y)
    return np.array(acts, np.uint8)


# ---------------------------------------------------------------------------------------------- closed-loop kinematics
# The world's answer to the policy's discrete actions (ids of vlfm_amd.policy_step: TorchActionIDs, habitat_policies.py:53-57),
# for E robots at once: poses stay on the lattice `integrate` walks (30 degree headings of the exact HEADINGS table, 0.25 m
# steps), so a robot that replays the planned tour's actions retraces the planned tour to the bit.
ACTION_STOP, ACTION_FORWARD, ACTION_TURN_LEFT, ACTION_TURN_RIGHT = 0, 1, 2, 3
STEP_MARGIN = 0.2          # the clearance plan_actions asserts for every pose of the tour


def step_poses(xy, k, actions, extra_boxes=None, boxes=None, grids=None):
    """Apply one action per robot: ``xy`` [E,2] f64 positions, ``k`` [E] heading indices (multiples of 30 degrees),
    ``actions`` [E] action ids -> (xy, k, collided [E] bool), new arrays.  A turn changes k by +-1 mod 12; FORWARD adds
    0.25 * HEADINGS[k] (the expression of `integrate`) unless the new position lies within STEP_MARGIN of a box, in which case
    the move is refused (pose unchanged, ``collided`` set: no sliding along walls); STOP changes nothing.  ``extra_boxes``
    [E,K,4] f64: per robot up to K more boxes (x0, y0, x1, y1; a NaN row is "none") that refuse its moves like the walls do:
    the objects of its own environment (world objects section below).  ``boxes`` [E,B,4] f64: per robot the walls of ITS world
    instead of the shared BOXES (a NaN row blocks nothing: the padding of a world table).  ``grids``: per robot a GridPlan or
    None; its occupied cells refuse moves as boxes do (`grid_blocked`: only the cells near the new position are looked at)."""
    xy = np.array(xy, np.float64).reshape(-1, 2)
    k = np.array(k, np.int64).reshape(-1)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    if not (len(xy) == len(k) == len(a)):
        raise ValueError("step_poses: xy, k and actions disagree in length")
    if np.any((a < ACTION_STOP) | (a > ACTION_TURN_RIGHT)):
        raise ValueError("step_poses: unknown action id")
    k = np.where(a == ACTION_TURN_LEFT, (k + 1) % 12, np.where(a == ACTION_TURN_RIGHT, (k - 1) % 12, k))
    heading = np.array(HEADINGS, np.float64)[k]
    new = xy + 0.25 * heading
    m = STEP_MARGIN
    if boxes is None:
        w = BOXES[None]
    else:
        w = np.asarray(boxes, np.float64)
        if w.ndim != 3 or w.shape[0] != len(xy) or w.shape[2] != 4:
            raise ValueError("step_poses: boxes must be [E,B,4]")
    blocked = _within(new[:, 0], new[:, 1], w, m)
    if extra_boxes is not None:
        x = np.asarray(extra_boxes, np.float64)
        if x.ndim != 3 or x.shape[0] != len(xy) or x.shape[2] != 4:
            raise ValueError("step_poses: extra_boxes must be [E,K,4]")
        blocked = blocked | _within(new[:, 0], new[:, 1], x, m)
    if grids is not None:
        if len(grids) != len(xy):
            raise ValueError("step_poses: grids must hold one plan or None per robot")
        for e, g in enumerate(grids):
            if g is not None and not blocked[e]:
                blocked[e] = grid_blocked(g, new[e, 0], new[e, 1], m)
    forward = a == ACTION_FORWARD
    collided = forward & blocked
    xy[forward & ~blocked] = new[forward & ~blocked]
    return xy, k, collided


class BangBangController:
    """A host stand-in for the PointNav controller, in the spirit of tests/golden/policy_script.py::ScriptedWorld.advance: a rule
    over what the policy decided for each environment this step -- its mode, (rho, theta) towards its goal in the robot frame,
    whether it stops -- and whether the world refused the robot's previous FORWARD.

        initialise                 -> TURN_LEFT          (habitat_policies.py:150-153)
        stop, or no (finite) goal  -> STOP
        theta >  15 degrees        -> TURN_LEFT
        theta < -15 degrees        -> TURN_RIGHT
        else                       -> FORWARD

    After a refused FORWARD the robot turns left by 60 degrees (two TURN_LEFT steps) and walks three detour steps FORWARD
    whatever theta says; a detour step that is refused costs one more TURN_LEFT and the detour goes on."""

    TURN_THRESHOLD = float(np.deg2rad(15.0))
    DETOUR_TURNS, DETOUR_STEPS = 2, 3

    def __init__(self) -> None:
        self.turns = self.detour = None

    def reset(self, envs=None) -> None:
        if envs is None or self.turns is None:
            self.turns = self.detour = None
        else:
            self.turns[envs] = 0
            self.detour[envs] = 0

    def act(self, modes, rho_theta, stops, collided) -> np.ndarray:
        E = len(modes)
        if self.turns is None or len(self.turns) != E:
            self.turns, self.detour = np.zeros(E, np.int64), np.zeros(E, np.int64)
        theta = np.asarray(rho_theta, np.float64).reshape(E, 2)[:, 1]
        out = np.empty(E, np.int64)
        for e in range(E):
            if collided[e]:
                if self.detour[e] > 0:
                    self.turns[e] = 1
                else:
                    self.turns[e], self.detour[e] = self.DETOUR_TURNS, self.DETOUR_STEPS
            if modes[e] == "initialize":
                out[e] = ACTION_TURN_LEFT
            elif stops[e] or not np.isfinite(theta[e]):
                out[e] = ACTION_STOP
            elif self.turns[e] > 0:
                self.turns[e] -= 1
                out[e] = ACTION_TURN_LEFT
            elif self.detour[e] > 0:
                self.detour[e] -= 1
                out[e] = ACTION_FORWARD
            elif theta[e] > self.TURN_THRESHOLD:
                out[e] = ACTION_TURN_LEFT
            elif theta[e] < -self.TURN_THRESHOLD:
                out[e] = ACTION_TURN_RIGHT
            else:
                out[e] = ACTION_FORWARD
        return out


class ReplayController:
    """Plays back a stored action table ``actions`` [L,E] (action ids), one row per step, whatever the policy decided;
    after the last row it starts over, as does ``reset()``."""

    def __init__(self, actions) -> None:
        self.actions = np.asarray(actions, np.int64)
        if self.actions.ndim != 2 or not len(self.actions):
            raise ValueError("ReplayController: actions must be a non-empty [L,E] table")
        self.i = 0

    def reset(self, envs=None) -> None:
        if envs is None:
            self.i = 0

    def act(self, modes, rho_theta, stops, collided) -> np.ndarray:
        row = self.actions[self.i % len(self.actions)]
        self.i += 1
        return row.copy()


# ---------------------------------------------------------------------------------------------- world objects
# Target and distractor objects standing IN the rooms world: an object is an axis-aligned box with a vertical extent,
# (x0, y0, x1, y1, z0, z1) in metres, plus a class name.  The ray caster renders them with occlusion (csrc/world_render.hip:
# vlfm_worlds_raycast with objects; `render_objects_numpy` below is the host statement of the same arithmetic), `step_poses` refuses
# moves into them, and the batched harness reports as detections what is actually in view (BatchedEpisodes(world_objects=...)).
WORLD_MAX_OBJECTS = 8
# free-standing centres, hand-placed over the hall and the ring rooms: `object_layout` asserts that each keeps 0.65 m to every
# wall (the largest footprint half-extent, 0.5 m, plus most of a robot's STEP_MARGIN)
OBJECT_SPOTS = [(0.0, 2.6), (3.2, 0.4), (-0.4, -1.8), (-3.2, 0.2), (3.2, -3.2), (-3.3, 3.2),            # hall
                (5.6, 3.0), (8.6, 0.6), (8.8, 8.6), (2.2, 5.6), (1.8, 8.8), (-5.2, 6.6), (-8.6, 8.6), (-8.6, 2.0),   # ring
                (-5.8, -1.2), (-8.6, -3.0), (-3.0, -6.0), (0.0, -8.6), (4.0, -5.4), (8.6, -8.0), (5.2, -8.6), (-8.0, -5.6)]
# class (the harness's TARGETS, in its order) -> (half-extent x, half-extent y, z0, z1).  All stand on the floor with a top
# between 0.7 and 1.5 m: they cut the obstacle map's 0.61-0.88 m band, so what refuses a move is also an obstacle on the map.
OBJECT_SIZES = {"chair": (0.25, 0.25, 0.0, 0.9), "bed": (0.5, 0.45, 0.0, 0.7), "potted plant": (0.2, 0.2, 0.0, 1.3),
                "toilet": (0.2, 0.3, 0.0, 0.8), "tv": (0.45, 0.1, 0.0, 1.2), "couch": (0.5, 0.35, 0.0, 0.85)}
OBJECT_START_CLEARANCE = 1.5   # no object on a spot nearer than this to the robot: no episode starts solved


def _mix32(a: int, b: int, salt: int) -> int:
    """The package's 32-bit mixer (a murmur3-style finaliser; harness.ScriptedSightings scripts its episodes with it): a pure
    function, no global RNG."""
    h = (a * 2654435761 + b * 40503 + salt * 97 + 0x9E3779B9) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def object_box(cls: str, cx: float, cy: float):
    """The box6 of an object of class ``cls`` centred on (cx, cy)."""
    hx, hy, z0, z1 = OBJECT_SIZES[cls]
    return (cx - hx, cy - hy, cx + hx, cy + hy, z0, z1)


def object_layout(env_id: int, episode: int, robot_xy):
    """[(class, box6)] of environment ``env_id``'s episode number ``episode`` for a robot that starts it at ``robot_xy``: the
    environment's target class (the harness's rule: class ``env_id mod 6``) on one spot, one distractor of another class on
    another; both spots picked by the hash of (env_id, episode) among the spots farther than OBJECT_START_CLEARANCE from the
    robot.  Deterministic."""
    assert len(OBJECT_SPOTS) >= 12
    for (sx, sy) in OBJECT_SPOTS:                       # hand-placed, like the legs of the tour
        assert not _blocked(sx, sy, 0.65), (sx, sy)
    classes = list(OBJECT_SIZES)
    target = classes[env_id % len(classes)]
    rx, ry = float(robot_xy[0]), float(robot_xy[1])
    free = [p for p in OBJECT_SPOTS if np.hypot(p[0] - rx, p[1] - ry) > OBJECT_START_CLEARANCE]
    a = _mix32(env_id, episode, 21) % len(free)
    b = (a + 1 + _mix32(env_id, episode, 22) % (len(free) - 1)) % len(free)
    other = [c for c in classes if c != target]
    distractor = other[_mix32(env_id, episode, 23) % len(other)]
    return [(target, object_box(target, *free[a])), (distractor, object_box(distractor, *free[b]))]


def rect_distance(xy, box) -> float:
    """Distance from the point ``xy`` to the rectangle box[:4] = (x0, y0, x1, y1); 0 inside."""
    dx = max(box[0] - xy[0], 0.0, xy[0] - box[2])
    dy = max(box[1] - xy[1], 0.0, xy[1] - box[3])
    return float(np.hypot(dx, dy))


def render_objects_numpy(x, y, c, s, height, fx, lo, hi, H, W, boxes6, boxes=None, grid=None):
    """(depth f32 [H,W], ids u8 [H,W]) seen by ONE camera at (x, y), heading (c, s) = (cos, sin), ``height`` above the floor,
    focal length ``fx`` pixels, range [lo, hi]: the walls and the floor of `wall_profile` / `depth_from_profile`, and the
    objects ``boxes6`` [K,6] in front of them.  Per column u an object is hit at t = f64(f32(tmin)) of the walls' slab test
    and covers the rows rr = r - H//2 with ceil((height - z1) fx / t) <= rr <= floor((height - z0) fx / t); the pixel's depth
    is the f32 minimum of the normalised wall, floor and covering objects, its id is k + 1 of the nearest covering object
    (lowest k among equals) where that is STRICTLY nearer than wall and floor, else 0.  ``boxes`` [B,4]: the walls (None: BOXES).
    ``grid``: a GridPlan whose occupied cells are walls as well (the f64 minimum of the two, then rounded to f32).
    Whole-array f64 NumPy."""
    boxes6 = np.asarray(boxes6, np.float64).reshape(-1, 6)
    dx, dy = _column_rays(c, s, fx, W)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        wall = _slab(_walls_of(boxes), x, y, dx, dy)[0].min(axis=1, initial=np.inf)
        if grid is not None:
            wall = np.minimum(wall, grid_profile_numpy(x, y, c, s, fx, W, grid))
        wall = wall.astype(np.float32).astype(np.float64)
        rr = (np.arange(H) - H // 2)[:, None]
        floor = np.where(rr > 0, (height * fx) / np.maximum(rr, 1), np.inf)
        bg = np.minimum(_normalise(wall, lo, hi)[None, :], _normalise(floor, lo, hi))              # [H,W] f32
        if not len(boxes6):
            return bg, np.zeros((H, W), np.uint8)
        t = _slab(boxes6, x, y, dx, dy)[0].astype(np.float32).astype(np.float64)                    # [W,K]
        rlo = np.ceil(((height - boxes6[None, :, 5]) * fx) / t)
        rhi = np.floor(((height - boxes6[None, :, 4]) * fx) / t)
        cover = np.isfinite(t)[None] & (rlo[None] <= rr[:, :, None]) & (rr[:, :, None] <= rhi[None])   # [H,W,K]
        layers = np.where(cover, _normalise(t, lo, hi)[None], np.float32(np.inf))
    best, arg = layers.min(axis=2), layers.argmin(axis=2)           # (argmin: the first, i.e. lowest, k among equals)
    return np.minimum(bg, best), np.where(best < bg, arg + 1, 0).astype(np.uint8)


def object_stats_numpy(ids, K: int = WORLD_MAX_OBJECTS) -> np.ndarray:
    """int32 [K,5] = (pixel count, first column, last column, first row, last row) of each object k in the id plane ``ids``
    (object k has id k + 1); (0, W, -1, H, -1) for an object with no pixel."""
    H, W = ids.shape
    out = np.empty((K, 5), np.int32)
    for k in range(K):
        r, c = np.nonzero(ids == k + 1)
        out[k] = (len(r), c.min(), c.max(), r.min(), r.max()) if len(r) else (0, W, -1, H, -1)
    return out


# ---------------------------------------------------------------------------------------------- world colours
# What the camera's RGB frame shows of the same world (csrc/world_render.hip: vlfm_worlds_raycast with d_rgb; `render_rgb_numpy` is the
# host statement).  Colours are packed 0x00RRGGBB integers and reach the kernel as arguments: it holds no colour constants.
WORLD_PALETTE = np.array([0xC8B7A6, 0xB5C4B1, 0xA9B8C8, 0xD6C58F, 0xC49A8A, 0x9FB7AD, 0xBFAFCB, 0xD9D4C7,      # 8 wall colours
                          0x8A6F4E, 0x6F5B41,                                                                  # 2 floor colours
                          0x87B5E8,                                                                            # sky
                          0], np.int32)                                                                        # spare: nothing reads it
OBJECT_COLOURS = {"chair": 0xB03A2E, "bed": 0x2E6FB0, "potted plant": 0x2F8F3A, "toilet": 0xE8E8F0, "tv": 0x202428,
                  "couch": 0x8E44AD}
assert set(OBJECT_COLOURS) == set(OBJECT_SIZES)
SKIRTING_HEIGHT = 0.12      # metres: below it a wall is drawn at half brightness


def _channels(packed) -> np.ndarray:
    """int64 [..., 3] = (R, G, B) of packed 0x00RRGGBB colours."""
    p = np.asarray(packed, np.int64)
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], axis=-1)


def render_rgb_numpy(x, y, c, s, height, fx, lo, hi, H, W, boxes6, colours, boxes=None, palette=WORLD_PALETTE):
    """(depth f32 [H,W], ids u8 [H,W], rgb u8 [H,W,3]) seen by ONE camera: the depth and id planes of `render_objects_numpy`
    for the same arguments, and the colour of every pixel.  ``colours`` [K] int: packed 0x00RRGGBB, one per object slot of
    ``boxes6``; ``palette`` int [12]: 8 wall colours, 2 floor colours, sky, one spare entry.

    Per column u (dx, dy clamped as in `wall_profile`): the wall is the box b_w with the least f64 tmin among the hit boxes
    (lowest index among equals) at t_w = f64(f32(tmin)); it shows a y-face iff min(ty0, ty1) > min(tx0, tx1) there (ties: an
    x-face); q = x + dx * t_w on a y-face, y + dy * t_w on an x-face, panel = int64(floor(q * 2.0)) & 1; the skirting starts at
    r_sk = ceil(((height - 0.12) * fx) / t_w), clamped to the int16 range (a NaN: never).  Every object slot has a face bit by
    the same rule from its own footprint.  Per pixel, rr = r - H//2, floor_d as in `render_objects_numpy`, the first that holds:
      object   ids > 0: colours[ids - 1]; on a y-face ch -= ch >> 2
      floor    floor_d < t_w: palette[8 + ((int64(floor(px * 2.0)) + int64(floor(py * 2.0))) & 1)], px = x + dx * floor_d,
               py = y + dy * floor_d
      wall     t_w finite: palette[_mix32(b_w, 0, 31) % 8] (b_w counts inside the camera's own world); then, in this order,
               an odd panel: ch -= ch >> 3; a y-face: ch -= ch >> 2; rr >= r_sk: ch >>= 1
      void     palette[10], as it is
    and on the first three the depth cue g = int(depth * 128.0f) (f32, truncated: 0..128), ch = (ch * (256 - g)) >> 8.
    Every multiply and add is rounded once; everything after the geometry is integer arithmetic.  The colour plane never shows
    an object the id plane does not: both clamp beyond ``hi``, where an object is not STRICTLY nearer than its background.
    Whole-array f64 NumPy."""
    depth, ids = render_objects_numpy(x, y, c, s, height, fx, lo, hi, H, W, boxes6, boxes)
    boxes6 = np.asarray(boxes6, np.float64).reshape(-1, 6)
    colours = np.asarray(colours, np.int64).reshape(-1)
    palette = np.asarray(palette, np.int64).reshape(-1)
    if len(colours) != len(boxes6) or len(palette) != 12:
        raise ValueError("render_rgb_numpy: one colour per object slot and a palette of 12")
    g = _rgb_geometry(x, y, c, s, height, fx, H, W, boxes6, boxes)
    rr = (np.arange(H) - H // 2)[:, None]
    wall_base = palette[np.array([_mix32(int(b), 0, 31) % 8 for b in g["b_w"]], np.int64)]
    ch = _channels(wall_base)[None].repeat(H, axis=0)                                              # [H,W,3]: the wall
    ch = np.where(g["panel"][None, :, None] == 1, ch - (ch >> 3), ch)
    ch = np.where(g["wall_y"][None, :, None], ch - (ch >> 2), ch)
    ch = np.where((rr >= g["r_sk"][None, :])[:, :, None], ch >> 1, ch)
    ch = np.where(g["on_floor"][:, :, None], _channels(palette[8 + g["check"]]), ch)
    if len(boxes6):
        k = np.maximum(ids.astype(np.int64) - 1, 0)
        oc = _channels(colours[k])
        oc = np.where(g["obj_y"][np.arange(W)[None, :], k][:, :, None], oc - (oc >> 2), oc)
        ch = np.where((ids > 0)[:, :, None], oc, ch)
    cue = (depth * np.float32(128.0)).astype(np.int64)[:, :, None]
    ch = (ch * (256 - cue)) >> 8
    void = (ids == 0) & ~g["on_floor"] & ~np.isfinite(g["t_w"])[None, :]
    ch = np.where(void[:, :, None], _channels(palette[10])[None, None, :], ch)
    return depth, ids, ch.astype(np.uint8)


def _rgb_geometry(x, y, c, s, height, fx, H, W, boxes6, boxes=None):
    """The geometry `render_rgb_numpy` colours by: per column b_w, t_w, wall_y (a y-face), panel, r_sk and obj_y [W,K]; per
    pixel on_floor (floor_d < t_w) and check (the floor's checker bit)."""
    walls = _walls_of(boxes)
    dx, dy = _column_rays(c, s, fx, W)

    def odd(v):        # int64(floor(v)) & 1, 0 where v is not finite
        return np.floor(np.where(np.isfinite(v), v, 0.0)).astype(np.int64) & 1

    cols = np.arange(W)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if len(walls):
            t, yface = _slab(walls, x, y, dx, dy)
            b_w = t.argmin(axis=1)                                      # (argmin: the first, i.e. lowest, index among equals)
            t_w = t[cols, b_w].astype(np.float32).astype(np.float64)
            wall_y = yface[cols, b_w]
        else:
            b_w, t_w, wall_y = np.zeros(W, np.int64), np.full(W, np.inf), np.zeros(W, bool)
        q = np.where(wall_y, x + dx * t_w, y + dy * t_w)
        r_sk = np.ceil(((height - SKIRTING_HEIGHT) * fx) / t_w)
        r_sk = np.where(np.isnan(r_sk), 32767.0, np.clip(r_sk, -32768.0, 32767.0))
        rr = (np.arange(H) - H // 2)[:, None]
        floor_d = np.where(rr > 0, (height * fx) / np.maximum(rr, 1), np.inf)                       # [H,1]
        on_floor = floor_d < t_w[None, :]                                                            # [H,W]
        fd = np.where(on_floor, floor_d, 0.0)
        px, py = x + dx[None, :] * fd, y + dy[None, :] * fd
        check = (odd(px * 2.0) + odd(py * 2.0)) & 1
        obj_y = _slab(np.asarray(boxes6, np.float64).reshape(-1, 6), x, y, dx, dy)[1]               # [W,K]
    return {"b_w": b_w, "t_w": t_w, "wall_y": wall_y, "panel": odd(q * 2.0), "r_sk": r_sk, "on_floor": on_floor,
            "check": check, "obj_y": obj_y}


def rgb_kinds_numpy(x, y, c, s, height, fx, lo, hi, H, W, boxes6, boxes=None):
    """What `render_rgb_numpy` shows where, for tests and probes: u8 [H,W] kind (0 void, 1 wall, 2 floor, 3 object) and bool
    [H,W] planes "skirting" (wall pixels at half brightness), "odd panel" and "y-face" (of the wall or object shown; False on
    floor and void)."""
    ids = render_objects_numpy(x, y, c, s, height, fx, lo, hi, H, W, boxes6, boxes)[1]
    g = _rgb_geometry(x, y, c, s, height, fx, H, W, boxes6, boxes)
    obj = ids > 0
    floor = ~obj & g["on_floor"]
    wall = ~obj & ~floor & np.isfinite(g["t_w"])[None, :]
    kind = np.where(obj, 3, np.where(floor, 2, np.where(wall, 1, 0))).astype(np.uint8)
    rr = (np.arange(H) - H // 2)[:, None]
    yface = wall & g["wall_y"][None, :]
    if obj.any():
        yface |= obj & g["obj_y"][np.arange(W)[None, :], np.maximum(ids.astype(np.int64) - 1, 0)]
    return kind, wall & (rr >= g["r_sk"][None, :]), wall & (g["panel"][None, :] == 1), yface


# ---------------------------------------------------------------------------------------------- ObjectNav metrics
# The length of the shortest collision-free path to an episode's goal, which SPL, SoftSPL and Habitat's distance_to_goal are
# made of (the reference reads them off Habitat's navmesh).  This section is the HOST STATEMENT of the rule; the device
# (csrc/geodesic.hip: vlfm_geodesic_fields / vlfm_geodesic_query) matches it bit for bit.  Everything is f64 with one rounding
# per operation (+ - * / sqrt, comparisons), no fused multiply-add, the expressions exactly as written here.
#
#   obstacles  the walls BOXES and the environment's valid object footprints, each inflated by STEP_MARGIN with the expressions
#              of `step_poses` (x0 - m, y0 - m, x1 + m, y1 + m): the doubles are the kinematics' own.  For the geodesic every
#              inflated rectangle is an OPEN set: a path may run along its boundary.
#   blocked    the segment p -> q is blocked by a rectangle iff some t in (0, 1) puts p + t (q - p) strictly inside it.  Per
#              axis, with d = q - p:  d == 0: the interval is everything if lo < p < hi, else empty;  otherwise
#              t0 = (lo - p) / d, t1 = (hi - p) / d and the interval is (min(t0, t1), max(t0, t1)).  Blocked iff
#              max(enter_x, enter_y, 0) < min(exit_x, exit_y, 1).  A segment along an edge or through a corner is free.  The
#              test is evaluated FROM p TO q as given (the roundings of the two directions may differ):
#              source -> corner, corner of lower index -> corner of higher index (one verdict per pair), query point -> source
#              or corner.
#   nodes      the corners (x0,y0) (x1,y0) (x1,y1) (x0,y1) of every inflated rectangle, in rectangle order, without those that
#              lie strictly inside some rectangle.  Edge weight w(a, b) = sqrt(dx*dx + dy*dy) (not hypot).
#   sources    Habitat's "view points": `goal_viewpoints`.
#   field      dist[c] = the least value with dist[c] <= w(s, c) for every source s that sees c and
#              dist[c] <= fl(dist[u] + w(u, c)) for every corner u that sees c, attained by one of them (inf: unreachable).
#              Adding a non-negative weight never decreases a value, so this least fixed point is unique, a heap Dijkstra with
#              the same additions returns it, and so does relaxing until nothing changes (the kernel).
#   query      d(p) = min(min over the sources p sees of w(p, s), min over the corners p sees of fl(w(p, c) + dist[c]));
#              inf when nothing is reachable -- every segment out of a p strictly inside a rectangle is blocked.
#
# Known looseness: two inflated rectangles that exactly abut leave a slit of zero width, which the open-set rule lets a path
# through.  That can only SHORTEN l, so SPL stays at or below its true value.  Among the built-in layouts it concerns four
# (class, spot) pairs -- a bed or a couch against the east wall or a pillar (tests/test_geodesic_cpu.py counts them).
GEODESIC_MAX_SOURCES = 256


def inflated_rects(objects=None, margin: float = STEP_MARGIN, boxes=None) -> np.ndarray:
    """[R,4] f64 (x0 - m, y0 - m, x1 + m, y1 + m): the walls ``boxes`` (default BOXES), then the objects in slot order.
    ``objects``: [K,8] ray-caster records (a slot counts iff its ``valid`` field, column 6, is non-zero) or [K,4] / [K,6]
    boxes (all count)."""
    b = _walls_of(boxes)
    if objects is not None and len(objects):
        o = np.asarray(objects, np.float64)
        o = o.reshape(-1, o.shape[-1])
        if o.shape[1] not in (4, 6, 8):
            raise ValueError("inflated_rects: objects must be [K,8] records or [K,4] / [K,6] boxes")
        if o.shape[1] == 8:
            o = o[o[:, 6] != 0.0]
        b = np.concatenate([b, o[:, :4]])
    m = float(margin)
    return np.stack([b[:, 0] - m, b[:, 1] - m, b[:, 2] + m, b[:, 3] + m], axis=1)


def segments_blocked_numpy(p, q, rects) -> np.ndarray:
    """bool [len(p), len(q)]: is the segment p[i] -> q[j] blocked by one of the OPEN rectangles ``rects`` [R,4] (the rule
    above, evaluated from p to q)."""
    p = np.asarray(p, np.float64).reshape(-1, 1, 1, 2)
    q = np.asarray(q, np.float64).reshape(1, -1, 1, 2)
    r = np.asarray(rects, np.float64).reshape(1, 1, -1, 4)
    out = np.zeros((p.shape[0], q.shape[1]), bool)
    rows = max(1, (1 << 21) // max(1, q.shape[1] * r.shape[2]))         # [rows, len(q), R] temporaries of 16 MB at the most
    for i in range(0, p.shape[0], rows):
        enter, leave = 0.0, 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            for ax in (0, 1):
                pa, lo, hi = p[i:i + rows, ..., ax], r[..., ax], r[..., ax + 2]
                d = q[..., ax] - pa
                t0, t1 = (lo - pa) / d, (hi - pa) / d
                inside = (lo < pa) & (pa < hi)
                a = np.where(d == 0.0, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
                b = np.where(d == 0.0, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
                enter, leave = np.maximum(enter, a), np.minimum(leave, b)
        out[i:i + rows] = np.any(enter < leave, axis=2)
    return out


def _edge_weights(a, b) -> np.ndarray:
    a, b = np.asarray(a, np.float64).reshape(-1, 1, 2), np.asarray(b, np.float64).reshape(1, -1, 2)
    dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
    return np.sqrt(dx * dx + dy * dy)


def goal_viewpoints(target_box, rects, success_distance: float, max_points: int = GEODESIC_MAX_SOURCES, boxes=None,
                    grid=None) -> np.ndarray:
    """[S,2] f64, the sources of a geodesic field: the points (0.25 i, 0.25 j), i and j integers, with
    dx*dx + dy*dy <= r*r for `rect_distance`'s clamped offsets (dx, dy) to ``target_box[:4]`` and r = ``success_distance``,
    that `step_poses`' CLOSED test against the inflated rectangles ``rects`` does not block -- where a robot can stand and
    have succeeded.  Ordered by (i, j).  More than ``max_points`` of them: ValueError.  ``boxes`` [B,4] (NOT inflated) and
    ``grid`` (a GridPlan): walls that block as well, by the same closed test with STEP_MARGIN (`_within`, `grid_blocked`)."""
    x0, y0, x1, y1 = (float(v) for v in np.asarray(target_box, np.float64).reshape(-1)[:4])
    r = float(success_distance)
    i = np.arange(int(np.floor((x0 - r) / 0.25)), int(np.ceil((x1 + r) / 0.25)) + 1, dtype=np.float64)
    j = np.arange(int(np.floor((y0 - r) / 0.25)), int(np.ceil((y1 + r) / 0.25)) + 1, dtype=np.float64)
    px, py = np.meshgrid(0.25 * i, 0.25 * j, indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    dx = np.maximum(np.maximum(x0 - px, 0.0), px - x1)
    dy = np.maximum(np.maximum(y0 - py, 0.0), py - y1)
    keep = dx * dx + dy * dy <= r * r
    keep &= ~_within(px, py, np.asarray(rects, np.float64).reshape(-1, 4), 0.0)     # (inflated already: e - 0.0 is e)
    if boxes is not None:
        keep &= ~_within(px, py, np.asarray(boxes, np.float64).reshape(-1, 4), STEP_MARGIN)
    if grid is not None:
        for i in np.flatnonzero(keep):
            keep[i] = not grid_blocked(grid, px[i], py[i], STEP_MARGIN)
    pts = np.stack([px[keep], py[keep]], axis=1)
    if len(pts) > max_points:
        raise ValueError(f"goal_viewpoints: {len(pts)} view points, at most {max_points} fit a geodesic field")
    return pts


def geodesic_nodes_numpy(rects) -> np.ndarray:
    """[N,2] the corner nodes of the rectangles ``rects`` [R,4]: (x0,y0) (x1,y0) (x1,y1) (x0,y1) per rectangle, in order,
    without the corners strictly inside some rectangle."""
    r = np.asarray(rects, np.float64).reshape(-1, 4)
    c = r[:, [0, 1, 2, 1, 2, 3, 0, 3]].reshape(-1, 2)
    inside = np.any((r[None, :, 0] < c[:, None, 0]) & (c[:, None, 0] < r[None, :, 2]) &
                    (r[None, :, 1] < c[:, None, 1]) & (c[:, None, 1] < r[None, :, 3]), axis=1)
    return c[~inside]


def geodesic_field_numpy(rects, sources):
    """(nodes [N,2], dist [N]) f64: the geodesic field of the OPEN rectangles ``rects`` [R,4] around the ``sources`` [S,2]
    (the rule above), by a heap Dijkstra from the goal outwards."""
    import heapq

    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    sources = np.asarray(sources, np.float64).reshape(-1, 2)
    nodes = geodesic_nodes_numpy(rects)
    N = len(nodes)
    dist = np.full(N, np.inf)
    if N == 0:
        return nodes, dist
    if len(sources):
        w = np.where(segments_blocked_numpy(sources, nodes, rects), np.inf, _edge_weights(sources, nodes))
        dist = w.min(axis=0)
    up = np.triu(segments_blocked_numpy(nodes, nodes, rects), 1)         # lower index -> higher index, one verdict per pair
    sees = ~(up | up.T)
    np.fill_diagonal(sees, False)
    w = _edge_weights(nodes, nodes)
    heap = [(float(d), c) for c, d in enumerate(dist) if np.isfinite(d)]
    heapq.heapify(heap)
    done = np.zeros(N, bool)
    while heap:
        d, u = heapq.heappop(heap)
        if done[u] or d > dist[u]:
            continue
        done[u] = True
        for c in np.flatnonzero(sees[u] & ~done):
            cand = d + float(w[u, c])
            if cand < dist[c]:
                dist[c] = cand
                heapq.heappush(heap, (cand, int(c)))
    return nodes, dist


def geodesic_query_numpy(rects, sources, nodes, dist, points) -> np.ndarray:
    """[m] f64: d(p) of the rule above for the ``points`` [m,2] in the field (``nodes``, ``dist``) of ``rects``, ``sources``."""
    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    sources = np.asarray(sources, np.float64).reshape(-1, 2)
    nodes, dist = np.asarray(nodes, np.float64).reshape(-1, 2), np.asarray(dist, np.float64).reshape(-1)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    out = np.full(len(points), np.inf)
    if len(sources) and len(points):
        out = np.where(segments_blocked_numpy(points, sources, rects), np.inf, _edge_weights(points, sources)).min(axis=1)
    if len(nodes) and len(points):
        via = np.where(segments_blocked_numpy(points, nodes, rects), np.inf, _edge_weights(points, nodes) + dist[None, :])
        out = np.minimum(out, via.min(axis=1))
    return out


def spl(success, l: float, p: float) -> float:
    """Habitat's SPL of one episode: S * l / max(p, l) for the geodesic start-to-goal distance ``l`` and the path length
    ``p``; the ratio is 1 when l == 0.  An episode without a finite ``l`` (no target, or no way to it) contributes 0."""
    if not success or not np.isfinite(l):
        return 0.0
    return 1.0 if l == 0.0 else float(l / max(p, l))


def soft_spl(d_end: float, l: float, p: float) -> float:
    """Habitat's SoftSPL of one episode: max(0, 1 - d_end / l) * l / max(p, l) with the geodesic distance ``d_end`` left at
    the end; with l == 0 the progress term is 1 iff d_end == 0.  0 without a finite ``l`` or ``d_end``."""
    if not np.isfinite(l) or not np.isfinite(d_end):
        return 0.0
    if l == 0.0:
        return 1.0 if d_end == 0.0 else 0.0
    return float(max(0.0, 1.0 - d_end / l) * (l / max(p, l)))


# ---------------------------------------------------------------------------------------------- procedural worlds
# A floor plan per (seed, env_id, episode) instead of the one hand-built BOXES: rooms on a jittered grid, doorways, pillars, and
# the spots objects may stand on.  Everything is drawn with `_mix32` (no global RNG) and laid out in INTEGER units of 0.05 m; a
# coordinate becomes a float by one division by 20, so a world is the same bytes on every platform.
#
#   plan     the square [-10, 10] m with a 0.3 m boundary wall, cut into nx x ny cells, nx, ny in {2, 3, 4}; the partition lines
#            sit at the even split, jittered in 0.1 m steps by up to +-1 m (+-0.7 m with four cells: every wall keeps room for a
#            doorway 1 m from both of its ends)
#   walls    between two adjacent cells a 0.3 m wall.  The edges of a spanning tree of the cell graph (Kruskal over hashed
#            weights) carry a 1.2 m doorway at least 1 m from either end; every other edge is solid (1/4), has a doorway (1/2) or
#            is absent (1/4).  A piece runs from partition line to partition line -- half a wall thickness past the cell at both
#            ends -- so pieces OVERLAP at junctions instead of abutting
#   pillars  a cell at least 4.5 m wide both ways gets, with probability 1/2, a free-standing square pillar of half extent
#            0.3-0.5 m within 0.5 m of its centre, while the box budget WORLD_MAX_BOXES lasts
#   spots    the quarter points of every cell, snapped to 0.25 m, that keep 0.65 m to every box and 1.6 m to every doorway centre
#            (no object can close a door) and on which no object class's inflated footprint exactly abuts an inflated wall (the
#            zero-width slit of the geodesic rule above does not arise)
#   start    a hashed spot, a hashed heading
# `tests/test_procedural_worlds_cpu.py` checks what the harness relies on: the box budget, the start's clearance, at least 12
# spots, every spot reachable from the start, no abutting inflated rectangles.
WORLD_MAX_BOXES = 64
_WORLD_HALF, _WORLD_WALL, _WORLD_DOOR, _WORLD_DOOR_END = 200, 6, 24, 20       # units of 0.05 m: 10 m, 0.3 m, 1.2 m, 1 m


class World(NamedTuple):
    boxes: np.ndarray        # [B,4] f64 walls and pillars (x0, y0, x1, y1), B <= WORLD_MAX_BOXES
    start_xy: np.ndarray     # [2] f64
    start_k: int             # heading index into HEADINGS
    spots: np.ndarray        # [S,2] f64 object centres
    doors: np.ndarray        # [D,2] f64 doorway centres
    grid: object = None      # a GridPlan whose occupied cells are walls as well (grid worlds section below), or None


def rects_abut(a, b) -> np.ndarray:
    """bool [len(a), len(b)]: do the rectangles a[i] and b[j] (x0, y0, x1, y1) exactly abut -- one ends on an axis where the
    other begins (equal doubles) while they overlap by a positive length on the other axis."""
    a, b = np.asarray(a, np.float64).reshape(-1, 1, 4), np.asarray(b, np.float64).reshape(1, -1, 4)
    ox = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
    oy = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
    return (((a[..., 2] == b[..., 0]) | (a[..., 0] == b[..., 2])) & (oy > 0)) | \
           (((a[..., 3] == b[..., 1]) | (a[..., 1] == b[..., 3])) & (ox > 0))


class ProceduralWorlds:
    """``worlds.world(env_id, episode)``: the floor plan of that environment's episode, a pure function of (seed, env_id, episode)
    (the rule above).  ``worlds.layout(env_id, episode, robot_xy)``: `object_layout`'s rule over the world's own spots."""

    def __init__(self, seed: int = 0) -> None:
        self.seed = int(seed)
        self._made = {}          # (env_id, episode) -> World: the harness asks for an episode's world more than once

    def world(self, env_id: int, episode: int) -> World:
        key = (int(env_id), int(episode))
        if key not in self._made:
            if len(self._made) >= 1024:
                self._made.clear()
            w = self._generate(*key)
            for a in (w.boxes, w.start_xy, w.spots, w.doors):
                a.setflags(write=False)
            self._made[key] = w
        return self._made[key]

    def _generate(self, env_id: int, episode: int) -> World:
        base = _mix32(_mix32(self.seed, int(env_id), 101), int(episode), 102)
        draws = iter(range(1 << 30))
        rnd = lambda n: _mix32(base, next(draws), 103) % n      # noqa: E731  the next draw, uniform over range(n)
        half, t, h = _WORLD_HALF, _WORLD_WALL, _WORLD_WALL // 2

        def lines(n):        # centre lines of the n + 1 walls across one axis, boundary included
            jitter = 10 if n < 4 else 7                         # in steps of 0.1 m = 2 units
            inner = [-half + 2 * ((half * i) // n) + 2 * (rnd(2 * jitter + 1) - jitter) for i in range(1, n)]
            return [-half + h] + inner + [half - h]

        nx, ny = 2 + rnd(3), 2 + rnd(3)
        X, Y = lines(nx), lines(ny)
        boxes = [(-half, -half, half, -half + t), (-half, half - t, half, half), (-half, -half, -half + t, half),
                 (half - t, -half, half, half)]
        # the cell graph: edge (a, b, vertical?) between cell a = (i, j) and its east / north neighbour
        edges = [((i, j), (i + 1, j), True) for j in range(ny) for i in range(nx - 1)] + \
                [((i, j), (i, j + 1), False) for j in range(ny - 1) for i in range(nx)]
        weight = [rnd(1 << 20) for _ in edges]
        kind = [rnd(4) for _ in edges]                           # off the tree: 0 solid, 1 / 2 doorway, 3 absent
        root = {(i, j): (i, j) for i in range(nx) for j in range(ny)}

        def find(c):
            while root[c] != c:
                c = root[c]
            return c

        for n in sorted(range(len(edges)), key=lambda n: (weight[n], n)):
            ra, rb = find(edges[n][0]), find(edges[n][1])
            if ra != rb:
                root[ra] = rb
                kind[n] = 1
        doors = []
        for n, ((i, j), _, vertical) in enumerate(edges):
            if kind[n] == 3:
                continue
            line = X[i + 1] if vertical else Y[j + 1]
            p0, p1 = (Y[j], Y[j + 1]) if vertical else (X[i], X[i + 1])   # the piece: partition line to partition line
            room = (p1 - h) - (p0 + h) - _WORLD_DOOR - 2 * _WORLD_DOOR_END
            assert room >= 0
            off = 2 * rnd(room // 2 + 1)                         # (drawn for a solid wall too: one draw per edge)
            pieces = [(p0, p1)]
            if kind[n] != 0:
                d0 = p0 + h + _WORLD_DOOR_END + off
                pieces = [(p0, d0), (d0 + _WORLD_DOOR, p1)]
                doors.append((line, d0 + _WORLD_DOOR // 2) if vertical else (d0 + _WORLD_DOOR // 2, line))
            for (a, b) in pieces:
                boxes.append((line - h, a, line + h, b) if vertical else (a, line - h, b, line + h))
        for j in range(ny):
            for i in range(nx):
                want, r, ox, oy = rnd(2), 6 + rnd(5), rnd(21) - 10, rnd(21) - 10
                x0, x1, y0, y1 = X[i] + h, X[i + 1] - h, Y[j] + h, Y[j + 1] - h
                if want and min(x1 - x0, y1 - y0) >= 90 and len(boxes) < WORLD_MAX_BOXES:
                    cx, cy = (x0 + x1) // 2 + ox, (y0 + y1) // 2 + oy
                    boxes.append((cx - r, cy - r, cx + r, cy + r))
        assert len(boxes) <= WORLD_MAX_BOXES
        fboxes = np.array(boxes, np.float64) / 20.0
        walls = inflated_rects(boxes=fboxes)
        sizes = list(OBJECT_SIZES.values())
        spots = []
        for j in range(ny):
            for i in range(nx):
                x0, x1, y0, y1 = X[i] + h, X[i + 1] - h, Y[j] + h, Y[j + 1] - h
                for qy in (1, 2, 3):
                    for qx in (1, 2, 3):
                        sx = 5 * ((2 * (4 * x0 + qx * (x1 - x0)) + 20) // 40)     # the quarter point, rounded to 0.25 m
                        sy = 5 * ((2 * (4 * y0 + qy * (y1 - y0)) + 20) // 40)
                        if (sx, sy) in spots:
                            continue
                        if any(max(b[0] - sx, 0, sx - b[2]) ** 2 + max(b[1] - sy, 0, sy - b[3]) ** 2 < 13 * 13 for b in boxes):
                            continue
                        if any((dx - sx) ** 2 + (dy - sy) ** 2 < 32 * 32 for (dx, dy) in doors):
                            continue
                        # the doubles the geodesic sees: object_box, then inflated_rects
                        obj = inflated_rects([(sx / 20.0 - hx, sy / 20.0 - hy, sx / 20.0 + hx, sy / 20.0 + hy)
                                              for (hx, hy, _, _) in sizes], boxes=np.zeros((0, 4)))
                        if rects_abut(obj, walls).any():
                            continue
                        spots.append((sx, sy))
        assert len(spots) >= 12
        start = spots[rnd(len(spots))]
        return World(fboxes, np.array(start, np.float64) / 20.0, rnd(12), np.array(spots, np.float64) / 20.0,
                     np.array(doors, np.float64).reshape(-1, 2) / 20.0)

    def layout(self, env_id: int, episode: int, robot_xy):
        """`object_layout` over the spots of ``world(env_id, episode)``: the target (class ``env_id mod 6``) and one distractor,
        both farther than OBJECT_START_CLEARANCE from the robot and more than 1.5 m apart."""
        return _layout_over_spots(self.world(env_id, episode).spots, env_id, episode, robot_xy)


def _layout_over_spots(spots, env_id: int, episode: int, robot_xy):
    """The layout rule of the generated worlds (ProceduralWorlds.layout, GridWorlds.layout) over the object spots ``spots``."""
    spots = [tuple(p) for p in np.asarray(spots, np.float64).reshape(-1, 2).tolist()]
    classes = list(OBJECT_SIZES)
    target = classes[env_id % len(classes)]
    rx, ry = float(robot_xy[0]), float(robot_xy[1])
    free = [p for p in spots if (p[0] - rx) ** 2 + (p[1] - ry) ** 2 > OBJECT_START_CLEARANCE ** 2]
    a = free[_mix32(env_id, episode, 21) % len(free)]
    apart = [p for p in free if (p[0] - a[0]) ** 2 + (p[1] - a[1]) ** 2 > 1.5 ** 2]
    b = apart[_mix32(env_id, episode, 22) % len(apart)]
    other = [c for c in classes if c != target]
    distractor = other[_mix32(env_id, episode, 23) % len(other)]
    return [(target, object_box(target, *a)), (distractor, object_box(distractor, *b))]


# ---------------------------------------------------------------------------------------------- grid worlds
# A floor plan as an occupancy grid: a top-down map someone already has (a scanned scene's occupancy export, an obstacle map
# recorded by this package, a drawn PNG with diagonal walls and round pillars) instead of at most WORLD_MAX_BOXES boxes.
#
#   plan        occ bool [ny, nx], xs f64 [nx + 1], ys f64 [ny + 1] strictly increasing.  Cell (i, j) is the box
#               (xs[i], ys[j], xs[i+1], ys[j+1]) and a full-height wall iff occ[j, i].
#   definition  a grid world IS the box world of its occupied cells: depth, ids, stats and refused moves are what the box
#               statements (`wall_profile`, `render_objects_numpy`, `step_poses`) give for boxes = grid_boxes(plan), with their
#               rules: closed slabs, tmin > 0 (a cell around the camera is transparent), |dx| < 1e-12 -> 1e-12, STEP_MARGIN with
#               closed comparisons.  With boxes AND a grid a column's wall is the f64 minimum of the two, rounded to f32 after.
#   algorithm   `grid_profile_numpy`, and csrc/world_render.hip's grid_walk with the same bits: per column, with the slab test's
#               own crossing times TX[e] = (xs[e] - x) / dx, TY[e] = (ys[e] - y) / dy (true divisions, nothing accumulated):
#               the x slab at t = 0+ is the i with TX[i] <= 0 < TX[i+1] (dx > 0; mirrored for dx < 0; -1 or nx: the camera is
#               outside), likewise in y; then repeatedly the smaller of the next x and the next y crossing is taken and the cell
#               behind it entered -- occupied: the answer is that crossing time.  Equal crossing times: the answer is that time
#               if any of (i+sx, j), (i, j+sy), (i+sx, j+sy) is occupied (all three have that tmin under the closed-slab rule),
#               else the walk steps diagonally.  Cells outside the grid are free; the walk ends once an index is past the far
#               side of its axis, after nx + ny + 2 steps at the most.
# TX and TY are monotone in e (a rounded subtraction and a rounded division are monotone), which is all the walk relies on.
GRID_MAX_CELLS = 1024
GRID_MIN_SPACING = 1e-3
GRID_MAX_EDGE = 1e4


class GridPlan:
    """An occupancy-grid floor plan: ``occ`` bool [ny,nx], ``xs`` f64 [nx+1], ``ys`` f64 [ny+1] (the rule above).  Refuses
    nx or ny outside [1, GRID_MAX_CELLS], edges that do not increase strictly, a spacing below GRID_MIN_SPACING metres and
    |edge| > GRID_MAX_EDGE.  The arrays are copies and read-only."""

    def __init__(self, occ, xs, ys) -> None:
        occ = np.array(occ)
        if occ.ndim != 2 or occ.dtype.kind not in "biu":
            raise ValueError("GridPlan: occ must be a [ny,nx] array of truth values")
        occ = occ.astype(bool)
        xs, ys = np.array(xs, np.float64).reshape(-1), np.array(ys, np.float64).reshape(-1)
        ny, nx = occ.shape
        if not (1 <= nx <= GRID_MAX_CELLS and 1 <= ny <= GRID_MAX_CELLS):
            raise ValueError(f"GridPlan: nx and ny must lie in [1, {GRID_MAX_CELLS}]")
        if len(xs) != nx + 1 or len(ys) != ny + 1:
            raise ValueError("GridPlan: xs must hold nx + 1 edges and ys ny + 1")
        for e in (xs, ys):
            if not np.all(np.isfinite(e)) or np.any(np.abs(e) > GRID_MAX_EDGE):
                raise ValueError(f"GridPlan: edges must be finite and within +-{GRID_MAX_EDGE:g} m")
            if not np.all(np.diff(e) > 0.0):
                raise ValueError("GridPlan: edges must increase strictly")
            if np.any(np.diff(e) < GRID_MIN_SPACING):
                raise ValueError(f"GridPlan: cells must be at least {GRID_MIN_SPACING:g} m wide")
        for a in (occ, xs, ys):
            a.setflags(write=False)
        self.occ, self.xs, self.ys = occ, xs, ys

    @property
    def nx(self) -> int:
        return self.occ.shape[1]

    @property
    def ny(self) -> int:
        return self.occ.shape[0]

    def packed_rows(self, words: int = None) -> np.ndarray:
        """uint32 [ny, words]: bit i % 32 of word i // 32 of row j is occ[j, i] (words >= ceil(nx / 32), the rest zero)."""
        need = (self.nx + 31) // 32
        words = need if words is None else int(words)
        if words < need:
            raise ValueError("GridPlan.packed_rows: too few words for a row")
        bits = np.zeros((self.ny, words * 32), np.uint8)
        bits[:, :self.nx] = self.occ
        return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(self.ny, words)

    @classmethod
    def uniform(cls, occ, cells_per_metre: int, i0: int, j0: int) -> "GridPlan":
        """Square cells on the lattice of 1 / ``cells_per_metre`` m: edge e of x is (i0 + e) / cells_per_metre -- ONE division,
        the procedural generator's own values -- and likewise (j0 + e) / cells_per_metre in y."""
        occ = np.asarray(occ)
        n = int(cells_per_metre)
        if n != cells_per_metre or n < 1 or int(i0) != i0 or int(j0) != j0 or occ.ndim != 2:
            raise ValueError("GridPlan.uniform: cells_per_metre >= 1, i0 and j0 must be integers, occ [ny,nx]")
        ny, nx = occ.shape
        return cls(occ, (int(i0) + np.arange(nx + 1, dtype=np.float64)) / float(n),
                   (int(j0) + np.arange(ny + 1, dtype=np.float64)) / float(n))

    @classmethod
    def from_boxes(cls, boxes, cells_per_metre: int = 20) -> "GridPlan":
        """The boxes ``boxes`` [B,4] rasterised on the lattice of 1 / ``cells_per_metre`` m over their bounding box.  Refuses
        boxes whose edges are not lattice values (k / cells_per_metre, the same double)."""
        b = np.asarray(boxes, np.float64).reshape(-1, 4)
        n = int(cells_per_metre)
        if n != cells_per_metre or n < 1 or not len(b) or not np.all(np.isfinite(b)):
            raise ValueError("GridPlan.from_boxes: cells_per_metre >= 1 and at least one finite box")
        k = np.rint(b * n)
        if not np.array_equal(k / float(n), b) or np.any(k[:, 2] <= k[:, 0]) or np.any(k[:, 3] <= k[:, 1]):
            raise ValueError(f"GridPlan.from_boxes: every box edge must be a multiple of 1/{n} m and x0 < x1, y0 < y1")
        k = k.astype(np.int64)
        i0, j0, i1, j1 = k[:, 0].min(), k[:, 1].min(), k[:, 2].max(), k[:, 3].max()
        if i1 - i0 > GRID_MAX_CELLS or j1 - j0 > GRID_MAX_CELLS:
            raise ValueError(f"GridPlan.from_boxes: the boxes span more than {GRID_MAX_CELLS} cells")
        occ = np.zeros((j1 - j0, i1 - i0), bool)
        for (a0, c0, a1, c1) in k.tolist():
            occ[c0 - j0:c1 - j0, a0 - i0:a1 - i0] = True
        return cls.uniform(occ, n, int(i0), int(j0))

    @classmethod
    def from_image(cls, array_or_path, cells_per_metre: int, i0: int, j0: int, occupied_below: int = 128) -> "GridPlan":
        """A greyscale picture of the plan seen from above: a uint8 [rows, columns] array, or a file Pillow opens (converted to
        greyscale).  A pixel darker than ``occupied_below`` is a wall; image row 0 is the HIGHEST y."""
        if isinstance(array_or_path, np.ndarray):
            img = array_or_path
        else:
            from PIL import Image

            with Image.open(array_or_path) as im:
                img = np.array(im.convert("L"))
        if img.ndim != 2 or img.dtype != np.uint8:
            raise ValueError("GridPlan.from_image: a uint8 [rows, columns] array or an image file")
        return cls.uniform(img[::-1] < int(occupied_below), cells_per_metre, i0, j0)


def grid_boxes(plan: GridPlan) -> np.ndarray:
    """[K,4] f64: the boxes (xs[i], ys[j], xs[i+1], ys[j+1]) of the occupied cells, rows first -- the definition of a grid world."""
    j, i = np.nonzero(plan.occ)
    return np.stack([plan.xs[i], plan.ys[j], plan.xs[i + 1], plan.ys[j + 1]], axis=1).reshape(-1, 4)


def _grid_first_slab(edges, p, d) -> np.ndarray:
    """int64 [W]: per column the slab of one axis at t = 0+: the i with T[i] <= 0 < T[i+1] for d > 0 (T[i+1] <= 0 < T[i] for
    d < 0), T[e] = (edges[e] - p) / d; -1 or len(edges) - 1 outside."""
    T = (edges[None, :] - p) / d[:, None]
    return np.where(d > 0.0, (T <= 0.0).sum(axis=1), (T > 0.0).sum(axis=1)) - 1


def grid_profile_numpy(x, y, c, s, fx, W: int, plan: GridPlan, return_steps: bool = False):
    """f64 [W]: per image column the ray parameter at which the ray of `wall_profile` enters the first occupied cell of
    ``plan`` (inf: none) -- the grid walk of the rule above, vectorised over columns; bit for bit
    min over grid_boxes(plan) of the slab test's tmin BEFORE the rounding to f32.  ``return_steps``: also int64 [W], the cells
    each column's walk entered."""
    dx, dy = _column_rays(c, s, fx, W)
    nx, ny, xs, ys = plan.nx, plan.ny, plan.xs, plan.ys
    occ = np.zeros((ny + 2, nx + 2), bool)              # a free ring around the grid: cell (i, j) is occ[j + 1, i + 1]
    occ[1:-1, 1:-1] = plan.occ
    sx, sy = np.where(dx > 0.0, 1, -1), np.where(dy > 0.0, 1, -1)
    i, j = _grid_first_slab(xs, x, dx), _grid_first_slab(ys, y, dy)
    out = np.full(W, np.inf)
    steps = np.zeros(W, np.int64)
    live = np.ones(W, bool)

    def at(ii, jj):         # occupancy of the cells (ii, jj), free outside [-1, nx] x [-1, ny]
        inside = (ii >= -1) & (ii <= nx) & (jj >= -1) & (jj <= ny)
        return inside & occ[np.clip(jj, -1, ny) + 1, np.clip(ii, -1, nx) + 1]

    for _ in range(nx + ny + 2):
        ex, ey = i + (sx > 0), j + (sy > 0)              # the next edge of each axis
        live &= (ex >= 0) & (ex <= nx) & (ey >= 0) & (ey <= ny)      # past the far side of an axis: nothing more to enter
        if not live.any():
            break
        tx = (xs[np.clip(ex, 0, nx)] - x) / dx
        ty = (ys[np.clip(ey, 0, ny)] - y) / dy
        gx, gy = live & (tx <= ty), live & (ty <= tx)    # which axes cross next; both: a corner
        tie = gx & gy
        i2, j2 = np.where(gx, i + sx, i), np.where(gy, j + sy, j)
        hit = live & (at(i2, j2) | (tie & (at(i + sx, j) | at(i, j + sy))))
        out[hit] = np.where(gx, tx, ty)[hit]
        steps += live
        live &= ~hit
        i, j = i2, j2
    return (out, steps) if return_steps else out


def grid_blocked(plan: GridPlan, x: float, y: float, margin: float = STEP_MARGIN) -> bool:
    """`_blocked` / `step_poses`' test against the occupied cells of ``plan``: is there an occupied cell (i, j) with
    xs[i] - m <= x <= xs[i+1] + m and ys[j] - m <= y <= ys[j+1] + m (the box rule's own comparisons on the cell's edges).  Only
    the cells near (x, y) are looked at: edge - m and edge + m are monotone in the edge, so the cells that pass each comparison
    are a run of indices."""
    m = float(margin)
    i0, i1 = np.searchsorted(plan.xs[1:] + m, x, side="left"), np.searchsorted(plan.xs[:-1] - m, x, side="right")
    j0, j1 = np.searchsorted(plan.ys[1:] + m, y, side="left"), np.searchsorted(plan.ys[:-1] - m, y, side="right")
    return bool(i0 < i1 and j0 < j1 and plan.occ[j0:j1, i0:i1].any())


def grid_spots(plan: GridPlan, clearance: float = 0.65, step: float = 0.25, start=None) -> np.ndarray:
    """[S,2] f64: the lattice points (step * a, step * b) inside the plan's extent that keep ``clearance`` to every occupied
    cell (`rect_distance` >= clearance), ordered by (a, b), restricted to those a 4-connected flood fill over the lattice points
    that the STEP_MARGIN-inflated grid does not block (`grid_blocked`) reaches from ``start`` (a lattice point; None: the first
    clear point in that order)."""
    a = np.arange(int(np.ceil(plan.xs[0] / step)), int(np.floor(plan.xs[-1] / step)) + 1)
    b = np.arange(int(np.ceil(plan.ys[0] / step)), int(np.floor(plan.ys[-1] / step)) + 1)
    free = np.zeros((len(a), len(b)), bool)
    clear = np.zeros((len(a), len(b)), bool)
    boxes = grid_boxes(plan)
    for p, ia in enumerate(a):
        px = step * float(ia)
        for q, ib in enumerate(b):
            py = step * float(ib)
            free[p, q] = not grid_blocked(plan, px, py, STEP_MARGIN)
            if free[p, q] and not grid_blocked(plan, px, py, clearance):     # (no cell within the square: the disc is inside it)
                clear[p, q] = True
            elif free[p, q] and len(boxes):
                i0, i1 = np.searchsorted(plan.xs[1:] + clearance, px, side="left"), np.searchsorted(plan.xs[:-1] - clearance, px, side="right")
                j0, j1 = np.searchsorted(plan.ys[1:] + clearance, py, side="left"), np.searchsorted(plan.ys[:-1] - clearance, py, side="right")
                jj, ii = np.nonzero(plan.occ[j0:j1, i0:i1])
                ddx = np.maximum(np.maximum(plan.xs[i0 + ii] - px, 0.0), px - plan.xs[i0 + ii + 1])
                ddy = np.maximum(np.maximum(plan.ys[j0 + jj] - py, 0.0), py - plan.ys[j0 + jj + 1])
                clear[p, q] = bool(np.all(ddx * ddx + ddy * ddy >= clearance * clearance))
    if not clear.any():
        return np.zeros((0, 2))
    if start is None:
        p0, q0 = (int(v) for v in np.argwhere(clear)[0])
    else:
        p0, q0 = int(round(float(start[0]) / step)) - int(a[0]), int(round(float(start[1]) / step)) - int(b[0])
        if not (0 <= p0 < len(a) and 0 <= q0 < len(b)) or step * float(a[p0]) != float(start[0]) or step * float(b[q0]) != float(start[1]):
            raise ValueError("grid_spots: start must be a lattice point inside the plan")
    seen = np.zeros_like(free)
    if free[p0, q0]:
        seen[p0, q0] = True
        todo = [(p0, q0)]
        while todo:
            p, q = todo.pop()
            for (u, v) in ((p + 1, q), (p - 1, q), (p, q + 1), (p, q - 1)):
                if 0 <= u < len(a) and 0 <= v < len(b) and free[u, v] and not seen[u, v]:
                    seen[u, v] = True
                    todo.append((u, v))
    pq = np.argwhere(clear & seen)
    return np.stack([step * a[pq[:, 0]].astype(np.float64), step * b[pq[:, 1]].astype(np.float64)], axis=1).reshape(-1, 2)


class GridWorlds:
    """``worlds.world(env_id, episode)`` over a list of GridPlans: a pure function of (seed, env_id, episode) through `_mix32` --
    the plan, and a hashed start among the plan's spots with a hashed heading unless ``starts`` gives one (x, y, k) per plan.
    ``spots``: per plan the object spots [S,2] (None: `grid_spots(plan)`).  The World has no boxes; its ``grid`` is the plan.
    ``layout`` is ProceduralWorlds.layout's rule over the plan's spots.  ``max_grid`` = (ny, nx): what a WorldTable must hold."""

    def __init__(self, plans, starts=None, spots=None, seed: int = 0) -> None:
        self.plans = list(plans)
        if not self.plans or not all(isinstance(p, GridPlan) for p in self.plans):
            raise ValueError("GridWorlds: a non-empty list of GridPlans")
        if (starts is not None and len(starts) != len(self.plans)) or (spots is not None and len(spots) != len(self.plans)):
            raise ValueError("GridWorlds: one start and one list of spots per plan")
        self.seed = int(seed)
        self.starts = None if starts is None else [(float(x), float(y), int(k) % 12) for (x, y, k) in starts]
        self._spots = [None] * len(self.plans) if spots is None else [np.array(s, np.float64).reshape(-1, 2) for s in spots]
        self.max_grid = (max(p.ny for p in self.plans), max(p.nx for p in self.plans))

    def spots(self, n: int) -> np.ndarray:
        if self._spots[n] is None:
            self._spots[n] = grid_spots(self.plans[n])
        self._spots[n].setflags(write=False)
        return self._spots[n]

    def plan_of(self, env_id: int, episode: int) -> int:
        return _mix32(_mix32(self.seed, int(env_id), 111), int(episode), 112) % len(self.plans)

    def world(self, env_id: int, episode: int) -> World:
        n = self.plan_of(env_id, episode)
        base = _mix32(_mix32(self.seed, int(env_id), 113), int(episode), 114)
        spots = self.spots(n)
        if self.starts is not None:
            x, y, k = self.starts[n]
        else:
            if not len(spots):
                raise ValueError("GridWorlds: a plan without a spot needs a start")
            (x, y), k = spots[_mix32(base, 0, 115) % len(spots)], _mix32(base, 1, 115) % 12
        start = np.array([x, y], np.float64)
        start.setflags(write=False)
        return World(np.zeros((0, 4)), start, int(k), spots, np.zeros((0, 2)), self.plans[n])

    def layout(self, env_id: int, episode: int, robot_xy):
        return _layout_over_spots(self.world(env_id, episode).spots, env_id, episode, robot_xy)


# ---------------------------------------------------------------------------------------------- Lattice geodesic
# The ObjectNav metrics' second backend: the geodesic on a metric LATTICE with integer costs, for worlds the visibility graph
# cannot hold (grid worlds: tens of thousands of occupied cells; box worlds beyond 141 rectangles).  This section is the HOST
# STATEMENT; the device (csrc/lattice_geodesic.hip: vlfm_lattice_free / vlfm_lattice_fields / vlfm_lattice_query) matches it
# bit for bit.  Everything is integers except the free test and the query, which are f64 with one rounding per operation.
#
#   lattice    n = cells_per_metre, an int and a multiple of 4 (every multiple of 0.25 m -- robot starts, grid_spots, view
#              points -- is a node).  Node (a, b), global integers, sits at (a / n, b / n): true f64 divisions.  A field covers
#              a0 .. a0 + na - 1 by b0 .. b0 + nb - 1 (`lattice_extent`: the hull of the world's boxes, the plan's extent and the
#              valid object footprints, widened by STEP_MARGIN + pad_m, floor / ceil of the bound times n); na, nb <= 1024.
#              Nodes outside the lattice do not exist.
#   free       the obstacles of the visibility-graph rule -- the world's boxes, its occupied grid cells, the valid object
#              footprints --, each inflated by STEP_MARGIN with `step_poses`' expressions, each an OPEN set: node (x, y) is
#              blocked iff some obstacle has lo_x < x < hi_x and lo_y < y < hi_y.  Grid cells: edge - m and edge + m are monotone
#              in the edge, so the cells passing each strict comparison are a run of indices, found by binary search; the node
#              is blocked iff any cell of that block of the plan is occupied.
#   moves      16-connected: 5 straight, 7 diagonal, 11 for a knight move (+-2, +-1) / (+-1, +-2).  Both ends free, and the
#              intermediate nodes: a diagonal needs the two nodes that share an edge with both ends; a knight move (2s, t) from
#              (a, b) needs (a + s, b) and (a + s, b + t); (s, 2t) needs (a, b + t) and (a + s, b + t).  Symmetric.
#   sources    `goal_viewpoints`' points, each the node round(0.25 i * n); cost 0 if that node is free (a closed-free point is
#              open-free, so every view point is a source).  A source outside the lattice or on a blocked node is ignored.
#   field      uint16 [nb][na]: the least cost over move sequences from a source; 0xFFFF: none, or above ``max_cost`` (<= 65534).
#   query      p = (x, y): fa = floor(x * n), fb = floor(y * n); over the four nodes (fa | fa + 1, fb | fb + 1) that lie in the
#              lattice and hold a cost: d = min fl(sqrt(dx*dx + dy*dy) + cost / (5.0 * n)), dx = x - a / n, dy = y - b / n;
#              inf if none qualifies.  No visibility test: p and the node are less than a cell apart.
#
# Known looseness: the chamfer is not Euclidean -- in free space cost / (5 n) over the true length lies in
# [5.5 / (5 sqrt(1.25)), 5.2 / (5 sqrt(1.04))] = [0.98387, 1.01980], plus O(1/n) at corners and at the query; paths cannot leave
# the padded lattice; a point inside an obstacle but within a cell of its border may get a finite value (robots never stand
# there).  Against the visibility-graph rule in the rooms world: tests/test_lattice_geodesic_cpu.py.
LATTICE_MAX_NODES = 1024
LATTICE_NONE = 0xFFFF
LATTICE_MAX_COST = 65534
LATTICE_MOVES = tuple([(dx, dy, 5) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))] +
                      [(dx, dy, 7) for dx in (1, -1) for dy in (1, -1)] +
                      [(2 * s, t, 11) for s in (1, -1) for t in (1, -1)] + [(s, 2 * t, 11) for s in (1, -1) for t in (1, -1)])


def _lattice_n(cells_per_metre) -> int:
    n = int(cells_per_metre)
    if n != cells_per_metre or n < 4 or n % 4:
        raise ValueError("lattice geodesic: cells_per_metre must be a positive multiple of 4 (every 0.25 m is a node)")
    return n


def _valid_footprints(objects) -> np.ndarray:
    """[K,4] f64: the footprints of ``objects`` -- [K,8] ray-caster records (valid: column 6 non-zero), [K,4] / [K,6] boxes, None."""
    if objects is None or not len(objects):
        return np.zeros((0, 4))
    o = np.asarray(objects, np.float64)
    o = o.reshape(-1, o.shape[-1])
    return (o[o[:, 6] != 0.0] if o.shape[1] == 8 else o)[:, :4]


def lattice_extent(boxes=None, grid=None, objects=None, cells_per_metre: int = 20, pad_m: float = 1.0):
    """(a0, b0, na, nb): the nodes a lattice field covers -- the hull of the walls ``boxes`` (None: BOXES), of ``grid``'s extent and
    of the valid footprints of ``objects``, widened by STEP_MARGIN + pad_m; floor / ceil of the bound times n (an empty hull is
    the origin).  ValueError when na or nb exceeds LATTICE_MAX_NODES."""
    n = _lattice_n(cells_per_metre)
    b = np.concatenate([_walls_of(boxes), _valid_footprints(objects)])
    if grid is not None:
        b = np.concatenate([b, [[grid.xs[0], grid.ys[0], grid.xs[-1], grid.ys[-1]]]])
    if not len(b):
        b = np.zeros((1, 4))
    if not np.all(np.isfinite(b)) or not np.isfinite(pad_m) or pad_m < 0.0:
        raise ValueError("lattice_extent: finite boxes and pad_m >= 0")
    w = STEP_MARGIN + float(pad_m)
    a0, b0 = int(np.floor((b[:, 0].min() - w) * n)), int(np.floor((b[:, 1].min() - w) * n))
    a1, b1 = int(np.ceil((b[:, 2].max() + w) * n)), int(np.ceil((b[:, 3].max() + w) * n))
    na, nb = a1 - a0 + 1, b1 - b0 + 1
    if na > LATTICE_MAX_NODES or nb > LATTICE_MAX_NODES:
        raise ValueError(f"lattice_extent: {na} x {nb} nodes, a lattice field holds at most {LATTICE_MAX_NODES} a side "
                         f"(fewer cells_per_metre, or a smaller pad_m)")
    return a0, b0, na, nb


def lattice_free_numpy(extent, boxes=None, grid=None, objects=None, cells_per_metre: int = 20,
                       margin: float = STEP_MARGIN) -> np.ndarray:
    """bool [nb, na]: the free nodes of the lattice ``extent`` = (a0, b0, na, nb) (the rule above): not strictly inside a wall of
    ``boxes`` (None: BOXES), an occupied cell of ``grid`` or a valid footprint of ``objects``, each inflated by ``margin``."""
    n, m = _lattice_n(cells_per_metre), float(margin)
    a0, b0, na, nb = (int(v) for v in extent)
    x = np.arange(a0, a0 + na, dtype=np.float64) / float(n)
    y = np.arange(b0, b0 + nb, dtype=np.float64) / float(n)
    blocked = np.zeros((nb, na), bool)
    for (x0, y0, x1, y1) in np.concatenate([_walls_of(boxes), _valid_footprints(objects)]):
        blocked |= ((y0 - m < y) & (y < y1 + m))[:, None] & ((x0 - m < x) & (x < x1 + m))[None, :]
    if grid is not None:
        i0, i1 = np.searchsorted(grid.xs[1:] + m, x, side="right"), np.searchsorted(grid.xs[:-1] - m, x, side="left")
        j0, j1 = np.searchsorted(grid.ys[1:] + m, y, side="right"), np.searchsorted(grid.ys[:-1] - m, y, side="left")
        area = np.zeros((grid.ny + 1, grid.nx + 1), np.int64)      # occ[j0:j1, i0:i1].any() of every node, from one summed table
        area[1:, 1:] = np.cumsum(np.cumsum(grid.occ, axis=0, dtype=np.int64), axis=1)
        i1, j1 = np.maximum(i0, i1), np.maximum(j0, j1)
        J0, J1, I0, I1 = j0[:, None], j1[:, None], i0[None, :], i1[None, :]
        blocked |= (area[J1, I1] - area[J0, I1] - area[J1, I0] + area[J0, I0]) > 0
    return ~blocked


def lattice_sources(points, cells_per_metre: int = 20) -> np.ndarray:
    """int64 [S,2]: the nodes (a, b) = round(p * n) of the view points ``points`` [S,2] (multiples of 0.25 m)."""
    return np.rint(np.asarray(points, np.float64).reshape(-1, 2) * float(_lattice_n(cells_per_metre))).astype(np.int64)


def _through(dx: int, dy: int):
    """The offsets, besides its two ends, of the cells the move (dx, dy) needs free: none for a straight move; for a diagonal the
    two cells that share an edge with both ends; for a knight move the two intermediate nodes, next to the source and to the
    target along the long axis."""
    if dx == 0 or dy == 0:
        return ()
    if abs(dx) == abs(dy):
        return ((dx, 0), (0, dy))
    return ((dx // 2, 0), (dx // 2, dy)) if abs(dx) == 2 else ((0, dy // 2), (dx, dy // 2))


def _move_masks(free, moves, through) -> np.ndarray:
    """bool [len(moves), h, w]: may the move ``moves[k]`` = (dx, dy) leave cell [y, x] of ``free`` [h, w] -- both ends and the
    cells at the offsets ``through[k]`` free, everything outside ``free`` blocked.  The one statement behind
    lattice_move_masks and plan_allowed_moves."""
    free = np.asarray(free, bool)
    h, w = free.shape
    pad = max(max(abs(dx), abs(dy)) for dx, dy in moves)
    f = np.zeros((h + 2 * pad, w + 2 * pad), bool)
    f[pad:pad + h, pad:pad + w] = free
    at = lambda dx, dy: f[pad + dy:pad + dy + h, pad + dx:pad + dx + w]      # noqa: E731  free[y + dy, x + dx]
    out = np.zeros((len(moves), h, w), bool)
    for k, (dx, dy) in enumerate(moves):
        out[k] = free & at(dx, dy)
        for ox, oy in through[k]:
            out[k] &= at(ox, oy)
    return out


def lattice_move_masks(free) -> np.ndarray:
    """bool [16, nb, na], in the order of LATTICE_MOVES: may the move leave node (b, a) (both ends and the intermediate nodes
    free, the target inside the lattice)."""
    steps = [(dx, dy) for dx, dy, _ in LATTICE_MOVES]
    return _move_masks(free, steps, [_through(dx, dy) for dx, dy in steps])


def lattice_field_numpy(free, sources, origin=(0, 0), max_cost: int = LATTICE_MAX_COST) -> np.ndarray:
    """uint16 [nb, na]: the field of the rule above over the free mask ``free`` [nb, na] of a lattice whose node [0, 0] is
    ``origin`` = (a0, b0), around the source nodes ``sources`` [S,2] (global a, b), by Dial's level sets: level d is what a
    straight move reaches from level d - 5, a diagonal from d - 7, a knight move from d - 11 and nothing settled earlier."""
    free = np.asarray(free, bool)
    nb, na = free.shape
    max_cost = int(max_cost)
    if not 0 <= max_cost <= LATTICE_MAX_COST:
        raise ValueError(f"lattice_field_numpy: max_cost in [0, {LATTICE_MAX_COST}]")
    dist = np.full(nb * na, LATTICE_NONE, np.uint16)
    s = np.asarray(sources, np.int64).reshape(-1, 2) - np.asarray(origin, np.int64)
    s = s[(s[:, 0] >= 0) & (s[:, 0] < na) & (s[:, 1] >= 0) & (s[:, 1] < nb)]
    s = np.unique(s[:, 1] * na + s[:, 0])
    s = s[free.reshape(-1)[s]]
    dist[s] = 0
    ok = lattice_move_masks(free).reshape(len(LATTICE_MOVES), -1)
    levels = {0: s}
    empty = 0 if len(s) else 11
    d = 0
    while d < max_cost and empty < 11:
        d += 1
        new = []
        for k, (dx, dy, c) in enumerate(LATTICE_MOVES):
            src = levels.get(d - c)
            if src is not None and len(src):
                new.append(src[ok[k][src]] + (dy * na + dx))
        levels.pop(d - 12, None)
        got = np.unique(np.concatenate(new)) if new else np.zeros(0, np.int64)
        got = got[dist[got] == LATTICE_NONE]
        dist[got] = d
        levels[d] = got
        empty = 0 if len(got) else empty + 1
    return dist.reshape(nb, na)


def lattice_query_numpy(dist, origin, points, cells_per_metre: int = 20) -> np.ndarray:
    """f64 [m]: the query of the rule above for the ``points`` [m,2] in the field ``dist`` uint16 [nb, na] whose node [0, 0] is
    ``origin`` = (a0, b0).  inf: none of the four nodes around the point is in the lattice with a cost."""
    n = float(_lattice_n(cells_per_metre))
    dist = np.asarray(dist, np.uint16)
    nb, na = dist.shape
    a0, b0 = (int(v) for v in origin)
    p = np.asarray(points, np.float64).reshape(-1, 2)
    with np.errstate(over="ignore"):
        fa, fb = np.floor(p[:, 0] * n), np.floor(p[:, 1] * n)
    out = np.full(len(p), np.inf)
    for ua in (0.0, 1.0):
        for ub in (0.0, 1.0):
            a, b = fa + ua, fb + ub
            inside = (a >= a0) & (a <= a0 + na - 1) & (b >= b0) & (b <= b0 + nb - 1)       # (False for a NaN)
            ia, ib = np.where(inside, a - a0, 0.0).astype(np.int64), np.where(inside, b - b0, 0.0).astype(np.int64)
            cost = dist[ib, ia]
            with np.errstate(invalid="ignore", over="ignore"):                             # (points at infinity: not inside)
                dx, dy = p[:, 0] - a / n, p[:, 1] - b / n
                d = np.sqrt(dx * dx + dy * dy) + cost.astype(np.float64) / (5.0 * n)
            out = np.where(inside & (cost != LATTICE_NONE), np.minimum(out, d), out)
    return out


# ---------------------------------------------------------------------------------------------- map planner
# Shortest paths over a navigable plane (ObstacleMapBatch.navigable_bits: the reference's _navigable_map, obstacles dilated by
# the robot's footprint, unexplored cells free).  `plan_paths_numpy` is the host statement of the rule; the device path
# (csrc/map_planner.hip: vlfm_plan_paths, ObstacleMapBatch.plan_paths) matches it bit for bit.  Integers only.  The contract is
# stated in full in include/vlfm_amd.h ("Map planner"); in short, per JOB (env, y0, y1, x0, x1, sx, sy, start_free, gx, gy,
# goal_free), cells (x, y) = (column, row):
#   free     inside the inclusive window: navigable, or dx*dx + dy*dy <= r*r about start (r = start_free) or goal (goal_free)
#   moves    8-connected, cost 2 (E/N/W/S) or 3 (diagonals); both cells free, and for a diagonal the two cells that share an
#            edge with both (no corner cutting, no squeezing through a diagonal gap)
#   field    dist[c]: least cost from the goal, uint16, 0xFFFF = none (blocked, outside, not reached, above max_cost)
#   descent  from start, at most `lookahead` steps, each to the FIRST chain code s = 0..7 (E NE N NW W SW S SE, y down) whose
#            move is allowed and has dist[next] + cost(s) == dist[cur]
# cost * 0.5 / pixels_per_meter is the path length in metres; it overstates pure diagonals by 6 % (3/2 against sqrt 2).
PLAN_OK, PLAN_UNREACHABLE, PLAN_TOO_LONG, PLAN_INVALID = 0, 1, 2, 3
PLAN_NONE = 0xFFFF
PLAN_MAX_RADIUS = 4096
PLAN_JOB_FIELDS = ("env", "y0", "y1", "x0", "x1", "sx", "sy", "start_free", "gx", "gy", "goal_free")
PLAN_CODE_DX = (1, 1, 0, -1, -1, -1, 0, 1)      # csrc/bitmap.h: code_dx / code_dy
PLAN_CODE_DY = (0, -1, -1, -1, 0, 1, 1, 1)


def plan_jobs_array(jobs) -> np.ndarray:
    """[n,11] int64 rows in PLAN_JOB_FIELDS order, from such rows or from a structured array with those field names."""
    a = np.asarray(jobs)
    if a.dtype.names:
        a = np.stack([a[f].astype(np.int64) for f in PLAN_JOB_FIELDS], axis=-1)
    return np.asarray(a, np.int64).reshape(-1, len(PLAN_JOB_FIELDS))


def plan_allowed_moves(free: np.ndarray) -> np.ndarray:
    """[8,h,w] bool: is the move with chain code s out of cell (x, y) = [s, y, x] of the window's ``free`` [h,w] allowed."""
    steps = list(zip(PLAN_CODE_DX, PLAN_CODE_DY))
    return _move_masks(free, steps, [_through(dx, dy) for dx, dy in steps])


def plan_paths_numpy(free_or_navigable, jobs, lookahead: int = 15, max_cost: int = 65534):
    """(results [n,5] int64: status, cost, waypoint_x, waypoint_y, steps;  fields: per job the uint16 [h,w] field of its window,
    None for an invalid job).  ``free_or_navigable``: [n_envs,S,S] or [S,S] (one slot) of truth values, rows y, columns x.
    Plain Dijkstra with a heap over the allowed moves, then the descent: slow, and the yardstick."""
    import heapq

    planes = np.asarray(free_or_navigable).astype(bool)
    if planes.ndim == 2:
        planes = planes[None]
    n_envs, S = planes.shape[0], planes.shape[1]
    if not 0 <= max_cost <= 65534 or lookahead < 0:
        raise ValueError("plan_paths_numpy: max_cost in [0, 65534], lookahead >= 0")
    jobs = plan_jobs_array(jobs)
    results = np.zeros((len(jobs), 5), np.int64)
    fields = []
    for n, (env, y0, y1, x0, x1, sx, sy, rs, gx, gy, rg) in enumerate(jobs.tolist()):
        results[n] = (PLAN_INVALID, PLAN_NONE, sx, sy, 0)
        if not (0 <= env < n_envs and 0 <= y0 <= y1 < S and 0 <= x0 <= x1 < S and x0 <= sx <= x1 and y0 <= sy <= y1 and
                x0 <= gx <= x1 and y0 <= gy <= y1 and 0 <= rs <= PLAN_MAX_RADIUS and 0 <= rg <= PLAN_MAX_RADIUS):
            fields.append(None)
            continue
        free = planes[env, y0:y1 + 1, x0:x1 + 1].copy()
        h, w = free.shape
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        free |= (xx - sx) ** 2 + (yy - sy) ** 2 <= rs * rs
        free |= (xx - gx) ** 2 + (yy - gy) ** 2 <= rg * rg
        # per cell a byte whose bit s says that the move with chain code s is allowed
        allowed = np.bitwise_or.reduce(plan_allowed_moves(free).astype(np.uint8) << np.arange(8, dtype=np.uint8)[:, None, None],
                                       axis=0).tobytes()
        step = [(1 << s, PLAN_CODE_DY[s] * w + PLAN_CODE_DX[s], 3 if s & 1 else 2) for s in range(8)]
        dist = [PLAN_NONE] * (h * w)                # settled costs
        best = {(gy - y0) * w + gx - x0: 0}         # tentative costs
        heap = [(0, (gy - y0) * w + gx - x0)]
        too_long = False
        while heap:
            c, i = heapq.heappop(heap)
            if dist[i] != PLAN_NONE or best[i] != c:
                continue                            # (settled already, or a stale entry)
            if c > max_cost:
                too_long = True                     # a cell with a finite cost above max_cost: still to expand
                break
            dist[i] = c
            moves = allowed[i]
            for bit, di, dc in step:
                if moves & bit and dist[i + di] == PLAN_NONE and c + dc < best.get(i + di, 1 << 30):
                    best[i + di] = c + dc
                    heapq.heappush(heap, (c + dc, i + di))
        fields.append(np.array(dist, np.uint16).reshape(h, w))
        cur = (sy - y0) * w + sx - x0
        if dist[cur] == PLAN_NONE:
            results[n, 0] = PLAN_TOO_LONG if too_long else PLAN_UNREACHABLE
            continue
        cost, steps = dist[cur], 0
        while dist[cur] > 0 and steps < lookahead:
            for bit, di, dc in step:
                if allowed[cur] & bit and dist[cur + di] + dc == dist[cur]:
                    cur, steps = cur + di, steps + 1
                    break
            else:
                raise AssertionError("plan_paths_numpy: a settled cell without a predecessor")
        results[n] = (PLAN_OK, cost, cur % w + x0, cur // w + y0, steps)
    return results, fields


class MapPlannerController:
    """Steers by the map: every environment that has a finite goal and neither stops nor initialises plans a shortest path over
    its navigable plane (``obstacles.plan_paths``: ONE launch and ONE read-back for all of them) and walks towards the cell
    ``lookahead_m`` along it instead of towards the goal's bearing.  The waypoint's (rho, theta) in the robot frame (the
    expression of BatchedEpisodes._navigate) replace the goal's; they stay as they are where the plan is not PLAN_OK, and where
    the descent ends in the goal's own cell (the goal's bearing is exact there, the cell centre's is not).  The action is then
    ``inner``'s (default: BangBangController): the turn threshold and the detour after a refused move are that rule, stated
    once.  ``act`` without maps is ``inner.act``.

    ``last_status`` [E]: the plan status of each environment in the last ``act_on_map`` (-1: it did not plan), ``last_cost_m``
    [E]: cost * 0.5 / pixels_per_meter of the PLAN_OK ones (NaN otherwise; overstates pure diagonals by 6 %)."""

    def __init__(self, lookahead_m: float = 0.75, inner=None) -> None:
        self.lookahead_m = float(lookahead_m)
        self.inner = inner if inner is not None else BangBangController()
        self.last_status = self.last_cost_m = None

    def reset(self, envs=None) -> None:
        if hasattr(self.inner, "reset"):
            self.inner.reset(envs)

    def act(self, modes, rho_theta, stops, collided) -> np.ndarray:
        return self.inner.act(modes, rho_theta, stops, collided)

    def act_on_map(self, obstacles, poses, goals, goal_free_m, modes, rho_theta, stops, collided) -> np.ndarray:
        E = len(modes)
        poses = np.asarray(poses, np.float64).reshape(E, 3)
        goals = np.asarray(goals, np.float64).reshape(E, 2)
        rt = np.array(rho_theta, np.float64).reshape(E, 2)
        plan = np.isfinite(goals).all(axis=1) & ~np.asarray(stops, bool) & np.array([m != "initialize" for m in modes], bool)
        self.last_status, self.last_cost_m = np.full(E, -1, np.int64), np.full(E, np.nan)
        idx = np.flatnonzero(plan)
        if len(idx):
            gf = None
            if goal_free_m is not None:
                gf = np.array([np.nan if g is None else g for g in np.asarray(goal_free_m, object).reshape(E)], np.float64)[idx]
            out = obstacles.plan_paths(poses[idx, :2], goals[idx], env_ids=idx, goal_free_m=gf, lookahead_m=self.lookahead_m)
            status = np.asarray(out["status"], np.int64)
            self.last_status[idx] = status
            self.last_cost_m[idx] = np.where(status == PLAN_OK, out["path_m"], np.nan)
            use = (status == PLAN_OK) & ~np.asarray(out["at_goal"], bool)
            d = np.asarray(out["waypoints"], np.float64)[use] - poses[idx[use], :2]
            c, s = np.cos(-poses[idx[use], 2]), np.sin(-poses[idx[use], 2])
            lx, ly = c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]
            rt[idx[use]] = np.stack([np.hypot(lx, ly), np.arctan2(ly, lx)], axis=1)
        return self.inner.act(modes, rt, stops, collided)


# ---------------------------------------------------------------------------------------------- depth sensor
# What a depth CAMERA makes of the exact ranges the ray caster writes: axial noise, disparity quantisation, holes (single
# pixels, 8 x 8 blocks, silhouettes, out of range).  `depth_sensor_numpy` is the HOST STATEMENT of the rule; the device
# (csrc/depth_sensor.hip: vlfm_depth_sensor, behind RoomsRenderer.sense_depth) matches it bit for bit.  A frame is a pure
# function of (sensor, env_id, clock, clean frame): the randomness is `_mix32` of those, there is no generator state.
DEPTH_SENSOR_BLOCK = 8                                              # patch dropout: blocks of 8 x 8 pixels
DEPTH_SENSOR_NOISE_SCALE = np.float32(1.0 / np.sqrt(1431655765.0))  # 1 / std of a sum of four uniform 16-bit integers


@dataclass(frozen=True)
class DepthSensor:
    """The depth camera of ``LiveWorld(depth_sensor=...)`` / ``BatchedEpisodes(closed_loop=True, depth_sensor=...)``.  Every
    default means "this stage is off"; a ``DepthSensor()`` returns its input.

    ``sigma0_m``, ``sigma2_per_m``: axial noise of sigma(z) = sigma0 + sigma2 * z * z metres.  ``disparity_k`` > 0: z becomes
    k / rint(k / z), k = baseline x focal length x sub-pixel steps in metres.  ``dropout``: probability that a pixel is invalid,
    ``patch_dropout``: that an 8 x 8 block is (both within [0, 0.5]).  ``edge_m`` > 0: invalid where a 4-neighbour inside the frame
    differs by more than ``edge_m`` metres in the clean frame.  ``min_range_m``, ``max_range_m``: a clean z outside [min, max] is
    invalid (off at 0 and inf).  Negative or non-finite values are refused here, before any device is touched."""
    seed: int = 0
    sigma0_m: float = 0.0
    sigma2_per_m: float = 0.0
    disparity_k: float = 0.0
    dropout: float = 0.0
    patch_dropout: float = 0.0
    edge_m: float = 0.0
    min_range_m: float = 0.0
    max_range_m: float = float("inf")

    def __post_init__(self) -> None:
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or not 0 <= self.seed < 2 ** 32:
            raise ValueError("DepthSensor: seed must be an integer in [0, 2**32)")
        for name in ("sigma0_m", "sigma2_per_m", "disparity_k", "dropout", "patch_dropout", "edge_m", "min_range_m"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v) and v >= 0):
                raise ValueError(f"DepthSensor: {name} must be finite and not negative")
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"DepthSensor: {name} does not fit an f32")
        m = self.max_range_m
        if not (isinstance(m, (int, float, np.integer, np.floating)) and not np.isnan(m) and m >= 0):
            raise ValueError("DepthSensor: max_range_m must not be negative (inf: no limit)")
        for name in ("dropout", "patch_dropout"):
            if getattr(self, name) > 0.5:
                raise ValueError(f"DepthSensor: {name} must lie in [0, 0.5]")

    @property
    def computes(self) -> bool:
        """Noise or quantisation is on: a valid pixel is computed through metres instead of passed through."""
        return self.sigma0_m != 0 or self.sigma2_per_m != 0 or self.disparity_k != 0

    @property
    def range_on(self) -> bool:
        return self.min_range_m > 0 or self.max_range_m < np.inf

    def thresholds(self):
        """(T_drop, T_patch): a hash below T makes a pixel / a block invalid; T = min(int(p * 2**32), 2**32 - 1)."""
        return tuple(min(int(float(p) * 2.0 ** 32), 2 ** 32 - 1) for p in (self.dropout, self.patch_dropout))

    def frame_keys(self, env_ids, clocks) -> np.ndarray:
        """uint32 [n]: kf = _mix32(_mix32(seed, env_id, 51), clock, 52) of each frame (env_id and clock taken modulo 2**32)."""
        env_ids = np.asarray(env_ids, np.int64).reshape(-1)
        clocks = np.asarray(clocks, np.int64).reshape(-1)
        return np.array([_mix32(_mix32(int(self.seed), int(e) & 0xFFFFFFFF, 51), int(c) & 0xFFFFFFFF, 52)
                         for e, c in zip(env_ids, clocks)], np.uint32).reshape(-1)


def _mix32_array(a: int, b, salt: int) -> np.ndarray:
    """`_mix32(a, b[i], salt)` for an array ``b`` of values below 2**32: uint64 arithmetic, masked to 32 bits."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(b, np.uint64) * np.uint64(40503) + np.uint64((a * 2654435761 + salt * 97 + 0x9E3779B9) & 0xFFFFFFFF)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def depth_sensor_noise(kf: int, H: int, W: int) -> np.ndarray:
    """f32 [H,W]: the unit-variance noise nf of the frame with key ``kf`` -- per pixel the sum of the four 16-bit halves of two
    hashes, centred (- 131070) and scaled by DEPTH_SENSOR_NOISE_SCALE: mean 0, variance 1 by construction, |nf| <= 3.47."""
    p = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    h1, h2 = _mix32_array(kf, p, 53), _mix32_array(kf, p, 54)
    m16 = np.uint64(0xFFFF)
    n = ((h1 & m16) + (h1 >> np.uint64(16)) + (h2 & m16) + (h2 >> np.uint64(16))).astype(np.int64) - 131070
    return n.astype(np.float32) * DEPTH_SENSOR_NOISE_SCALE


def depth_sensor_numpy(clean, lo, hi, sensor: DepthSensor, env_id: int, clock: int):
    """(f32 [H,W], invalid pixel count): what ``sensor`` makes of the normalised frame ``clean`` [H,W] (as the ray caster writes
    it) of a camera with the range [lo, hi] metres, for environment ``env_id`` at sensor clock ``clock``.  Whole-array NumPy; all
    arithmetic is f32 with one rounding per operation, the expressions exactly as written here, no fused multiply-add.

      keys     kf = _mix32(_mix32(seed, env_id, 51), clock, 52); with p = r * W + u (u32):
               h1 = _mix32(kf, p, 53), h2 = _mix32(kf, p, 54), hd = _mix32(kf, p, 55),
               hb = _mix32(kf, (r >> 3) * ((W + 7) >> 3) + (u >> 3), 56)
      metres   span = hi - lo;  z = lo + d * span
      invalid  any of: the range stage is on (min_range > 0 or max_range < inf) and not (z >= min_range and z <= max_range) -- a
               NaN is invalid there; with the stage off nothing is compared and a NaN passes like any other value --;
               the edge stage is on and |z_n - z| > edge_m for a neighbour above, below, left or right inside the frame (a NaN
               difference is not greater: a NaN pixel invalidates no neighbour);  hd < T_drop;  hb < T_patch
               (`DepthSensor.thresholds`; T == 0: the stage is off and its hash is not evaluated).  An invalid pixel is 0.0f.
      noise    n = (h1 & 0xFFFF) + (h1 >> 16) + (h2 & 0xFFFF) + (h2 >> 16) - 131070;  nf = f32(n) * DEPTH_SENSOR_NOISE_SCALE;
               z1 = z + (sigma0 + sigma2 * (z * z)) * nf
      quantise (k > 0)  z1 = z1 < 1e-3f ? 1e-3f : z1;  m = rint(k / z1), half to even;  m = m < 1 ? 1 : m;  z1 = k / m
      output   v = (z1 - lo) / span;  v < 1e-3f ? 1e-3f : (v > 1 ? 1 : v)
               (the selects are max / clip for every number and keep a NaN a NaN, which pins what max and clip leave open)
      pass-through  with noise and quantisation both off (sigma0 == sigma2 == k == 0) a valid pixel is the INPUT value, bit for
               bit: the trip through metres is not the identity, so it is not made."""
    f = np.float32
    d = np.ascontiguousarray(clean, np.float32)
    if d.ndim != 2:
        raise ValueError("depth_sensor_numpy: clean must be [H,W]")
    H, W = d.shape
    lo, hi = f(lo), f(hi)
    span = f(hi - lo)
    t_drop, t_patch = sensor.thresholds()
    kf = int(sensor.frame_keys([env_id], [clock])[0])
    rows, cols = np.arange(H, dtype=np.uint64)[:, None], np.arange(W, dtype=np.uint64)[None, :]
    p = rows * np.uint64(W) + cols
    invalid = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        z = lo + d * span
        if sensor.range_on:
            invalid |= ~((z >= f(sensor.min_range_m)) & (z <= f(sensor.max_range_m)))
        if sensor.edge_m > 0:
            e = f(sensor.edge_m)
            dv, dh = np.abs(z[1:] - z[:-1]) > e, np.abs(z[:, 1:] - z[:, :-1]) > e
            invalid[1:] |= dv
            invalid[:-1] |= dv
            invalid[:, 1:] |= dh
            invalid[:, :-1] |= dh
        if t_drop:
            invalid |= _mix32_array(kf, p, 55) < np.uint64(t_drop)
        if t_patch:
            block = (rows >> np.uint64(3)) * np.uint64((W + 7) >> 3) + (cols >> np.uint64(3))
            invalid |= _mix32_array(kf, block, 56) < np.uint64(t_patch)
        if not sensor.computes:
            out = d
        else:
            z1 = z
            if sensor.sigma0_m != 0 or sensor.sigma2_per_m != 0:
                z1 = z + (f(sensor.sigma0_m) + f(sensor.sigma2_per_m) * (z * z)) * depth_sensor_noise(kf, H, W)
            if sensor.disparity_k > 0:
                k = f(sensor.disparity_k)
                z1 = np.where(z1 < f(1e-3), f(1e-3), z1)
                m = np.rint(k / z1)
                m = np.where(m < f(1.0), f(1.0), m)
                z1 = k / m
            v = (z1 - lo) / span
            out = np.where(v < f(1e-3), f(1e-3), np.where(v > f(1.0), f(1.0), v))
        out = np.where(invalid, f(0.0), out).astype(np.float32)
    return out, int(invalid.sum())


# ---------------------------------------------------------------------------------------------- depth filter
# What stands between the depth camera and every reader of its frames: the holes (zeros, NaN, negatives) are filled from the
# nearest valid pixels of their row and column.  `depth_filter_numpy` is the HOST STATEMENT of the rule; the device
# (csrc/depth_filter.hip: vlfm_depth_filter, behind utils.depth_filter.filter_depth_batch / RoomsRenderer.filter_depth) matches
# it bit for bit.  The rule is this project's own: it follows the contract of depth_camera_filtering.filter_depth as SURVEY B4
# words it, and claims no arithmetic parity with that library, whose source is pinned nowhere.
DEPTH_FILTER_MAX_REACH = 65535


@dataclass(frozen=True)
class DepthFilter:
    """The hole filling of ``LiveWorld(depth_filter=...)`` / ``BatchedEpisodes(closed_loop=True, depth_filter=...)`` and of
    ``utils.depth_filter.filter_depth_batch``.

    ``fill``: a hole becomes the farthest ("far", the maximum) or the nearest ("near", the minimum) of its candidates -- the
    nearest source pixel to its left, right, above and below.  ``reach_px``: a candidate counts only within that many steps (None:
    no limit).  ``clip_far_thresh`` > 0: a value above it is no source.  ``recover_nonzero``: every positive input pixel keeps its
    value (False: only the sources do; a clipped pixel becomes a hole).  ``set_black_value``: what a hole without a candidate
    becomes (None: 0.0).  Refused here, before any device is touched: anything else."""
    fill: str = "far"
    reach_px: Optional[int] = None
    clip_far_thresh: float = 0.0
    recover_nonzero: bool = True
    set_black_value: Optional[float] = None

    def __post_init__(self) -> None:
        if self.fill not in ("far", "near"):
            raise ValueError('DepthFilter: fill must be "far" or "near"')
        r = self.reach_px
        if r is not None and (isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= r <= DEPTH_FILTER_MAX_REACH):
            raise ValueError(f"DepthFilter: reach_px must be None or an integer in [1, {DEPTH_FILTER_MAX_REACH}]")
        c = self.clip_far_thresh
        if isinstance(c, bool) or not (isinstance(c, (int, float, np.integer, np.floating)) and np.isfinite(c) and c >= 0):
            raise ValueError("DepthFilter: clip_far_thresh must be finite and not negative")
        with np.errstate(over="ignore"):
            if not np.isfinite(np.float32(c)):
                raise ValueError("DepthFilter: clip_far_thresh does not fit an f32")
        if not isinstance(self.recover_nonzero, (bool, np.bool_)):
            raise ValueError("DepthFilter: recover_nonzero must be a bool")
        b = self.set_black_value
        if b is not None:
            if isinstance(b, bool) or not (isinstance(b, (int, float, np.integer, np.floating)) and np.isfinite(b)):
                raise ValueError("DepthFilter: set_black_value must be None or finite")
            with np.errstate(over="ignore"):
                if not np.isfinite(np.float32(b)):
                    raise ValueError("DepthFilter: set_black_value does not fit an f32")


def _nearest_source_before(frame: np.ndarray, src: np.ndarray, reach):
    """Along axis 1, towards lower indices: (value of the nearest ``src`` pixel at or before each pixel, whether there is one
    within ``reach`` steps).  Whole-array: a running maximum of the source indices."""
    cols = np.arange(frame.shape[1], dtype=np.int64)[None, :]
    last = np.maximum.accumulate(np.where(src, cols, -1), axis=1)
    ok = last >= 0
    if reach is not None:
        ok &= cols - last <= int(reach)
    return np.take_along_axis(frame, np.maximum(last, 0), axis=1), ok


def depth_filter_numpy(frame, flt: DepthFilter):
    """(f32 [H,W], filled, left): what ``flt`` makes of the frame ``frame`` [H,W].  Whole-array NumPy; values are only selected,
    never computed, so nothing depends on rounding.

      positive   pos = frame > 0 (NaN, +0.0, -0.0 and negatives are not)
      sources    src = pos, and with clip_far_thresh > 0 also not (frame > f32(clip_far_thresh)): a value equal to it stays one
      kept       keep = pos if recover_nonzero else src; a kept pixel leaves with its input bits, every other pixel is a hole
      candidates per direction left, right, up, down: the value of the nearest src pixel in that direction inside the frame, if
                 it is at most reach_px steps away (None: any distance).  They come from INPUT pixels only: a filled value never
                 feeds another fill
      fill       a hole with candidates becomes their maximum ("far") or minimum ("near"); one without becomes
                 set_black_value, else 0.0f
      counts     filled: the holes that had a candidate; left: those that had none (whatever they were then set to)"""
    f = np.float32
    d = np.ascontiguousarray(frame, np.float32)
    if d.ndim != 2:
        raise ValueError("depth_filter_numpy: frame must be [H,W]")
    if not isinstance(flt, DepthFilter):
        raise ValueError("depth_filter_numpy: flt must be a DepthFilter")
    with np.errstate(invalid="ignore"):
        pos = d > 0
        src = pos & ~(d > f(flt.clip_far_thresh)) if flt.clip_far_thresh > 0 else pos
    keep = pos if flt.recover_nonzero else src
    far = flt.fill == "far"
    best, has = np.zeros_like(d), np.zeros(d.shape, bool)
    views = (lambda a: a, lambda a: a[:, ::-1], lambda a: a.T, lambda a: a.T[:, ::-1])      # left, right, up, down
    for view in views:
        val, ok = _nearest_source_before(view(d), view(src), flt.reach_px)
        b, h = view(best), view(has)                                                        # (views: written through)
        better = ok & (~h | ((val > b) if far else (val < b)))
        b[better] = val[better]
        h |= ok
    hole = ~keep
    black = f(0.0) if flt.set_black_value is None else f(flt.set_black_value)
    out = np.where(keep, d, np.where(has, best, black)).astype(np.float32)
    return out, int((hole & has).sum()), int((hole & ~has).sum())
