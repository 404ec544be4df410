"""Seeded inputs for the depth-ingest edge tests (tests/test_depth_ingest_edges_cpu.py, tests/test_depth_ingest_edges_gpu.py) and
the HOST STATEMENT of the obstacle scatter.  No device is needed here.

Why a host statement next to the oracle: the oracle's ``apply_tf`` is ``np.dot`` (BLAS: its summation order and its use of FMA are
the BLAS build's), the kernel evaluates ``((t0 c0 + t1 c1) + t2 c2) + t3`` left to right with every operation rounded.  Under a
tilted camera the two differ in the last bit of many coordinates; a coordinate within an ulp of a cell boundary or a band edge
would make a GPU comparison depend on the BLAS build.  ``host_statement`` restates the scatter in elementwise NumPy in the kernel's
order; the CPU test asserts that statement and oracle set the same cells for EVERY input generated here (a condition on the inputs:
where they disagree the seed of the case is changed, never the texel), and the GPU tests then compare with the oracle alone.

Groups: A tilted cameras, B image shapes, C exact boundaries, D depth values, E a tilted rig, F refusal (see the GPU test)."""
import functools
from typing import NamedTuple

import numpy as np

from vlfm_amd.synthetic import CAMERA_HEIGHT, MAX_DEPTH, MIN_DEPTH, Trajectory, camera_intrinsics, depth_frame

OM_KW = dict(min_height=0.61, max_height=0.88, agent_radius=0.18, area_thresh=1.5)
SIDE = 300          # map side of groups A, B, D, E, F
PPM = 20
FILL_ALL = 100000   # the reference's default hole_area_thresh: larger than every hole of these frames


# ------------------------------------------------------------------------------------------------ the host statement
def patch_holes(depth, hole_thresh):
    """The reference's vlfm/mapping/obstacle_map.py:87-91: zero texels become 1.0 (all of them with -1, else those fill_small_holes covers)."""
    from oracle.ref_geometry import fill_small_holes

    if hole_thresh == -1:
        return np.where(depth == 0, np.float32(1.0), depth)
    return np.asarray(fill_small_holes(depth, hole_thresh), np.float32)


class Placed(NamedTuple):
    inband: np.ndarray   # [H, W] bool: texels that pass the depth mask and the height band
    rows: np.ndarray     # per in-band texel (row-major texel order): map row BEFORE the wrap
    cols: np.ndarray     # ... map column before the wrap
    x20: np.ndarray      # ... X * pixels_per_meter, the argument of rint for the row
    y20: np.ndarray      # ... Y * pixels_per_meter, the argument of rint for the column
    plane: np.ndarray    # [S, S] bool: the cells one frame sets in an empty map


def host_statement(depth, tf, min_depth, max_depth, fx, fy, min_height, max_height, size, hole_thresh=FILL_ALL, ppm=PPM,
                   place=True) -> Placed:
    """The reference's vlfm/mapping/obstacle_map.py:86-101 for one frame, elementwise (never ``np.dot`` / ``@``), every operation rounded once, in the order of
    csrc/depth_ingest.hip: f32 scaling, ``z < max_depth`` in f32, ``(u - W//2) z / fx`` in f64, the transform left to right, the
    inclusive band, rint half-to-even, NumPy's negative-index wrap; IndexError for a cell outside [-S, S) (``place=False``: no
    cells, no error -- only the in-band mask)."""
    d = np.asarray(patch_holes(np.asarray(depth, np.float32), hole_thresh), np.float32)
    H, W = d.shape
    z32 = d * np.float32(max_depth - min_depth) + np.float32(min_depth)
    v, u = np.nonzero(z32 < np.float32(max_depth))
    z = z32[v, u].astype(np.float64)
    x = (u - W // 2).astype(np.float64) * z / fx
    y = (v - H // 2).astype(np.float64) * z / fy
    c0, c1, c2 = z, -x, -y
    t = np.asarray(tf, np.float64)
    X = ((t[0, 0] * c0 + t[0, 1] * c1) + t[0, 2] * c2) + t[0, 3]
    Y = ((t[1, 0] * c0 + t[1, 1] * c1) + t[1, 2] * c2) + t[1, 3]
    Z = ((t[2, 0] * c0 + t[2, 1] * c1) + t[2, 2] * c2) + t[2, 3]      # (the reference's division by w = 1 changes nothing)
    band = (Z >= min_height) & (Z <= max_height)
    inband = np.zeros((H, W), bool)
    inband[v[band], u[band]] = True
    x20, y20 = X[band] * ppm, Y[band] * ppm
    rows = (np.rint(x20) + size // 2).astype(np.int64)
    cols = (size - (np.rint(y20) + size // 2)).astype(np.int64)
    plane = np.zeros((size, size), bool)
    if place:
        if ((rows < -size) | (rows >= size) | (cols < -size) | (cols >= size)).any():
            raise IndexError("host statement: obstacle point off the map")
        plane[rows % size, cols % size] = True
    return Placed(inband, rows, cols, x20, y20, plane)


def oracle_plane(depth, tf, min_depth, max_depth, fx, fy, size, hole_thresh=FILL_ALL, **kw):
    """The cells the oracle sets for one frame in an empty map (IndexError propagates)."""
    from oracle.ref_obstacle_map import RefObstacleMap

    args = dict(OM_KW)
    args.update(kw)
    ref = RefObstacleMap(hole_area_thresh=hole_thresh, size=size, **args)
    fov = 2 * np.arctan(depth.shape[1] / 2 / fx)
    ref.update_map(np.asarray(depth, np.float32).copy(), np.asarray(tf, np.float64), min_depth, max_depth, fx, fy, fov, explore=False)
    return ref._map.astype(bool)


def filled_texels(depth, hole_thresh):
    """[H, W] bool: texels the reference rewrites to 1.0 (probe image, as tests/test_obstacle_map_gpu.py reads it)."""
    from oracle.ref_geometry import fill_small_holes

    return fill_small_holes(np.where(depth == 0, 0, 0.5).astype(np.float32), hole_thresh) == 1


# ------------------------------------------------------------------------------------------------ cameras and frames
def camera_tf(x, y, h, yaw, pitch, roll):
    """R = Rz(yaw) Ry(pitch) Rx(roll) on the camera's (forward, left, up) axes, translation (x, y, h).  Positive pitch looks
    down: row 2 of R is (t8, t9, t10) = (-sin p, cos p sin r, cos p cos r)."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    R = np.zeros((3, 3))
    for i in range(3):              # elementwise products: the transform itself must not depend on a BLAS either
        for j in range(3):
            R[i, j] = sum(Rz[i, a] * sum(Ry[a, b] * Rx[b, j] for b in range(3)) for a in range(3))
    tf = np.eye(4)
    tf[:3, :3] = R
    tf[:3, 3] = (x, y, h)
    return tf


PITCH_30 = float(np.deg2rad(30.0))


def noise_frame(rng, H, W):
    """Uniform depth in [0.02, 1): texels fill the whole frustum, no zero."""
    return rng.uniform(0.02, 1.0, (H, W)).astype(np.float32)


def ring(d, cx, cy, r_out, r_in):
    yy, xx = np.mgrid[0:d.shape[0], 0:d.shape[1]]
    rr = (xx - cx) ** 2 + (yy - cy) ** 2
    d[(rr <= r_out ** 2) & (rr > r_in ** 2)] = 0.0
    return d


def zero_rects(rng, d, count=3):
    H, W = d.shape
    for _ in range(count):
        h, w = int(rng.integers(2, H // 6 + 3)), int(rng.integers(2, W // 6 + 3))
        r0, c0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        d[r0:r0 + h, c0:c0 + w] = 0.0
    return d


def ring_at_centroid(d, inband, r_in):
    """A zero ring (2 texels thick, whole inside the image) around the centroid of the in-band texels."""
    H, W = d.shape
    r_out = r_in + 2
    vs, us = np.nonzero(inband)
    cy = int(np.clip(int(round(vs.mean())) if len(vs) else H // 2, r_out + 1, H - r_out - 2))
    cx = int(np.clip(int(round(us.mean())) if len(us) else W // 2, r_out + 1, W - r_out - 2))
    return ring(d, cx, cy, r_out, r_in)


def island_ring(d, inband, r_in, need):
    """The ring of an island frame: ``ring_at_centroid`` where its inside holds ``need`` in-band texels; otherwise (a thin strip of
    in-band texels, or one along an image border, which a circle kept inside the image cannot enclose) a rectangular zero frame, one
    texel thick, of half-size r_in about the centroid and clipped to the image -- a side on the image border still closes it."""
    H, W = d.shape
    vs, us = np.nonzero(inband)
    cy, cx = (int(round(vs.mean())), int(round(us.mean()))) if len(vs) else (H // 2, W // 2)
    r_out = r_in + 2
    ccy, ccx = int(np.clip(cy, r_out + 1, H - r_out - 2)), int(np.clip(cx, r_out + 1, W - r_out - 2))
    yy, xx = np.mgrid[0:H, 0:W]
    if int((inband & ((xx - ccx) ** 2 + (yy - ccy) ** 2 <= r_in ** 2)).sum()) >= need:
        return ring(d, ccx, ccy, r_out, r_in)
    y0, y1, x0, x1 = max(cy - r_in, 0), min(cy + r_in, H - 1), max(cx - r_in, 0), min(cx + r_in, W - 1)
    d[[y0, y1], x0:x1 + 1] = 0.0
    d[y0:y1 + 1, [x0, x1]] = 0.0
    return d


def island_texels(depth, inband_clean, hole_thresh=FILL_ALL):
    """Valid in-band texels the reference drops because a filled contour covers them."""
    return filled_texels(depth, hole_thresh) & (depth != 0) & inband_clean


class Case(NamedTuple):
    name: str
    depth: np.ndarray
    tf: np.ndarray
    fx: float
    hole_thresh: int
    lo: float = MIN_DEPTH
    hi: float = MAX_DEPTH
    om_kw: dict = OM_KW
    size: int = SIDE

    def statement(self, place=True) -> Placed:
        return host_statement(self.depth, self.tf, self.lo, self.hi, self.fx, self.fx, self.om_kw["min_height"],
                              self.om_kw["max_height"], self.size, self.hole_thresh, place=place)

    def oracle(self):
        return oracle_plane(self.depth, self.tf, self.lo, self.hi, self.fx, self.fx, self.size, self.hole_thresh, **self.om_kw)


def statement_or_error(case):
    try:
        return case.statement().plane
    except IndexError:
        return "IndexError"


def oracle_or_error(case):
    try:
        return case.oracle()
    except IndexError:
        return "IndexError"


def agrees(case) -> bool:
    """The condition on every input: host statement and oracle set the same cells (or both raise IndexError)."""
    a, b = statement_or_error(case), oracle_or_error(case)
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str)
    return bool(np.array_equal(a, b))


# ------------------------------------------------------------------------------------------------ group A: tilted cameras
A_SHAPES = [(48, 64), (240, 424)]
A_MODES = ("clean", "minus1", "island")
_deg = np.deg2rad


def _a_angles():
    """(name, pitch, roll): fixed pitches, fixed rolls, and 16 seeded random combinations."""
    out = [(f"pitch{p:+d}", float(_deg(p)), 0.0) for p in (10, -10, 30, -30, 60, -60)]
    out.append(("pitch+90", float(np.pi / 2), 0.0))                  # straight down: sin(pi/2) == 1.0, t8 == -1 exactly
    out += [(f"roll{r:+d}", 0.0, float(_deg(r))) for r in (15, -15)]
    out.append(("roll+90", 0.0, float(np.pi / 2)))                   # a camera on its side: t9 == 1, t10 ~ 6e-17
    out.append(("roll180", 0.0, float(np.pi)))
    rng = np.random.default_rng(4100)
    out += [(f"random{k:02d}", float(rng.uniform(-1.6, 1.6)), float(rng.uniform(-np.pi, np.pi))) for k in range(16)]
    return out


A_ANGLES = _a_angles()
A_NAMES = [a[0] for a in A_ANGLES]
A_ROLLED = [a[0] for a in A_ANGLES if abs(np.cos(a[1]) * np.sin(a[2])) > 0.15]       # cases whose t9 is far from zero
A_STEEP = 0.6       # |pitch| above this (rad): the camera gets noise frames.  A steep camera sees the 0.61-0.88 m band only at short range,
                    # where a ``depth_frame`` wall (>= 1 m) has nothing; 14 of the 27 cameras are steep: half noise, half ``depth_frame``
A_MIN_INBAND, A_MIN_ISLAND = 200, 20
# The five cameras pitched UP by more than 1 rad (A_ANGLES: -1.05 .. -1.24): every ray of a 48x64 image rises, the band is met only by the nearest texels of the
# lowest rows of a low camera, and the best of seeds 0..2999 gives 91, 63, 70, 55 and 55 in-band texels of 3072.  Their 48x64 frames are
# excepted from the two counts (they keep the floors below); their 240x424 frames are not.
A_UPWARD = ("pitch-60", "random00", "random13", "random14", "random15")
A_UPWARD_MIN_INBAND, A_UPWARD_MIN_ISLAND = 40, 4
# Per (camera, image height) the smallest seed >= 0 for which the CPU test's conditions hold FOR THAT FRAME (host statement == oracle
# in all three hole modes, no cell off the 300-cell map, >= 200 in-band texels in the clean frame, >= 20 in-band valid texels inside
# the island frame's ring; for the excepted frames the floors above): searched once, asserted by the CPU test.  0 where not listed.
A_SEEDS = {('pitch+30', 48): 1, ('pitch-30', 48): 1, ('pitch-30', 240): 2, ('pitch+60', 48): 45, ('pitch+60', 240): 7, ('pitch-60', 48): 8,
           ('pitch-60', 240): 7, ('pitch+90', 48): 674, ('pitch+90', 240): 1, ('random00', 48): 50, ('random00', 240): 2, ('random04', 240): 2,
           ('random05', 48): 224, ('random05', 240): 3, ('random07', 48): 138, ('random08', 48): 2, ('random08', 240): 3, ('random09', 48): 402,
           ('random09', 240): 1, ('random10', 48): 3, ('random11', 48): 4, ('random13', 48): 6, ('random13', 240): 3, ('random14', 48): 11,
           ('random14', 240): 1, ('random15', 48): 67, ('random15', 240): 55}


def a_kind(name) -> str:
    return "noise" if abs(A_ANGLES[A_NAMES.index(name)][1]) > A_STEEP else "profile"


def a_minimum(name, H):
    """(in-band texels, island texels) a frame of group A must hold."""
    return (A_UPWARD_MIN_INBAND, A_UPWARD_MIN_ISLAND) if name in A_UPWARD and H == 48 else (A_MIN_INBAND, A_MIN_ISLAND)


def a_frame(name, shape, seed=None):
    """{mode: Case} for one tilted camera and one image shape: height in [0.3, 1.5] m, position within +-3 m, any yaw (each frame
    has its own pose and seed; the angles are the camera's)."""
    k = A_NAMES.index(name)
    _, pitch, roll = A_ANGLES[k]
    H, W = shape
    seed = A_SEEDS.get((name, H), 0) if seed is None else seed
    rng = np.random.default_rng([41, k, H, seed])
    tf = camera_tf(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0.3, 1.5), rng.uniform(-np.pi, np.pi), pitch, roll)
    base = noise_frame(rng, H, W) if a_kind(name) == "noise" else depth_frame(rng, H, W)
    fx = camera_intrinsics(W)[0]
    clean = Case(f"{name}-{H}x{W}-clean", base, tf, fx, FILL_ALL)
    inband = clean.statement(place=False).inband
    holed = zero_rects(rng, base.copy())
    isl = island_ring(zero_rects(rng, base.copy()), inband, max(8, H // 5), a_minimum(name, H)[1])
    return {"clean": clean, "minus1": Case(f"{name}-{H}x{W}-minus1", holed, tf, fx, -1),
            "island": Case(f"{name}-{H}x{W}-island", isl, tf, fx, FILL_ALL)}


def a_case(name):
    """{mode: [Case 48x64, Case 240x424]} for one tilted camera."""
    frames = [a_frame(name, shape) for shape in A_SHAPES]
    return {m: [f[m] for f in frames] for m in A_MODES}


def a_frame_counts(frame):
    """(in-band texels of the clean frame, in-band valid texels the island frame's filled contours cover)."""
    inband = frame["clean"].statement(place=False).inband
    return int(inband.sum()), int(island_texels(frame["island"].depth, inband).sum())


def a_frame_ok(name, shape, frame) -> bool:
    """The per-frame conditions of group A (used by the seed search and asserted, one by one, by the CPU test)."""
    n, isl = a_frame_counts(frame)
    lo_n, lo_isl = a_minimum(name, shape[0])
    if n < lo_n or isl < lo_isl:
        return False
    return all(not isinstance(oracle_or_error(c), str) and agrees(c) for c in frame.values())


TRAJ_STEPS = 24
TRAJ_SEED = 0       # asserted by the CPU test: host statement == oracle on every frame, at most 2 steps skipped by the tie guard


def a_trajectory(seed=None):
    """24 steps of ``Trajectory`` (kept within +-2 m so that 5 m of range stays on the 300-cell map) for a camera pitched 30 degrees
    down at the usual height; 240x424 ``depth_frame`` images."""
    seed = TRAJ_SEED if seed is None else seed
    traj = Trajectory(seed, limit=2.0)
    rng = np.random.default_rng([42, seed])
    fx = camera_intrinsics(424)[0]
    out = []
    for _ in range(TRAJ_STEPS):
        x, y, yaw = traj.step()
        out.append(Case("trajectory", depth_frame(rng, 240, 424), camera_tf(x, y, CAMERA_HEIGHT, yaw, PITCH_30, 0.0), fx, FILL_ALL))
    return out


# ------------------------------------------------------------------------------------------------ group B: image shapes
B_SHAPES = [(1, 4), (7, 36), (15, 124), (16, 128), (17, 132), (33, 260), (240, 424), (480, 848)]
B_THRESH = {"all": FILL_ALL, "some": 8, "minus1": -1}     # 8: single-texel-wide holes are filled (area 0), blobs and rings are not
B_CAMERAS = {"level": 0.0, "pitched": PITCH_30}


def b_camera(H, W, cam, seed=0):
    rng = np.random.default_rng([43, H, W, list(B_CAMERAS).index(cam), seed])
    return rng, camera_tf(rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), CAMERA_HEIGHT, rng.uniform(-np.pi, np.pi), B_CAMERAS[cam], 0.0)


def b_patterns(H, W):
    """Names of the zero patterns that fit the shape; 480x848 runs them combined in one frame only."""
    if (H, W) == (480, 848):
        return ["combined"]
    names = ["right_blob"] + (["seam"] if W > 36 else []) + ["last_col", "last_row"] + (["ring"] if H >= 15 else [])
    return names + ["combined"]


def b_zero(d, name, inband):
    H, W = d.shape
    if name in ("right_blob", "combined"):      # touches the right border, inside the (partial) last word
        d[H // 3:H // 3 + 4, max(W - 5, 0):] = 0.0
    if name in ("seam", "combined") and W > 36:  # across columns 31 | 32
        d[max(H // 2 - 2, 0):H // 2 + 2, 29:35] = 0.0
    if name in ("last_col", "combined"):
        d[H // 4:H // 4 + max(1, H // 3), W - 1] = 0.0
    if name in ("last_row", "combined"):
        d[H - 1, W // 5:W // 5 + max(1, W // 4)] = 0.0
        if H >= 3:
            d[H - 3:, 1:3] = 0.0
    if name in ("ring", "combined") and H >= 15:
        ring_at_centroid(d, inband, max(4, min(H // 5, 40, (H - 7) // 2)))
    return d


def b_frames(H, W, cam, thresh_name):
    """[Case] for one shape, camera and threshold: one frame per zero pattern (noise and ``depth_frame`` alternate)."""
    rng, tf = b_camera(H, W, cam)
    fx = camera_intrinsics(W)[0]
    out = []
    for k, name in enumerate(b_patterns(H, W)):
        base = noise_frame(rng, H, W) if k % 2 == 0 else depth_frame(rng, H, W)
        inband = Case("", base, tf, fx, FILL_ALL).statement(place=False).inband
        out.append(Case(f"{H}x{W}-{cam}-{thresh_name}-{name}", b_zero(base.copy(), name, inband), tf, fx, B_THRESH[thresh_name]))
    return out


def b_cameras_of(H, W, thresh_name):
    """Both cameras for every shape but the largest, which runs once per threshold (cameras alternate)."""
    if (H, W) == (480, 848):
        return ["level"] if thresh_name == "some" else ["pitched"]
    return list(B_CAMERAS)


BATCH_SHAPE = (33, 260)
BATCH_DISTINCT = 50
BATCH_SIZES = (1, 5, 700)
BATCH_SEED = 0


def launch_bands(n, H, W):
    """Row bands of the ingest launch (csrc/depth_ingest.hip, vlfm_depth_ingest_batched), restated: 128 columns per workgroup in
    x, about 2048 workgroups wanted, never more bands than 16-row groups."""
    gx = -(-(W // 4) // 32)
    return max(1, min(-(-2048 // (n * gx)), -(-H // 16)))


@functools.lru_cache(maxsize=None)
def b_batch_cases(thresh, seed=None):
    """50 distinct (frame, camera) pairs at 33x260 -- clean, rectangles, island in turn; level, pitched and rolled cameras -- which a
    batch of n slots cycles through (slot i holds pair i % 50: the oracle runs 50 times whatever n)."""
    seed = BATCH_SEED if seed is None else seed
    H, W = BATCH_SHAPE
    fx = camera_intrinsics(W)[0]
    out = []
    for j in range(BATCH_DISTINCT):
        rng = np.random.default_rng([44, j, seed])
        pitch, roll = [(0.0, 0.0), (PITCH_30, 0.0), (0.0, float(_deg(15)))][j % 3]
        tf = camera_tf(rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), CAMERA_HEIGHT, rng.uniform(-np.pi, np.pi), pitch, roll)
        base = noise_frame(rng, H, W) if j % 2 else depth_frame(rng, H, W)
        kind = (j // 3) % 3
        if kind == 1:
            zero_rects(rng, base)
        elif kind == 2:
            inband = Case("", base, tf, fx, FILL_ALL).statement(place=False).inband
            ring_at_centroid(zero_rects(rng, base, 1), inband, 6)
        out.append(Case(f"batch{j:02d}", base, tf, fx, thresh))
    return out


def colmax_frames(H, W, count):
    """Frames for the column maxima: positive, entirely negative, mixed signs, a wide dynamic range; no NaN, no zero of either sign."""
    out = []
    for j in range(count):
        rng = np.random.default_rng([45, H, W, j])
        d = rng.uniform(0.02, 1.0, (H, W)).astype(np.float32)
        kind = j % 4
        if kind == 1:
            d = -d
        elif kind == 2:
            d = d * rng.choice(np.array([-1.0, 1.0], np.float32), (H, W))
        elif kind == 3:
            d = (d * np.float32(2.0) ** rng.integers(-120, 120, (H, W)).astype(np.float32) *
                 rng.choice(np.array([-1.0, 1.0], np.float32), (H, W))).astype(np.float32)
        out.append(np.ascontiguousarray(d, np.float32))
    return np.stack(out)


def decode_keys(keys):
    """Inverse of the order-preserving key of csrc/depth_ingest.hip (f32_key): a non-negative float has its sign bit set in the
    key, a negative one is complemented."""
    k = np.asarray(keys).view(np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return bits.view(np.float32)


# ------------------------------------------------------------------------------------------------ group C: exact boundaries
C_SIDE, C_F, C_LO, C_HI, C_SHAPE = 96, 64.0, 0.0, 4.0, (40, 64)
C_WIDE = dict(OM_KW, min_height=-10.0, max_height=10.0)


def c_tf(diag=(1.0, 1.0, 1.0), t=(0.0, 0.0, 1.0)):
    tf = np.eye(4)
    tf[0, 0], tf[1, 1], tf[2, 2] = diag
    tf[:3, 3] = t
    return tf


C_BAND = (0.5, 0.875)
C_BAND_INSIDE = (float(np.nextafter(0.5, 1.0)), float(np.nextafter(0.875, 0.0)))
C_EDGE_ROWS = (24, 36)      # v - 20 = 4 -> Z = 0.875, v - 20 = 16 -> Z = 0.5


def c_band_cases(band):
    """tf = I at height 1.0, d = 0.5 -> z = 2, Z = 1 - (v - 20)/32 exactly.  "all": every texel at 0.5; "row24" / "row36": only that
    row at 0.5, the rest at 1.0 (masked) -- every row sets the same 40 cells, so only a frame that holds nothing but an edge row can
    show in the planes whether the edge row was placed."""
    H, W = C_SHAPE
    kw = dict(OM_KW, min_height=band[0], max_height=band[1])
    out = {"all": np.full((H, W), 0.5, np.float32)}
    for v in C_EDGE_ROWS:
        d = np.ones((H, W), np.float32)
        d[v] = 0.5
        out[f"row{v}"] = d
    tag = "band" if tuple(band) == C_BAND else "shrunk"
    return {k: Case(f"{tag}-{k}", d, c_tf(), C_F, FILL_ALL, C_LO, C_HI, kw, C_SIDE) for k, d in out.items()}


C_TIE_TFS = {"pos": c_tf((1.0, 1.0, 1.0)), "neg": c_tf((-1.0, -1.0, 1.0)),
             "pos_shifted": c_tf((1.0, 1.0, 1.0), (-2.0, 0.0, 1.0)), "neg_shifted": c_tf((-1.0, -1.0, 1.0), (2.0, 0.0, 1.0)),
             "col_pos": np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]]),
             "col_neg": np.array([[0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]])}


def c_tie_case(name):
    """Column u holds z = 0.125 (2 j + 1), j = u mod J: z * 20 = 5 j + 2.5 is exactly k + 0.5 with k of both parities.  J keeps
    every row on the 96-cell map (9 for the unshifted positive transform: z <= 2.125; 16 otherwise: z <= 3.875 < max_depth)."""
    H, W = C_SHAPE
    J = 9 if name == "pos" else 16
    j = np.arange(W) % J
    d = np.broadcast_to(((2 * j + 1) / 32.0).astype(np.float32), (H, W)).copy()     # d * 4 = z, exact
    return Case(f"tie-{name}", d, C_TIE_TFS[name], C_F, FILL_ALL, C_LO, C_HI, C_WIDE, C_SIDE)


def exact_ties(case):
    """(positive, negative) counts of in-band texels whose row or column argument of rint is exactly k + 0.5."""
    p = case.statement()
    a = np.concatenate([p.x20, p.y20])
    tie = a - np.floor(a) == 0.5
    return int((tie & (a > 0)).sum()), int((tie & (a < 0)).sum())


C_TARGETS = {"m1": -1, "mS": -C_SIDE, "mS1": -C_SIDE - 1, "S1": C_SIDE - 1, "S": C_SIDE}
C_RAISES = ("mS1", "S")
C_PATHS = ("clean", "zeros", "island")


def c_wrap_case(axis, target, path):
    """Only image column 32 (x = 0) is unmasked, at d = 0.5 (z = 2): every texel lands on ONE cell, X = 2 + tx, Y = ty.  The
    translation puts that cell's row (``axis`` 0) or column (1) on the target and the other coordinate on 10.  ``path``: no zero
    texel; a solid zero block (no island: the fill kernel promotes the speculative pass's note); a zero ring around in-band texels of
    column 32 (an island frame: the hole scatter places the surviving texels and raises itself)."""
    H, W = C_SHAPE
    S, t = C_SIDE, C_TARGETS[target]
    row, col = (t, 10) if axis == 0 else (10, t)
    tx = (row - S // 2) / PPM - 2.0          # row = rint((2 + tx) 20) + S/2
    ty = (S // 2 - col) / PPM                # col = S - (rint(ty 20) + S/2)
    d = np.ones((H, W), np.float32)
    d[:, 32] = 0.5
    if path == "zeros":
        d[3:7, 4:10] = 0.0
    elif path == "island":
        ring(d, 32, 20, 6, 4)
    return Case(f"wrap-{'row' if axis == 0 else 'col'}-{target}-{path}", d, c_tf(t=(tx, ty, 1.0)), C_F, FILL_ALL, C_LO, C_HI,
                C_WIDE, C_SIDE)


def c_ordinary_case():
    rng = np.random.default_rng(46)
    return Case("wrap-ordinary", rng.uniform(0.05, 0.45, C_SHAPE).astype(np.float32), c_tf(), C_F, FILL_ALL, C_LO, C_HI, C_WIDE, C_SIDE)


# ------------------------------------------------------------------------------------------------ group D: depth values
D_MODES = ("fill", "minus1", "island")
D_SPECIALS = (np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0.0)), np.float32(2.0 ** -149), np.float32(0.0),
              np.float32(-0.0))


def d_case(cam, mode):
    """48x64 noise frame with 6 texels each of 1.0 (masked), the float below 1 (kept), the smallest subnormal (not a hole), +0 and -0
    (both holes), on in-band texels where there are enough of them."""
    H, W = 48, 64
    rng, tf = b_camera(H, W, cam)
    fx = camera_intrinsics(W)[0]
    d = noise_frame(rng, H, W)
    inband = Case("", d, tf, fx, FILL_ALL).statement(place=False).inband
    if mode == "island":
        ring_at_centroid(d, inband, 9)
    spots = np.flatnonzero(inband & (d != 0))
    spots = rng.permutation(spots)[:30]
    spots = np.concatenate([spots, rng.permutation(H * W)[:30 - len(spots)]])
    for k, value in enumerate(D_SPECIALS):
        d.reshape(-1)[spots[6 * k:6 * k + 6]] = value
    return Case(f"values-{cam}-{mode}", d, tf, fx, -1 if mode == "minus1" else FILL_ALL)


# ------------------------------------------------------------------------------------------------ group E: a tilted rig
E_SLOTS, E_STEPS, E_SEED = 2, 6, 0
E_CAMERAS = ((0.0, 0.0), (PITCH_30, 0.0), (0.0, float(np.pi / 2)))      # level, pitched 30 degrees down, rolled 90 degrees


def e_steps(seed=None):
    """[steps][observations in call order] of (slot, Case) for 2 robots x 3 body cameras (same position, yaw offsets of +-0.15 rad so
    that the cameras see common cells), 48x64 frames of the kinds of rig_cases.ObstacleRig: clean, rectangles, island; and per step
    {slot: reveal pose}."""
    from rig_cases import interleave

    seed = E_SEED if seed is None else seed
    rng = np.random.default_rng([47, seed])
    H, W = 48, 64
    fx = camera_intrinsics(W)[0]
    pose = {s: np.array([*rng.uniform(-1.0, 1.0, 2), rng.uniform(-np.pi, np.pi)]) for s in range(E_SLOTS)}
    steps = []
    for _ in range(E_STEPS):
        per_slot, reveal = {}, {}
        for s in range(E_SLOTS):
            p = pose[s]
            p[:2] = np.clip(p[:2] + rng.uniform(-0.2, 0.2, 2), -1.5, 1.5)
            p[2] += rng.uniform(-0.3, 0.3)
            reveal[s] = camera_tf(p[0], p[1], CAMERA_HEIGHT, p[2], 0.0, 0.0)
            obs = []
            for (pitch, roll), off in zip(E_CAMERAS, (-0.15, 0.0, 0.15)):
                tf = camera_tf(p[0], p[1], CAMERA_HEIGHT, p[2] + off, pitch, roll)
                d = noise_frame(rng, H, W)
                kind = int(rng.integers(0, 3))
                if kind == 1:
                    zero_rects(rng, d)
                elif kind == 2:
                    inband = Case("", d, tf, fx, FILL_ALL).statement(place=False).inband
                    ring_at_centroid(d, inband, 9)
                obs.append((s, Case(f"rig-slot{s}-kind{kind}", d, tf, fx, FILL_ALL)))
            per_slot[s] = obs
        steps.append((interleave(rng, per_slot), reveal))
    return steps


def e_undo_steps(steps):
    """Number of steps in which an island frame's SPECULATIVE placement (every non-zero texel, i.e. the -1 rule) and a sibling frame of
    the same slot set a common cell that the slot's map did not hold before the step: the sibling finds the bit set, journals
    nothing, and the island frame's undo takes it -- what the device's per-slot "undone" flag repairs."""
    maps = {s: np.zeros((SIDE, SIDE), bool) for s in range(E_SLOTS)}
    hits = 0
    for obs, _ in steps:
        found = False
        for s in range(E_SLOTS):
            frames = [c for slot, c in obs if slot == s]
            finals = [c.statement().plane for c in frames]
            for i, c in enumerate(frames):
                if not (filled_texels(c.depth, c.hole_thresh) & (c.depth != 0)).any():
                    continue
                spec = c._replace(hole_thresh=-1).statement().plane & ~maps[s]
                found |= any((spec & finals[k]).any() for k in range(len(frames)) if k != i)
            for f in finals:
                maps[s] |= f
        hits += found
    return hits


# ------------------------------------------------------------------------------------------------ group F: refusal
def f_cases():
    """(an ordinary 48x64 frame, a 48x62 frame the ingest refuses, a 48x64 island frame), one pitched camera."""
    rng, tf = b_camera(48, 64, "pitched", 7)
    fx = camera_intrinsics(64)[0]
    first = noise_frame(rng, 48, 64)
    odd = noise_frame(rng, 48, 62)
    last = noise_frame(rng, 48, 64)
    inband = Case("", last, tf, fx, FILL_ALL).statement(place=False).inband
    ring_at_centroid(last, inband, 9)
    return [Case(n, d, tf, fx, FILL_ALL) for n, d in (("refusal-first", first), ("refusal-odd", odd), ("refusal-island", last))]
