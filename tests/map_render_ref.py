"""Test-side restatement of the reference's map images (not a test module).

* cv2 stand-ins for the entry points ValueMap.visualize / ObstacleMap.visualize / TrajectoryVisualizer need and
  oracle/ref_shim.py does not plant (applyColorMap(INFERNO), line, circle with any thickness on 1- or 3-channel images,
  flip, cvtColor(BGR2RGB)); ``plant(cv2)`` puts them on the shim's cv2 module for one test (the autouse fixture of
  tests/conftest.py removes the whole module again).
* A NumPy renderer over host snapshots (value array, planes, trajectory, markers) that follows the reference's drawing
  order, built on the same primitives.

Rasterisation: filled circles and two-point thick lines are oracle/cvport.c's (the facade's ``circle`` / ``polylines``);
the thick circle outline (EllipseEx -> ellipse2Poly -> PolyLine(shift=16) -> ThickLine -> FillConvexPoly + Line2) and
the midpoint outline are restated below from OpenCV 4.5.5's drawing.cpp rules.
"""
import os
import re

import numpy as np

from oracle import cv as ocv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT


def hip_lut() -> np.ndarray:
    """The 256 x 3 BGR table embedded in vlfm_amd/csrc/map_render.hip."""
    src = open(os.path.join(ROOT, "vlfm_amd", "csrc", "map_render.hip")).read()
    body = src[src.index("kInfernoBGR[256][3] = {"):]
    body = body[:body.index("};")]
    vals = [int(v) for v in re.findall(r"\d+", body[body.index("{") + 1:])]
    return np.array(vals, np.uint8).reshape(256, 3)


def matplotlib_lut() -> np.ndarray:
    """round(255 * f32(matplotlib inferno)) in BGR: what OpenCV 4.5.5's COLORMAP_INFERNO table holds."""
    import matplotlib._cm_listed as cm

    d = np.array(cm._inferno_data, np.float64).astype(np.float32)
    return np.rint(d * np.float32(255)).astype(np.uint8)[:, ::-1].copy()


LUT = None


def lut() -> np.ndarray:
    global LUT
    if LUT is None:
        LUT = hip_lut()
    return LUT


# ------------------------------------------------------------------------------------------------ rasterisation (masks)
def _clip_line(w, h, x1, y1, x2, y2):
    right, bottom = w - 1, h - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def _cdiv(a, b):   # C integer division (toward zero)
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _line2(m, x1, y1, x2, y2):
    rows, cols = m.shape
    ok, x1, y1, x2, y2 = _clip_line(cols << XY_SHIFT, rows << XY_SHIFT, x1, y1, x2, y2)
    if not ok:
        return

    def put(x, y):
        if 0 <= x < cols and 0 <= y < rows:
            m[y, x] = 1

    dx, dy = x2 - x1, y2 - y1
    horizontal = abs(dx) > abs(dy)
    if horizontal:
        if dx < 0:
            x1, y1, x2, y2 = x2, y2, x1, y1
        y_step = _cdiv((y2 - y1) << XY_SHIFT, abs(dx) | 1)
        ecount = (x2 - x1) >> XY_SHIFT
    else:
        if dy < 0:
            x1, y1, x2, y2 = x2, y2, x1, y1
        x_step = _cdiv((x2 - x1) << XY_SHIFT, abs(dy) | 1)
        ecount = (y2 - y1) >> XY_SHIFT
    x1 += XY_ONE >> 1
    y1 += XY_ONE >> 1
    put((x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT)
    if horizontal:
        x1 >>= XY_SHIFT
        while ecount >= 0:
            put(x1, y1 >> XY_SHIFT)
            x1 += 1
            y1 += y_step
            ecount -= 1
    else:
        y1 >>= XY_SHIFT
        while ecount >= 0:
            put(x1 >> XY_SHIFT, y1)
            x1 += x_step
            y1 += 1
            ecount -= 1


def _fill_convex_poly16(m, v):
    """FillConvexPoly(shift = XY_SHIFT, LINE_8) of 16.16 points."""
    rows, cols = m.shape
    npts, shift = len(v), XY_SHIFT
    delta = 1 << shift >> 1
    xs = [int(p[0]) for p in v]
    ys = [int(p[1]) for p in v]
    imin = 0
    xmin = xmax = xs[0]
    ymin = ymax = ys[0]
    p0 = (xs[-1], ys[-1])
    for i in range(npts):
        if ys[i] < ymin:
            ymin, imin = ys[i], i
        ymax = max(ymax, ys[i])
        xmax = max(xmax, xs[i])
        xmin = min(xmin, xs[i])
        _line2(m, p0[0], p0[1], xs[i], ys[i])
        p0 = (xs[i], ys[i])
    xmin, xmax = (xmin + delta) >> shift, (xmax + delta) >> shift
    ymin, ymax = (ymin + delta) >> shift, (ymax + delta) >> shift
    if npts < 3 or xmax < 0 or ymax < 0 or xmin >= cols or ymin >= rows:
        return
    ymax = min(ymax, rows - 1)
    edge = [dict(idx=imin, di=1, x=-XY_ONE, dx=0, ye=ymin), dict(idx=imin, di=npts - 1, x=-XY_ONE, dx=0, ye=ymin)]
    y = ymin
    edges = npts
    while True:
        for e in edge:
            if y >= e["ye"]:
                idx0, di = e["idx"], e["di"]
                idx = idx0 + di
                if idx >= npts:
                    idx -= npts
                while True:
                    edges -= 1
                    if edges < 0:
                        break
                    ty = (ys[idx] + delta) >> shift
                    if ty > y:
                        e["ye"] = ty
                        e["dx"] = _cdiv((xs[idx] - xs[idx0]) * 2 + (ty - y), 2 * (ty - y))
                        e["x"] = xs[idx0]
                        e["idx"] = idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= npts:
                        idx -= npts
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if edge[0]["x"] > edge[1]["x"] else (0, 1)
            x1 = (edge[left]["x"] + (XY_ONE >> 1)) >> XY_SHIFT
            x2 = (edge[right]["x"] + (XY_ONE >> 1)) >> XY_SHIFT
            if x2 >= 0 and x1 < cols:
                m[y, max(x1, 0):min(x2, cols - 1) + 1] = 1
        edge[0]["x"] += edge[0]["dx"]
        edge[1]["x"] += edge[1]["dx"]
        y += 1
        if y > ymax:
            break


def _thick_line16(m, p0, p1, thickness, flags):
    """ThickLine(thickness > 1, LINE_8) between 16.16 points."""
    dx = (p0[0] - p1[0]) / XY_ONE
    dy = (p1[1] - p0[1]) / XY_ONE
    r = dx * dx + dy * dy
    odd = thickness & 1
    th = thickness << (XY_SHIFT - 1)
    if abs(r) > np.finfo(np.float64).eps:
        r = (th + odd * XY_ONE * 0.5) / np.sqrt(r)
        dpx, dpy = int(np.rint(dy * r)), int(np.rint(dx * r))
        _fill_convex_poly16(m, [(p0[0] + dpx, p0[1] + dpy), (p0[0] - dpx, p0[1] - dpy), (p1[0] - dpx, p1[1] - dpy),
                                (p1[0] + dpx, p1[1] + dpy)])
    for i in range(2):
        if flags & (i + 1):
            ocv.lib().cvp_circle_fill(m, m.shape[0], m.shape[1], (p0[0] + (XY_ONE >> 1)) >> XY_SHIFT,
                                      (p0[1] + (XY_ONE >> 1)) >> XY_SHIFT, (th + (XY_ONE >> 1)) >> XY_SHIFT, 1)
        p0 = p1


def circle_mask(shape, center, radius, thickness) -> np.ndarray:
    """cv2.circle(mask, center, radius, 1, thickness) on a zero uint8 mask (drawing.cpp: circle)."""
    m = np.zeros(shape, np.uint8)
    cx, cy, radius = int(center[0]), int(center[1]), int(radius)
    assert radius >= 0
    if thickness > 1:
        v = ocv.ellipse_polygon((cx, cy), (radius, radius), 0, 0, 360)   # EllipseEx's 16.16 vertices
        for i in range(1, len(v)):                                        # PolyLine(is_closed = false)
            _thick_line16(m, (int(v[i - 1][0]), int(v[i - 1][1])), (int(v[i][0]), int(v[i][1])), int(thickness),
                          3 if i == 1 else 2)
    elif thickness < 0:
        ocv.lib().cvp_circle_fill(m, shape[0], shape[1], cx, cy, radius, 1)
    else:                                                                 # midpoint outline
        err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
        while dx >= dy:
            for x, y in ((cx - dx, cy - dy), (cx + dx, cy - dy), (cx - dx, cy + dy), (cx + dx, cy + dy),
                         (cx - dy, cy - dx), (cx + dy, cy - dx), (cx - dy, cy + dx), (cx + dy, cy + dx)):
                if 0 <= x < shape[1] and 0 <= y < shape[0]:
                    m[y, x] = 1
            dy += 1
            err += plus
            plus += 2
            mask = (err <= 0) - 1
            err -= minus & mask
            dx += mask
            minus -= 2 & mask
    return m


def line_mask(shape, p0, p1, thickness) -> np.ndarray:
    """cv2.line(mask, p0, p1, 1, thickness >= 2) == the facade's two-point polylines (ThickLine flags 3)."""
    m = np.zeros(shape, np.uint8)
    assert thickness >= 2
    seg = np.array([[[int(p0[0]), int(p0[1])], [int(p1[0]), int(p1[1])]]], np.int32)
    ocv.polylines(m, seg, False, 1, int(thickness))
    return m


# ------------------------------------------------------------------------------------------------ cv2 stand-ins
def _paint(img, mask, color):
    if img.ndim == 2:
        img[mask > 0] = color if np.isscalar(color) else color[0]
    else:
        img[mask > 0] = tuple(color)[: img.shape[2]]
    return img


def applyColorMap(src, colormap):
    assert src.dtype == np.uint8 and src.ndim == 2
    return lut()[src]


def line(img, pt1, pt2, color, thickness=1):
    return _paint(img, line_mask(img.shape[:2], pt1, pt2, thickness), color)


def circle(img, center, radius, color, thickness=1):
    return _paint(img, circle_mask(img.shape[:2], center, radius, thickness), color)


def flip(src, flipCode):
    assert flipCode == 0
    return src[::-1].copy()


def cvtColor(src, code):
    return src[..., ::-1].copy()


def plant(cv2_module) -> None:
    """Adds the stand-ins to the shim's cv2 module (keeps COLORMAP_INFERNO / COLOR_BGR2RGB constants it defines)."""
    for f in (applyColorMap, line, circle, flip, cvtColor):
        setattr(cv2_module, f.__name__, f)


# ------------------------------------------------------------------------------------------------ NumPy renderer
def metric_to_pixel(pt, ppm, origin):
    return (pt * ppm * np.array([-1, -1]) + origin).astype(np.int32)


def draw_trajectory(img, positions, yaw, ppm, size):
    """TrajectoryVisualizer.draw_trajectory with a fresh cache (== any sequence of incremental calls)."""
    origin = np.array([size // 2, size // 2])
    if len(positions) >= 2:
        mask = np.zeros(img.shape[:2], np.uint8)
        for a, b in zip(positions[:-1], positions[1:]):
            pa, pb = metric_to_pixel(a, ppm, origin), metric_to_pixel(b, ppm, origin)
            if not np.array_equal(pa, pb):
                mask |= line_mask(mask.shape, pa[::-1], pb[::-1], 3)
        img[mask > 0] = (0, 255, 0)
    px = metric_to_pixel(positions[-1], ppm, origin)
    _paint(img, circle_mask(img.shape[:2], px[::-1], 8, -1), (255, 192, 15))
    end = (int(px[0] - 10 * 1.0 * np.cos(yaw)), int(px[1] - 10 * 1.0 * np.sin(yaw)))
    _paint(img, line_mask(img.shape[:2], px[::-1], end[::-1], 3), (0, 0, 0))
    return img


def render_value(reduced, explored=None, positions=(), yaw=0.0, markers=(), ppm=20):
    """ValueMap.visualize on a reduced plane (its dtype is the normalisation's); markers: (x, y, radius, thickness, bgr)
    in image pixels, drawn only with a trajectory (value_map.py:206-217)."""
    reduced = np.array(reduced, copy=True)
    if explored is not None:
        reduced[np.asarray(explored) == 0] = 0
    img = np.flipud(reduced)
    zero = img == 0
    img[zero] = np.max(img)
    lo, hi = np.min(img), np.max(img)
    ptp = hi - lo
    norm = np.zeros_like(img) if ptp == 0 else (img - lo) / ptp
    out = lut()[(norm * 255).astype(np.uint8)]
    out[zero] = (255, 255, 255)
    if len(positions) > 0:
        draw_trajectory(out, list(positions), yaw, ppm, reduced.shape[0])
        for x, y, r, t, bgr in markers:
            _paint(out, circle_mask(out.shape[:2], (x, y), r, t), bgr)
    return out


def render_obstacle(obstacle, navigable, explored, frontiers_px, positions=(), yaw=0.0, ppm=20,
                    padding_color=(100, 100, 100)):
    size = obstacle.shape[0]
    img = np.ones((size, size, 3), np.uint8) * 255
    img[np.asarray(explored) == 1] = (200, 255, 200)
    img[np.asarray(navigable) == 0] = padding_color
    img[np.asarray(obstacle) == 1] = (0, 0, 0)
    for f in np.asarray(frontiers_px, np.float64).reshape(-1, 2):
        _paint(img, circle_mask(img.shape[:2], (int(f[0]), int(f[1])), 5, 2), (200, 0, 0))
    img = img[::-1].copy()
    if len(positions) > 0:
        draw_trajectory(img, list(positions), yaw, ppm, size)
    return img


def max_reduce(v):
    return np.max(v, axis=-1)


def explore_reduce(thresh):
    """ITMPolicyV3's visual reducer (itm_policy.py:275-287)."""
    def f(arr):
        first = arr[:, :, 0]
        return np.where(first > thresh, first, np.max(arr, axis=2))
    f.thresh = thresh
    return f


# ------------------------------------------------------------------------------------------------ random sessions
def random_value_state(seed: int):
    """A seeded random value-map state: cases cycle through f64 / f32 maps, 1 or 2 channels (2: ITMPolicyV3's reducer),
    explored masks, negative values, all-zero and single-cell maps, trajectories leaving the map, markers partly
    outside the image."""
    rng = np.random.default_rng(1000 + seed)
    case = seed % 8
    S = 1000 if case in (0, 5) else int(rng.integers(60, 200))
    C = 2 if case in (2, 6) else 1
    dtype = np.float32 if case in (1, 3, 6) else np.float64
    v = np.zeros((S, S, C), np.float64)
    for _ in range(int(rng.integers(1, 6))):
        r0, c0 = rng.integers(0, S, 2)
        h, w = rng.integers(1, max(2, S // 2), 2)
        v[r0:r0 + h, c0:c0 + w] = rng.uniform(0.0, 1.0, (min(h, S - r0), min(w, S - c0), C))
    if case == 4:
        v -= 0.5 * (v != 0)                   # negative values
    if case == 7:
        v[:] = 0                              # all-zero map
    if seed % 16 == 15:
        v[:] = 0
        v[int(rng.integers(0, S)), int(rng.integers(0, S))] = rng.uniform(0.1, 1.0, C)   # a single cell
    v = v.astype(dtype)
    explored = (rng.uniform(0, 1, (S, S)) < 0.7) if case in (3, 5) else None
    steps = 0 if case == 7 and seed % 2 else int(rng.integers(1, 12))
    p = rng.uniform(-0.4, 0.4, 2) * S / 20
    positions = []
    for _ in range(steps):
        p = p + rng.uniform(-1.5, 1.5, 2) if rng.uniform() < 0.8 else p   # repeated positions: skipped segments
        positions.append(np.array(p, np.float64))
    if steps and seed % 3 == 0:
        positions.append(np.array([S / 20 * 0.6, -S / 20 * 0.55]))        # off the map
    yaw = float(rng.uniform(-np.pi, np.pi))
    markers = []
    for k in range(int(rng.integers(0, 9))):
        pos = rng.uniform(-0.6, 0.6, 2) * S / 20                           # some outside the image
        th = int(rng.choice([2, 2, 2, -1, 1, 3]))
        color = tuple(int(c) for c in rng.integers(0, 256, 3))
        if k % 3 == 2:
            color = (0, 0, 255)                                            # runs of one colour
        markers.append((pos, {"radius": int(rng.choice([5, 5, 0, 2, 9, 17])), "thickness": th, "color": color}))
    reduce_fn = explore_reduce(float(rng.uniform(0.2, 0.6))) if C == 2 else max_reduce
    return dict(size=S, channels=C, value=v, explored=explored, positions=positions, yaw=yaw, markers=markers,
                reduce_fn=reduce_fn, thresh=getattr(reduce_fn, "thresh", None))


def pixel_markers(markers, size, ppm=20):
    origin = np.array([size // 2, size // 2])
    out = []
    for pos, kw in markers:
        px = metric_to_pixel(pos, ppm, origin)
        out.append((int(px[1]), int(px[0]), kw["radius"], kw["thickness"], kw["color"]))
    return out


def random_obstacle_state(seed: int):
    rng = np.random.default_rng(2000 + seed)
    S = 1000 if seed % 4 == 0 else int(rng.integers(60, 200))
    obstacle = rng.uniform(0, 1, (S, S)) < 0.05
    navigable = ~(rng.uniform(0, 1, (S, S)) < 0.1) & ~obstacle
    explored = rng.uniform(0, 1, (S, S)) < 0.5
    frontiers = rng.uniform(-10, S + 10, (int(rng.integers(0, 12)), 2))
    if seed % 2:
        frontiers = np.round(frontiers * 2) / 2
    steps = int(rng.integers(0, 10))
    p = rng.uniform(-0.4, 0.4, 2) * S / 20
    positions = []
    for _ in range(steps):
        p = p + rng.uniform(-2.0, 2.0, 2)
        positions.append(np.array(p, np.float64))
    return dict(size=S, obstacle=obstacle, navigable=navigable, explored=explored, frontiers=frontiers,
                positions=positions, yaw=float(rng.uniform(-np.pi, np.pi)))


# ------------------------------------------------------------------------------------------------ mapped sessions
SESSION_KW = dict(min_height=0.61, max_height=0.88, agent_radius=0.18, area_thresh=1.5)
SESSION_STEPS = (4, 3)   # steps of the two episodes; reset() of both maps in between


def frontier_markers(frontiers):
    """_get_policy_info's frontier markers (itm_policy.py:162-171) for a frontier list, plus a goal marker on the first."""
    mk = [(f[:2], {"radius": 5, "thickness": 2, "color": (0, 0, 255)}) for f in np.asarray(frontiers).reshape(-1, 2)]
    if mk:
        mk.append((mk[0][0], {"radius": 5, "thickness": 2, "color": (0, 255, 255)}))
    return mk


def run_session(vm, om, on_step, seed: int = 11):
    """Drives a value map + obstacle map through two seeded synthetic episodes (reset in between); ``on_step(k)`` after
    each step, once the agent's trajectory holds the step's pose."""
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, SyntheticEnv, camera_intrinsics

    fx, fy, fov = camera_intrinsics(640)
    k = 0
    for episode, steps in enumerate(SESSION_STEPS):
        env = SyntheticEnv(seed + episode)
        if episode:
            vm.reset()
            om.reset()
        for _ in range(steps):
            depth, tf, values = env.observe()
            om.update_map(depth.copy(), tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov)
            vm.update_map(values, depth.copy(), tf, MIN_DEPTH, MAX_DEPTH, fov)
            xy, yaw = tf[:2, 3].copy(), float(np.arctan2(tf[1, 0], tf[0, 0]))
            vm.update_agent_traj(xy, yaw)
            om.update_agent_traj(xy, yaw)
            on_step(k)
            k += 1
