"""What tests/test_live_world_cpu.py and tests/test_live_world_gpu.py share: the planes the NumPy statements give for the
cameras of a LiveWorld, a host renderer that answers with them, and the scripted actions."""
import numpy as np
import torch

import vlfm_amd.synthetic as S
from vlfm_amd.harness import TARGETS, WorldTable

H = W = 16
E = 3
TARGETS3 = [TARGETS[e % len(TARGETS)] for e in range(E)]
_F, _L, _R = S.ACTION_FORWARD, S.ACTION_TURN_LEFT, S.ACTION_TURN_RIGHT
PATTERN = [_F, _F, _L, _F, _R, _F, _F, _R]


def actions_at(t: int) -> np.ndarray:
    """The scripted actions of step ``t``: every environment walks PATTERN, environment e shifted by e."""
    return np.array([PATTERN[(t + e) % len(PATTERN)] for e in range(E)], np.int64)


def ring_layout(env_id: int, episode: int, robot_xy):
    """Four objects 1.25 m east, north, west and south of where the episode starts, the environment's target first: at 16 x 16
    pixels something is in view at every heading, and a walk in any direction is soon refused by a footprint."""
    classes = [TARGETS3[env_id]] + [c for c in S.OBJECT_SIZES if c != TARGETS3[env_id]][:3]
    return [(c, S.object_box(c, robot_xy[0] + 1.25 * dx, robot_xy[1] + 1.25 * dy))
            for c, (dx, dy) in zip(classes, ((1, 0), (0, 1), (-1, 0), (0, -1)))]


def object_colours(classes) -> np.ndarray:
    colours = np.zeros((len(classes), S.WORLD_MAX_OBJECTS), np.int32)
    for e, names in enumerate(classes):
        colours[e, :len(names)] = [S.OBJECT_COLOURS.get(c, 0x808080) for c in names]
    return colours


def numpy_planes(tf, table, world_of, objects=None, env_of=None, colours=None, rgb=False):
    """(depth f32 [n,H,W], ids u8 [n,H,W], stats int32 [n,8,5], rgb u8 [n,H,W,3] or None) of the cameras ``tf`` [n,4,4], camera
    i in world ``world_of[i]`` of ``table`` among the objects ``objects[env_of[i]]`` (records [8,8]; None: none): one call of
    render_objects_numpy / render_rgb_numpy and one of object_stats_numpy per camera."""
    tf = np.asarray(tf, np.float64).reshape(-1, 4, 4)
    fx, n = S.camera_intrinsics(W)[0], len(tf)
    depth, ids = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.uint8)
    stats = np.empty((n, S.WORLD_MAX_OBJECTS, 5), np.int32)
    col = np.empty((n, H, W, 3), np.uint8) if rgb else None
    for i, t in enumerate(tf):
        w = int(world_of[i])
        rec = np.zeros((S.WORLD_MAX_OBJECTS, 8)) if objects is None else objects[env_of[i]]
        valid = rec[:, 6] != 0.0
        assert valid[:valid.sum()].all()           # the valid slots come first: id k + 1 is slot k
        args = (t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], fx, S.MIN_DEPTH, S.MAX_DEPTH, H, W, rec[valid, :6])
        if rgb:
            c = np.zeros(S.WORLD_MAX_OBJECTS, np.int64) if colours is None else np.asarray(colours[env_of[i]])
            depth[i], ids[i], col[i] = S.render_rgb_numpy(*args, c[valid], boxes=table.world(w))
        else:
            depth[i], ids[i] = S.render_objects_numpy(*args, boxes=table.world(w), grid=table.grids[w])
        stats[i] = S.object_stats_numpy(ids[i])
    return depth, ids, stats, col


def planes_of(live):
    """``numpy_planes`` of what the robots of the LiveWorld ``live`` see from where they stand."""
    objects = env_of = colours = None
    if live.world_objects is not None:
        objects, env_of, colours = live.objects, np.arange(live.E), object_colours(live.object_classes)
    return numpy_planes(live.poses_tf()[1], live.table, live.world_of, objects, env_of, colours, live.render_rgb)


class _Fields:
    def __init__(self, fields, has_target) -> None:
        self.fields, self.has_target = list(fields), np.array(has_target, bool)

    def assign(self, rows, other) -> None:
        for r, f, h in zip(rows, other.fields, other.has_target):
            self.fields[r], self.has_target[r] = f, h


class NumpyRenderer:
    """The part of RoomsRenderer a LiveWorld uses, answered on the host by the NumPy statements: everybody starts at the
    origin of the rooms world, heading east."""

    def __init__(self) -> None:
        self.H, self.W, self.device = H, W, torch.device("cpu")
        self.pose_table, self.k_table = np.zeros((1, E, 3)), np.zeros((1, E), np.int64)
        self.table = WorldTable(1, self.device, len(S.BOXES))
        self.table.assign([0], [S.BOXES])

    def cast_worlds(self, tf, table, world_of, objects=None, env_of=None, out=None):
        d, ids, stats, _ = numpy_planes(tf, table, world_of, objects, env_of)
        d = torch.from_numpy(d) if out is None else out.copy_(torch.from_numpy(d))
        return d if objects is None else (d, torch.from_numpy(ids), torch.from_numpy(stats))

    def cast_worlds_rgb(self, tf, table, world_of, objects=None, env_of=None, colours=None, out=None, rgb_out=None):
        d, ids, stats, rgb = numpy_planes(tf, table, world_of, objects, env_of, colours, True)
        return out.copy_(torch.from_numpy(d)), torch.from_numpy(ids), torch.from_numpy(stats), rgb_out.copy_(torch.from_numpy(rgb))

    def geodesic_fields_worlds(self, table, world_of, objects, targets_boxes, success_distance):
        fields = []
        for w, rec, box in zip(world_of, objects, targets_boxes):
            fields.append(None)
            if np.all(np.isfinite(box)):
                rects = S.inflated_rects(rec, S.STEP_MARGIN, table.world(w))
                src = S.goal_viewpoints(box, rects, success_distance)
                fields[-1] = (rects, src, *S.geodesic_field_numpy(rects, src))
        return _Fields(fields, [f is not None for f in fields])

    def geodesic_distances(self, handle, field_of, xy):
        return torch.tensor([np.nan if f < 0 else S.geodesic_query_numpy(*handle.fields[f], [p])[0]
                             for f, p in zip(field_of, xy)], dtype=torch.float64)
