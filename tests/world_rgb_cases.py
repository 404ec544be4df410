"""Inputs shared by tests/test_world_rgb_cpu.py and tests/test_world_rgb_gpu.py: four worlds (0, 1, 37 and 64 boxes), seven
cameras and three object rows -- the scene tests/test_procedural_worlds_gpu.py lays out, restated --, object colours, and the
NumPy reference frames (synthetic.render_rgb_numpy) of a frame size, rendered once per process and read-only."""
import functools

import numpy as np

from vlfm_amd import synthetic as S
from world_object_cases import ENV_OBJECTS, objects_array

WORLD_OF = [3, 0, 2, 2, 1, 3, 0]
ENV_OF = [2, 0, 1, 0, 0, 2, 1]
SIZES = [(12, 20), (9, 18), (48, 64)]            # (H, W): 18 is no multiple of 4 -- the byte-store path
SIZE_IDS = ["20x12", "18x9", "64x48"]


@functools.lru_cache(maxsize=None)
def worlds():
    """(the four worlds, the generated world the 64-box one is made of)."""
    gen = S.ProceduralWorlds(0).world(7, 0)
    n = S.WORLD_MAX_BOXES - len(gen.boxes)
    assert n >= 0
    pad = np.array([(-9.0 + 0.3 * i, 9.0 - 0.05 * i, -8.9 + 0.3 * i, 9.1 - 0.05 * i) for i in range(n)]).reshape(-1, 4)
    out = (np.zeros((0, 4)), np.array([(1.0, -0.5, 1.5, 0.1)]), S.BOXES.copy(), np.concatenate([gen.boxes, pad]))
    assert [len(b) for b in out] == [0, 1, 37, 64]
    for b in out:
        b.setflags(write=False)
    return out, gen


def cameras():
    """7 cameras (tf, hfov, lo, hi): lattice poses in their worlds; three with an arbitrary yaw, height, field of view and range."""
    gen = worlds()[1]
    gx, gy = gen.start_xy
    tf = np.stack([S.tf_of(gx, gy, gen.start_k), S.tf_of(0.0, 0.0, 0), S.tf_of(0.5, -0.5, 4), S.pose_to_tf(0.2, 0.4, 0.2, 1.1),
                   S.tf_of(-0.5, 0.0, 0), S.pose_to_tf(gen.spots[3][0], gen.spots[3][1], -2.5, 0.5), S.pose_to_tf(0.3, 0.1, 1.0, 0.88)])
    hfov = np.deg2rad([79.0, 79.0, 79.0, 60.0, 79.0, 100.0, 42.0])
    lo = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.3, 0.05])
    hi = np.array([5.0, 5.0, 5.0, 2.5, 5.0, 3.5, 9.0])
    return tf, hfov, lo, hi


def objects():
    """Three object rows: around the origin, the ring of 8, and in the generated world one object in front of its start pose and
    one in front of camera 5."""
    gen = worlds()[1]
    c, s = S.HEADINGS[gen.start_k]
    x, y = gen.start_xy[0] + 1.0 * c, gen.start_xy[1] + 1.0 * s
    u, v = gen.spots[3][0] + 1.2 * np.cos(-2.5), gen.spots[3][1] + 1.2 * np.sin(-2.5)
    near = [(x - 0.2, y - 0.2, x + 0.2, y + 0.2, 0.0, 1.0), (u - 0.1, v - 0.1, u + 0.1, v + 0.1, 0.2, 1.4)]
    return [ENV_OBJECTS[0], ENV_OBJECTS[2], near]


def colours() -> np.ndarray:
    """int32 [3,8]: a distinct colour per (row, slot), the slots beyond a row's objects included."""
    return np.array([[(0x30 + 0x18 * e) << 16 | (0xF0 - 0x19 * k) << 8 | (0x21 * (k + 1) + 7 * e) & 255 for k in range(8)]
                     for e in range(3)], np.int32)


PALETTE = np.array([0xE0D0C0, 0x60C080, 0x8090F0, 0xF0E040, 0xC05050, 0x40B0B0, 0xB070D0, 0xFFFFFF, 0x906030, 0x504030, 0x70A0FF,
                    0x123456], np.int32)         # not the default: the palette is an argument


def poison(tf, world_of=WORLD_OF):
    """Per world a finite box in front of the first camera that stands in it: what the table tails are filled with."""
    out = np.zeros((4, 4))
    for w in range(4):
        t = tf[list(world_of).index(w)]
        x, y = t[0, 3] + 0.8 * t[0, 0], t[1, 3] + 0.8 * t[1, 0]
        out[w] = (x - 0.3, y - 0.3, x + 0.3, y + 0.3)
    return out


def _args(i, H, W):
    tf, hfov, lo, hi = cameras()
    t = tf[i]
    return (t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(hfov[i] / 2)), lo[i], hi[i], H, W, objects()[ENV_OF[i]])


@functools.lru_cache(maxsize=None)
def reference(H, W):
    """(depth [7,H,W], ids, stats [7,8,5], rgb [7,H,W,3]) of the seven cameras; read-only."""
    w = worlds()[0]
    col = colours()
    ref = [S.render_rgb_numpy(*_args(i, H, W), col[ENV_OF[i]][:len(objects()[ENV_OF[i]])], boxes=w[WORLD_OF[i]], palette=PALETTE)
           for i in range(7)]
    out = (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), np.stack([S.object_stats_numpy(r[1]) for r in ref]),
           np.stack([r[2] for r in ref]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def kinds(H, W):
    """(kind u8 [7,H,W], skirting, odd panel, y-face bool [7,H,W]) of the seven cameras (synthetic.rgb_kinds_numpy)."""
    w = worlds()[0]
    k = [S.rgb_kinds_numpy(*_args(i, H, W), boxes=w[WORLD_OF[i]]) for i in range(7)]
    return tuple(np.stack([r[j] for r in k]) for j in range(4))
