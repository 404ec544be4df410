"""Masks and plans the lattice-geodesic tests share (tests/test_lattice_geodesic_cpu.py, tests/test_lattice_geodesic_gpu.py).
Everything is drawn from seeds or by rule; nothing here touches a device."""
import numpy as np

from vlfm_amd import synthetic as S

# (environment, episode) of the rooms-world layouts the band against the visibility graph is measured on, robot at (0, 0)
BAND_LAYOUTS = [(0, 0), (1, 3), (2, 1), (5, 2)]
# the chamfer against the visibility-graph rule, points farther than 1 m from the goal: the lower bound is the derivation's
# (5.5 / (5 sqrt(1.25)) = 0.98387 in free space); the upper bound was measured on BAND_LAYOUTS (1.0477) and rounded up
BAND_LO, BAND_HI = 0.9838, 1.05


def spiral(size: int = 40) -> np.ndarray:
    """bool [size, size] free mask: a corridor two nodes wide that winds inwards between walls one node thick."""
    free = np.ones((size, size), bool)
    lo, hi = 0, size - 1
    while hi - lo >= 6:
        free[lo + 2, lo:hi - 2] = False          # wall under the next ring's top corridor, open at the right end
        free[lo + 2:hi - 2, hi - 2] = False
        free[hi - 2, lo + 2:hi - 1] = False
        free[lo + 5:hi - 1, lo + 2] = False
        lo, hi = lo + 3, hi - 3
    return free


def comb(size: int = 40) -> np.ndarray:
    """bool [size, size] free mask: a spine along row 0 and dead-end teeth: reaching one tooth from the next costs two tooth
    lengths, and most levels touch only a few rows."""
    free = np.ones((size, size), bool)
    free[1:, 1::2] = False
    return free


def serpentine(size: int = 41) -> np.ndarray:
    """bool [size, size] free mask: single-node corridors on the even rows joined at alternating ends -- a path of about
    size * size / 2 nodes from one corner to the other."""
    free = np.zeros((size, size), bool)
    free[0::2, :] = True
    for k, r in enumerate(range(1, size, 2)):
        free[r, size - 1 if k % 2 == 0 else 0] = True
    return free


def random_mask(rng, nb: int, na: int, density: float) -> np.ndarray:
    return rng.random((nb, na)) >= density


def random_plan(rng, ny: int, nx: int, density: float = 0.15, uniform: bool = False) -> S.GridPlan:
    """A plan of ny x nx cells about 5 cm wide, lower left corner near (-1, -1): lattice edges, or jittered ones."""
    occ = rng.random((ny, nx)) < density
    if uniform:
        return S.GridPlan.uniform(occ, 20, -20, -20)
    xs = -1.0 + np.cumsum(np.concatenate([[0.0], rng.uniform(0.03, 0.07, nx)]))
    ys = -1.0 + np.cumsum(np.concatenate([[0.0], rng.uniform(0.03, 0.07, ny)]))
    return S.GridPlan(occ, xs, ys)


def drawn_plans():
    """Two drawn floor plans at 10 cells per metre, with a diagonal wall and a round pillar (what boxes cannot say): a 10 m x 8 m
    room with a partition, and an 8 m square with two pillars."""
    plans = []
    for (w, h, pillars) in ((100, 80, [(30, 25, 6)]), (80, 80, [(25, 55, 5), (55, 25, 7)])):
        occ = np.zeros((h, w), bool)
        occ[:2], occ[-2:], occ[:, :2], occ[:, -2:] = True, True, True, True
        jj, ii = np.mgrid[0:h, 0:w]
        for (ci, cj, r) in pillars:
            occ |= (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r
        occ |= (np.abs(ii - jj - 20) <= 1) & (ii > 50) & (ii < w - 12)            # a diagonal wall
        occ[h // 2 - 1:h // 2 + 1, :w // 3] = True                                  # a partition with a gap
        plans.append(S.GridPlan.uniform(occ, 10, -w // 2, -h // 2))
    return plans
