"""Wall time of single ObjectPointCloudMap.update_map calls (each a batch of one job): the six updates of
tests/golden/make_golden.py:object_map_script() at 640x480, erosion 5, on one map that is reset before every round; 3 warm-up
rounds, then 20 timed rounds, the device synchronised after every update.  Median (min-max) per round and per update, the
object-cloud kernel launches and host read-backs of a round, and a digest of the final clouds.

    python tools/update_map_probe.py [ROOT]        # ROOT: the tree to measure (default: this one), e.g. a copy of a parent commit"""
import hashlib
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

WARMUP, ROUNDS = 3, 20


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def main() -> None:
    import numpy as np
    import torch

    import vlfm_amd
    from make_golden import object_map_script
    from vlfm_amd import _lib
    from vlfm_amd.mapping import object_point_cloud_map as opm
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

    assert os.path.abspath(vlfm_amd.__file__).startswith(ROOT), vlfm_amd.__file__
    assert torch.cuda.is_available(), "update_map_probe measures on the GPU; there is no CPU path"
    L = _lib.lib()
    fx, fy, _ = camera_intrinsics(640)
    ups = [op for op in object_map_script() if op[0] == "update"]
    m = opm.ObjectPointCloudMap(erosion_size=5, device=torch.device("cuda:0"))
    rounds, per_update, digest = [], [[] for _ in ups], None
    for r in range(WARMUP + ROUNDS):
        np.random.seed(1234)
        m.reset()
        torch.cuda.synchronize()
        before = (L.vlfm_object_cloud_launch_count(), opm.SYNCS[0])
        t0 = time.perf_counter()
        for k, op in enumerate(ups):
            t1 = time.perf_counter()
            m.update_map(op[1], op[2], op[3], op[4], MIN_DEPTH, MAX_DEPTH, fx, fy)
            torch.cuda.synchronize()
            per_update[k].append((time.perf_counter() - t1) * 1e6)
        rounds.append((time.perf_counter() - t0) * 1e6)
        work = (L.vlfm_object_cloud_launch_count() - before[0], opm.SYNCS[0] - before[1])
        now = {n: "%d rows %s" % (len(c), hashlib.sha256(np.ascontiguousarray(c).tobytes()).hexdigest()[:16])
               for n, c in sorted(m.clouds.items())}
        assert digest is None or now == digest
        digest = now
    print("update_map  ABI %d  six updates: %.1f us (%.1f-%.1f) over %d rounds after %d; %d launches, %d read-backs per round; clouds %s"
          % (L.vlfm_abi_version(), *stats(rounds[WARMUP:]), ROUNDS, WARMUP, *work, digest), flush=True)
    for k, xs in enumerate(per_update):
        print("update_map  update %d (%s): %.1f us (%.1f-%.1f)" % (k, ups[k][1], *stats(xs[WARMUP:])), flush=True)


if __name__ == "__main__":
    main()
