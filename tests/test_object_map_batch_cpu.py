"""The host-side planning of the batched object-map update (vlfm_amd/mapping/object_point_cloud_map.py: plan_waves,
plan_chunks, the refusals update_maps_batch makes before it touches a device).  No GPU."""
import numpy as np
import pytest

from vlfm_amd.mapping import object_point_cloud_map as opm


# ---------------------------------------------------------------------------------------------- waves
def test_one_job_per_generator_is_one_wave():
    assert opm.plan_waves([10, 11, 12, 13], [True, False, True, True]) == [[0, 1, 2, 3]]


def test_shared_generator_without_a_choice_is_one_wave():
    assert opm.plan_waves([7, 7, 7], [False, False, False]) == [[0, 1, 2]]


def test_shared_generator_splits_before_a_later_choice():
    assert opm.plan_waves([7, 7], [False, True]) == [[0], [1]]
    # the other generator's jobs do not matter, and the wave after the split starts a new account
    assert opm.plan_waves([7, 8, 7, 7, 8], [False, True, True, False, True]) == [[0, 1], [2, 3, 4]]
    assert opm.plan_waves([7, 7, 7], [True, True, True]) == [[0], [1], [2]]


def test_shared_generator_with_the_first_job_choosing_is_one_wave():
    assert opm.plan_waves([7, 7, 7], [True, False, False]) == [[0, 1, 2]]


def test_waves_keep_the_order_and_every_job():
    rng = np.random.default_rng(0)
    for _ in range(50):
        n = int(rng.integers(0, 12))
        gens = [int(g) for g in rng.integers(0, 3, n)]
        need = [bool(b) for b in rng.integers(0, 2, n)]
        waves = opm.plan_waves(gens, need)
        assert [j for w in waves for j in w] == list(range(n)) and all(waves)
        for w in waves:   # within a wave only the first job of a generator may draw a choice
            seen = set()
            for j in w:
                assert not (need[j] and gens[j] in seen), (gens, need, waves)
                seen.add(gens[j])
    with pytest.raises(ValueError):
        opm.plan_waves([1, 2], [True])


def _draws_per_detection(gens, need, nonempty):
    log = {g: [] for g in gens}
    for j, g in enumerate(gens):
        if need[j]:
            log[g].append(("choice", j))
        if nonempty[j]:
            log[g].append(("rand", j))
    return log


def test_wave_order_of_draws_is_the_per_detection_order():
    rng = np.random.default_rng(1)
    for _ in range(200):
        n = int(rng.integers(1, 10))
        gens = [int(g) for g in rng.integers(0, 3, n)]
        need = [bool(b) for b in rng.integers(0, 2, n)]
        nonempty = [bool(b) for b in rng.integers(0, 2, n)]
        log = {g: [] for g in gens}
        for w in opm.plan_waves(gens, need):
            for j in w:
                if need[j]:
                    log[gens[j]].append(("choice", j))
            for j in w:
                if nonempty[j]:
                    log[gens[j]].append(("rand", j))
        assert log == _draws_per_detection(gens, need, nonempty), (gens, need, nonempty)


# ---------------------------------------------------------------------------------------------- chunks
def test_job_bytes_is_the_library_formula():
    from vlfm_amd import _lib

    L = _lib.lib()
    for n in (0, 1, 63, 64, 65, 129, 4999, 5000):
        assert opm.dbscan_job_bytes(n) == L.vlfm_dbscan_batch_scratch_bytes(n), n
    assert opm.dbscan_job_bytes(5000) == 5000 * 79 * 8 + 16 * 5000 + 192       # 3.2 MB


def test_chunks_fill_the_budget_in_order():
    full = opm.dbscan_job_bytes(5000)
    assert opm.plan_chunks([full] * 5, 2 * full) == [[0, 1], [2, 3], [4]]
    assert opm.plan_chunks([full] * 3, full) == [[0], [1], [2]]
    assert opm.plan_chunks([full, 0, 0, full], full) == [[0, 1, 2], [3]]
    assert opm.plan_chunks([full] * 4, opm.DEFAULT_SCRATCH_BUDGET) == [[0, 1, 2, 3]]
    assert opm.plan_chunks([], full) == []


def test_a_budget_below_one_full_job_is_refused():
    full = opm.dbscan_job_bytes(5000)
    with pytest.raises(ValueError, match="scratch_budget_bytes"):
        opm.plan_chunks([1024], full - 1)
    with pytest.raises(ValueError, match="scratch_budget_bytes"):
        opm.update_maps_batch([object()], ["chair"], np.zeros((1, 4, 4), np.float32), [0], np.zeros((1, 4, 4), np.uint8),
                              [np.eye(4)], 0.5, 5.0, 1.0, 1.0, scratch_budget_bytes=full - 1)


# ---------------------------------------------------------------------------------------------- refusals before the device
def _args(D=2, F=2):
    return dict(maps=[object()] * D, object_names=["chair"] * D, depth_frames=np.zeros((F, 6, 8), np.float32),
                frame_index=[0] * D, masks=np.zeros((D, 6, 8), np.uint8), tfs=[np.eye(4)] * D)


@pytest.mark.parametrize("short", ["object_names", "frame_index", "masks", "tfs"])
def test_mismatched_lengths_are_refused(short):
    a = _args()
    a[short] = a[short][:1]
    with pytest.raises(ValueError, match="one entry per job"):
        opm.update_maps_batch(**a, min_depth=0.5, max_depth=5.0, fx=1.0, fy=1.0)


@pytest.mark.parametrize("frame", [-1, 2])
def test_a_frame_index_out_of_range_is_refused(frame):
    a = _args()
    a["frame_index"] = [0, frame]
    with pytest.raises(ValueError, match="frame index"):
        opm.update_maps_batch(**a, min_depth=0.5, max_depth=5.0, fx=1.0, fy=1.0)


def test_masks_of_another_size_are_refused():
    a = _args()
    a["masks"] = np.zeros((2, 6, 9), np.uint8)
    with pytest.raises(ValueError, match="masks"):
        opm.update_maps_batch(**a, min_depth=0.5, max_depth=5.0, fx=1.0, fy=1.0)


def test_no_jobs_is_a_no_op():
    assert opm.update_maps_batch([], [], np.zeros((1, 6, 8), np.float32), [], np.zeros((0, 6, 8), np.uint8), [], 0.5, 5.0, 1.0,
                                 1.0) == []


def test_too_offset_from_the_extent_is_too_offset():
    rng = np.random.default_rng(3)
    for _ in range(200):
        W = int(rng.integers(8, 90))
        m = np.zeros((5, W), np.uint8)
        if rng.random() > 0.1:
            a, b = sorted(int(x) for x in rng.integers(0, W, 2))
            m[2, a:b + 1] = 1
        cols = np.flatnonzero(m.any(0))
        left, right = (int(cols[0]), int(cols[-1]) + 1) if len(cols) else (0, 0)
        assert opm.extent_too_offset(left, right, W) == opm.too_offset(m)
