"""The CPU oracle's KITTI evaluator routines (oracle.KittiBackend: kitti_stats_frame, the overlap routines) against
tests/golden/kitti_stats_ref.npz -- what the reference's own compute_statistics_jit, image_box_overlap, bev_box_overlap,
d3_box_overlap and eval_class return on the crowded and adversarial inputs of kitti_stats_cases.py.  The GPU test holds the HIP
kernels to the same fixture; this one keeps the oracle, which the kernels are also compared with bit for bit, honest."""
import numpy as np
import pytest

import kitti_stats_cases as K


@pytest.fixture(scope="module")
def backend():
    import oracle
    return oracle.KittiBackend()


@pytest.fixture(scope="module")
def g():
    return K.golden()


@pytest.mark.parametrize("name", sorted(K.families()))
def test_statistics_family_equals_reference(backend, g, name):
    K.check_case(backend, g, K.families()[name])


def test_hand_cases(backend):
    K.check_hand_cases(backend)


def test_overlap_cases_equal_reference(backend, g):
    K.check_overlaps(backend, g)
    assert 0 < g["ov_flag"].sum() <= 0.05 * len(g["ov_flag"])


def test_eval_class_on_crowded_annotations(backend, g):
    K.check_eval_class(backend, g)
