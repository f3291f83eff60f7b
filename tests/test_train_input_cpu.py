"""GT-augmentation sampling on the host side (csrc/train_input.hip, csrc/quad_clip.h): the Python restatement in
tests/train_input_twin.py against the reference's own apply_gt_aug_to_one_scene (tests/golden/train_input_ref.npz, written by
tests/golden/ref_train_input.py), the double clip against analytic overlaps, and the C ABI surface of the two new entry points."""
import os
import re

import numpy as np
import pytest

import train_input_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "train_input_ref.npz")


def _case_cfg(z, k):
    extra, rand_num, prob, ratio, use_scope = z["c%d_cfg" % k]
    return {"GT_EXTRA_NUM": int(extra), "GT_AUG_RAND_NUM": bool(rand_num), "GT_AUG_APPLY_PROB": float(prob),
            "GT_AUG_HARD_RATIO": float(ratio), "PC_AREA_SCOPE": tuple(z["scope"]) if use_scope else None, "TRY_TIMES": 100}


def test_twin_sampler_reproduces_reference():
    z = np.load(GOLD)
    seen = set()
    for k in range(int(z["ncases"])):
        got = tw.gt_aug_sample(z["c%d_gt" % k], z["c%d_plane" % k], z["db_boxes"], z["db_alpha"], z["db_npts"], _case_cfg(z, k),
                               int(z["c%d_seed" % k]), 0)
        assert got["status"] == int(z["c%d_status" % k]), k
        assert got["stats"][0] == int(z["c%d_applied" % k]), k
        if got["status"] == 0:
            assert got["stats"][3] == int(z["c%d_started" % k]), k
        assert np.array_equal(got["ids"], z["c%d_ids" % k]), k
        assert np.array_equal(got["boxes"].view(np.uint32), z["c%d_boxes" % k].view(np.uint32)), k
        assert np.array_equal(got["alpha"], z["c%d_alpha" % k]), k
        seen.add((got["stats"][0], len(got["ids"]) > 0, got["stats"][3] == 100, got["status"]))
        if got["status"] == 0 and got["stats"][2] > got["stats"][1]:
            seen.add("cnt-stop")
            if got["stats"][2] > len(got["ids"]):
                seen.add("cnt-stop-with-rejections")
    # the fixture covers: nothing applied, budget exhausted, the cnt stop with rejected tries counted, a raising frame
    assert (0, False, False, 0) in seen and (1, False, True, 0) in seen and "cnt-stop-with-rejections" in seen
    assert any(s[3] == 1 for s in seen if isinstance(s, tuple))


def test_fixture_draws_both_lists():
    z = np.load(GOLD)
    ids = np.concatenate([z["c%d_ids" % k] for k in range(int(z["ncases"])) if z["c%d_cfg" % k][3] > 0])
    n = z["db_npts"][ids]
    assert (n > 100).any() and (n <= 100).any()


def test_pasted_points_shift_in_double():
    """the reference moves the pasted points by the float64 move_height and stores fp32: y' = fp32(double(y) - move)"""
    z = np.load(GOLD)
    off = np.concatenate([[0], np.cumsum(z["db_npts"])])
    for k in range(int(z["ncases"])):
        got = tw.gt_aug_sample(z["c%d_gt" % k], z["c%d_plane" % k], z["db_boxes"], z["db_alpha"], z["db_npts"], _case_cfg(z, k),
                               int(z["c%d_seed" % k]), 0)
        if not len(got["ids"]):
            continue
        rows = []
        for i, mv in zip(got["ids"], got["y_shift"]):
            p = z["db_points"][off[i]:off[i + 1]].copy()
            p[:, 1] = (p[:, 1].astype(np.float64) - mv).astype(np.float32)
            rows.append(p)
        assert np.array_equal(np.concatenate(rows), z["c%d_pasted" % k]), k


@pytest.mark.parametrize("seed", range(4))
def test_clip_matches_analytic_rectangles(seed):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        cx, cz, qx, qz = rng.uniform(-5, 5, 4)
        hx, hz, gx, gz = rng.uniform(0.2, 3, 4)
        rot90 = rng.random() < 0.5
        a = tw.rect_corners(cx, cz, hx, hz, y0=1.0, h=2.0)
        if rot90:            # the same rectangle as a box rotated by 90 degrees: corners permuted, extents swapped
            b = tw.rect_corners(qx, qz, gz, gx, y0=1.5, h=2.0)[[1, 2, 3, 0, 5, 6, 7, 4]]
            gx, gz = gz, gx
        else:
            b = tw.rect_corners(qx, qz, gx, gz, y0=1.5, h=2.0)
        fa, fb = a.astype(np.float64), b.astype(np.float64)
        ox = max(0.0, min(fa[:4, 0].max(), fb[:4, 0].max()) - max(fa[:4, 0].min(), fb[:4, 0].min()))
        oz = max(0.0, min(fa[:4, 2].max(), fb[:4, 2].max()) - max(fa[:4, 2].min(), fb[:4, 2].min()))
        area_a = (fa[:4, 0].max() - fa[:4, 0].min()) * (fa[:4, 2].max() - fa[:4, 2].min())
        area_b = (fb[:4, 0].max() - fb[:4, 0].min()) * (fb[:4, 2].max() - fb[:4, 2].min())
        o = ox * oz
        h = 1.5                                   # heights [-1, 1] and [-1.5, 0.5] overlap by 1.5
        iou3d, bev = tw.pair_iou(a, b)
        want3 = o * h / (area_a * 2.0 + area_b * 2.0 - o * h)
        assert abs(float(iou3d) - want3) <= 1e-6 * max(want3, 1e-30) + (0 if o else 0), (a, b)
        assert abs(float(bev) - o / (area_a + area_b - o)) <= 1e-6 * max(o, 1e-30)
        assert (o == 0) == (iou3d == 0)


def test_degenerate_and_self_intersecting_quads_give_zero():
    a = tw.rect_corners(0, 0, 1, 1)
    flat = tw.rect_corners(0, 0, 1, 0)                          # zero width
    bow = a[[0, 2, 1, 3, 4, 6, 5, 7]]                             # self-intersecting order
    for q in (flat, bow):
        assert tw.pair_iou(a, q) == (0, 0) and tw.pair_iou(q, a) == (0, 0)
    assert tw.pair_iou(a, a)[0] == np.float32(1.0)


def test_height_disjoint_pair_is_zero():
    a = tw.rect_corners(0, 0, 1, 1, y0=0.0, h=1.0)
    b = tw.rect_corners(0, 0, 1, 1, y0=-1.0, h=1.0)             # stacked: touching faces, no height overlap
    assert tw.pair_iou(a, b) == (0, 0)


def test_header_and_binding_declare_the_sampling_entry_points():
    from pointrcnn_amd import _cabi
    with open(os.path.join(os.path.dirname(HERE), "include", "prcnn_pointops.h")) as f:
        names = re.findall(r"^(?:int|size_t)\s+(prcnn_\w+)\s*\(", f.read(), flags=re.M)
    for n in ("prcnn_corner_iou3d", "prcnn_gt_aug_sample"):
        assert n in names and n in _cabi.SIGNATURES
    assert _cabi.REQUIRED_ABI == 12
