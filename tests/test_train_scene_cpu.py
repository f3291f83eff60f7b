"""The RPN training batch on the host side (csrc/train_scene.hip): the numpy restatement in tests/train_scene_twin.py against the
reference's own get_rpn_sample(mode='TRAIN') (tests/golden/train_scene_ref.npz, written by tests/golden/ref_train_scene.py), and the
C ABI surface of the two new entry points."""
import os
import re

import numpy as np
import pytest

import train_scene_twin as ts

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "train_scene_ref.npz")


@pytest.fixture(scope="module")
def cases():
    from pointrcnn_amd import kitti_input
    z = np.load(GOLD)
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT).packed()
    out = []
    for k in range(int(z["ncases"])):
        kw = ts.fixture_case(z, k)
        out.append((kw, ts.train_scene(calib24=calib, rect_flag=ts.fixture_rect(z, k, calib, kw), atan2=np.arctan2, **kw)))
    return z, calib, out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_twin_reproduces_reference_bit_for_bit(cases):
    """Everything downstream of the projection, on the reference's own rect cloud: bit for bit.  The projection itself is the
    canonical one of csrc/scene.hip; the reference's is a BLAS sgemm that differs from it by up to 7.6e-6 m (test_oracle_scene.py), so
    the fixture carries the reference's cloud as an offset in fp32 steps from the canonical one -- see test_canonical_projection_same_sample.
    Likewise the ry update runs numpy's fp32 arctan2 here, as the reference did; the contract's atan2f (csrc/ref_trig.h = glibc's)
    differs from it on about 41 % of all arguments, by up to 3 fp32 steps (on 20 of the 39 rotated box centres met while generating
    this fixture, by one step each), so no set of cases
    exists on which the two agree throughout -- test_canonical_projection_same_sample holds the contract's ry to that one step."""
    z, _, out = cases
    for k, (kw, got) in enumerate(out):
        assert got["status"] == 0 and got["gt_aug_status"] == 0, k
        assert np.array_equal(got["ids"], z["c%d_ids" % k]), k
        assert got["nvalid"] == int(z["c%d_nedit" % k]), k
        want_angle, want_scale, want_flip = z["c%d_method" % k]
        assert np.array_equal(got["aug"][[3, 6, 7]], [want_angle, want_scale, want_flip], equal_nan=True), k
        ng = got["num_gt"]
        assert ng == z["c%d_gt_boxes3d" % k].shape[0], k
        assert np.array_equal(_bits(got["pts_rect"]), _bits(z["c%d_pts_rect" % k])), k
        assert np.array_equal(_bits(got["pts_features"]), _bits(z["c%d_pts_features" % k])), k
        assert np.array_equal(_bits(got["gt_boxes3d"][:ng]), _bits(z["c%d_gt_boxes3d" % k])), k
        assert np.array_equal(got["rpn_cls_label"], z["c%d_cls" % k].astype(np.int32)), k
        assert np.array_equal(_bits(got["rpn_reg_label"]), _bits(z["c%d_reg" % k])), k


def test_canonical_projection_same_sample(cases):
    """with the canonical projection (what the device computes) the same points are selected in the same order and labelled the same;
    coordinates differ from the reference's by the sgemm's rounding only (tolerance of test_oracle_scene.py)"""
    z, calib, out = cases
    for k, (kw, ref) in enumerate(out):
        got = ts.train_scene(calib24=calib, **kw)
        assert np.array_equal(got["src"], ref["src"]) and got["nvalid"] == ref["nvalid"], k
        np.testing.assert_allclose(got["pts_rect"], z["c%d_pts_rect" % k], rtol=2e-6, atol=2e-5)
        assert np.array_equal(_bits(got["pts_features"]), _bits(z["c%d_pts_features" % k])), k
        assert np.array_equal(_bits(got["gt_boxes3d"][:, :6]), _bits(ref["gt_boxes3d"][:, :6])), k
        # ry = (sign(beta) * pi / 2 + alpha) - beta with |beta| < pi: one fp32 step of beta (what the two atan2 differ by on these centres) is
        # at most 2.4e-7, and the result's own rounding
        assert np.abs(got["gt_boxes3d"][:, 6].astype(np.float64) - ref["gt_boxes3d"][:, 6]).max(initial=0) <= 2 * 2.4e-7, k
        assert np.array_equal(got["rpn_cls_label"], z["c%d_cls" % k].astype(np.int32)), k
        np.testing.assert_allclose(got["rpn_reg_label"], z["c%d_reg" % k], rtol=2e-6, atol=2e-5)


def test_fixture_covers_the_case_list(cases):
    z, _, out = cases
    n = int(z["npoints"])
    got = [g for _, g in out]
    assert any(g["nvalid"] > n and int(z["c%d_nfar_pasted" % k]) > 0 for k, g in enumerate(got))       # far pasted object
    assert any(g["nvalid"] < n for g in got)                                                          # top-up
    assert any(kw["gt_aug"] and g["sampler"]["stats"][0] == 1 and len(g["ids"]) == 0 for kw, g in out)   # nothing accepted
    assert any(kw["gt_aug"] and g["sampler"]["stats"][0] == 0 for kw, g in out)                        # apply draw fails
    assert any(len(kw["gt_boxes3d"]) == 0 and len(kw["all_gt_boxes3d"]) > 0 and len(g["ids"]) > 0 for kw, g in out)
    assert any(kw["scope"] is None for kw, _ in out) and any(kw["gt_aug"] is None for kw, _ in out)
    for col in (3, 6):                                                                              # rotation, scaling on and off
        assert any(np.isnan(g["aug"][col]) for g in got) and any(not np.isnan(g["aug"][col]) for g in got)
    assert {g["aug"][7] for g in got} == {0.0, 1.0}
    assert any(len(z["c%d_redrawn" % k]) == 0 and len(z["c%d_ids" % k]) > 0 for k in range(len(got)))


class NoHPlus2(ts.Steps):
    extra_h = 0.0


class IdentityOffByObject(ts.Steps):
    @staticmethod
    def paste_identity(n_raw, npts):
        total = int(np.sum(npts))
        return n_raw + (np.arange(total) + (int(npts[0]) if total else 0)) % max(total, 1)


class NoFarRuleForPasted(ts.Steps):
    @staticmethod
    def far(cloud, n_scene):
        far = ts.Steps.far(cloud, n_scene)
        far[n_scene:] = False
        return far


class ScaleBeforeRotation(ts.Steps):
    @staticmethod
    def augment(pts, boxes, alpha, a, atan2=None):
        first, then = a.copy(), a.copy()
        first[3], first[7], then[6] = np.nan, 0.0, np.nan
        return ts.augment(*ts.augment(pts, boxes, alpha, first, atan2), alpha, then, atan2)


class RyFromUnrotatedCentre(ts.Steps):
    @staticmethod
    def augment(pts, boxes, alpha, a, atan2=None):
        apts, aboxes = ts.augment(pts, boxes, alpha, a, atan2)
        if not np.isnan(a[3]) and len(boxes):
            beta = (atan2 or np.arctan2)(boxes[:, 2].astype(np.float32), boxes[:, 0].astype(np.float32))
            ry = ((np.sign(beta) * ts.F32_PI) / np.float32(2) + np.asarray(alpha, np.float32)) - beta
            aboxes[:, 6] = np.sign(ry) * ts.F32_PI - ry if a[7] != 0 else ry
        return apts, aboxes


@pytest.fixture(scope="module")
def stated_steps_match(cases):
    return _matches_fixture(cases, ts.Steps)


def _matches_fixture(cases, steps):
    """per case: does train_scene with these steps give the fixture's points, boxes and both labels, bit for bit"""
    z, calib, out = cases
    same = []
    for k, (kw, _) in enumerate(out):
        got = ts.train_scene(calib24=calib, steps=steps, rect_flag=ts.fixture_rect(z, k, calib, kw), atan2=np.arctan2, **kw)
        ng = got["num_gt"]
        same.append(got["pts_rect"].shape == z["c%d_pts_rect" % k].shape and ng == len(z["c%d_gt_boxes3d" % k]) and
                    np.array_equal(_bits(got["pts_rect"]), _bits(z["c%d_pts_rect" % k])) and
                    np.array_equal(_bits(got["pts_features"]), _bits(z["c%d_pts_features" % k])) and
                    np.array_equal(_bits(got["gt_boxes3d"][:ng]), _bits(z["c%d_gt_boxes3d" % k])) and
                    np.array_equal(got["rpn_cls_label"], z["c%d_cls" % k].astype(np.int32)) and
                    np.array_equal(_bits(got["rpn_reg_label"]), _bits(z["c%d_reg" % k])))
    return same


@pytest.mark.parametrize("wrong", [NoHPlus2, IdentityOffByObject, NoFarRuleForPasted, ScaleBeforeRotation, RyFromUnrotatedCentre])
def test_fixture_rejects_wrong_restatements(cases, stated_steps_match, wrong):
    """the fixture tells the stated semantics from near misses: the stated steps match every case, each wrong one misses some case"""
    assert all(stated_steps_match)
    assert not all(_matches_fixture(cases, wrong)), wrong.__name__


def test_draw_rule_properties():
    """the draw of train_scene_twin.draw: all far points kept, no repeats when n >= npoints, every point at least once in a top-up"""
    ident = np.arange(5000) * 3
    far = (np.arange(5000) % 10) == 0
    src, st = ts.draw(ident, far, 1024, 5, 2)
    assert st == 0 and len(np.unique(src)) == 1024 and set(ident[far]) <= set(src)
    src, st = ts.draw(ident[:700], far[:700], 1024, 5, 2)
    assert st == 0 and set(src) == set(ident[:700]) and np.bincount(src // 3).max() == 2
    assert ts.draw(ident[:100], far[:100], 1024, 5, 2)[1] == 1 and ts.draw(ident[:0], far[:0], 16, 5, 2)[1] == 2


def test_header_and_bindings_declare_the_entry_points():
    from pointrcnn_amd import _cabi
    hdr = open(os.path.join(REPO, "include", "prcnn_pointops.h")).read()
    for name in ("prcnn_train_scene_workspace_bytes", "prcnn_train_scene_prepare"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _cabi.SIGNATURES, name
    m = re.search(r"int prcnn_train_scene_prepare\((.*?)\);", hdr, re.S)
    assert len(m.group(1).split(",")) == len(_cabi.SIGNATURES["prcnn_train_scene_prepare"][1])
    assert re.search(r"prcnn_abi_version\(void\)\s*\{\s*return 12;", open(os.path.join(REPO, "pointrcnn_amd", "csrc", "cabi_common.hip")).read())


def test_stream_table_lists_the_augmentation_streams():
    src = open(os.path.join(REPO, "pointrcnn_amd", "csrc", "scene.hip")).read()
    head = src[:src.index("#include")]
    for stream in (34, 35, 36):
        assert re.search(r"^//\s+%d\s+train_scene\.hip" % stream, head, re.M), stream
