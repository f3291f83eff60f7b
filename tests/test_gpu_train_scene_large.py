"""The RPN training batch above 16384 points per frame (prcnn_train_scene_prepare_large, kitti_input.TrainScenePreparer with
large_clouds=True) against the numpy restatement tests/train_scene_twin.py, bit for bit on the keys tests/test_gpu_train_scene.py
compares, with that file's fixture cases, database and helpers."""
import numpy as np
import pytest

import train_scene_twin as ts
from test_gpu_train_scene import _big_db, _preparer, _run, _same, _twin, env          # noqa: F401  (env: the module's fixture)
from util import synthetic_scan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("npoints", [16385, 40000])
def test_ragged_batch_large(env, npoints):          # noqa: F811
    """GT augmentation and all three methods on: a 240 000-point scan, a short frame, an empty one (its cloud is exactly the pasted
    points) and the fixture frame whose accepted objects are pasted"""
    z, calib, cases = env
    base = cases[0]
    db = _big_db(base["db"])
    dense = dict(cases[6], raw=synthetic_scan(240000, 5, 0.5, 0.02))
    short = dict(cases[2], raw=synthetic_scan(3000, 35, 0.5))
    empty = dict(cases[1], raw=np.zeros((0, 4), np.float32))
    frames = [dict(f, db=db) for f in (dense, short, empty, cases[0])]
    settings = dict(base, npoints=npoints, aug={"AUG_METHOD_LIST": ts.METHODS, "AUG_METHOD_PROB": (1.0, 1.0, 0.5), "AUG_ROT_RANGE": 18})
    prep = _preparer(settings, db=db, large_clouds=True)
    got = _run(prep, calib, frames, 11)
    G = max(len(f["gt_boxes3d"]) for f in frames)
    for b, f in enumerate(frames):
        _same(got, b, _twin(calib, f, b, got, settings, 11, G + 16), (npoints, b))
    print("status", list(got["status"]), "nvalid", list(got["nvalid"]), "count", list(got["count"]))
    assert got["pts_rect"].shape == (4, npoints, 3) and got["rpn_cls_label"].shape == (4, npoints)
    assert got["status"][0] == 0 and got["nvalid"][0] > npoints
    pasted = [int((got["src"][b] >= len(f["raw"])).sum()) for b, f in enumerate(frames)]
    assert sum(pasted) > 0 and got["count"][3] > 0 and pasted[2] == npoints          # pasted identities go through the large path


def test_large_degenerates_to_scene_preparer(env):          # noqa: F811
    """without GT augmentation and without AUG_DATA the training builder at 40 000 points is the inference builder"""
    import torch
    from pointrcnn_amd import kitti_input, ops
    z, calib, cases = env
    npoints = 40000
    frames = [dict(cases[0], raw=synthetic_scan(240000, 5, 0.5, 0.02)), cases[1], dict(cases[2], raw=synthetic_scan(36000, 32, 0.9)),
              dict(cases[3], raw=np.zeros((0, 4), np.float32))]                       # the last one: no valid point, status 2
    settings = dict(cases[7], npoints=npoints, aug={"AUG_METHOD_LIST": (), "AUG_METHOD_PROB": (1, 1, 1), "AUG_ROT_RANGE": 18})
    got = _run(_preparer(settings, large_clouds=True), calib, frames, 9)
    inf = kitti_input.ScenePreparer(npoints=npoints)
    ref = inf(inf.pack([f["raw"] for f in frames], [calib] * 4, [f["hw"] for f in frames], pin=False), 9)
    for key in ("pts_input", "pts_features", "src", "nvalid", "status"):
        assert np.array_equal(got[key], ref[key].cpu().numpy()), key
    assert got["status"][3] == 2 and got["status"][0] == 0
    cls, reg = ops.rpn_labels(ref["pts_rect"], torch.from_numpy(got["gt_boxes3d"]).cuda(), torch.from_numpy(got["num_gt"]).cuda())
    assert np.array_equal(got["rpn_cls_label"], cls.cpu().numpy()) and np.array_equal(got["rpn_reg_label"], reg.cpu().numpy())


def test_default_still_refuses_16385(env):          # noqa: F811
    from pointrcnn_amd import _cabi
    z, calib, cases = env
    kw = cases[0]
    with pytest.raises(_cabi.PointOpsError, match="1..16384"):
        _run(_preparer(kw, npoints=16385), calib, [kw], 1)
    out = _run(_preparer(kw, npoints=16385, large_clouds=True), calib, [kw], 1)
    assert out["pts_rect"].shape == (1, 16385, 3)
