"""The RPN training batch on the device (csrc/train_scene.hip, kitti_input.TrainScenePreparer) against the numpy restatement
tests/train_scene_twin.py (itself pinned to the reference's own get_rpn_sample by tests/test_train_scene_cpu.py).  The device's
double cos / sin may differ from numpy's in the last bit, so the twin is run with the (cos, sin) the kernel reports and those are
held to one double ulp of numpy's."""
import os

import numpy as np
import pytest
import torch

import train_scene_twin as ts
from util import synthetic_scan

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("pts_rect", "pts_features", "gt_boxes3d", "rpn_cls_label", "rpn_reg_label", "src")


@pytest.fixture(scope="module")
def env():
    from pointrcnn_amd import kitti_input
    z = np.load(os.path.join(HERE, "golden", "train_scene_ref.npz"))
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    cases = [ts.fixture_case(z, k) for k in range(int(z["ncases"]))]
    return z, calib, cases


def _database(db, hard_ratio):
    from pointrcnn_amd import kitti_input
    off = np.concatenate([[0], np.cumsum(db["npts"])])
    return kitti_input.GTDatabase.from_arrays(db["boxes"], db["alpha"], [db["points"][a:b] for a, b in zip(off[:-1], off[1:])],
                                              [db["intensity"][a:b] for a, b in zip(off[:-1], off[1:])], hard_ratio)


def _preparer(kw, db=None, **over):
    from pointrcnn_amd import kitti_input
    g = kw["gt_aug"]
    sc = kw["scope"]
    args = dict(npoints=kw["npoints"], area_scope=None if sc is None else (sc[0:2], sc[2:4], sc[4:6]), GT_AUG_ENABLED=g is not None,
                AUG_DATA=True, AUG_METHOD_LIST=kw["aug"]["AUG_METHOD_LIST"], AUG_METHOD_PROB=kw["aug"]["AUG_METHOD_PROB"])
    if g is not None:
        args.update(gt_database=_database(db or kw["db"], g["GT_AUG_HARD_RATIO"]), GT_EXTRA_NUM=g["GT_EXTRA_NUM"],
                    GT_AUG_RAND_NUM=g["GT_AUG_RAND_NUM"], GT_AUG_APPLY_PROB=g["GT_AUG_APPLY_PROB"])
    args.update(over)
    return kitti_input.TrainScenePreparer(**args)


def _run(prep, calib, frames, seed):
    """frames: list of fixture_case-style dicts -> the preparer's output as numpy"""
    packed = prep.pack([f["raw"] for f in frames], [calib] * len(frames), [f["hw"] for f in frames], [f["gt_boxes3d"] for f in frames],
                       [f["gt_alpha"] for f in frames], [f["all_gt_boxes3d"] for f in frames], [f["plane"] for f in frames], pin=False)
    out = prep(packed, seed)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _twin(calib, f, b, got, settings, seed, width, max_accept=16, device_trig=True):
    a = got["aug"][b]
    cs = (a[4], a[5]) if device_trig and not np.isnan(a[3]) else None
    kw = dict(f)
    kw.update(gt_aug=settings["gt_aug"], aug=settings["aug"], scope=settings["scope"], npoints=settings["npoints"], seed=seed, frame=b)
    return ts.train_scene(calib24=calib.packed(), width=width, cos_sin=cs, max_accept=max_accept, **kw)


def _same(got, b, want, tag):
    for key in KEYS:
        g, w = got[key][b], want[key]
        assert g.shape == w.shape, (tag, key, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), (tag, key)
    assert got["nvalid"][b] == want["nvalid"] and got["status"][b] == want["status"], tag
    assert got["num_gt"][b] == want["num_gt"] and got["gt_aug_status"][b] == want["gt_aug_status"], tag
    assert np.array_equal(got["db_id"][b][:got["count"][b]], want["ids"]) or want["gt_aug_status"] in (1, 3), tag
    assert np.array_equal(got["aug"][b][[0, 1, 2, 3, 6, 7]], want["aug"][[0, 1, 2, 3, 6, 7]], equal_nan=True), tag


def _ulp_close(a, b):
    return np.isnan(b) and np.isnan(a) or abs(a - b) <= np.spacing(abs(b))


def _same_as_fixture(z, k, got, n_raw):
    """Frame k of the device's output against the reference's own (the fixture), for a frame whose reported cos and sin are numpy's:
    bit for bit wherever the reference computed what the contract states, and to a stated bound in the two places where it did not
     --
      * its lidar_to_rect is a BLAS sgemm whose rounding differs from the canonical projection of csrc/scene.hip; the fixture records
        the difference per raw point (c<k>_rect_ulp), so scene rows with no recorded difference and all pasted rows are held bit for
        bit and the rest to the tolerance of tests/test_oracle_scene.py;
      * its ry update ran numpy's fp32 arctan2, the contract's is csrc/ref_trig.h's atan2f: on this fixture's 39 rotated box
        centres the two differ by at most one fp32 step of beta (|beta| < pi: 2.4e-7; up to 3 steps on arbitrary arguments), and
        ry = (sign(beta) * pi / 2 + alpha) - beta adds its own rounding, hence 2 * 2.4e-7 for these cases.
    Box columns 0..5 depend on neither and are held bit for bit; rpn_reg_label depends on both (tolerance of the CPU test)."""
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)          # noqa: E731
    want_boxes = z["c%d_gt_boxes3d" % k]
    ng = int(got["num_gt"][k])
    assert ng == len(want_boxes), k
    assert np.array_equal(bits(got["gt_boxes3d"][k][:ng, :6]), bits(want_boxes[:, :6])), k
    assert not got["gt_boxes3d"][k][ng:].any(), k
    assert np.abs(got["gt_boxes3d"][k][:ng, 6].astype(np.float64) - want_boxes[:, 6]).max(initial=0) <= 2 * 2.4e-7, k
    src, want_pts = got["src"][k], z["c%d_pts_rect" % k]
    moved = z["c%d_rect_ulp" % k].reshape(n_raw, 3).any(1)
    exact = (src >= n_raw) | ~moved[np.minimum(src, n_raw - 1)]
    assert exact.any() and (src >= 0).all(), k
    assert np.array_equal(bits(got["pts_rect"][k][exact]), bits(want_pts[exact])), k
    np.testing.assert_allclose(got["pts_rect"][k], want_pts, rtol=2e-6, atol=2e-5)
    assert np.array_equal(bits(got["pts_features"][k]), bits(z["c%d_pts_features" % k])), k
    assert np.array_equal(got["rpn_cls_label"][k], z["c%d_cls" % k].astype(np.int32)), k
    np.testing.assert_allclose(got["rpn_reg_label"][k], z["c%d_reg" % k], rtol=2e-6, atol=2e-5)


def test_fixture_parity(env):
    z, calib, cases = env
    B = len(cases)
    held = 0
    for k, kw in enumerate(cases):
        prep = _preparer(kw)
        got = _run(prep, calib, cases, kw["seed"])
        G = max(len(c["gt_boxes3d"]) for c in cases)
        K = 16 if kw["gt_aug"] is not None else 0
        want = _twin(calib, kw, k, got, kw, kw["seed"], G + K)
        _same(got, k, want, k)
        numpy_aug = ts.aug_params(kw["seed"], k, kw["aug"])
        assert _ulp_close(got["aug"][k][4], numpy_aug[4]) and _ulp_close(got["aug"][k][5], numpy_aug[5]), k
        assert got["gt_boxes3d"].shape == (B, G + K, 7)
        # where the reported cos and sin are numpy's bits (trivially so when the rotation did not run): the reference's own output
        rotated = not np.isnan(got["aug"][k][3])
        if not rotated or (got["aug"][k][4:6].view(np.uint64) == numpy_aug[4:6].view(np.uint64)).all():
            _same_as_fixture(z, k, got, len(kw["raw"]))
            held += 1
    assert held > 0


def _big_db(db):
    """the fixture's database plus one object of 1 500 points in front of the car"""
    r = np.random.default_rng(3)
    box = np.array([[2.0, 1.7, 18.0, 1.6, 1.7, 4.2, 0.4]], np.float32)
    p = np.stack([2.0 + r.uniform(-1, 1, 1500), 1.7 - r.uniform(0, 1.6, 1500), 18.0 + r.uniform(-1, 1, 1500)], 1).astype(np.float32)
    return {"boxes": np.concatenate([db["boxes"], box]), "alpha": np.concatenate([db["alpha"], [0.3]]).astype(np.float32),
            "npts": np.concatenate([db["npts"], [1500]]).astype(np.int32), "points": np.concatenate([db["points"], p]),
            "intensity": np.concatenate([db["intensity"], r.uniform(0, 1, 1500).astype(np.float32)])}


def test_ragged_batch(env):
    z, calib, cases = env
    base = cases[0]
    db = _big_db(base["db"])
    empty = dict(cases[1], raw=np.zeros((0, 4), np.float32))
    back = synthetic_scan(4000, 77, 0.5, 0.1)
    back[:, 0] = -np.abs(back[:, 0]) - np.float32(1.0)                          # lidar x is forward: every point behind the camera
    behind = dict(cases[4], raw=back)
    raises = dict(cases[5], all_gt_boxes3d=np.zeros((0, 7), np.float32))           # empty collision list: the reference raises
    large = dict(cases[6], raw=synthetic_scan(115000, 5, 0.5, 0.02))
    frames = [cases[0], empty, cases[2], behind, raises, cases[1], large]
    frames = [dict(f, db=db) for f in frames]
    settings = dict(base, aug={"AUG_METHOD_LIST": ts.METHODS, "AUG_METHOD_PROB": (1.0, 1.0, 0.5), "AUG_ROT_RANGE": 18})
    prep = _preparer(settings, db=db)
    got = _run(prep, calib, frames, 11)
    G = max(len(f["gt_boxes3d"]) for f in frames)
    for b, f in enumerate(frames):
        _same(got, b, _twin(calib, f, b, got, settings, 11, G + 16), b)
    # an empty scan / a scan behind the camera still receives the pasted objects: its edited cloud is exactly their points
    for b in (1, 3):
        assert got["count"][b] > 0 and (got["src"][b] >= len(frames[b]["raw"])).all() and got["status"][b] in (0, 1), b
    assert got["gt_aug_status"][4] == 1 and got["count"][0] > 0


def test_kitti_sized_frame(env):
    """~115 k raw points, npoints 16384, a pasted object of more than 1024 points: multi-block flag pass, paste pass, full LDS sort"""
    z, calib, cases = env
    db = _big_db(cases[0]["db"])
    frames = [dict(cases[0], raw=synthetic_scan(115000, 21, 0.5, 0.05), db=db), dict(cases[4], raw=synthetic_scan(113517, 22, 0.45, 0.05), db=db)]
    settings = dict(cases[0], npoints=16384, gt_aug=dict(cases[0]["gt_aug"], GT_AUG_HARD_RATIO=0.0))
    prep = _preparer(settings, db=db)
    hit = False
    for seed in (4, 7):
        got = _run(prep, calib, frames, seed)
        for b, f in enumerate(frames):
            _same(got, b, _twin(calib, f, b, got, settings, seed, max(len(x["gt_boxes3d"]) for x in frames) + 16), (seed, b))
            hit |= len(db["npts"]) - 1 in got["db_id"][b][:got["count"][b]]
        assert (got["status"] == 0).all() and (got["nvalid"] > 16384).all()
    assert hit, "the 1500-point object was never pasted: choose other seeds"


def test_degenerates_to_scene_preparer(env):
    from pointrcnn_amd import kitti_input, ops
    z, calib, cases = env
    frames = cases[:3] + [dict(cases[3], raw=np.zeros((0, 4), np.float32))]         # the last one: no valid point, status 2
    prep = _preparer(dict(cases[7], aug={"AUG_METHOD_LIST": (), "AUG_METHOD_PROB": (1, 1, 1), "AUG_ROT_RANGE": 18}))
    got = _run(prep, calib, frames, 9)
    inf = kitti_input.ScenePreparer(npoints=1024)
    ref = inf(inf.pack([f["raw"] for f in frames], [calib] * 4, [f["hw"] for f in frames], pin=False), 9)
    for key in ("pts_input", "pts_features", "src", "nvalid", "status"):
        assert np.array_equal(got[key], ref[key].cpu().numpy()), key
    assert got["status"][3] == 2
    G = got["gt_boxes3d"].shape[1]
    cls, reg = ops.rpn_labels(ref["pts_rect"], torch.from_numpy(got["gt_boxes3d"]).cuda(), torch.from_numpy(got["num_gt"]).cuda())
    assert np.array_equal(got["rpn_cls_label"], cls.cpu().numpy()) and np.array_equal(got["rpn_reg_label"], reg.cpu().numpy())
    assert G == max(len(f["gt_boxes3d"]) for f in frames)


@pytest.mark.parametrize("methods", [(), ("rotation",), ("scaling",), ("flip",), ("rotation", "scaling"), ("rotation", "flip"),
                                     ("scaling", "flip"), ts.METHODS])
def test_method_subsets_and_probabilities(env, methods):
    z, calib, cases = env
    frames = [cases[0], cases[5]]
    for prob in ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)):
        settings = dict(cases[0], aug={"AUG_METHOD_LIST": methods, "AUG_METHOD_PROB": prob, "AUG_ROT_RANGE": 18})
        got = _run(_preparer(settings), calib, frames, 13)
        on = prob[0] == 1.0
        for b, f in enumerate(frames):
            _same(got, b, _twin(calib, f, b, got, settings, 13, got["gt_boxes3d"].shape[1]), (methods, prob, b))
            assert (not np.isnan(got["aug"][b][3])) == (on and "rotation" in methods)
            assert (not np.isnan(got["aug"][b][6])) == (on and "scaling" in methods)
            assert (got["aug"][b][7] == 1.0) == (on and "flip" in methods)


def test_flip_probability_and_intensity(env):
    z, calib, cases = env
    small = dict(cases[7], raw=cases[7]["raw"][:600])
    settings = dict(cases[7], npoints=256, aug={"AUG_METHOD_LIST": ts.METHODS, "AUG_METHOD_PROB": (1.0, 1.0, 0.5), "AUG_ROT_RANGE": 18})
    got = _run(_preparer(settings), calib, [small] * 64, 17)
    flips = got["aug"][:, 7]
    assert 0 < flips.sum() < 64
    want = np.array([ts.aug_params(17, b, settings["aug"])[7] for b in range(64)])
    assert np.array_equal(flips, want)
    both = _run(_preparer(settings, use_intensity=True), calib, [small] * 4, 17)
    assert both["pts_input"].shape == (4, 256, 4)
    assert np.array_equal(both["pts_input"][..., :3], both["pts_rect"]) and np.array_equal(both["pts_input"][..., 3:], both["pts_features"])
    assert np.array_equal(both["pts_rect"], got["pts_rect"][:4])


def test_invariants_and_order(env):
    from pointrcnn_amd import ops
    z, calib, cases = env
    frames = [cases[0], cases[5], cases[6]]
    settings = dict(cases[0], aug={"AUG_METHOD_LIST": (), "AUG_METHOD_PROB": (1, 1, 1), "AUG_ROT_RANGE": 18})
    prep = _preparer(settings)
    runs = [_run(prep, calib, frames, 23) for _ in range(3)]
    for r in runs[1:]:
        assert all(np.array_equal(r[k], runs[0][k], equal_nan=True) for k in runs[0])
    other = _run(prep, calib, frames, 24)
    assert not np.array_equal(other["src"], runs[0]["src"])
    got = runs[0]
    db = frames[0]["db"]
    off = np.concatenate([[0], np.cumsum(db["npts"])])
    for b, f in enumerate(frames):
        n_raw = len(f["raw"])
        want = _twin(calib, f, b, got, settings, 23, got["gt_boxes3d"].shape[1])
        src, pts = got["src"][b], got["pts_rect"][b]
        boxes = want["sampler"]["boxes"].copy()
        assert len(boxes) == got["count"][b] > 0
        boxes[:, 3] += np.float32(2.0)
        inside = ops.pts_in_boxes3d(torch.from_numpy(pts).cuda(), torch.from_numpy(boxes).cuda()).cpu().numpy().any(0)
        assert not inside[src < n_raw].any(), b                            # no scene point inside an accepted box with h + 2
        ids, shift = want["sampler"]["ids"], want["sampler"]["y_shift"]
        start = n_raw + np.concatenate([[0], np.cumsum(db["npts"][ids])])
        for j in np.nonzero(src >= n_raw)[0]:                               # every pasted row is the right database point, shifted
            a = np.searchsorted(start, src[j], side="right") - 1
            p = db["points"][off[ids[a]] + src[j] - start[a]]
            assert pts[j, 0] == p[0] and pts[j, 2] == p[2] and pts[j, 1] == np.float32(np.float64(p[1]) - shift[a]), (b, j)
        assert (src >= n_raw).any()
        far = want["ident"][~(want["cloud"][:, 2] < np.float32(40.0))]
        assert got["status"][b] == 0 and set(far) <= set(src), b           # every far point of the edited cloud is present


def test_argument_errors(env):
    from pointrcnn_amd import _cabi, ops
    z, calib, cases = env
    kw = cases[0]
    with pytest.raises((ValueError, _cabi.PointOpsError)):
        _run(_preparer(kw, max_accept=65), calib, [kw], 1)
    # the entry point's own bounds on K and G + K, with hand-made accepted objects (count 0: nothing would be pasted)
    dev = torch.device("cuda")
    one = _preparer(kw).pack([kw["raw"]], [calib], [kw["hw"]], [kw["gt_boxes3d"]], [kw["gt_alpha"]], [kw["all_gt_boxes3d"]], [kw["plane"]], pin=False)
    one = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in one.items()}
    db = _database(kw["db"], 0.5)

    def accepted(K):
        return {"count": torch.zeros(1, dtype=torch.int32, device=dev), "db_id": torch.zeros((1, K), dtype=torch.int32, device=dev),
                "boxes3d": torch.zeros((1, K, 7), device=dev), "alpha": torch.zeros((1, K), device=dev),
                "y_shift": torch.zeros((1, K), dtype=torch.float64, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}

    def direct(G, K):
        return ops.train_scene_prepare(one["raw"], one["offsets"], one["max_points"], one["calib"], one["img_hw"], None, 1024, 1,
                                       torch.zeros((1, G, 7), device=dev), torch.zeros((1, G), device=dev),
                                       torch.zeros(1, dtype=torch.int32, device=dev), accepted(K), db)
    with pytest.raises(_cabi.PointOpsError, match="K=65"):
        direct(4, 65)
    with pytest.raises(_cabi.PointOpsError, match=r"G \+ K = 129"):
        direct(65, 64)
    assert direct(64, 64)["gt_boxes3d"].shape == (1, 128, 7)
    with pytest.raises(_cabi.PointOpsError):
        _run(_preparer(kw, npoints=16385), calib, [kw], 1)
    prep = _preparer(cases[7])
    t = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in
         prep.pack([kw["raw"]], [calib], [kw["hw"]], [kw["gt_boxes3d"]], [kw["gt_alpha"]], [kw["all_gt_boxes3d"]], [kw["plane"]], pin=False).items()}
    with pytest.raises(_cabi.PointOpsError, match="workspace too small"):
        ops.train_scene_prepare(t["raw"], t["offsets"], t["max_points"], t["calib"], t["img_hw"], None, 1024, 1, t["gt_boxes3d"],
                                t["gt_alpha"], t["num_gt"], workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
