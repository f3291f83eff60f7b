"""GPU: the RCNN offline training batch on the device (csrc/rcnn_offline.hip, kitti_input.RCNNOfflinePreparer).

prcnn_rcnn_offline_sample against the numpy twin (tests/rcnn_offline_twin.py, sine / cosine /
clip as csrc/ref_trig.h and csrc/quad_clip.h state them), BIT FOR BIT on every output: the IoU matrix, row maxima and labels,
counts, status, the source RoI of every slot, the slot's RoI after the noise loop, its label and the loop's last IoU.

Frames: tests/rcnn_offline_cases.py (every list combination the reference distinguishes, the case it raises on, duplicates in the
foreground list, identical RoIs, M = 2 / G = 1, M = 300 / G = 17, an odd slot quota), padded with NaN rows past the counts; one
frame at the workload's shape (M = 300, G = 17, R = 64); one with M = 2500 (past the 48 KB of dynamic LDS a kernel gets unasked).
The batch order must not matter: the frame id keys the random table.

RCNNOfflinePreparer (sample + prcnn_roipool3d + prcnn_rcnn_offline_finish) against the twin's whole frame
(rcnn_offline_twin.offline_frame: the host twin of roipool3d_cpu, csrc/ref_trig.h's sine / cosine / atan2), BIT FOR BIT on every
key: the fixture's frames (AUG_DATA and USE_INTENSITY on and off) and one frame of N = 4096, M = 300, G = 17, R = 64, S = 512; the
packed batch in another order; the frames the reference raises on; eval_batch against the oracle; RCNNNet's ROI_SAMPLE_JIT False
entry and one RCNNOfflineTrainer step on the preparer's batch."""
import numpy as np
import pytest
import torch

import rcnn_offline_cases as rc
import rcnn_offline_twin as ot

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(rc.CASES)
KEYS = ("iou3d", "max_overlaps", "gt_assignment", "counts", "status", "src", "rois", "gt_of_rois", "roi_iou")
_runs = {}


def groups():
    """case names that can share a launch: same slot count and noise method"""
    g = {}
    for n in NAMES:
        g.setdefault((rc.CASES[n][1], rc.METHOD.get(n, "multiple")), []).append(n)
    return g


def run(dev, names, R, method, ids="case", pad=(5, 2), order=None):
    from pointrcnn_amd import ops
    key = (tuple(names), R, method, ids, pad, order)
    if key not in _runs:
        roi, nroi, gt, ngt = rc.batch(names, *pad)
        fid = np.array([NAMES.index(n) for n in names], np.int32)
        o = np.arange(len(names)) if order is None else np.asarray(order)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a[o])).to(dev)          # noqa: E731
        out = ops.rcnn_offline_sample(T(roi), T(nroi), T(gt), T(ngt), R, aug_method=method, seed=rc.SEED,
                                      frame_ids=T(fid) if ids == "case" else None)
        _runs[key] = {k: v.cpu().numpy() for k, v in out.items()}
    return _runs[key]


def compare(got, b, want, m, g, what):
    """frame b of a device result against one twin frame of m RoIs and g labels"""
    for k in KEYS:
        a, w = np.atleast_1d(got[k][b]), np.atleast_1d(want[k])
        if k == "iou3d":
            assert not a[m:].any() and not a[:, g:].any(), (what, "padding of iou3d")
            a = a[:m, :g]
        elif k in ("max_overlaps", "gt_assignment"):
            assert (a[m:] == (0 if k == "max_overlaps" else -1)).all(), (what, "padding of " + k)
            a = a[:m]
        same = np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(w.astype(a.dtype)).view(np.uint32)
        assert same.all(), "%s: %s differs at %s: %s != %s" % (what, k, np.argwhere(~same)[0], a[~same][0], w.astype(a.dtype)[~same][0])


@pytest.mark.parametrize("R,method", list(groups()))
def test_every_output_equals_the_twin_bit_for_bit(dev, R, method):
    names = groups()[(R, method)]
    got = run(dev, names, R, method)
    for b, n in enumerate(names):
        roi, gt = rc.CASES[n][0]()
        compare(got, b, rc.twin_result(n, NAMES.index(n)), len(roi), len(gt), n)


def test_frames_the_reference_raises_on_report_status_and_are_cleared(dev):
    names = groups()[(16, "multiple")]
    got = run(dev, names, 16, "multiple")
    b = names.index("foreground only")
    assert got["status"][b] == 1 and got["counts"][b][0] > 0 and got["counts"][b][3] == 0
    assert (got["src"][b] == -1).all() and not got["rois"][b].any() and not got["gt_of_rois"][b].any() and not got["roi_iou"][b].any()
    assert got["max_overlaps"][b].max() >= F32(0.55)                    # the matrix side of the frame is still there
    assert [s for i, s in enumerate(got["status"]) if i != b] == [0] * (len(names) - 1)
    # no label / no RoI: counted, not read
    from pointrcnn_amd import ops
    roi, nroi, gt, ngt = rc.batch(["M 2 G 1", "M 2 G 1", "M 2 G 1"], 1, 1)
    nroi[1], ngt[2] = 0, 0
    T = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    out = {k: v.cpu().numpy() for k, v in ops.rcnn_offline_sample(T(roi), T(nroi), T(gt), T(ngt), 16, seed=rc.SEED).items()}
    assert list(out["status"]) == [0, 1, 2]
    for b in (1, 2):
        assert (out["src"][b] == -1).all() and not out["rois"][b].any() and not out["roi_iou"][b].any() and not out["iou3d"][b].any()
        assert (out["gt_assignment"][b] == -1).all() and not out["counts"][b].any()
    r, g = rc.CASES["M 2 G 1"][0]()
    compare(out, 0, ot.sample_frame(r, g, rc.SEED, 0, dict(ROI_PER_IMAGE=16)), 2, 1, "frame id = position when no ids are given")


def test_batch_order_does_not_matter(dev):
    names = groups()[(16, "multiple")]
    order = tuple(reversed(range(len(names))))
    a, b = run(dev, names, 16, "multiple"), run(dev, names, 16, "multiple", order=order)
    for k in KEYS:
        assert np.array_equal(a[k][list(order)].view(np.uint32), b[k].view(np.uint32)), k
    c = run(dev, names, 16, "multiple", ids="position")
    assert not np.array_equal(a["src"][1:], c["src"][1:])                # and the ids are what keys the table


def test_workload_shape_and_large_roi_count(dev):
    from pointrcnn_amd import ops
    T = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    for what, (roi, gt), R, method in (("M 300 G 17 R 64", rc.frame(21, 300, 17, ("near", "hard", "far", "graze")), 64, "multiple"),
                                       ("M 2500", rc.frame(22, 2500, 3, ("far", "far", "far", "near", "far", "hard", "far")), 16, "single")):
        fid = np.array([1234567], np.int32)
        out = ops.rcnn_offline_sample(T(roi[None]), T(np.array([len(roi)], np.int32)), T(gt[None]), T(np.array([len(gt)], np.int32)), R,
                                      aug_method=method, seed=7, frame_ids=T(fid))
        want = ot.sample_frame(roi, gt, 7, 1234567, dict(ROI_PER_IMAGE=R, REG_AUG_METHOD=method))
        assert want["status"] == 0 and want["counts"][3] == R // 2
        compare({k: v.cpu().numpy() for k, v in out.items()}, 0, want, len(roi), len(gt), what)


def test_unsupported_requests_are_refused(dev):
    from pointrcnn_amd import _cabi, ops
    roi, nroi, gt, ngt = (torch.from_numpy(a).to(dev) for a in rc.batch(["M 2 G 1"]))
    with pytest.raises(ValueError, match="normal"):
        ops.rcnn_offline_sample(roi, nroi, gt, ngt, 16, aug_method="normal")
    with pytest.raises(_cabi.PointOpsError, match="aug_times"):
        ops.rcnn_offline_sample(roi, nroi, gt, ngt, 16, aug_times=17)
    with pytest.raises(_cabi.PointOpsError, match="bad shape"):
        ops.rcnn_offline_sample(torch.zeros((1, 4097, 7), device=dev), nroi, gt, ngt, 16)


# ---------------------------------------------------------------------------------------------- the whole batch
OUT_KEYS = ("pts_input", "pts_features", "cls_label", "reg_valid_mask", "gt_boxes3d_ct", "roi_boxes3d", "gt_boxes3d", "gt_iou", "src")
_prep = {}


def _cfg(R, method, aug, ui, S=rc.S_POINTS):
    from pointrcnn_amd.rcnn import RCNNConfig
    return type("Cfg", (RCNNConfig,), dict(ROI_SAMPLE_JIT=False, NUM_POINTS=S, ROI_PER_IMAGE=R, REG_AUG_METHOD=method, AUG_DATA=aug,
                                           USE_INTENSITY=ui))


def _frame(k, n=rc.N_POINTS, c=rc.N_CHANNELS):
    name = NAMES[k]
    roi, gt = rc.CASES[name][0]()
    return dict(rc.frame_points(k, gt, n, c), roi_boxes3d=roi, gt_boxes3d=gt, roi_scores=np.linspace(1, 0, len(roi)).astype(F32), sample_id=k)


def _twin_rows(fr, cfg, seed):
    t = ot.offline_frame(fr, seed, fr["sample_id"], dict(ROI_PER_IMAGE=cfg.ROI_PER_IMAGE, REG_AUG_METHOD=cfg.REG_AUG_METHOD), S=cfg.NUM_POINTS,
                         use_intensity=cfg.USE_INTENSITY, methods=("rotation", "scaling", "flip") if cfg.AUG_DATA else ())
    t["gt_iou"] = t["roi_iou"]
    return t


def _check_frame(out, b, R, want, what):
    for k in OUT_KEYS + ("status",):
        a = out[k][b] if k == "status" else out[k][b * R:(b + 1) * R]
        a, w = np.atleast_1d(a), np.atleast_1d(np.asarray(want[k]).astype(a.dtype))
        same = np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(w).view(np.uint32)
        assert same.all(), "%s: %s differs at %s (%d values): %s != %s" % (what, k, np.argwhere(~same)[0], (~same).sum(), a[~same][0], w[~same][0])
    assert np.array_equal(out["roi_size"][b * R:(b + 1) * R], out["roi_boxes3d"][b * R:(b + 1) * R, 3:6])
    if not want["status"]:
        assert np.array_equal(out["pooled_empty_flag"][b * R:(b + 1) * R], want["empty"])


def _fixture_groups():
    g = {}
    for k, n in enumerate(NAMES):
        g.setdefault((rc.CASES[n][1], rc.METHOD.get(n, "multiple")) + rc.frame_config(k), []).append(k)
    return g


def _prepared(dev, key, order=None):
    from pointrcnn_amd import kitti_input
    if (key, order) not in _prep:
        ks = _fixture_groups()[key]
        ks = ks if order is None else [ks[i] for i in order]
        prep = kitti_input.RCNNOfflinePreparer(_cfg(*key), dev)
        out = prep(prep.pack([_frame(k) for k in ks]), seed=rc.SEED)
        _prep[(key, order)] = (ks, {k: v.cpu().numpy() for k, v in out.items()})
    return _prep[(key, order)]


@pytest.mark.parametrize("key", list(_fixture_groups()), ids=lambda k: "R%d-%s-aug%d-intensity%d" % k)
def test_preparer_equals_the_twin_on_the_fixture_frames(dev, key):
    ks, out = _prepared(dev, key)
    cfg = _cfg(*key)
    assert out["pts_input"].shape == (len(ks) * key[0], rc.S_POINTS, 3 + 1 + int(key[3]) + 1) and out["pts_features"].shape[2] == rc.N_CHANNELS
    for b, k in enumerate(ks):
        want = _twin_rows(_frame(k), cfg, rc.SEED)
        _check_frame(out, b, key[0], want, NAMES[k])
        if want["status"]:                                  # the frame the reference raises on: nothing to train on
            rows = slice(b * key[0], (b + 1) * key[0])
            assert (out["cls_label"][rows] == -1).all() and not out["reg_valid_mask"][rows].any() and not out["roi_boxes3d"][rows].any()
            assert not out["pts_input"][rows][:, :, :3].any() and (out["src"][rows] == -1).all()


def test_packed_batch_in_another_order_gives_the_same_frames(dev):
    key = max(_fixture_groups(), key=lambda k: len(_fixture_groups()[k]))
    n = len(_fixture_groups()[key])
    assert n >= 2
    (ka, a), (kb, b) = _prepared(dev, key), _prepared(dev, key, order=tuple(reversed(range(n))))
    R = key[0]
    for i, k in enumerate(ka):
        j = kb.index(k)
        for name in OUT_KEYS:
            assert np.array_equal(a[name][i * R:(i + 1) * R].view(np.uint32), b[name][j * R:(j + 1) * R].view(np.uint32)), (NAMES[k], name)
        assert a["status"][i] == b["status"][j]


def test_preparer_at_the_workload_shape(dev):
    """N = 4096, M = 300, G = 17, R = 64, S = 512, 128 feature channels: twin only"""
    from pointrcnn_amd import kitti_input
    roi, gt = rc.frame(21, 300, 17, ("near", "hard", "far", "graze"))
    fr = dict(rc.frame_points(40, gt, 4096, 128), roi_boxes3d=roi, gt_boxes3d=gt, roi_scores=np.zeros(300, F32), sample_id=4321)
    cfg = _cfg(64, "multiple", True, False, S=512)
    prep = kitti_input.RCNNOfflinePreparer(cfg, dev)
    out = {k: v.cpu().numpy() for k, v in prep(prep.pack([fr]), seed=9).items()}
    want = _twin_rows(fr, cfg, 9)
    assert want["status"] == 0 and want["empty"].any() and not want["empty"].all()
    _check_frame(out, 0, 64, want, "workload shape")


def test_eval_batch_pools_every_roi_into_its_canonical_frame(dev, cpu):
    from pointrcnn_amd import kitti_input, rcnn
    cfg = _cfg(16, "multiple", True, False)
    prep = kitti_input.RCNNOfflinePreparer(cfg, dev)
    frames = [_frame(0), _frame(7)]
    out = {k: v.cpu().numpy() for k, v in prep.eval_batch(prep.pack(frames)).items()}
    M = max(len(f["roi_boxes3d"]) for f in frames)
    assert list(out["num_roi"]) == [len(f["roi_boxes3d"]) for f in frames] and out["pts_input"].shape == (2 * M, rc.S_POINTS, 5)
    for b, f in enumerate(frames):
        m = len(f["roi_boxes3d"])
        xyz = f["rpn_xyz"]
        feat = np.concatenate([f["seg_mask"][:, None], (np.linalg.norm(xyz, axis=1) / 70.0 - 0.5).astype(F32)[:, None], f["rpn_features"]], 1)
        pooled, empty = cpu.roipool3d(xyz[None], ot.enlarge(f["roi_boxes3d"], 1.0)[None], feat[None], rc.S_POINTS)
        want = cpu.canonical_transform(pooled, f["roi_boxes3d"][None])[0]
        rows = slice(b * M, b * M + m)
        assert np.array_equal(out["pts_input"][rows], want[..., :5])
        assert np.array_equal(out["pts_features"][rows], want[..., 5:]) and np.array_equal(out["pooled_empty_flag"][rows], empty[0])
        assert np.array_equal(out["roi_boxes3d"][rows], f["roi_boxes3d"]) and np.array_equal(out["roi_size"][rows], f["roi_boxes3d"][:, 3:6])
    with pytest.raises(NotImplementedError):
        kitti_input.RCNNOfflinePreparer(_cfg(16, "multiple", True, True), dev).eval_batch(prep.pack(frames))
    assert rcnn.RCNNConfig.ROI_SAMPLE_JIT is True


# ---------------------------------------------------------------------------------------------- the network entry and the trainer
def _train_batch(dev):
    """two fixture frames with 128 feature channels through the preparer: what RCNNOfflineTrainer.step consumes"""
    from pointrcnn_amd import kitti_input
    cfg = _cfg(16, "multiple", True, False, S=128)
    prep = kitti_input.RCNNOfflinePreparer(cfg, dev)
    return cfg, prep(prep.pack([_frame(k, c=128) for k in (0, 4)]), seed=5)


def test_offline_entry_keys_shapes_and_both_layouts(dev):
    from pointrcnn_amd import rcnn
    cfg, batch = _train_batch(dev)
    torch.manual_seed(4)
    net = rcnn.RCNNNet(cfg=cfg).to(dev)
    rows = 2 * cfg.ROI_PER_IMAGE
    assert (batch["cls_label"] == 1).any() and (batch["cls_label"] == 0).any() and (batch["reg_valid_mask"] == 1).any()
    net.train()
    out = net(batch)
    assert set(out) == {"rcnn_cls", "rcnn_reg", "pts_input", "roi_boxes3d", "cls_label", "reg_valid_mask", "gt_of_rois"}      # rcnn_net.py:155-190
    assert out["rcnn_cls"].shape == (rows, 1) and out["rcnn_reg"].shape == (rows, net.reg_channel)
    assert out["pts_input"].shape == (rows, cfg.NUM_POINTS, 5 + 128) and out["roi_boxes3d"].shape == (rows, 7)
    assert out["cls_label"].shape == (rows,) and out["reg_valid_mask"].shape == (rows,) and out["gt_of_rois"].shape == (rows, 7)
    assert torch.equal(out["gt_of_rois"], batch["gt_boxes3d_ct"])
    # with the frame axis collate_batch leaves in front of the RoI axis: the same rows, the same outputs
    keys = ("pts_input", "pts_features", "cls_label", "reg_valid_mask", "gt_boxes3d_ct", "roi_boxes3d")
    framed = {k: batch[k].reshape((2, cfg.ROI_PER_IMAGE) + tuple(batch[k].shape[1:])) for k in keys}
    out2 = net(framed)
    assert torch.equal(out2["rcnn_cls"], out["rcnn_cls"]) and torch.equal(out2["rcnn_reg"], out["rcnn_reg"])
    net.eval()
    with torch.no_grad():
        assert set(net({"pts_input": out["pts_input"], "roi_boxes3d": batch["roi_boxes3d"]})) == {"rcnn_cls", "rcnn_reg"}
    with pytest.raises(ValueError, match="rows"):
        net({"pts_input": out["pts_input"], "roi_boxes3d": batch["roi_boxes3d"][:3]})


@pytest.mark.parametrize("fused_loss", [True, False], ids=["fused-loss", "composed-loss"])
def test_offline_trainer_step_against_the_composed_path(dev, fused_loss):
    """RCNNOfflineTrainer on the preparer's batch: the hand-written training stacks against the same modules run through torch
    (pointnet2_modules.TRAIN_FUSED off), loss 1e-5 and every parameter gradient 5e-3 in norm (tests/test_gpu_train_rcnn.py's bars);
    then the step itself lowers the loss on that batch"""
    import copy
    from pointrcnn_amd import rcnn, train_functions as tf
    import pointnet2_lib.pointnet2.pointnet2_modules as pm
    cfg, batch = _train_batch(dev)
    torch.manual_seed(4)
    net = rcnn.RCNNNet(cfg=cfg).to(dev)
    ref = copy.deepcopy(net)
    ta, tb = tf.RCNNOfflineTrainer(net, fused_loss=fused_loss), tf.RCNNOfflineTrainer(ref, fused_loss=False)
    net.train(), ref.train()
    la = ta.loss(batch)
    la.backward()
    pm.TRAIN_FUSED = False
    try:
        lb = tb.loss(batch)
        lb.backward()
    finally:
        pm.TRAIN_FUSED = True
    assert abs(la.item() - lb.item()) <= 1e-5 * max(1.0, abs(lb.item())), (la.item(), lb.item())
    pa, pb = dict(net.named_parameters()), dict(ref.named_parameters())
    worst = 0.0
    for n in pa:
        assert pa[n].grad is not None and pb[n].grad is not None, n
        worst = max(worst, (pa[n].grad - pb[n].grad).double().norm().item() / max(1e-12, pb[n].grad.double().norm().item()))
    assert worst <= 5e-3, worst
    l0 = float(ta.step(batch).item())
    for _ in range(5):
        l1 = float(ta.step(batch).item())
    assert np.isfinite(l1) and l1 < l0, (l0, l1)
    with pytest.raises(ValueError, match="ROI_SAMPLE_JIT"):
        tf.RCNNOfflineTrainer(rcnn.RCNNNet())
