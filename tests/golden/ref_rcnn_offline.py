"""Run the REFERENCE's own KittiRCNNDataset.get_rcnn_training_sample_batch (lib/datasets/kitti_rcnn_dataset.py:876-1022) on the
synthetic frames of tests/rcnn_offline_cases.py, with its random calls answered from the counter table of csrc/rcnn_offline.hip.

Only used to GENERATE tests/golden/rcnn_offline_ref.npz (python tests/golden/ref_rcnn_offline.py) where the reference tree is:
no test reads that tree.  Every frame is a small tree on disk: label_2 and proposal text files the reference parses itself
(get_objects_from_label, objs_to_boxes3d, filtrate_objects) and the five RPN dumps written by kitti_output.save_rpn_features.
What is replaced:
  - kitti_utils.get_iou3d -> tests/train_input_twin.py corner_iou3d (shapely is not installed here).  The corners it is given are
    the reference's own boxes3d_to_corners3d (numpy's float32 cosine / matmul, the float64 path of a noisy box);
  - roipool3d_cuda.roipool3d_cpu (a compiled extension) -> this library's host twin of the same C++ code;
  - np.random.permutation / rand / randint while the method runs -> the table (streams 40, 42, 43, 50).
aug_roi_by_noise_batch is called through a wrapper that hands it one slot at a time (its slots are independent) so that every draw
knows its slot, and records what it returns: the fixture holds the sampled source boxes, the boxes after the noise loop, the
loop's last IoU and the labels of every slot, plus the whole of sample_info.  data_augmentation is wrapped the same way (the slot
keys its draws, streams 51-53) and roipool3d_cpu's return is recorded (the pooled points before the augmentation, the empty flags).
AUG_DATA and USE_INTENSITY are on and off across the frames (rcnn_offline_cases.frame_config).
"""
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
REFERENCE = os.environ.get("PRCNN_REFERENCE", "/root/reference")
for p in (TESTS, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import rcnn_offline_cases as rc          # noqa: E402
import rcnn_offline_twin as ot           # noqa: E402
import train_input_twin as tw            # noqa: E402

S = rc.S_POINTS


class Answers:
    """the random calls of one get_rcnn_training_sample_batch call, answered from the table"""

    def __init__(self, seed, frame):
        self.seed, self.frame, self.bg, self.slot, self.attempt, self.q, self.aug_slot = seed, frame, [], None, -1, 0, None

    def permutation(self, n):
        keys = [tw.rand32(self.seed, ot.STREAM_FG_KEY, self.frame, t) for t in range(n)]
        return np.array(sorted(range(n), key=lambda t: (keys[t], t)), np.int64)

    def uniform(self, lo, hi):
        stream = ot.STREAM_AUG_SCALE if lo == 0.95 else ot.STREAM_AUG_ANGLE
        return lo + (hi - lo) * tw.u01(tw.rand32(self.seed, stream, self.frame, self.aug_slot))

    def rand(self, *shape):
        if self.aug_slot is not None:                       # data_augmentation: aug_enable = 1 - rand(3)
            return np.array([tw.u01(tw.rand32(self.seed, ot.STREAM_AUG_ENABLE, self.frame, self.aug_slot * 4 + i)) for i in range(shape[0])])
        if self.slot is None:                               # sample_bg_inds: floor(u * len) == below(r, len) for u = r / 2^32
            stream = self.bg.pop(0) if self.bg else 41      # 41: the draw with replacement of the foreground-only case, which raises next (:923)
            return np.array([tw.rand32(self.seed, stream, self.frame, t) / 4294967296.0 for t in range(shape[0])])
        base = (self.slot * 16 + self.attempt) * 16
        if not shape:                                       # the keep-the-original draw opens an attempt
            self.attempt += 1
            self.q = 1
            return tw.u01(tw.rand32(self.seed, ot.STREAM_NOISE, self.frame, base + 16 + 8))
        q, self.q = self.q, self.q + shape[0]
        return np.array([tw.u01(tw.rand32(self.seed, ot.STREAM_NOISE, self.frame, base + q + k)) for k in range(shape[0])])

    def randint(self, n):
        return tw.below(tw.rand32(self.seed, ot.STREAM_NOISE, self.frame, (self.slot * 16 + self.attempt) * 16), n)


def main():
    for p in (os.path.join(TESTS, "compat"), REFERENCE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from pointrcnn_amd import _cabi, kitti_output
    lib = _cabi.lib()
    mod = sys.modules.setdefault("roipool3d_cuda", types.ModuleType("roipool3d_cuda"))

    def roipool3d_cpu(pts, boxes3d, feat, pooled_pts, pooled_features, pooled_empty_flag):      # roipool3d.cpp:127-195 through the host twin
        assert pooled_empty_flag.dtype == torch.int64
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (pts, boxes3d, feat, pooled_pts, pooled_features))
        _cabi.check(lib.prcnn_host_roipool3d(pts.data_ptr(), boxes3d.data_ptr(), feat.data_ptr(), pts.shape[0], boxes3d.shape[0],
                                             feat.shape[1], pooled_pts.shape[1], pooled_pts.data_ptr(), pooled_features.data_ptr(),
                                             pooled_empty_flag.data_ptr()))
        return 1
    mod.roipool3d_cpu = roipool3d_cpu
    sys.modules.setdefault("iou3d_cuda", types.ModuleType("iou3d_cuda"))
    import yaml
    _load = yaml.load
    yaml.load = lambda f, Loader=yaml.SafeLoader: _load(f, Loader=Loader)      # lib/config.py predates PyYAML 6
    from lib.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(REFERENCE, "tools/cfgs/default.yaml"))
    yaml.load = _load
    import lib.utils.kitti_utils as kitti_utils
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    kitti_utils.get_iou3d = tw.corner_iou3d
    cfg.RCNN.NUM_POINTS = S
    cfg.RCNN.ROI_SAMPLE_JIT = False

    root = os.path.join(HERE, "_rcnn_offline_tmp")
    shutil.rmtree(root, ignore_errors=True)
    for d in ("label_2", "rois", "features"):
        os.makedirs(os.path.join(root, d))
    rng = np.random.default_rng(99)
    out = {"names": np.array(list(rc.CASES)), "seed": rc.SEED, "numpy": np.__version__}
    saved = (np.random.permutation, np.random.rand, np.random.randint, np.random.uniform)
    import lib.utils.roipool3d.roipool3d_utils as roipool3d_utils
    pool_orig = roipool3d_utils.roipool3d_cpu
    steps = {"xyz": 0.0, "ct": 0.0, "ry": 0.0}
    for k, name in enumerate(rc.CASES):
        roi, gt = rc.CASES[name][0]()
        R, method = rc.CASES[name][1], rc.METHOD.get(name, "multiple")
        cfg.RCNN.ROI_PER_IMAGE, cfg.RCNN.REG_AUG_METHOD = R, method
        with open(os.path.join(root, "label_2", "%06d.txt" % k), "w") as f:   # with objects that filtrate_objects drops
            f.write("".join(ln + "\n" for ln in rc.label_text(gt)))
        with open(os.path.join(root, "rois", "%06d.txt" % k), "w") as f:
            f.write("".join(ln + "\n" for ln in rc.roi_text(roi)))
        cfg.AUG_DATA, cfg.RCNN.USE_INTENSITY = rc.frame_config(k)
        fp = rc.frame_points(k, gt)
        kitti_output.save_rpn_features(fp["seg_mask"], fp["rawscore"], fp["rpn_intensity"].reshape(-1, 1), fp["rpn_xyz"], fp["rpn_features"],
                                       os.path.join(root, "features"), k)
        ds = KittiRCNNDataset.__new__(KittiRCNNDataset)
        ds.mode, ds.classes, ds.sample_id_list = "TRAIN", ("Background", "Car"), [k]
        ds.label_dir = os.path.join(root, "label_2")
        ds.rcnn_training_roi_dir, ds.rcnn_training_feature_dir = os.path.join(root, "rois"), os.path.join(root, "features")
        ans = Answers(rc.SEED, k)
        rec = {"calls": []}
        bg_orig, noise_orig = ds.sample_bg_inds, ds.aug_roi_by_noise_batch

        def sample_bg_inds(hard, easy, n, ans=ans, bg_orig=bg_orig):
            ans.bg = ([ot.STREAM_HARD] if hard.size else []) + ([ot.STREAM_EASY] if easy.size else [])
            return bg_orig(hard, easy, n)

        def aug_roi_by_noise_batch(rois, gts, aug_times=10, ans=ans, rec=rec, noise_orig=noise_orig):
            first = sum(len(c[0]) for c in rec["calls"])
            src, iou = rois.copy(), np.zeros(len(rois), np.float32)
            for i in range(len(rois)):
                ans.slot, ans.attempt = first + i, -1
                rois[i:i + 1], iou[i:i + 1] = noise_orig(rois[i:i + 1], gts[i:i + 1], aug_times=aug_times)
            ans.slot = None
            rec["calls"].append((src, rois.copy(), iou.copy(), gts.copy(), aug_times))
            return rois, iou
        aug_orig = ds.data_augmentation

        def data_augmentation(pts, boxes, alpha, ans=ans, rec=rec, aug_orig=aug_orig, **kw):
            ans.aug_slot = rec.setdefault("aug", 0)
            rec["aug"] += 1
            try:
                return aug_orig(pts, boxes, alpha, **kw)
            finally:
                ans.aug_slot = None

        def roipool3d_cpu(*a, rec=rec, **kw):
            r = pool_orig(*a, **kw)
            rec["pooled_xyz"], rec["empty"] = r[0][:, :, 0:3].copy(), np.asarray(r[2]).copy()
            return r
        ds.sample_bg_inds, ds.aug_roi_by_noise_batch, ds.data_augmentation = sample_bg_inds, aug_roi_by_noise_batch, data_augmentation
        roipool3d_utils.roipool3d_cpu = roipool3d_cpu
        np.random.permutation, np.random.rand, np.random.randint, np.random.uniform = ans.permutation, ans.rand, ans.randint, ans.uniform
        raised, info = "", None
        try:
            info = ds.get_rcnn_training_sample_batch(0)
        except Exception as e:      # noqa: BLE001
            raised = "%s: %s" % (type(e).__name__, e)
        finally:
            np.random.permutation, np.random.rand, np.random.randint, np.random.uniform = saved
            roipool3d_utils.roipool3d_cpu = pool_orig
        parsed_roi = kitti_utils.objs_to_boxes3d(kitti_utils.get_objects_from_label(os.path.join(root, "rois", "%06d.txt" % k)))
        parsed_gt = kitti_utils.objs_to_boxes3d(ds.filtrate_objects(ds.get_label(k)))
        out.update({"c%d_roi" % k: parsed_roi, "c%d_gt" % k: parsed_gt, "c%d_raised" % k: raised, "c%d_R" % k: R, "c%d_method" % k: method})
        if info is not None:
            cat = lambda j: np.concatenate([c[j] for c in rec["calls"]])          # noqa: E731
            fs = sum(len(c[0]) for c in rec["calls"] if c[4] == 10)
            out.update({"c%d_src_boxes" % k: cat(0), "c%d_rois" % k: cat(1), "c%d_roi_iou" % k: cat(2), "c%d_gt_of_rois" % k: cat(3),
                        "c%d_fs" % k: fs, "c%d_cls_label" % k: info["cls_label"], "c%d_reg_valid_mask" % k: info["reg_valid_mask"],
                        "c%d_info_rois" % k: info["roi_boxes3d"], "c%d_info_gt" % k: info["gt_boxes3d"],
                        "c%d_pts_input" % k: info["pts_input"], "c%d_pts_features" % k: info["pts_features"],
                        "c%d_gt_ct" % k: info["gt_boxes3d_ct"], "c%d_empty" % k: rec["empty"].astype(np.int8),
                        "c%d_pooled_xyz" % k: rec["pooled_xyz"]})
            # how far the twin in the CONTRACT's arithmetic (csrc/ref_trig.h sine / cosine / atan2) is from the reference, in float32
            # steps of the frame's largest coordinate: the bar of tests/test_rcnn_offline_cpu.py is this maximum plus one step
            aug, ui = rc.frame_config(k)
            t = ot.offline_frame(dict(fp, roi_boxes3d=parsed_roi, gt_boxes3d=parsed_gt), rc.SEED, k,
                                 dict(ROI_PER_IMAGE=R, REG_AUG_METHOD=method), S=S, use_intensity=ui,
                                 methods=tuple(cfg.AUG_METHOD_LIST) if aug else (), flip_prob=cfg.AUG_METHOD_PROB[2],
                                 rot_range=cfg.AUG_ROT_RANGE, sample_trig=(np.cos, np.sin))
            step = float(np.spacing(np.float32(max(np.abs(fp["rpn_xyz"]).max(), np.abs(parsed_roi[:, :3]).max()))))
            steps["xyz"] = max(steps["xyz"], float(np.abs(t["pts_input"][:, :, :3].astype(np.float64) - info["pts_input"][:, :, :3]).max()) / step)
            steps["ct"] = max(steps["ct"], float(np.abs(t["gt_boxes3d_ct"][:, :6].astype(np.float64) - info["gt_boxes3d_ct"][:, :6]).max()) / step)
            rys = np.stack([t["roi_boxes3d"][:, 6], t["gt_boxes3d"][:, 6], t["gt_boxes3d_ct"][:, 6]]).astype(np.float64)
            ref_rys = np.stack([info["roi_boxes3d"][:, 6], info["gt_boxes3d"][:, 6], info["gt_boxes3d_ct"][:, 6]])
            steps["ry"] = max(steps["ry"], float(np.abs(rys - ref_rys).max()) / float(np.spacing(np.float32(2 * np.pi))))
            out["c%d_step" % k] = step
        print("case %d (%s): %s" % (k, name, raised or "fg slots %d of %d, empty %d, steps so far %s" % (out["c%d_fs" % k], R, int(rec["empty"].sum()), steps)))
    shutil.rmtree(root, ignore_errors=True)
    out.update({"steps_xyz": steps["xyz"], "steps_ct": steps["ct"], "steps_ry": steps["ry"]})
    np.savez_compressed(os.path.join(HERE, "rcnn_offline_ref.npz"), **out)


if __name__ == "__main__":
    main()
