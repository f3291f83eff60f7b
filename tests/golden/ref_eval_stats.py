"""Run the REFERENCE's own eval_one_epoch_rpn / eval_one_epoch_rcnn / eval_one_epoch_joint (tools/eval_rcnn.py:113-253, :256-456,
:459-683) on the CPU over recorded model outputs and keep their returned dictionaries.

Only used to GENERATE tests/golden/eval_stats_ref.npz (needs the reference tree; build container only).  tools/eval_rcnn.py is imported as
a module with `sys.argv` set to the command line of the mode, inside cpu_ops.oracle_ops() (the compiled extensions -> the CPU oracle in the
kernels' arithmetic) and cpu_ops.cuda_is_cpu() (`.cuda()` a no-op).  What is replaced around the three functions, all of it outside
them: the model (a stub that replays recorded outputs: rois, rcnn_reg, rcnn_cls, seg_result, rpn_cls ...; in rpn mode also
model.rpn.proposal_layer), the dataloader (a list of batch dictionaries with a stub `.dataset`), `save_kitti_format` (a recorder of the
number of boxes per final result file -- the `num` of the detection select) and `decode_bbox_target` (the reference's own function,
wrapped to keep the boxes it returns: they are an INPUT of EvalStats.update).  cfg.TEST.SPLIT = 'test' skips the AP call.  The loops
themselves -- what is counted, compared, divided and summed -- run unmodified.

Per mode two batches of B = 3 frames (rcnn mode: six iterations of its batch_size == 1 loop): frame 1 of the first batch has an all-zero
ground truth (rpn mode keeps row 0 as a box that is never recalled, joint mode counts nothing), the second batch has gt_cols = 8 in rpn
and joint mode, an all-zero row sits in the middle of one frame's boxes.  make_golden() checks on the reference's numbers alone that the
committed inputs discriminate (see `_check`)."""
import importlib.util
import logging
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

REFERENCE = os.environ.get("PRCNN_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
B, M, G, N = 3, 24, 6, 192
THRESH = (0.1, 0.3, 0.5, 0.7, 0.9)
F32 = np.float32


def available():
    return os.path.isfile(os.path.join(REFERENCE, "tools", "eval_rcnn.py"))


def _paths():
    for p in (os.path.join(REFERENCE, "tools"), REFERENCE, ROOT, TESTS, os.path.join(TESTS, "compat")):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("prcnn_compat_adapters", os.path.join(TESTS, "compat", "usercustomize.py"))
    spec.loader.exec_module(importlib.util.module_from_spec(spec))


def load(mode, batch_size):
    """tools/eval_rcnn.py as a module, its argument parser fed the command line of `--eval_mode <mode>`"""
    argv = sys.argv
    sys.argv = ["eval_rcnn.py", "--cfg_file", "cfgs/default.yaml", "--eval_mode", mode, "--batch_size", str(batch_size)]
    try:
        spec = importlib.util.spec_from_file_location("prcnn_ref_eval_rcnn_" + mode, os.path.join(REFERENCE, "tools", "eval_rcnn.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    mod.cfg_from_file(os.path.join(REFERENCE, "tools", "cfgs", "default.yaml"))
    mod.cfg.TEST.SPLIT = "test"
    return mod


class _Dataset:
    def __init__(self, root, ids):
        self.imageset_dir = os.path.join(root, "KITTI", "object", "training")
        self.split, self.ids = "val", list(ids)
        os.makedirs(self.imageset_dir, exist_ok=True)
        os.makedirs(os.path.join(root, "KITTI", "ImageSets"), exist_ok=True)
        with open(os.path.join(root, "KITTI", "ImageSets", "val.txt"), "w") as f:
            f.write("".join("%06d\n" % i for i in self.ids))

    def get_calib(self, sample_id):
        return None

    def get_image_shape(self, sample_id):
        return (375, 1242, 3)

    def __len__(self):
        return len(self.ids)


class _Loader(list):
    dataset = None


class _Replay:
    """a model that returns recorded outputs, batch after batch"""

    def __init__(self, outputs, proposals=None):
        self.outputs = iter(outputs)
        if proposals is not None:
            it = iter(proposals)
            self.rpn = types.SimpleNamespace(proposal_layer=lambda scores, reg, xyz: next(it))

    def eval(self):
        return self

    def __call__(self, input_data):
        return next(self.outputs)


def _nudge(raw, thresh):
    """keep raw scores >= 1e-3 away from logit(thresh): a last-bit difference in sigmoid cannot flip the mask"""
    edge = math.log(thresh / (1 - thresh))
    near = np.abs(raw - edge) < 2e-3
    raw[near] = edge + 0.05
    assert np.abs(raw.astype(np.float64) - edge).min() >= 1e-3
    return raw


def scenes(seed, gt_cols):
    """one batch: rois (B,M,7), gt (B,G,gt_cols), regression rows (B,M,46) that decode to boxes near the RoIs, rcnn / rpn raw scores,
    point labels.  Per frame: ground-truth box k is approached by RoIs at a jitter that grows with k (1 cm for box 0 -> IoU > 0.9), the last
    live box by none; the remaining RoIs are random."""
    _paths()
    from util import rand_boxes3d
    rng = np.random.default_rng(seed)
    pts = rng.uniform([-30, 0, 5], [30, 2, 65], (4000, 3)).astype(F32)
    gt = np.zeros((B, G, gt_cols), F32)
    rois = np.zeros((B, M, 7), F32)
    scale = np.array([1, 0.3, 1, 0.2, 0.2, 0.4, 0.15])
    jit = [0.01, 0.12, 0.3, 0.55, 0.9]
    for b in range(B):
        ng = 0 if (b == 1 and seed % 2 == 1) else 4 + (b + seed) % 2                 # frame 1 of the odd-seed batch: no ground truth at all
        g = rand_boxes3d(pts, ng, seed=seed * 10 + b) if ng else np.zeros((0, 7), F32)
        gt[b, :ng, :7] = g
        if gt_cols > 7:
            gt[b, :ng, 7:] = 1.0                                                      # the class column of a wider ground truth
        if b == 2 and ng > 3:
            gt[b, 2] = 0                                                              # an all-zero row in the middle: it stays live
        r = rand_boxes3d(pts, M, seed=seed * 10 + 5 + b)
        k = 0
        for j in range(max(ng - 1, 0)):
            for rep in range(3):
                r[k] = g[j] + (rng.normal(0, 1, 7) * scale * jit[min(j, 4)] * (1 + rep)).astype(F32)
                k += 1
        rois[b] = r[rng.permutation(M)]
    reg = np.zeros((B, M, 46), F32)
    reg[:, :, 0:12] = rng.normal(0, 0.3, (B, M, 12))
    reg[:, :, 3] += 4; reg[:, :, 9] += 4                                              # x / z bin 3, whose centre is +0.25 m ...
    reg[:, :, 12:24] = rng.normal(0, 0.05, (B, M, 12))
    reg[:, :, 15] -= 0.5; reg[:, :, 21] -= 0.5                                        # ... taken back by the residual
    reg[:, :, 24] = rng.normal(0, 0.03, (B, M))
    reg[:, :, 25:34] = rng.normal(0, 0.3, (B, M, 9))
    reg[:, :, 29] += 4                                                                # angle bin 4: no turn
    reg[:, :, 34:43] = rng.normal(0, 0.1, (B, M, 9))
    mean = np.array([1.52563191462, 1.62856739989, 3.88311640418])
    reg[:, :, 43:46] = (rois[:, :, 3:6] - mean) / mean + rng.normal(0, 0.02, (B, M, 3))
    rcnn_cls = _nudge(rng.normal(-0.5, 1.5, (B, M)).astype(F32), 0.3)
    rpn_raw = _nudge(rng.normal(-0.8, 1.5, (B, N)).astype(F32), 0.3)
    label = rng.choice([-1, 0, 1], (B, N), p=[0.1, 0.6, 0.3]).astype(np.int64)
    if seed % 2 == 1:
        label[2] = np.where(label[2] > 0, 0, label[2])                               # a frame without a foreground point ...
        rpn_raw[2] = -np.abs(rpn_raw[2]) - 1.0                                       # ... and without a predicted one: union == 0
    gt_iou = rng.uniform(0, 1, (B, M)).astype(F32)
    gt_iou[:, 0], gt_iou[:, 1], gt_iou[:, 2] = F32(0.6), F32(0.45), F32(0.7)          # the three thresholds themselves
    gt_iou[:, 3], gt_iou[:, 4] = np.nextafter(F32(0.6), F32(1)), np.nextafter(F32(0.45), F32(0))
    if seed % 2 == 1:
        gt_iou[1] = F32(0.5)                                                          # a frame without a valid RoI: sum(valid) == 0
    return {"rois": rois, "gt": gt, "rcnn_reg": reg, "rcnn_cls": rcnn_cls, "rpn_raw": rpn_raw, "label": label, "gt_iou": gt_iou,
            "roi_scores": rng.normal(0, 1, (B, M)).astype(F32), "sample_id": np.arange(B) + 100 * seed}


def _live(gt):
    k = gt.shape[0]
    while k > 0 and gt[k - 1].sum() == 0:
        k -= 1
    return k


def run_reference(mode, batches):
    """-> (the reference's ret_dict, per batch the decoded boxes (B,M,7) and the detections per frame (B))"""
    _paths()
    import cpu_ops
    with cpu_ops.oracle_ops(), cpu_ops.cuda_is_cpu(), tempfile.TemporaryDirectory() as tmp:
        mod = load(mode, 1 if mode == "rcnn" else B)
        cfg = mod.cfg
        cfg.RPN.ENABLED, cfg.RCNN.ENABLED = mode != "rcnn", mode != "rpn"
        cfg.RPN.FIXED = False                       # joint mode: the segmentation IoU is reported only for a trainable RPN (:533, :568)
        decoded, kept = [], {}
        real_decode = mod.decode_bbox_target

        def decode(*a, **k):
            out = real_decode(*a, **k)
            decoded.append(out.detach().numpy().copy())
            return out

        def save_kitti_format(sample_id, calib, bbox3d, out_dir, scores, img_shape):
            kept[int(sample_id)] = int(bbox3d.shape[0])
        mod.decode_bbox_target, mod.save_kitti_format = decode, save_kitti_format
        ids = [int(i) for s in batches for i in s["sample_id"]]
        loader = _Loader()
        loader.dataset = _Dataset(tmp, ids)
        logger = logging.getLogger("ref_eval_stats")
        t = torch.from_numpy
        if mode == "rpn":
            for s in batches:
                loader.append({"sample_id": s["sample_id"], "pts_rect": np.zeros((B, N, 3), F32), "pts_features": np.zeros((B, N, 1), F32),
                               "pts_input": np.zeros((B, N, 3), F32), "rpn_cls_label": s["label"], "rpn_reg_label": np.zeros((B, N, 7), F32),
                               "gt_boxes3d": s["gt"]})
            outs = [{"rpn_cls": t(s["rpn_raw"]).unsqueeze(-1), "rpn_reg": torch.zeros(B, N, 76), "backbone_xyz": torch.zeros(B, N, 3),
                     "backbone_features": torch.zeros(B, 128, N)} for s in batches]
            model = _Replay(outs, [(t(s["rois"]), t(s["roi_scores"])) for s in batches])
            ret = mod.eval_one_epoch_rpn(model, loader, "no_number", tmp, logger)
        elif mode == "joint":
            for s in batches:
                loader.append({"sample_id": s["sample_id"], "pts_rect": np.zeros((B, N, 3), F32), "pts_features": np.zeros((B, N, 1), F32),
                               "pts_input": np.zeros((B, N, 3), F32), "rpn_cls_label": s["label"], "rpn_reg_label": np.zeros((B, N, 7), F32),
                               "gt_boxes3d": s["gt"]})
            outs = [{"roi_scores_raw": t(s["roi_scores"]), "rois": t(s["rois"]),
                     "seg_result": (torch.sigmoid(t(s["rpn_raw"])) > cfg.RPN.SCORE_THRESH).float(),
                     "rcnn_cls": t(s["rcnn_cls"]).reshape(B * M, 1), "rcnn_reg": t(s["rcnn_reg"]).reshape(B * M, -1)} for s in batches]
            ret = mod.eval_one_epoch_joint(_Replay(outs), loader, "no_number", tmp, logger)
        else:
            outs = []
            for s in batches:
                for b in range(B):                  # batch_size == 1 (:283): a frame per iteration, its ground truth as the dataset gives it
                    loader.append({"sample_id": int(s["sample_id"][b]), "roi_boxes3d": s["rois"][b], "roi_scores": s["roi_scores"][b],
                                   "gt_iou": s["gt_iou"][b], "gt_boxes3d": s["gt"][b, :_live(s["gt"][b]), :7],
                                   "pts_input": np.zeros((M, 8, 3), F32)})
                    outs.append({"rcnn_cls": t(s["rcnn_cls"][b]).reshape(M, 1), "rcnn_reg": t(s["rcnn_reg"][b])})
            ret = mod.eval_one_epoch_rcnn(_Replay(outs), loader, "no_number", tmp, logger)
        per = len(decoded) // len(batches)              # rpn mode decodes nothing: its "refined" boxes are the RoIs, unused
        pred = [np.concatenate(decoded[i * per:(i + 1) * per], 0).reshape(B, M, 7) if per else s["rois"] for i, s in enumerate(batches)]
        num = [np.array([kept.get(int(i), 0) for i in s["sample_id"]], np.int32) for s in batches]
    return ret, pred, num


def _check(name, ret, total_gt_expected=None):
    """conditions on the committed inputs, from the reference's numbers alone"""
    rec = [ret["rpn_recall(thresh=%.2f)" % th] for th in THRESH]
    assert all(0.0 < r < 1.0 for r in rec), (name, rec)                   # every RoI count strictly between 0 and the ground-truth total
    assert len(set(rec)) >= 3, (name, rec)
    print(name, {k: v for k, v in ret.items()})


def make_golden(path=None):
    out = {}
    for mode in ("rpn", "rcnn", "joint"):
        batches = [scenes(1, 7), scenes(2, 7 if mode == "rcnn" else 8)]
        ret, pred, num = run_reference(mode, batches)
        _check(mode, ret)
        for i, s in enumerate(batches):
            tag = "%s_b%d_" % (mode, i)
            for k in ("rois", "gt", "rcnn_cls", "rpn_raw", "label", "gt_iou"):
                out[tag + k] = s[k]
            out[tag + "pred"], out[tag + "num"] = pred[i].astype(F32), num[i]
        for k, v in ret.items():
            out["%s_ret_%s" % (mode, k)] = np.float64(v)
        if mode != "rpn":
            assert sum(int(n.sum()) for n in num) > 0
    for s in (scenes(1, 7), scenes(2, 8)):
        assert all(v in s["gt_iou"] for v in (F32(0.6), F32(0.45), F32(0.7)))
    np.savez_compressed(path or os.path.join(HERE, "eval_stats_ref.npz"), **out)
    print("wrote eval_stats_ref.npz")


if __name__ == "__main__":
    make_golden()
