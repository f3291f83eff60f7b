"""The numbers tools/eval_rcnn.py reports next to the AP -- recall of the ground truth by the RoIs and by the refined boxes, segmentation
IoU, RCNN classification accuracy, detections per frame -- counted on the device (csrc/eval_stats.hip).

`EvalStats.update` stands for the per-frame Python loop inside eval_one_epoch_rpn (:171-202), eval_one_epoch_rcnn (:336-364) and
eval_one_epoch_joint (:539-573): two launches per batch, no host read.  `result` reads the 160-byte state once and forms the reference's
dictionary with the reference's denominators.  `eval_one_epoch_joint` is the device loop a user calls: model -> detections -> update ->
result files, then the empty-file dump and the AP evaluator.

Two things are reproduced as the reference has them, not as one would write them:
  * joint mode's `rpn_iou` (:568-573) is computed over the WHOLE batch inside the `for k in range(batch_size)` loop, so the batch's ratio
    is added once per frame, B times, and the sum is divided by the number of batches;
  * a recall threshold meets a float32 IoU in float32 (torch casts the Python scalar): float32(0.1) is not recalled at 0.1.
"""
import os

import numpy as np
import torch

from . import kitti_eval, kitti_output, ops

THRESH_LIST = (0.1, 0.3, 0.5, 0.7, 0.9)
_SEG_MODE = {"rpn": 0, "joint": 1}


class EvalStats:
    """mode "rpn" | "rcnn" | "joint"; classes: cfg.CLASSES (the refined accuracy's IoU threshold is 0.7 for Car, 0.5 otherwise);
    cls_fg / cls_bg: cfg.RCNN.CLS_FG_THRESH / CLS_BG_THRESH."""

    def __init__(self, mode="joint", device="cuda:0", classes="Car", cls_fg=0.6, cls_bg=0.45):
        if mode not in ("rpn", "rcnn", "joint"):
            raise ValueError("EvalStats: mode must be 'rpn', 'rcnn' or 'joint', got %r" % (mode,))
        self.mode, self.device, self.classes = mode, torch.device(device), classes
        self.cls_fg, self.cls_bg = float(cls_fg), float(cls_bg)
        self.refine_thresh = 0.7 if classes == "Car" else 0.5                      # eval_rcnn.py:359
        self.state = torch.zeros((ops.EVAL_STATS_STATE_BYTES,), dtype=torch.uint8, device=self.device)
        self._work = {}

    def reset(self):
        self.state.zero_()

    def update(self, rois, gt_boxes3d, pred_boxes3d=None, det_num=None, seg_result=None, rpn_cls_label=None, pred_class=None, gt_iou=None):
        """one batch: rois (B,M,7) and, in rcnn / joint mode, pred_boxes3d (B,M,7) against gt_boxes3d (B,G,>=7, zero rows at the end,
        G <= 128; G = 0: no ground truth in the batch); det_num (B) i32: the `num` of PointRCNN.detections; seg_result (B,N) f32 0 / 1 with
        rpn_cls_label (B,N) i32 | i64 (rpn and joint mode); pred_class (B,R) bool | u8 = sigmoid(rcnn_cls) > SCORE_THRESH with gt_iou (B,R)
        (rcnn mode).  Everything on the device; two launches, no synchronisation, capturable in a torch.cuda.graph.
        rcnn mode: the reference's loop asserts batch_size == 1, every frame here is one of its iterations."""
        B = rois.shape[0]
        sets = [rois] if self.mode == "rpn" else [rois, pred_boxes3d]
        if self.mode != "rpn" and pred_boxes3d is None:
            raise ValueError("EvalStats.update: %s mode needs pred_boxes3d" % self.mode)
        if (seg_result is not None or rpn_cls_label is not None) and self.mode == "rcnn":
            raise ValueError("EvalStats.update: rcnn mode has no segmentation IoU")
        gt_max = num_gt = None
        if gt_boxes3d is not None and gt_boxes3d.shape[1] > 0:
            key = (len(sets), B, gt_boxes3d.shape[1])
            if key not in self._work:                  # reused batch after batch: the two launches are ordered on one stream
                self._work = {key: ops.eval_stats_workspace(*key, self.device)}
            gt_max, num_gt = ops.eval_gt_max_iou(sets, gt_boxes3d, ops.EVAL_TRIM[self.mode], out=self._work[key])
        if pred_class is not None and pred_class.dtype == torch.bool:
            pred_class = pred_class.to(torch.uint8)
        ops.eval_stats_accumulate(self.state, gt_max, num_gt, B, det_num=det_num, seg=seg_result, cls_label=rpn_cls_label,
                                  seg_mode=_SEG_MODE.get(self.mode, 0), pred_class=pred_class, gt_iou=gt_iou, cls_fg=self.cls_fg,
                                  cls_bg=self.cls_bg, refine_thresh=self.refine_thresh)

    def raw(self):
        """-> (counters (16,) int64, sums (4,) float64) on the host: the one device-to-host read"""
        host = self.state.cpu().numpy()
        return host[:128].view(np.int64).copy(), host[128:160].view(np.float64).copy()

    def result(self, num_frames=None):
        """the reference's ret_dict entries (eval_rcnn.py:244-250, :424-444, :649-672), every denominator max(., 1.0).
        num_frames: joint mode's len(dataset) for rcnn_avg_num (default: the frames seen).  One device-to-host read."""
        return result_from_state(self.mode, *self.raw(), num_frames=num_frames)


def result_from_state(mode, counters, sums, num_frames=None):
    """EvalStats.result from a state already on the host: counters (16,) int64, sums (4,) float64"""
    c, s = [int(v) for v in counters], [float(v) for v in sums]
    total_gt, frames, batches = c[10], c[12], c[13]
    ret = {}
    if mode == "rpn":
        ret["max_obj_num"] = 0                                                     # never updated by the reference either (:133, :244)
        ret["rpn_iou"] = s[0] / max(frames, 1.0)
    else:
        cnt = frames if mode == "rcnn" else batches                                # rcnn: batch_size == 1, a batch is a frame (:282-283)
        ret["rpn_iou"] = s[0] / max(cnt, 1.0)
        ret["rcnn_cls_acc"] = s[1] / max(cnt, 1.0)
        ret["rcnn_cls_acc_refined"] = s[2] / max(cnt, 1.0)
        ret["rcnn_avg_num"] = c[11] / max(cnt if mode == "rcnn" else (frames if num_frames is None else num_frames), 1.0)
    for idx, thresh in enumerate(THRESH_LIST):
        ret["rpn_recall(thresh=%.2f)" % thresh] = c[idx] / max(total_gt, 1.0)
    if mode != "rpn":
        for idx, thresh in enumerate(THRESH_LIST):
            ret["rcnn_recall(thresh=%.2f)" % thresh] = c[5 + idx] / max(total_gt, 1.0)
    return ret


def _on_device(a, device, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device, non_blocking=True)
    return (t if dtype is None else t.to(dtype)).contiguous()


def dump_empty_files(output_dir, split_file):
    """eval_rcnn.py:631-642: an empty result file for every frame of the split that has none -> their count"""
    with open(split_file) as f:
        ids = [x.strip() for x in f.readlines()]
    empty = 0
    for name in ids:
        path = os.path.join(output_dir, "%s.txt" % name)
        if not os.path.exists(path):
            open(path, "w").close()
            empty += 1
    return empty


def eval_one_epoch_joint(model, batches, result_dir, calib_of, image_shape_of, split_file=None, label_dir=None, stats=None, classes="Car",
                         score_thresh=0.3):
    """eval_one_epoch_joint (tools/eval_rcnn.py:459-683) on the device.  batches: dictionaries with `sample_id`, `pts_input` (B,N,3) and,
    when there are labels, `gt_boxes3d` (B,G,>=7) and optionally `rpn_cls_label` (B,N) -- numpy or tensors; calib_of / image_shape_of:
    sample id -> calibration (anything with a (3,4) P2) / image shape.  Per batch: model -> model.detections -> stats.update ->
    kitti_output.write_detections into <result_dir>/final_result/data; the host waits for the device only there.  After the last batch
    the empty result files of split_file are dumped; with label_dir the AP dictionary of kitti_eval.evaluate is merged.
    -> the reference's ret_dict."""
    final_output_dir = os.path.join(result_dir, "final_result", "data")
    os.makedirs(final_output_dir, exist_ok=True)
    model.eval()
    device = next(model.parameters()).device
    stats = EvalStats("joint", device, classes) if stats is None else stats
    for data in batches:
        sample_id = [int(v) for v in data["sample_id"]]
        with torch.no_grad():
            ret = model({"pts_input": _on_device(data["pts_input"], device, torch.float32)})
            pred, raw, keep, num = model.detections(ret, score_thresh=score_thresh)
        if data.get("gt_boxes3d") is not None:
            label = data.get("rpn_cls_label")
            label = None if label is None else _on_device(label, device)
            if label is not None and label.dtype not in (torch.int32, torch.int64):
                label = label.long()
            stats.update(ret["rois"].contiguous(), _on_device(data["gt_boxes3d"], device, torch.float32), pred_boxes3d=pred, det_num=num,
                         seg_result=None if label is None else ret["seg_result"].contiguous(), rpn_cls_label=label)
        # the reference writes no file for a frame without a box above the score threshold (:607-610); the dump below counts those
        num_h = num.cpu().numpy()
        sel = np.flatnonzero(num_h > 0)
        if len(sel):
            ids = [sample_id[k] for k in sel]
            kitti_output.write_detections(pred.cpu().numpy()[sel], raw.cpu().numpy()[sel], keep.cpu().numpy()[sel], num_h[sel], ids,
                                          [calib_of(i) for i in ids], [image_shape_of(i) for i in ids], final_output_dir, classes)
    ret_dict = {"empty_cnt": dump_empty_files(final_output_dir, split_file) if split_file is not None else 0}
    num_frames = len(batches.dataset) if hasattr(batches, "dataset") else None
    ret_dict.update(stats.result(num_frames=num_frames))
    if label_dir is not None:
        if split_file is None:
            raise ValueError("eval_one_epoch_joint: the AP evaluation needs split_file")
        _, ap_dict = kitti_eval.evaluate(label_dir, final_output_dir, split_file,
                                         current_class={"Car": 0, "Pedestrian": 1, "Cyclist": 2}[classes])
        ret_dict.update(ap_dict)
    return ret_dict
