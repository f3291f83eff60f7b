"""The numbers tools/eval_rcnn.py reports next to the AP -- recall of the ground truth by the RoIs and by the refined boxes, segmentation
IoU, RCNN classification accuracy, detections per frame -- counted on the device (csrc/eval_stats.hip).

`EvalStats.update` stands for the per-frame Python loop inside eval_one_epoch_rpn (:171-202), eval_one_epoch_rcnn (:336-364) and
eval_one_epoch_joint (:539-573): two launches per batch, no host read.  `result` reads the 160-byte state once and forms the reference's
dictionary with the reference's denominators.  `eval_one_epoch_joint` is the device loop a user calls: model -> detections -> update ->
result files, then the empty-file dump and the AP evaluator.  `eval_one_epoch_rpn` (with the RPN feature dumps of the offline recipe's
second step) and `eval_one_epoch_rcnn` (over those dumps) are the other two loops; all three can have the result files' text formatted
on the device (kitti_output.DeviceResultWriter) and then write one batch behind it.

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


class _OneBehind:
    """the loops' file side, one batch behind the device: `push(job)` runs the PREVIOUS job (a callable that waits for its own event
    and writes its files) and keeps this one; `flush()` runs the last.  While job i - 1 writes, batch i computes."""

    def __init__(self):
        self.job = None

    def push(self, job):
        prev, self.job = self.job, job
        if prev is not None:
            prev()

    def flush(self):
        self.push(None)


def _to_pinned(tensors):
    """device tensors -> (pinned host copies queued on the current stream, the event that says they are complete)"""
    host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in tensors]
    ev = torch.cuda.Event()
    ev.record()
    return host, ev


def eval_one_epoch_joint(model, batches, result_dir, calib_of, image_shape_of, split_file=None, label_dir=None, stats=None, classes="Car",
                         score_thresh=0.3, writer=None):
    """eval_one_epoch_joint (tools/eval_rcnn.py:459-683) on the device.  batches: dictionaries with `sample_id`, `pts_input` (B,N,3) and,
    when there are labels, `gt_boxes3d` (B,G,>=7) and optionally `rpn_cls_label` (B,N) -- numpy or tensors; calib_of / image_shape_of:
    sample id -> calibration (anything with a (3,4) P2) / image shape.  Per batch: model -> model.detections -> stats.update ->
    kitti_output.write_detections into <result_dir>/final_result/data; the host waits for the device only there.  After the last batch
    the empty result files of split_file are dumped; with label_dir the AP dictionary of kitti_eval.evaluate is merged.
    writer: a kitti_output.DeviceResultWriter formats the files' text on the device instead; batch i is formatted while the host writes
    the files of batch i - 1, and nothing but that text returns to the host.
    -> the reference's ret_dict."""
    final_output_dir = os.path.join(result_dir, "final_result", "data")
    os.makedirs(final_output_dir, exist_ok=True)
    model.eval()
    device = next(model.parameters()).device
    stats = EvalStats("joint", device, classes) if stats is None else stats
    behind = _OneBehind()
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
        if writer is not None:
            handle = writer.format(pred, raw, keep, num, [calib_of(i) for i in sample_id], [image_shape_of(i) for i in sample_id], classes)
            behind.push(lambda h=handle, ids=sample_id: writer.write(h, ids, final_output_dir, skip_empty=True))
            continue
        num_h = num.cpu().numpy()
        sel = np.flatnonzero(num_h > 0)
        if len(sel):
            ids = [sample_id[k] for k in sel]
            kitti_output.write_detections(pred.cpu().numpy()[sel], raw.cpu().numpy()[sel], keep.cpu().numpy()[sel], num_h[sel], ids,
                                          [calib_of(i) for i in ids], [image_shape_of(i) for i in ids], final_output_dir, classes)
    behind.flush()
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


def eval_one_epoch_rpn(model, batches, result_dir, calib_of, image_shape_of, save_result=False, save_rpn_feature=False, score_thresh=0.3,
                       stats=None, classes="Car", writer=None):
    """eval_one_epoch_rpn (tools/eval_rcnn.py:113-253) on the device: the second step of the offline recipe with save_rpn_feature.
    model: a PointRCNN (its `rpn` is used) or an RPN carrying a `proposal_layer`.  batches: dictionaries with `sample_id`, `pts_input`
    (B,N,3), `pts_rect` (B,N,3), `pts_features` (B,N,>=1) and, with labels, `rpn_cls_label` (B,N) and `gt_boxes3d` (B,G,>=7).
    Per batch: RPN forward, seg_result = sigmoid(rpn_cls) > score_thresh, proposal layer, EvalStats("rpn").update.  With either flag
    <result_dir>/seg_result/<id>.npy = [pts_rect, gt_cls, pred_cls] (without labels [pts_rect, pred_cls]) packed and rounded to float16
    on the device, and <result_dir>/detections/data/<id>.txt = every proposal, formatted on the device (kitti_output.DeviceResultWriter).
    With save_rpn_feature the five dumps of kitti_output.save_rpn_features in <result_dir>/features, the (C,N) -> (N,C) transposition
    on the device.  One host copy of each kind per batch, written while the next batch computes.  -> the reference's ret_dict."""
    rpn = getattr(model, "rpn", model)
    if not hasattr(rpn, "proposal_layer"):
        raise ValueError("eval_one_epoch_rpn: the model's RPN carries no proposal_layer")
    saving = save_result or save_rpn_feature
    if saving:
        kitti_output_dir, seg_output_dir = os.path.join(result_dir, "detections", "data"), os.path.join(result_dir, "seg_result")
        os.makedirs(kitti_output_dir, exist_ok=True)
        os.makedirs(seg_output_dir, exist_ok=True)
        writer = kitti_output.DeviceResultWriter(next(rpn.parameters()).device) if writer is None else writer
    if save_rpn_feature:
        features_dir = os.path.join(result_dir, "features")
        os.makedirs(features_dir, exist_ok=True)
    model.eval()
    device = next(rpn.parameters()).device
    stats = EvalStats("rpn", device, classes) if stats is None else stats
    behind = _OneBehind()
    for data in batches:
        sample_id = [int(v) for v in data["sample_id"]]
        with torch.no_grad():
            ret = rpn({"pts_input": _on_device(data["pts_input"], device, torch.float32)})
            raw = ret["rpn_cls"][:, :, 0].contiguous()
            seg = (torch.sigmoid(raw) > score_thresh).float()
            rois, roi_scores_raw = rpn.proposal_layer(raw, ret["rpn_reg"], ret["backbone_xyz"])
        label = data.get("rpn_cls_label")
        if label is not None:
            label = _on_device(label, device).long()                                         # :147
            gt = data.get("gt_boxes3d")
            stats.update(rois.contiguous(), None if gt is None else _on_device(gt, device, torch.float32), seg_result=seg, rpn_cls_label=label)
        if not saving:
            continue
        with torch.no_grad():
            cols = [_on_device(data["pts_rect"], device, torch.float32)] + ([] if label is None else [label.float().unsqueeze(2)])
            seg_pack = torch.cat(cols + [seg.unsqueeze(2)], dim=2).to(torch.float16)          # :219-224, float16 rounded to nearest even
            dumps = [seg_pack]
            if save_rpn_feature:
                dumps += [ret["backbone_features"].transpose(1, 2).contiguous(), ret["backbone_xyz"].contiguous(), seg, raw]
            host, event = _to_pinned(dumps)
        handle = writer.format(rois.contiguous(), roi_scores_raw.contiguous(), None, None, [calib_of(i) for i in sample_id],
                               [image_shape_of(i) for i in sample_id], classes)
        intensity = data["pts_features"] if save_rpn_feature else None

        def job(host=host, event=event, handle=handle, ids=sample_id, intensity=intensity):
            event.synchronize()
            arrays = [h.numpy() for h in host]
            for b, sid in enumerate(ids):
                np.save(os.path.join(seg_output_dir, "%06d.npy" % sid), arrays[0][b])
                if save_rpn_feature:
                    f = intensity[b]
                    kitti_output.save_rpn_features(arrays[3][b], arrays[4][b], f.cpu().numpy() if hasattr(f, "cpu") else np.asarray(f),
                                                   arrays[2][b], arrays[1][b], features_dir, sid)
            writer.write(handle, ids, kitti_output_dir)
        behind.push(job)
    behind.flush()
    return stats.result()


def eval_one_epoch_rcnn(rcnn_net, prep, frame_batches, result_dir, calib_of, image_shape_of, split_file=None, label_dir=None, save_result=False,
                        score_thresh=0.3, stats=None, classes="Car", writer=None):
    """eval_one_epoch_rcnn (tools/eval_rcnn.py:256-456) on the device, over the dumps of eval_one_epoch_rpn.  rcnn_net: an RCNNNet with
    ROI_SAMPLE_JIT False; prep: a kitti_input.RCNNOfflinePreparer; frame_batches: lists of kitti_input.load_rcnn_offline_frame
    dictionaries (a frame's `gt_iou` (M), when present, feeds the classification accuracy; its gt_boxes3d the recall).  Per batch:
    prep.eval_batch, RCNNNet, ops.decode_bbox_target (SIZE_RES_ON_ROI: the RoI's own size as the anchor), score threshold and
    ops.nms_batched; EvalStats("rcnn") counts every frame as one of the reference's batch-size-1 iterations.  final_result (and with
    save_result roi_result and refine_result) are formatted on the device and written one batch behind; then the empty-file dump
    and, with label_dir, kitti_eval.evaluate.  -> the reference's ret_dict."""
    from .proposal_layer import CLS_MEAN_SIZE, _anchor3
    cfg = prep.cfg
    device = next(rcnn_net.parameters()).device
    final_output_dir = os.path.join(result_dir, "final_result", "data")
    os.makedirs(final_output_dir, exist_ok=True)
    if save_result:
        roi_output_dir, refine_output_dir = os.path.join(result_dir, "roi_result", "data"), os.path.join(result_dir, "refine_result", "data")
        os.makedirs(roi_output_dir, exist_ok=True)
        os.makedirs(refine_output_dir, exist_ok=True)
    rcnn_net.eval()
    stats = EvalStats("rcnn", device, classes, cls_fg=cfg.CLS_FG_THRESH, cls_bg=cfg.CLS_BG_THRESH) if stats is None else stats
    writer = kitti_output.DeviceResultWriter(device, depth=6) if writer is None else writer       # three handles per batch, two batches in flight
    behind = _OneBehind()
    for frames in frame_batches:
        sample_id = [int(f["sample_id"]) for f in frames]
        packed = prep.pack(frames)
        B, M = packed["roi_boxes3d"].shape[:2]
        with torch.no_grad():
            d = prep.eval_batch(packed)
            ret = rcnn_net({"pts_input": d["pts_input"], "pts_features": d["pts_features"], "roi_boxes3d": d["roi_boxes3d"]})
            rcnn_cls, rcnn_reg = ret["rcnn_cls"], ret["rcnn_reg"].reshape(B * M, -1).contiguous()
            if rcnn_cls.numel() != B * M:
                raise NotImplementedError("eval_one_epoch_rcnn: a multi-class rcnn_cls %s is not supported (single-channel classifier only)"
                                          % (tuple(rcnn_cls.shape),))
            rois = d["roi_boxes3d"].contiguous()
            pred = ops.decode_bbox_target(rois, rcnn_reg, cfg.LOC_SCOPE, cfg.LOC_BIN_SIZE, cfg.NUM_HEAD_BIN, _anchor3(CLS_MEAN_SIZE[0]), True,
                                          cfg.LOC_Y_BY_BIN, cfg.LOC_Y_SCOPE, cfg.LOC_Y_BIN_SIZE, True)
            if cfg.SIZE_RES_ON_ROI:                                                          # :306-308: hwl = res * roi_size + roi_size
                pred[:, 3:6] = rcnn_reg[:, -3:] * d["roi_size"] + d["roi_size"]
            pred, rois = pred.view(B, M, 7), rois.view(B, M, 7)
            raw = rcnn_cls.reshape(B, M).contiguous()
            in_frame = torch.arange(M, device=device).unsqueeze(0) < d["num_roi"].unsqueeze(1)    # rows past num_roi are padding
            pred_class = (torch.sigmoid(raw) > score_thresh) & in_frame
            keep, num = ops.nms_batched(pred, raw, pred_class, cfg.NMS_THRESH, True)
            # one frame is one iteration of the reference: frames are counted one by one, each with its own RoI and GT count
            for b, f in enumerate(frames):
                if f.get("gt_boxes3d") is None:                                              # a frame without labels (--test) counts nothing
                    continue
                n = int(packed["num_roi"][b])
                if n == 0:
                    continue
                gt = np.asarray(f["gt_boxes3d"], np.float32).reshape(-1, 7)
                if f.get("gt_iou") is not None:
                    gt_iou = _on_device(np.asarray(f["gt_iou"], np.float32).reshape(1, -1), device, torch.float32)
                elif len(gt):                                                                # kitti_rcnn_dataset.py:862-872
                    corners = [_on_device(kitti_output.box_corners(x), device, torch.float32) for x in (f["roi_boxes3d"], gt)]
                    gt_iou = ops.corner_iou3d(*corners).max(dim=1)[0].view(1, -1).contiguous()
                else:
                    gt_iou = torch.zeros((1, n), dtype=torch.float32, device=device)
                stats.update(rois[b:b + 1, :n].contiguous(), _on_device(gt[None], device, torch.float32),
                             pred_boxes3d=pred[b:b + 1, :n].contiguous(), det_num=num[b:b + 1].contiguous(),
                             pred_class=pred_class[b:b + 1, :n].contiguous(), gt_iou=gt_iou)
        calibs, shapes = [calib_of(i) for i in sample_id], [image_shape_of(i) for i in sample_id]
        handles = [(writer.format(pred, raw, keep, num, calibs, shapes, classes), final_output_dir, True)]
        if save_result:
            all_rows = torch.arange(M, dtype=torch.int32, device=device).unsqueeze(0).expand(B, M).contiguous()
            handles.append((writer.format(rois, d["roi_scores"].view(B, M), all_rows, d["num_roi"], calibs, shapes, classes), roi_output_dir, False))
            handles.append((writer.format(pred, raw, all_rows, d["num_roi"], calibs, shapes, classes), refine_output_dir, False))

        def job(handles=handles, ids=sample_id):
            for h, out_dir, skip in handles:
                writer.write(h, ids, out_dir, skip_empty=skip)
        behind.push(job)
    behind.flush()
    ret_dict = {"empty_cnt": dump_empty_files(final_output_dir, split_file) if split_file is not None else 0}
    res = stats.result()
    res.pop("rpn_iou", None)                                                                 # the rcnn loop reports no segmentation IoU
    ret_dict.update(res)
    if label_dir is not None:
        if split_file is None:
            raise ValueError("eval_one_epoch_rcnn: the AP evaluation needs split_file")
        _, ap_dict = kitti_eval.evaluate(label_dir, final_output_dir, split_file, current_class={"Car": 0, "Pedestrian": 1, "Cyclist": 2}[classes])
        ret_dict.update(ap_dict)
    return ret_dict
