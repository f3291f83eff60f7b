"""TEST INFRASTRUCTURE shared by tests/test_eval_stats_math_cpu.py and tests/test_gpu_eval_stats.py: the fixture of the reference's own
evaluation loops (tests/golden/eval_stats_ref.npz, written by tests/golden/ref_eval_stats.py), the oracle-side per-ground-truth maximum
IoU, and the record format of tests/eval_stats_math_host.cpp."""
import os
import struct

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
THRESH = (0.1, 0.3, 0.5, 0.7, 0.9)
MODES = ("rpn", "rcnn", "joint")
TRIM = {"rpn": 1, "rcnn": 0, "joint": 0}
SEG_MODE = {"rpn": 0, "rcnn": 0, "joint": 1}
RPN_SCORE_THRESH = RCNN_SCORE_THRESH = 0.3               # cfg.RPN.SCORE_THRESH, cfg.RCNN.SCORE_THRESH
CLS_FG, CLS_BG, REFINE = 0.6, 0.45, 0.7                  # cfg.RCNN.CLS_FG_THRESH, CLS_BG_THRESH; 0.7 for Car

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(os.path.join(HERE, "golden", "eval_stats_ref.npz")))
    return _fixture


def ref_dict(mode):
    """the dictionary the reference's eval_one_epoch_<mode> returned"""
    pre = mode + "_ret_"
    return {k[len(pre):]: float(v) for k, v in fixture().items() if k.startswith(pre)}


def batches(mode):
    """the two recorded batches of a mode -> per batch what EvalStats.update takes, as CPU tensors (masks formed with torch, as the caller
    of update forms them)"""
    fx, out = fixture(), []
    for i in range(2):
        g = lambda k: fx["%s_b%d_%s" % (mode, i, k)]      # noqa: E731
        b = {"rois": torch.from_numpy(g("rois")), "gt_boxes3d": torch.from_numpy(g("gt"))}
        if mode != "rpn":
            b["pred_boxes3d"], b["det_num"] = torch.from_numpy(g("pred")), torch.from_numpy(g("num"))
        if mode != "rcnn":
            b["seg_result"] = (torch.sigmoid(torch.from_numpy(g("rpn_raw"))) > RPN_SCORE_THRESH).float()
            b["rpn_cls_label"] = torch.from_numpy(g("label"))
        if mode == "rcnn":
            b["pred_class"] = (torch.sigmoid(torch.from_numpy(g("rcnn_cls"))) > RCNN_SCORE_THRESH).to(torch.uint8)
            b["gt_iou"] = torch.from_numpy(g("gt_iou"))
        out.append(b)
    return out


def live_rows(gt, keep):
    """rows of one frame's ground truth (G, gt_cols) that stay: trailing rows whose float32 sum, added in column order, is 0 are dropped,
    `keep` rows always stay"""
    n = gt.shape[0]
    while n > keep:
        s = F32(0)
        for v in gt[n - 1]:
            s = F32(s + F32(v))
        if s != 0:
            break
        n -= 1
    return n


def oracle_gt_max(sets, gt, trim_mode):
    """oracle boxes_iou3d(boxes[b], gt[b, :n, :7]).max(0) per set and frame -> gt_max (S,B,G) with -1 past n, num_gt (B) int32"""
    import oracle
    cpu = oracle.cpu()
    gt = np.asarray(gt, F32)
    B, G = gt.shape[:2]
    gt_max = np.full((len(sets), B, G), -1, F32)
    num = np.zeros((B,), np.int32)
    for b in range(B):
        n = num[b] = live_rows(gt[b], trim_mode)
        for s, boxes in enumerate(sets):
            if n:
                with np.errstate(invalid="ignore"):
                    gt_max[s, b, :n] = cpu.boxes_iou3d(np.asarray(boxes[b], F32), np.ascontiguousarray(gt[b, :n, :7])).max(0)
    return gt_max, num


def pack(gt_max=None, num_gt=None, B=1, det_num=None, seg=None, label=None, seg_mode=0, pred=None, gt_iou=None, thr=(CLS_FG, CLS_BG, REFINE)):
    """one batch record of tests/eval_stats_math_host.cpp"""
    S, G = (gt_max.shape[0], gt_max.shape[2]) if gt_max is not None else (0, 0)
    N = seg.shape[1] if seg is not None else 0
    R = pred.shape[1] if pred is not None else 0
    is64 = int(label is not None and label.dtype == np.int64)
    out = struct.pack("8i3f", S, B, G, int(det_num is not None), N, is64, seg_mode, R, *[float(F32(t)) for t in thr])
    num_gt = np.zeros((B,), np.int32) if num_gt is None else num_gt
    for a, dt in ((gt_max, F32), (num_gt, np.int32), (det_num, np.int32), (seg, F32), (label, None), (pred, np.uint8), (gt_iou, F32)):
        if a is not None:
            out += np.ascontiguousarray(a, dtype=dt).tobytes()
    return out


def unpack_states(blob):
    """EsState records -> list of (counters (16,) int64, sums (4,) float64)"""
    assert len(blob) % 160 == 0
    return [(np.frombuffer(blob[o:o + 128], np.int64), np.frombuffer(blob[o + 128:o + 160], np.float64)) for o in range(0, len(blob), 160)]
