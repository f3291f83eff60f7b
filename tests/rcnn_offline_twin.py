"""numpy / Python restatement of the RCNN offline RoI sampler on the device (csrc/rcnn_offline.hip, csrc/rcnn_offline_math.h): the
sampling part of KittiRCNNDataset.get_rcnn_training_sample_batch (lib/datasets/kitti_rcnn_dataset.py:890-957) with sample_bg_inds,
aug_roi_by_noise_batch and random_aug_box3d, random calls from the counter table (streams 40, 42, 43, 50).

    corners_f32(boxes, trig, fused)   boxes3d_to_corners3d of float32 boxes, sine / cosine as parameters (default: csrc/ref_trig.h's),
                                in the several-box or the one-box (fused) form of numpy's matmul
    corners_f64(box)            boxes3d_to_corners3d of one float64 box: float32 local corners, float64 rotation and shift, one rounding
    iou_matrix / noise_slot / sample_frame

The clip is train_input_twin.pair_iou, WITHOUT the separating-axis test of the header: agreement bit for bit is what shows that the
test changes no result.  Pure host code: the expected value of the CPU and GPU tests."""
import math

import numpy as np

import oracle
import train_input_twin as tw

STREAM_FG_KEY, STREAM_HARD, STREAM_EASY, STREAM_NOISE = 40, 42, 43, 50
RANGES = ((0.2, 0.1, math.pi / 12), (0.3, 0.15, math.pi / 12), (0.5, 0.15, math.pi / 9), (0.8, 0.15, math.pi / 6), (1.0, 0.15, math.pi / 3))
DEFAULT_CFG = dict(REG_FG_THRESH=0.55, CLS_FG_THRESH=0.6, CLS_BG_THRESH=0.45, CLS_BG_THRESH_LO=0.05, FG_RATIO=0.5, HARD_BG_RATIO=0.8,
                   ROI_PER_IMAGE=64, AUG_TIMES=10, REG_AUG_METHOD="multiple")
F32 = np.float32


def ref_trig():
    cpu = oracle.cpu()
    return (lambda a: cpu.ref_trig("cosf", a)), (lambda a: cpu.ref_trig("sinf", a))


def _fma(a, b, c):
    """float32 fma on float32 arrays: the product is exact in double; the double sum is rounded again to float32 (the two roundings
    differ from one only on a 2^-29 set of operands)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def corners_f32(boxes, trig=None, fused=False):
    """train_input_twin.corners3d with the cosine and sine as parameters: trig = (cos, sin) on float32 arrays.  fused: the form of a
    call on ONE box, which numpy hands to sgemm: fma(z, sin, x * cos) (csrc/rcnn_offline_math.h)"""
    cos, sin = trig or ref_trig()
    b = np.asarray(boxes, F32).reshape(-1, 7)
    h, w, l, ry = b[:, 3], b[:, 4], b[:, 5], np.ascontiguousarray(b[:, 6])
    hl, hw = l / F32(2), w / F32(2)
    xs = np.stack([hl, hl, -hl, -hl, hl, hl, -hl, -hl], 1)
    zs = np.stack([hw, -hw, -hw, hw, hw, -hw, -hw, hw], 1)
    zero = np.zeros_like(h)
    ys = np.stack([zero] * 4 + [-h] * 4, 1)
    cs, sn = np.asarray(cos(ry), F32).reshape(-1, 1), np.asarray(sin(ry), F32).reshape(-1, 1)
    f0, f1 = F32(0), F32(1)
    yr = (xs * f0 + ys * f1) + zs * f0
    if fused:
        xr, zr = _fma(zs, sn, xs * cs), _fma(zs, cs, xs * -sn)
    else:
        xr, zr = (xs * cs + ys * f0) + zs * sn, (xs * -sn + ys * f0) + zs * cs
    return np.stack([b[:, 0:1] + xr, b[:, 1:2] + yr, b[:, 2:3] + zr], 2).astype(F32)


def corners_f64(box):
    """(7,) float64 -> (8,3) float32 (kitti_utils.py:74-101 on a float64 box)"""
    box = [float(v) for v in box]
    cs, sn = math.cos(box[6]), math.sin(box[6])
    hl, hw, nh = float(F32(box[5] / 2.0)), float(F32(box[4] / 2.0)), float(F32(-box[3]))
    out = np.empty((8, 3), F32)
    for k in range(8):
        xs = -hl if k & 2 else hl
        zs = -hw if (k + 1) & 2 else hw
        ys = 0.0 if k < 4 else nh
        xr = (xs * cs + ys * 0.0) + zs * sn
        yr = (xs * 0.0 + ys * 1.0) + zs * 0.0
        zr = (xs * -sn + ys * 0.0) + zs * cs
        out[k] = (F32(box[0] + xr), F32(box[1] + yr), F32(box[2] + zr))
    return out


def iou_matrix(roi, gt, trig=None):
    """(m,7), (g,7) float32 -> (m,g) float32: get_iou3d(boxes3d_to_corners3d(roi), boxes3d_to_corners3d(gt))"""
    return tw.corner_iou3d(corners_f32(roi, trig, len(roi) == 1), corners_f32(gt, trig, len(gt) == 1))


def noise_box(box, seed, frame, base, method):
    """random_aug_box3d -> (7,) float64"""
    u = lambda q: tw.u01(tw.rand32(seed, STREAM_NOISE, frame, base + q)) - 0.5          # noqa: E731
    box = [float(v) for v in np.asarray(box, F32)]
    if method == "multiple":
        pr, hr, ar = RANGES[tw.below(tw.rand32(seed, STREAM_NOISE, frame, base), 5)]
        ps = [(u(1 + c) / 0.5) * pr for c in range(3)]
        hs = [(u(4 + c) / 0.5) * hr + 1.0 for c in range(3)]
        rot = (u(7) / 0.5) * ar
    elif method == "single":
        ps = [u(1 + c) for c in range(3)]
        hs = [u(4 + c) / (0.5 / 0.15) + 1.0 for c in range(3)]
        rot = u(7) / (0.5 / (math.pi / 12))
    else:
        raise NotImplementedError(method)
    return np.array([box[c] + ps[c] for c in range(3)] + [box[3 + c] * hs[c] for c in range(3)] + [box[6] + rot], np.float64)


def noise_slot(box, gt_box, times, pos_thresh, seed, frame, slot, method, trig=None):
    """aug_roi_by_noise_batch for one slot -> (roi (7,) float32, iou float32, attempts)"""
    box = np.asarray(box, F32)
    gtc = corners_f32(gt_box, trig, True)[0]
    roi, iou, cnt = box.copy(), F32(0), 0
    while float(iou) < pos_thresh and cnt < times:
        base = (slot * 16 + cnt) * 16
        if tw.u01(tw.rand32(seed, STREAM_NOISE, frame, base + 8)) < 0.2:
            roi, c = box.copy(), corners_f32(box, trig, True)[0]
        else:
            aug = noise_box(box, seed, frame, base, method)
            roi, c = aug.astype(F32), corners_f64(aug)
        iou = tw.pair_iou(c, gtc)[0]
        cnt += 1
    return roi, F32(iou), cnt


def sample_frame(roi, gt, seed, frame, cfg=None, trig=None, iou=None):
    """One frame of prcnn_rcnn_offline_sample.  roi (m,7), gt (g,7) float32 (the counted rows only); cfg: DEFAULT_CFG's keys.
    iou: the (m,g) matrix if the caller has it already.
    -> dict iou3d, max_overlaps, gt_assignment, counts (4,), status, src, rois, gt_of_rois, roi_iou (R rows; cleared when status != 0)"""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    roi, gt = np.asarray(roi, F32).reshape(-1, 7), np.asarray(gt, F32).reshape(-1, 7)
    m, g, R = len(roi), len(gt), int(cfg["ROI_PER_IMAGE"])
    out = dict(iou3d=np.zeros((m, g), F32), max_overlaps=np.zeros(m, F32), gt_assignment=np.full(m, -1, np.int32),
               counts=np.zeros(4, np.int32), status=0, src=np.full(R, -1, np.int32), rois=np.zeros((R, 7), F32),
               gt_of_rois=np.zeros((R, 7), F32), roi_iou=np.zeros(R, F32))
    if g == 0:
        out["status"] = 2
        return out
    if m == 0:
        out["status"] = 1
        return out
    iou3d = iou_matrix(roi, gt, trig) if iou is None else np.asarray(iou, F32)
    mo, ga = iou3d.max(axis=1), iou3d.argmax(axis=1)
    col, ra = iou3d.max(axis=0), iou3d.argmax(axis=0)
    out.update(iou3d=iou3d, max_overlaps=mo, gt_assignment=ga.astype(np.int32))
    pos_thresh = min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
    fg = np.concatenate([np.nonzero(mo >= F32(pos_thresh))[0], ra[col > 0]])
    easy = np.nonzero(mo < F32(cfg["CLS_BG_THRESH_LO"]))[0]
    hard = np.nonzero((mo < F32(cfg["CLS_BG_THRESH"])) & (mo >= F32(cfg["CLS_BG_THRESH_LO"])))[0]
    nfg, nbg = len(fg), len(hard) + len(easy)
    fs = bs = 0
    if nfg > 0 and nbg > 0:
        fs = min(int(np.round(cfg["FG_RATIO"] * R)), nfg)
        bs = R - fs
    elif nbg > 0:
        bs = R
    else:
        out["status"] = 1
    out["counts"][:] = (nfg, len(hard), len(easy), fs)
    if out["status"]:
        return out
    src = []
    if fs:
        keys = [tw.rand32(seed, STREAM_FG_KEY, frame, t) for t in range(nfg)]
        src += [int(fg[t]) for t in sorted(range(nfg), key=lambda t: (keys[t], t))[:fs]]
    if len(hard) and len(easy):
        nh = int(bs * cfg["HARD_BG_RATIO"])
    else:
        nh = bs if len(hard) else 0
    for t in range(bs):
        if t < nh:
            src.append(int(hard[tw.below(tw.rand32(seed, STREAM_HARD, frame, t), len(hard))]))
        else:
            src.append(int(easy[tw.below(tw.rand32(seed, STREAM_EASY, frame, t - nh), len(easy))]))
    for t, i in enumerate(src):
        times = int(cfg["AUG_TIMES"]) if t < fs else min(int(cfg["AUG_TIMES"]), 1)
        out["rois"][t], out["roi_iou"][t], _ = noise_slot(roi[i], gt[ga[i]], times, pos_thresh, seed, frame, t, cfg["REG_AUG_METHOD"], trig)
        out["gt_of_rois"][t] = gt[ga[i]]
    out["src"][:] = src
    return out


# ------------------------------------------------------------------------------------------------ after pooling (:959-1010)
STREAM_AUG_ENABLE, STREAM_AUG_ANGLE, STREAM_AUG_SCALE = 51, 52, 53
PI_F = F32(np.pi)
METHOD_BITS = {"rotation": 1, "scaling": 2, "flip": 4}


def aug_draw(seed, frame, slot, methods=("rotation", "scaling", "flip"), flip_prob=0.5, rot_range=18):
    """data_augmentation(mustaug=True)'s draws for one slot -> dict rot, scl, flip, cs, sn (float64 of the angle), scale (float32)"""
    a = dict(rot="rotation" in methods, scl="scaling" in methods, cs=1.0, sn=0.0, scale=F32(1), angle=0.0)
    a["flip"] = "flip" in methods and 1.0 - tw.u01(tw.rand32(seed, STREAM_AUG_ENABLE, frame, slot * 4 + 2)) < flip_prob
    if a["rot"]:
        lo, hi = -math.pi / rot_range, math.pi / rot_range
        a["angle"] = lo + (hi - lo) * tw.u01(tw.rand32(seed, STREAM_AUG_ANGLE, frame, slot))
        a["cs"], a["sn"] = math.cos(a["angle"]), math.sin(a["angle"])
    if a["scl"]:
        a["scale"] = F32(0.95 + (1.05 - 0.95) * tw.u01(tw.rand32(seed, STREAM_AUG_SCALE, frame, slot)))
    return a


def _rot64(x, z, cs, sn):
    x64, z64 = np.asarray(x, np.float64), np.asarray(z, np.float64)
    return (x64 * cs + z64 * (-sn)).astype(F32), (x64 * sn + z64 * cs).astype(F32)


def _atan2_ref(y, x):
    return oracle.cpu().ref_trig("atan2f", np.asarray(y, F32).reshape(-1), np.asarray(x, F32).reshape(-1))[0]


def aug_box(box, a, atan2=None):
    """rotate_box3d_along_y + scale + flip on one float32 box, every box operation a float32 one"""
    atan2 = atan2 or _atan2_ref
    b = np.asarray(box, F32).copy()
    if a["rot"]:
        beta = F32(atan2(b[2], b[0]))
        alpha = ((-np.sign(beta) * PI_F) / F32(2) + beta) + b[6]
        b[0], b[2] = _rot64(b[0], b[2], a["cs"], a["sn"])
        nb = F32(atan2(b[2], b[0]))
        b[6] = ((np.sign(nb) * PI_F) / F32(2) + alpha) - nb
    if a["scl"]:
        b[0:6] = b[0:6] * a["scale"]
    if a["flip"]:
        b[0] = -b[0]
        b[6] = np.sign(b[6]) * PI_F - b[6]
    return b


def finish_slot(pts, roi, gt, a, trig=None, atan2=None):
    """pts (S,3) float32 pooled points of the slot -> (points in the augmented RoI's canonical frame, roi, gt, gt_boxes3d_ct)"""
    cos, sin = trig or ref_trig()
    p = np.asarray(pts, F32).copy()
    if a["rot"]:
        p[:, 0], p[:, 2] = _rot64(p[:, 0], p[:, 2], a["cs"], a["sn"])
    if a["scl"]:
        p = p * a["scale"]
    if a["flip"]:
        p[:, 0] = -p[:, 0]
    roi, gt = aug_box(roi, a, atan2), aug_box(gt, a, atan2)
    ry = np.mod(roi[6:7], F32(2 * np.pi))
    cs, sn = F32(np.asarray(cos(ry), F32).reshape(-1)[0]), F32(np.asarray(sin(ry), F32).reshape(-1)[0])

    def canon(v):
        x, y, z = v[..., 0] - roi[0], v[..., 1] - roi[1], v[..., 2] - roi[2]
        return np.stack([x * cs + z * (-sn), y, x * sn + z * cs], -1).astype(F32)
    ct = gt.copy()
    ct[0:3] = canon(gt[0:3])
    ct[6] = gt[6] - ry[0]
    return canon(p), roi, gt, ct


def labels(iou, empty, cfg=None):
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    iou, valid = np.asarray(iou, F32), np.asarray(empty) == 0
    mask = ((iou > F32(cfg["REG_FG_THRESH"])) & valid).astype(np.int32)
    lab = (iou > F32(cfg["CLS_FG_THRESH"])).astype(np.int32)
    lab[(iou > F32(cfg["CLS_BG_THRESH"])) & (iou < F32(cfg["CLS_FG_THRESH"]))] = -1
    lab[~valid] = -1
    return lab, mask


def host_roipool(xyz, boxes3d, feat, S):
    """roipool3d_cpu (lib/utils/roipool3d/src/roipool3d.cpp:127-195) through the library's host twin: boxes already enlarged"""
    import torch
    import pointrcnn_amd
    pointrcnn_amd.install()
    import roipool3d_cuda
    M, C = len(boxes3d), feat.shape[1]
    pp, pf, pe = torch.zeros(M, S, 3), torch.zeros(M, S, C), torch.zeros(M, dtype=torch.int64)
    roipool3d_cuda.roipool3d_cpu(torch.from_numpy(np.ascontiguousarray(xyz, F32)), torch.from_numpy(np.ascontiguousarray(boxes3d, F32)),
                                 torch.from_numpy(np.ascontiguousarray(feat, F32)), pp, pf, pe)
    return pp.numpy(), pf.numpy(), pe.numpy().astype(np.int32)


def enlarge(boxes, w):
    b = np.asarray(boxes, F32).copy()
    b[:, 3:6] += F32(w * 2)
    b[:, 1] += F32(w)
    return b


def offline_frame(fr, seed, frame, cfg=None, S=512, use_intensity=False, use_depth=True, methods=("rotation", "scaling", "flip"),
                  flip_prob=0.5, rot_range=18, pool_extra_width=1.0, trig=None, atan2=None, sample_trig=None):
    """The whole of get_rcnn_training_sample_batch for one frame.  fr: dict rpn_xyz (N,3), rpn_features (N,C), rpn_intensity (N),
    seg_mask (N), roi_boxes3d (M,7), gt_boxes3d (G,7).  -> sample_frame's dict plus pts_input (R,S,3+extras), pts_features (R,S,C),
    empty (R), cls_label, reg_valid_mask, gt_boxes3d_ct, roi_boxes3d, gt_boxes3d (the last two augmented), pooled_xyz (before the finish)"""
    s = sample_frame(fr["roi_boxes3d"], fr["gt_boxes3d"], seed, frame, cfg, sample_trig)
    R = len(s["src"])
    xyz = np.asarray(fr["rpn_xyz"], F32)
    extras = ([fr["rpn_intensity"].reshape(-1, 1)] if use_intensity else []) + [fr["seg_mask"].reshape(-1, 1)]
    if use_depth:
        extras.append((np.linalg.norm(xyz, ord=2, axis=1) / 70.0 - 0.5).astype(F32).reshape(-1, 1))
    extras = np.concatenate(extras, 1).astype(F32)
    E, C = extras.shape[1], fr["rpn_features"].shape[1]
    out = dict(s, pts_input=np.zeros((R, S, 3 + E), F32), pts_features=np.zeros((R, S, C), F32), empty=np.zeros(R, np.int32),
               cls_label=np.full(R, -1, np.int32), reg_valid_mask=np.zeros(R, np.int32), gt_boxes3d_ct=np.zeros((R, 7), F32),
               roi_boxes3d=np.zeros((R, 7), F32), gt_boxes3d=np.zeros((R, 7), F32), pooled_xyz=np.zeros((R, S, 3), F32))
    if s["status"]:
        return out
    pp, pf, pe = host_roipool(xyz, enlarge(s["rois"], pool_extra_width), np.concatenate([extras, fr["rpn_features"]], 1), S)
    out["pooled_xyz"], out["empty"], out["pts_features"] = pp, pe, pf[:, :, E:]
    out["pts_input"][:, :, 3:] = pf[:, :, :E]
    for t in range(R):
        a = aug_draw(seed, frame, t, methods, flip_prob, rot_range)
        out["pts_input"][t, :, :3], out["roi_boxes3d"][t], out["gt_boxes3d"][t], out["gt_boxes3d_ct"][t] = \
            finish_slot(pp[t], s["rois"][t], s["gt_of_rois"][t], a, trig, atan2)
    out["cls_label"], out["reg_valid_mask"] = labels(s["roi_iou"], pe, cfg)
    return out
