"""numpy restatement of the RPN training batch on the device (csrc/train_scene.hip, pointrcnn_amd.kitti_input.TrainScenePreparer):
KittiRCNNDataset.get_rpn_sample in TRAIN mode, one frame at a time, out of parts that are pinned elsewhere --

    oracle.scene_project              lidar -> rect + get_valid_flag (tests/test_oracle_scene.py)
    train_input_twin.gt_aug_sample    the GT-augmentation sampling loop (tests/test_train_input_cpu.py)
    oracle gt_aug_edit / rpn_labels   the h + 2 removal test and the label generation (tests/test_oracle_round2.py)
    oracle ref_trig("atan2f")         csrc/ref_trig.h's atan2f

plus the two pieces that exist nowhere else: the npoints draw over the EDITED cloud (rule of scene_sample_kernel, candidate identity =
raw index, or n_raw + j for the j-th pasted point) and data_augmentation (streams 34-36 of csrc/scene.hip's table).
Pure host code: the expected value of the CPU and GPU tests."""
import math

import numpy as np

import oracle
import train_input_twin as tw

STREAM_ENABLE, STREAM_ANGLE, STREAM_SCALE = 34, 35, 36
METHODS = ("rotation", "scaling", "flip")
F32_PI = np.float32(np.pi)


def _mix(x):
    x = x & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def rand32_vec(seed, stream, frame, idx):
    """train_input_twin.rand32 for an array of positions -> uint64 array of 32-bit values"""
    inner = tw.mix((frame * 0x9E3779B9 + tw.mix((seed + stream * 0x85EBCA6B) & tw.M32)) & tw.M32)
    return _mix(np.asarray(idx, np.uint64) ^ np.uint64(inner))


def draw(ident, far, npoints, seed, frame):
    """The npoints draw of scene_sample_kernel over candidates with the given identities and far flags.
    -> (identity of every output row (npoints,), status); n == 0 -> (all -1, 2)"""
    ident = np.asarray(ident, np.uint64)
    far = np.asarray(far, bool)
    n, f = len(ident), int(far.sum())
    if n == 0:
        return np.full(npoints, -1, np.int64), 2
    st = 0
    if n > npoints:
        keep_all = False
        if f > npoints:
            st, keep_far, k = 1, False, npoints
        else:
            keep_far, k = True, npoints - f
    else:
        keep_all, keep_far = True, False
        k = npoints - n
        if k > n:
            st, k = 1, n
    cand = ~far if keep_far else np.ones(n, bool)
    key0 = rand32_vec(seed, 0, frame, ident) >> np.uint64(2)
    ci = np.nonzero(cand)[0]
    order = ci[np.lexsort((ident[ci], key0[ci]))]                 # ascending (key, identity)
    drawn = order[:k]
    kept = np.nonzero(np.ones(n, bool) if keep_all else (far if keep_far else np.zeros(n, bool)))[0]
    sel = np.concatenate([ident[kept], ident[drawn]])
    skey = np.concatenate([rand32_vec(seed, 1, frame, ident[kept]), rand32_vec(seed, 2 if keep_all else 1, frame, ident[drawn])])
    out = sel[np.lexsort((sel, skey))]
    total = len(out)
    rows = np.arange(npoints)
    return out[np.where(rows < total, rows, rows % total)].astype(np.int64), st


def aug_params(seed, frame, aug):
    """aug: dict AUG_METHOD_LIST (names; () = AUG_DATA false), AUG_METHOD_PROB, AUG_ROT_RANGE
    -> (8,) f64 enable[3], angle, cos, sin, scale, flip; NaN where the rotation / scaling did not run"""
    e = [1.0 - tw.u01(tw.rand32(seed, STREAM_ENABLE, frame, i)) for i in range(3)]
    lst, prob = aug["AUG_METHOD_LIST"], aug["AUG_METHOD_PROB"]
    angle = cs = sn = scale = float("nan")
    flip = 0.0
    if "rotation" in lst and e[0] < prob[0]:
        lo, hi = -(math.pi / aug["AUG_ROT_RANGE"]), math.pi / aug["AUG_ROT_RANGE"]
        angle = lo + (hi - lo) * tw.u01(tw.rand32(seed, STREAM_ANGLE, frame, 0))
        cs, sn = float(np.cos(angle)), float(np.sin(angle))
    if "scaling" in lst and e[1] < prob[1]:
        scale = 0.95 + (1.05 - 0.95) * tw.u01(tw.rand32(seed, STREAM_SCALE, frame, 0))
    if "flip" in lst and e[2] < prob[2]:
        flip = 1.0
    return np.array(e + [angle, cs, sn, scale, flip], np.float64)


def _rotate(x, z, cs, sn):
    x64, z64 = x.astype(np.float64), z.astype(np.float64)
    return (x64 * cs + z64 * (-sn)).astype(np.float32), (x64 * sn + z64 * cs).astype(np.float32)


def augment(pts, boxes, alpha, a, atan2=None):
    """data_augmentation stage 1 on fp32 points (n,3) and boxes (g,7) with the parameters of aug_params"""
    pts, boxes = pts.astype(np.float32).copy(), boxes.astype(np.float32).copy()
    alpha = np.asarray(alpha, np.float32)
    if not np.isnan(a[3]):
        pts[:, 0], pts[:, 2] = _rotate(pts[:, 0], pts[:, 2], a[4], a[5])
        boxes[:, 0], boxes[:, 2] = _rotate(boxes[:, 0], boxes[:, 2], a[4], a[5])
        if len(boxes):
            beta = (atan2 or (lambda y, x: oracle.cpu().ref_trig("atan2f", y, x)))(boxes[:, 2].copy(), boxes[:, 0].copy())
            boxes[:, 6] = ((np.sign(beta) * F32_PI) / np.float32(2) + alpha) - beta
    if not np.isnan(a[6]):
        fs = np.float32(a[6])
        pts = pts * fs
        boxes[:, 0:6] = boxes[:, 0:6] * fs
    if a[7] != 0:
        pts[:, 0] = -pts[:, 0]
        boxes[:, 0] = -boxes[:, 0]
        boxes[:, 6] = np.sign(boxes[:, 6]) * F32_PI - boxes[:, 6]
    return pts, boxes


class Steps:
    """The four places of train_scene where a near miss of the stated semantics is easy to write.  train_scene runs these; the wrong
    restatements of tests/test_train_scene_cpu.py override one each."""
    extra_h = 2.0                                        # the removal box is the accepted box with h + 2

    @staticmethod
    def paste_identity(n_raw, npts):
        """npts: point count of every accepted object, in accepted order -> identity of every pasted point"""
        return n_raw + np.arange(int(np.sum(npts)))

    @staticmethod
    def far(cloud, n_scene):
        """cloud: the edited cloud, its first n_scene rows from the scan, the rest pasted -> the points the draw always keeps"""
        return ~(cloud[:, 2] < np.float32(40.0))

    augment = staticmethod(augment)


def train_scene(raw, calib24, hw, scope, npoints, seed, frame, gt_boxes3d, gt_alpha, all_gt_boxes3d, plane, db, gt_aug, aug,
                max_accept=16, width=None, cos_sin=None, rect_flag=None, atan2=None, steps=Steps):
    """One frame.  raw (n,4), calib24 (24,), hw (H, W), scope 6 floats or None; gt_boxes3d (g,7) / gt_alpha (g,) the training labels;
    all_gt_boxes3d (m,7) + plane (4,) for the sampler; db: dict boxes (D,7), alpha (D,), npts (D,), points (P,3), intensity (P,);
    gt_aug: train_input_twin.gt_aug_sample's cfg dict or None (GT_AUG_ENABLED false); aug: see aug_params.
    width: rows of the returned gt_boxes3d (G + K of the batch; default g + accepted).  cos_sin: (cos, sin) to use instead of numpy's.
    atan2: the fp32 atan2 of the ry update (default: csrc/ref_trig.h's, the contract's; the reference itself ran numpy's arctan2).
    rect_flag: (rect (n,3), flag (n,)) to use instead of oracle.scene_project's (the reference's own sgemm projection).
    steps: the Steps to run (the tests' sensitivity checks pass deliberately wrong ones).
    -> dict pts_rect, pts_features, gt_boxes3d, num_gt, rpn_cls_label, rpn_reg_label, src, nvalid, status, gt_aug_status, ids, aug"""
    cpu = oracle.cpu()
    raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 4)
    n_raw = raw.shape[0]
    gt = np.asarray(gt_boxes3d, np.float32).reshape(-1, 7)
    galpha = np.asarray(gt_alpha, np.float32).reshape(-1)
    if rect_flag is not None:
        rect, flag = np.ascontiguousarray(rect_flag[0], np.float32), np.asarray(rect_flag[1], bool)
    elif n_raw:
        rect, _, _, flag = oracle.scene_project(raw, calib24, hw[0], hw[1], scope)
    else:
        rect, flag = np.zeros((0, 3), np.float32), np.zeros(0, bool)
    ids, placed, palpha, shift, gstat = np.zeros(0, np.int32), np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0), 0
    sampler = None
    if gt_aug is not None:
        sampler = tw.gt_aug_sample(all_gt_boxes3d, plane, db["boxes"], db["alpha"], db["npts"], gt_aug, seed, frame, max_accept)
        gstat = sampler["status"]
        if gstat not in (1, 3):
            ids, placed, palpha, shift = sampler["ids"], sampler["boxes"], sampler["alpha"], sampler["y_shift"]
    keep = flag.copy()
    if len(ids) and n_raw:
        removed = cpu.gt_aug_edit(rect[None], np.zeros((1, n_raw), np.float32), placed[None], np.zeros((1, 0, 3), np.float32),
                                  np.zeros((1, 0), np.float32), extra_h=steps.extra_h)[3][0]
        keep &= removed == 0
    off = np.concatenate([[0], np.cumsum(db["npts"])]).astype(np.int64) if db is not None else None
    ppts, pint = [np.zeros((0, 3), np.float32)], [np.zeros(0, np.float32)]
    for a, i in enumerate(ids):
        p = np.asarray(db["points"][off[i]:off[i + 1]], np.float32).copy()
        p[:, 1] = (p[:, 1].astype(np.float64) - shift[a]).astype(np.float32)
        ppts.append(p)
        pint.append(np.asarray(db["intensity"][off[i]:off[i + 1]], np.float32))
    ppts, pint = np.concatenate(ppts), np.concatenate(pint)
    raw_idx = np.nonzero(keep)[0]
    ident = np.concatenate([raw_idx, steps.paste_identity(n_raw, [db["npts"][i] for i in ids])]).astype(np.int64)
    cloud = np.concatenate([rect[keep], ppts])
    inten = np.concatenate([raw[keep, 3], pint])
    far = steps.far(cloud, len(raw_idx))
    src, status = draw(ident, far, npoints, seed, frame)
    if status == 2:
        pts, feat = np.zeros((npoints, 3), np.float32), np.zeros(npoints, np.float32)
    else:
        pos = np.full(n_raw + len(ppts) + 1, -1, np.int64)
        pos[ident] = np.arange(len(ident))
        rows = pos[src]
        pts, feat = cloud[rows], inten[rows] - np.float32(0.5)
    boxes = np.concatenate([gt, placed]).astype(np.float32)
    alphas = np.concatenate([galpha, palpha]).astype(np.float32)
    a = aug_params(seed, frame, aug)
    if cos_sin is not None and not np.isnan(a[3]):
        a[4], a[5] = cos_sin
    apts, aboxes = steps.augment(pts, boxes, alphas, a, atan2)
    if status == 2:
        apts = np.zeros((npoints, 3), np.float32)
    ng = len(aboxes)
    width = ng if width is None else width
    out_boxes = np.zeros((width, 7), np.float32)
    out_boxes[:ng] = aboxes
    cls, reg = cpu.rpn_labels(apts[None], out_boxes[None] if width else np.zeros((1, 0, 7), np.float32), np.array([ng], np.int32))
    return {"pts_rect": apts, "pts_features": feat.reshape(-1, 1), "gt_boxes3d": out_boxes, "num_gt": ng, "rpn_cls_label": cls[0],
            "rpn_reg_label": reg[0], "src": src.astype(np.int32), "nvalid": len(ident), "status": status, "gt_aug_status": gstat,
            "ids": ids, "aug": a, "sampler": sampler, "cloud": cloud, "ident": ident}


def fixture_case(z, k):
    """case k of tests/golden/train_scene_ref.npz -> the keyword arguments of train_scene (and of TrainScenePreparer, see the tests)"""
    from util import synthetic_scan
    n, scan_seed, fov, far = z["c%d_scan" % k]
    enabled, extra, rand_num, prob, ratio, use_scope = z["c%d_gt_aug" % k]
    a = z["c%d_aug" % k]
    scope = tuple(z["scope"]) if use_scope else None
    gt_aug = {"GT_EXTRA_NUM": int(extra), "GT_AUG_RAND_NUM": bool(rand_num), "GT_AUG_APPLY_PROB": float(prob),
              "GT_AUG_HARD_RATIO": float(ratio), "PC_AREA_SCOPE": scope, "TRY_TIMES": 100} if enabled else None
    aug = {"AUG_METHOD_LIST": tuple(m for m, on in zip(METHODS, a[1:4]) if on) if a[0] else (), "AUG_METHOD_PROB": tuple(a[4:7]),
           "AUG_ROT_RANGE": 18}
    db = {"boxes": z["db_boxes"], "alpha": z["db_alpha"], "npts": z["db_npts"], "points": z["db_points"], "intensity": z["db_intensity"]}
    return dict(raw=synthetic_scan(int(n), int(scan_seed), float(fov), float(far)), hw=tuple(int(v) for v in z["c%d_hw" % k]),
                scope=scope, npoints=int(z["npoints"]), seed=int(z["c%d_seed" % k]), frame=int(z["c%d_frame" % k]),
                gt_boxes3d=z["c%d_train_gt" % k], gt_alpha=z["c%d_train_alpha" % k], all_gt_boxes3d=z["c%d_all_gt" % k],
                plane=z["c%d_plane" % k], db=db, gt_aug=gt_aug, aug=aug)


def fixture_rect(z, k, calib24, kw):
    """the reference's own projection of case k: the canonical rect moved by the recorded number of fp32 steps, and its valid flags"""
    can = oracle.scene_project(kw["raw"], calib24, kw["hw"][0], kw["hw"][1], kw["scope"])[0]
    rect = (can.view(np.int32) + z["c%d_rect_ulp" % k].astype(np.int32)).view(np.float32)
    return rect, np.unpackbits(z["c%d_flag" % k])[:len(rect)].astype(bool)
