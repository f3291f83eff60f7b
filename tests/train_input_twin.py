"""numpy / Python restatement of the GT-augmentation sampling on the device (csrc/train_input.hip, csrc/quad_clip.h).

    corners3d(boxes)            kitti_utils.boxes3d_to_corners3d in fp32, accumulated as numpy's matmul does
    corner_iou3d(a, b, bev)     kitti_utils.get_iou3d with shapely's clip restated in Python doubles (same steps as quad_clip.h)
    gt_aug_sample(...)          apply_gt_aug_to_one_scene's sampling loop for one frame, random calls from the counter table

Pure host code: used by the CPU tests, by the GPU tests as the expected value, and by tests/golden/ref_train_input.py in place of
the reference's shapely-based get_iou3d.
"""
import numpy as np

M32 = 0xFFFFFFFF
STREAM_APPLY, STREAM_EXTRA, STREAM_HARD, STREAM_INDEX = 30, 31, 32, 33


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def rand32(seed, stream, frame, i):
    return mix(i ^ mix((frame * 0x9E3779B9 + mix((seed + stream * 0x85EBCA6B) & M32)) & M32))


def u01(r):
    return float(np.float32(r >> 8) * np.float32(1.0 / 16777216.0))


def below(r, n):
    return (r * n) >> 32


def corners3d(boxes):
    """(N,7) fp32 [x,y,z,h,w,l,ry] -> (N,8,3) fp32: local corners x = +-l/2, z = +-w/2, y = 0 / -h, rotated about y by a
    row-vector product summed left to right from zero (numpy's matmul on these strides), then shifted"""
    b = np.asarray(boxes, np.float32).reshape(-1, 7)
    h, w, l, ry = b[:, 3], b[:, 4], b[:, 5], b[:, 6]
    hl, hw = l / np.float32(2), w / np.float32(2)
    xs = np.stack([hl, hl, -hl, -hl, hl, hl, -hl, -hl], 1)
    zs = np.stack([hw, -hw, -hw, hw, hw, -hw, -hw, hw], 1)
    zero = np.zeros_like(h)
    ys = np.stack([zero] * 4 + [-h] * 4, 1)
    cs, sn = np.cos(ry)[:, None], np.sin(ry)[:, None]
    f0, f1 = np.float32(0), np.float32(1)
    xr = (xs * cs + ys * f0) + zs * sn
    yr = (xs * f0 + ys * f1) + zs * f0
    zr = (xs * -sn + ys * f0) + zs * cs
    return np.stack([b[:, 0:1] + xr, b[:, 1:2] + yr, b[:, 2:3] + zr], 2).astype(np.float32)


def _heights(c):
    y = c[:, 1]
    lo = -(((y[0] + y[1]) + y[2]) + y[3]) / np.float32(4)
    hi = -(((y[4] + y[5]) + y[6]) + y[7]) / np.float32(4)
    return np.float32(lo), np.float32(hi)


def _cross(ax, az, bx, bz, px, pz):
    return (bx - ax) * (pz - az) - (bz - az) * (px - ax)


def _shoelace(x, z):
    s = 0.0
    n = len(x)
    for i in range(n):
        j = 0 if i + 1 == n else i + 1
        s = s + (x[i] * z[j] - x[j] * z[i])
    return abs(s) * 0.5


def _quad(c):
    """corners 0:4 in (x, z) as doubles, counter-clockwise; area 0 when not strictly convex"""
    x = [float(c[k, 0]) for k in range(4)]
    z = [float(c[k, 2]) for k in range(4)]
    pos = neg = 0
    for k in range(4):
        a, b, n = k, (k + 1) & 3, (k + 2) & 3
        t = _cross(x[a], z[a], x[b], z[b], x[n], z[n])
        pos += t > 0.0
        neg += t < 0.0
    if neg == 4:
        x, z = x[::-1], z[::-1]
    area = _shoelace(x, z) if (pos == 4 or neg == 4) else 0.0
    return x, z, area


def _overlap(qa, qb):
    px, pz = list(qa[0]), list(qa[1])
    bx, bz = qb[0], qb[1]
    for e in range(4):
        if not px:
            break
        ex0, ez0, ex1, ez1 = bx[e], bz[e], bx[(e + 1) & 3], bz[(e + 1) & 3]
        qx, qz = [], []
        n = len(px)
        sp = _cross(ex0, ez0, ex1, ez1, px[n - 1], pz[n - 1])
        for i in range(n):
            j = n - 1 if i == 0 else i - 1
            sc = _cross(ex0, ez0, ex1, ez1, px[i], pz[i])
            if (sc >= 0.0) != (sp >= 0.0) and len(qx) < 16:
                t = sp / (sp - sc)
                qx.append(px[j] + t * (px[i] - px[j]))
                qz.append(pz[j] + t * (pz[i] - pz[j]))
            if sc >= 0.0 and len(qx) < 16:
                qx.append(px[i])
                qz.append(pz[i])
            sp = sc
        px, pz = qx, qz
    return 0.0 if len(px) < 3 else _shoelace(px, pz)


def pair_iou(ca, cb):
    """(iou3d, iou_bev) as fp32 for two (8,3) corner sets"""
    lo_a, hi_a = _heights(ca)
    lo_b, hi_b = _heights(cb)
    h = np.float32(min(hi_a, hi_b) - max(lo_a, lo_b))
    if not h > 0:
        return np.float32(0), np.float32(0)
    qa, qb = _quad(ca), _quad(cb)
    if qa[2] == 0.0 or qb[2] == 0.0:
        return np.float32(0), np.float32(0)
    o = _overlap(qa, qb)
    o3 = o * float(h)
    iou3d = o3 / ((qa[2] * float(np.float32(hi_a - lo_a)) + qb[2] * float(np.float32(hi_b - lo_b))) - o3)
    return np.float32(iou3d), np.float32(o / ((qa[2] + qb[2]) - o))


def corner_iou3d(corners_a, corners_b, need_bev=False):
    """kitti_utils.get_iou3d's signature and result, without shapely"""
    A = np.asarray(corners_a, np.float32)
    B = np.asarray(corners_b, np.float32)
    iou3d = np.zeros((A.shape[0], B.shape[0]), np.float32)
    bev = np.zeros_like(iou3d)
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            iou3d[i, j], bev[i, j] = pair_iou(A[i], B[j])
    return (iou3d, bev) if need_bev else iou3d


def gt_aug_sample(gt_boxes3d, plane, db_boxes, db_alpha, db_npts, cfg, seed, frame, max_accept=16, iou=None):
    """One frame of prcnn_gt_aug_sample.  cfg: dict GT_EXTRA_NUM, GT_AUG_RAND_NUM, GT_AUG_APPLY_PROB, GT_AUG_HARD_RATIO,
    PC_AREA_SCOPE (6 floats or None), TRY_TIMES.  -> dict(ids, boxes, alpha, y_shift, stats=(applied, extra, cnt, started), status)
    iou(corners_new, corners_entry) -> fp32 iou3d replaces pair_iou in the collision test (tests/exact_quad.py plugs in here)"""
    if iou is None:
        iou = lambda p, q: pair_iou(p, q)[0]            # noqa: E731
    db_boxes = np.asarray(db_boxes, np.float32)
    db_npts = np.asarray(db_npts)
    ratio = float(cfg["GT_AUG_HARD_RATIO"])
    easy = np.nonzero(db_npts > 100)[0]
    hard = np.nonzero(db_npts <= 100)[0]
    a, b, c, d = (float(v) for v in plane)
    scope = cfg["PC_AREA_SCOPE"]
    cur = np.asarray(gt_boxes3d, np.float32).reshape(-1, 7).copy()
    cur[:, 4] += np.float32(0.5)
    cur[:, 5] += np.float32(0.5)
    lst = list(corners3d(cur))
    out = dict(ids=[], boxes=[], alpha=[], y_shift=[], status=0)
    applied = int(u01(rand32(seed, STREAM_APPLY, frame, 0)) < float(cfg["GT_AUG_APPLY_PROB"]))
    extra = int(cfg["GT_EXTRA_NUM"])
    cnt = started = 0
    if applied and cfg["GT_AUG_RAND_NUM"]:
        if extra <= 10:
            out["status"] = 1
        else:
            extra = 10 + below(rand32(seed, STREAM_EXTRA, frame, 0), extra - 10)
    if applied and out["status"] == 0:
        for t in range(int(cfg["TRY_TIMES"])):
            if cnt > extra:
                break
            started = t + 1
            if ratio > 0:
                use_easy = u01(rand32(seed, STREAM_HARD, frame, t)) > ratio
                lst_ids = easy if use_easy else hard
                if len(lst_ids) == 0:
                    out["status"] = 1
                    break
                i = int(lst_ids[below(rand32(seed, STREAM_INDEX, frame, t), len(lst_ids))])
            else:
                if len(db_boxes) == 0:
                    out["status"] = 1
                    break
                i = below(rand32(seed, STREAM_INDEX, frame, t), len(db_boxes))
            box = db_boxes[i].copy()
            x, y, z = (float(v) for v in box[:3])
            if scope is not None and not (scope[0] <= x <= scope[1] and scope[2] <= y <= scope[3] and scope[4] <= z <= scope[5]):
                continue
            if db_npts[i] < 5:
                continue
            cur_h = ((-d - a * x) - c * z) / b
            move = y - cur_h
            box[1] = np.float32(y - move)
            enl = box.copy()
            enl[4] += np.float32(0.5)
            enl[5] += np.float32(0.5)
            cnt += 1
            if not lst:
                out["status"] = 1
                break
            nc = corners3d(enl)[0]
            if not all(iou(nc, e) < np.float32(1e-8) for e in lst):
                continue
            if len(out["ids"]) >= max_accept:
                out["status"] = 2
                break
            lst.append(nc)
            out["ids"].append(i)
            out["boxes"].append(box)
            out["alpha"].append(np.float32(db_alpha[i]))
            out["y_shift"].append(move)
    out["stats"] = (applied, extra, cnt, started)
    out["ids"] = np.asarray(out["ids"], np.int32)
    out["boxes"] = np.asarray(out["boxes"], np.float32).reshape(-1, 7)
    out["alpha"] = np.asarray(out["alpha"], np.float32)
    out["y_shift"] = np.asarray(out["y_shift"], np.float64)
    return out


def rect_corners(cx, cz, hx, hz, y0=0.0, h=1.0):
    """(8,3) corners of an axis-aligned box with bottom y0 and height h: bottom (x, z) = [cx +- hx] x [cz +- hz]"""
    xs = [cx + hx, cx + hx, cx - hx, cx - hx]
    zs = [cz + hz, cz - hz, cz - hz, cz + hz]
    c = [(xs[k], y0, zs[k]) for k in range(4)] + [(xs[k], y0 - h, zs[k]) for k in range(4)]
    return np.asarray(c, np.float32)
