"""TEST INFRASTRUCTURE: numpy / Python twin of the offline GT-augmented scene generator (csrc/aug_scene.hip, csrc/aug_scene_math.h;
tools/generate_aug_scene.py of the reference), the synthetic tree it runs on, and the table tests/aug_scene_host.cpp is run against.

    sample(...)        AugSceneGenerator.aug_one_scene's sampling loop for one frame; random calls from the counter table
                       (stream 60: extra_gt_num, stream 61: the index of try t), the pair IoU from the CPU oracle's boxes_iou3d
    build(...)         the augmented cloud of one frame: the oracle's scene_project (canonical lidar -> rect, valid flag), the oracle's
                       pts_in_boxes3d on the accepted boxes with h + 2, the pasted points with y - y_shift
    write_aug_tree     tests/kitti_tree.py's tree plus planes/ and the labels of CASE frames; database(): the GT database the tests use
    generate(...)      every epoch and frame of the tree -> {new id: dict}, split list (label text through the package's formatters)
Pure host code: the expected value of the CPU and the GPU tests, checked itself against the reference's own tool through the fixture
tests/golden/aug_scene_ref.npz (tests/golden/ref_aug_scene.py).
"""
import os
import struct

import numpy as np

import kitti_tree
from train_input_twin import below, rand32

F32 = np.float32
STREAM_EXTRA, STREAM_INDEX = 60, 61
TRIES = 50
SCOPE = (-40.0, 40.0, -1.0, 3.0, 0.0, 70.4)                       # generate_aug_scene.py:27, --class_name Car


def sample(all_gt, plane, db_boxes, db_npts, seed, frame, scope=SCOPE, iou=None):
    """-> dict ids (n) i32, boxes (n,7) f32 placed and unenlarged, y_shift (n) f64, stats (extra_gt_num, cnt, tries spent), status.
    iou(a (1,7), b (M,7)) -> (1,M) f32; default: the CPU oracle's boxes_iou3d"""
    if iou is None:
        import oracle
        iou = oracle.cpu().boxes_iou3d
    cur = np.array(all_gt, F32).reshape(-1, 7)
    cur[:, 4] += F32(0.5)
    cur[:, 5] += F32(0.5)
    db_boxes = np.asarray(db_boxes, F32).reshape(-1, 7)
    D = len(db_boxes)
    a, b, c, d = (float(v) for v in plane)
    extra = 10 + below(rand32(seed, STREAM_EXTRA, frame, 0), 5)
    ids, boxes, shifts, status, cnt, spent = [], [], [], 0, 0, 0
    for t in range(TRIES):
        spent = t + 1
        if D - 1 <= 0:                                            # np.random.randint(0, 0) raises
            status = 1
            break
        i = below(rand32(seed, STREAM_INDEX, frame, t), D - 1)
        box = db_boxes[i].copy()
        x, y, z = (float(v) for v in box[:3])
        if not (scope[0] <= x <= scope[1] and scope[2] <= y <= scope[3] and scope[4] <= z <= scope[5]):
            continue
        if cnt > extra:
            break
        if db_npts[i] < 5:
            continue
        with np.errstate(all="ignore"):
            cur_h = np.float64((-d - a * x) - c * z) / np.float64(b)
            move = float(y - cur_h)
            box[1] = F32(y - move)
        cnt += 1
        if len(cur) == 0:                                         # max() of an empty array raises
            status = 1
            break
        v = np.asarray(iou(box.reshape(1, 7), cur), F32)
        if not v.max() < F32(1e-8):
            continue
        enl = box.copy()
        enl[4] += F32(0.5)
        enl[5] += F32(0.5)
        cur = np.concatenate([cur, enl.reshape(1, 7)])
        ids.append(i); boxes.append(box); shifts.append(move)
    return {"ids": np.asarray(ids, np.int32), "boxes": np.asarray(boxes, F32).reshape(-1, 7), "y_shift": np.asarray(shifts, np.float64),
            "stats": (extra, cnt, spent), "status": status}


def build(scan, calib24, img_hw, acc, db_points, db_intensity, db_offsets, scope=SCOPE):
    """-> cloud (n,4) f32 [x y z intensity], src (n) i32 (raw index; -1 - database row for a pasted point), kept (survivors)"""
    import oracle
    from util import KERNEL_TRIG
    scan = np.ascontiguousarray(scan, F32).reshape(-1, 4)
    rect, _, _, flag = oracle.scene_project(scan, calib24, img_hw[0], img_hw[1], scope)
    keep = flag.copy()
    use = acc["status"] != 1 and len(acc["ids"]) > 0
    if use and len(scan):
        big = acc["boxes"].copy()
        big[:, 3] += F32(2)
        keep &= ~(oracle.cpu().pts_in_boxes3d(rect, big, trig_mode=KERNEL_TRIG) == 1).any(axis=0)
    rows, src = [np.concatenate([rect[keep], scan[keep, 3:4]], 1)], [np.nonzero(keep)[0].astype(np.int32)]
    if use:
        for i, move in zip(acc["ids"], acc["y_shift"]):
            o, e = int(db_offsets[i]), int(db_offsets[i + 1])
            p = np.array(db_points[o:e], F32).reshape(-1, 3)
            p[:, 1] = (p[:, 1].astype(np.float64) - move).astype(F32)
            rows.append(np.concatenate([p, np.asarray(db_intensity[o:e], F32).reshape(-1, 1)], 1))
            src.append((-1 - np.arange(o, e)).astype(np.int32))
    return np.concatenate(rows).astype(F32).reshape(-1, 4), np.concatenate(src).astype(np.int32), int(keep.sum())


# ---- the synthetic tree ----------------------------------------------------------------------------------------------------------
FRAMES = (0, 1, 2, 3)                     # the train split
DB_FRAMES = (7, 8)                        # frames whose Car labels are the GT database (not in the split)
SEED0, N_SCAN = 900, 2500
DONTCARE = "DontCare -1 -1 -10 500.00 160.00 520.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10"
PLANES = {0: (0.0, -1.0, 0.0, 1.65), 1: (0.02, -1.0, 0.01, 1.7), 2: (0.0, -1.0, 0.0, 1.65), 3: (-0.01, 1.0, 0.02, -1.6)}
TRUNC_OCCL = ((0.0, 0), (0.1, 1), (0.35, 2), (0.55, 3))


def _line(cls, trunc, occ, alpha, dims, pos, ry):
    return "%s %.2f %d %.2f 100.00 150.00 300.00 250.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % ((cls, trunc, occ, alpha) + tuple(dims) + tuple(pos) + (ry,))


def frame_labels(frame):
    """the label text of a tree frame.  0: Car, Van, Pedestrian, a Car outside the scope, DontCare; 1: Cyclist, Car, two DontCare;
    2: only DontCare (the collision list starts empty: the reference raises); 3: large boxes tile the road (most tries collide);
    7, 8: the database's cars on a grid, far apart, with two centres outside the scope"""
    rng = np.random.default_rng(4000 + frame)
    car = (1.5, 1.6, 3.9)
    if frame == 0:
        return [_line("Car", 0.0, 0, 0.1, car, (6.0, 1.6, 30.0), 0.3), DONTCARE, _line("Van", 0.2, 1, -0.4, (2.2, 1.9, 5.0), (-8.0, 1.7, 45.0), 1.2),
                _line("Pedestrian", 0.0, 2, 0.0, (1.7, 0.6, 0.8), (12.0, 1.5, 12.0), 0.0), _line("Car", 0.5, 3, 1.0, car, (60.0, 1.7, 20.0), 0.1)]
    if frame == 1:
        return [DONTCARE, _line("Cyclist", 0.0, 0, 0.3, (1.7, 0.6, 1.8), (0.0, 1.6, 20.0), 1.5), DONTCARE,
                _line("Car", 0.12, 1, -1.3, car, (-10.0, 1.65, 25.0), -2.0)]
    if frame == 2:
        return [DONTCARE]
    if frame == 3:
        return [DONTCARE] + [_line("Truck", 0.0, 0, 0.0, (4.2, 9.5, 9.5), (x, 1.6, z), 0.0) for x in np.arange(-36.0, 37.0, 9.0)
                             for z in np.arange(6.0, 70.0, 9.0)]
    out, k = [], 0
    for x in np.arange(-33.0, 34.0, 11.0):
        for z in (10.0, 28.0, 46.0, 64.0):
            if (k % 2 == 0) == (frame == 7):
                t, o = TRUNC_OCCL[k % 4]
                out.append(_line("Car", t, o, rng.uniform(-3, 3), (rng.uniform(1.4, 1.7), rng.uniform(1.5, 1.8), rng.uniform(3.4, 4.4)),
                                 (x + rng.uniform(-1, 1), rng.uniform(1.2, 2.0), z + rng.uniform(-1, 1)), rng.uniform(-3.14, 3.14)))
            k += 1
    out.insert(3, _line("Car", 0.0, 0, 0.0, car, (45.0 if frame == 7 else 5.0, 1.6, 20.0 if frame == 7 else 75.0), 0.5))
    return out


def write_aug_tree(root):
    """kitti_tree.write_tree for FRAMES + DB_FRAMES, their labels, planes/ for FRAMES, ImageSets/train.txt = FRAMES.  -> training dir"""
    base = kitti_tree.write_tree(root, FRAMES + DB_FRAMES, seed0=SEED0, n_scan=N_SCAN)
    os.makedirs(os.path.join(base, "planes"), exist_ok=True)
    for f in FRAMES + DB_FRAMES:
        with open(os.path.join(base, "label_2", "%06d.txt" % f), "w") as fh:
            fh.write("".join(ln + "\n" for ln in frame_labels(f)))
    for f in FRAMES:
        with open(os.path.join(base, "planes", "%06d.txt" % f), "w") as fh:
            fh.write("# Plane\nWidth 4\nHeight 1\n%s\n" % " ".join("%.6e" % v for v in PLANES[f]))
    with open(os.path.join(str(root), "KITTI", "ImageSets", "train.txt"), "w") as fh:
        fh.write("".join("%06d\n" % f for f in FRAMES))
    return base


def database_arrays():
    """the GT database of the tree: the Car labels of DB_FRAMES in file order, with synthetic points (2 .. 120 per object; the objects
    with 2 and 4 points are never accepted) -> dict boxes (D,7), alpha, sample_id, cls_type, truncation, occlusion, points, intensity"""
    from pointrcnn_amd import kitti_input
    rng = np.random.default_rng(77)
    boxes, alpha, sid, trunc, occl, pts, inten = [], [], [], [], [], [], []
    for f in DB_FRAMES:
        lab = kitti_input.read_label_lines(frame_labels(f))
        for k in range(len(lab["cls_type"])):
            n = (2, 4, 30, 60, 120, 17, 5)[len(boxes) % 7]
            b = lab["boxes3d"][k]
            boxes.append(b); alpha.append(lab["alpha"][k]); sid.append(f); trunc.append(lab["truncation"][k]); occl.append(lab["occlusion"][k])
            pts.append(np.stack([b[0] + rng.uniform(-1, 1, n), b[1] - rng.uniform(0, b[3], n), b[2] + rng.uniform(-1, 1, n)], 1).astype(F32))
            inten.append(rng.uniform(0, 1, n).astype(F32))
    return {"boxes": np.stack(boxes).astype(F32), "alpha": np.asarray(alpha, F32), "sample_id": np.asarray(sid, np.int64),
            "cls_type": np.array(["Car"] * len(boxes), np.str_), "truncation": np.asarray(trunc), "occlusion": np.asarray(occl),
            "points": pts, "intensity": inten}


def database(device="cpu"):
    from pointrcnn_amd import kitti_input
    d = database_arrays()
    return kitti_input.GTDatabase(d["boxes"], d["alpha"], d["points"], d["intensity"], 0.0, device, d["sample_id"], d["cls_type"])


def generate(root, aug_times, seed, iou=None):
    """the twin's train_aug split of the tree at root -> ({new id: dict ids, boxes, y_shift, stats, status, cloud, src, labels}, split list)"""
    from pointrcnn_amd import kitti_input
    base = os.path.join(str(root), "KITTI", "object", "training")
    d = database_arrays()
    npts = np.array([len(p) for p in d["points"]], np.int32)
    off = np.concatenate([[0], np.cumsum(npts)])
    dbp, dbi = np.concatenate(d["points"]), np.concatenate(d["intensity"])
    out, split = {}, ["%06d" % f for f in FRAMES]
    for epoch in range(aug_times):
        for f in FRAMES:
            new_id = (epoch + 1) * 10000 + f
            with open(os.path.join(base, "label_2", "%06d.txt" % f)) as fh:
                lines = [ln for ln in fh.readlines() if ln.strip()]
            lab = kitti_input.read_label_lines(lines)
            with open(os.path.join(base, "planes", "%06d.txt" % f)) as fh:
                plane = kitti_input.road_plane_from_lines(fh.readlines())
            calib = kitti_input.Calibration(os.path.join(base, "calib", "%06d.txt" % f))
            hw = kitti_tree.image_shape(f)
            acc = sample(lab["boxes3d"][lab["cls_type"] != "DontCare"], plane, d["boxes"], npts, seed, new_id, iou=iou)
            cloud, src, _ = build(kitti_input.get_lidar(os.path.join(base, "velodyne", "%06d.bin" % f)), calib.packed(), hw, acc, dbp, dbi, off)
            text = [kitti_input.reprint_label_line(ln) for ln, c in zip(lines, lab["cls_type"]) if c == "Car"]
            if acc["status"] != 1 and len(acc["ids"]):
                text += kitti_input.aug_object_lines(acc["boxes"], d["truncation"][acc["ids"]], d["occlusion"][acc["ids"]], calib.P2, hw, "Car")
            out[new_id] = dict(acc, cloud=cloud, src=src, labels=text)
            split.append("%06d" % new_id)
    return out, split


# ---- the table of tests/aug_scene_host.cpp ----------------------------------------------------------------------------------------
def host_table(path, seed, frames, D, boxes, planes, scope=SCOPE):
    """records for aug_scene_host: header [seed, nframes, D, nboxes] i32 + 6 doubles scope, frames i32, then per box 7 f32 + 4 f64 plane
    + 1 f32 iou.  -> the expected words: per frame extra + TRIES draws, per box (in_scope, new y bits, move (2 words), enlarged w, l bits,
    collides) as the twin's arithmetic gives them"""
    rng = np.random.default_rng(5)
    edge = F32(1e-8)                                              # the threshold as float32, its two neighbours, nan, -0
    ious = np.concatenate([np.array([0.0, edge, np.nextafter(edge, F32(0)), np.nextafter(edge, F32(1)), np.nan, -0.0, 1.0], F32),
                           rng.uniform(0, 2e-8, len(boxes)).astype(F32)])[:len(boxes)]
    with open(path, "wb") as f:
        f.write(struct.pack("<4i6d", seed, len(frames), D, len(boxes), *scope))
        f.write(np.asarray(frames, np.int32).tobytes())
        for b, p, v in zip(boxes, planes, ious):
            f.write(np.asarray(b, F32).tobytes() + np.asarray(p, np.float64).tobytes() + F32(v).tobytes())
    want = []
    for fr in frames:
        want.append(10 + below(rand32(seed, STREAM_EXTRA, int(fr), 0), 5))
        want += [below(rand32(seed, STREAM_INDEX, int(fr), t), D - 1) for t in range(TRIES)]
    for b, p, v in zip(boxes, planes, ious):
        b = np.asarray(b, F32)
        x, y, z = (float(t) for t in b[:3])
        with np.errstate(all="ignore"):
            move = float(y - np.float64((-p[3] - p[0] * x) - p[2] * z) / np.float64(p[1]))
            ny = F32(y - move)
        want.append(int(scope[0] <= x <= scope[1] and scope[2] <= y <= scope[3] and scope[4] <= z <= scope[5]))
        want += list(struct.unpack("<i", struct.pack("<f", ny))) + list(struct.unpack("<2i", struct.pack("<d", move)))
        want += list(struct.unpack("<2i", struct.pack("<2f", b[4] + F32(0.5), b[5] + F32(0.5))))
        want.append(int(not (v < F32(1e-8))))
    return np.asarray(want, np.int32)
