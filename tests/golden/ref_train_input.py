"""Run the REFERENCE's own KittiRCNNDataset.apply_gt_aug_to_one_scene (lib/datasets/kitti_rcnn_dataset.py:408-497) on a small
synthetic KITTI tree and GT database, with its random calls answered from the counter-based table of csrc/train_input.hip.

Only used to GENERATE tests/golden/train_input_ref.npz (python tests/golden/ref_train_input.py) in the build container: it needs
the reference tree.  What is replaced:
  - kitti_utils.get_iou3d -> tests/train_input_twin.py corner_iou3d, the float64 restatement of shapely's clip (shapely is not
    installed here).  This is the only replaced piece of the reference's arithmetic.  So every IoU behind the fixture is the
    TWIN's: the fixture pins the sampling loop and the random stream, not get_iou3d.  The twin and the kernel are pinned to an
    exact rational clip instead (tests/exact_quad.py, tests/test_quad_exact_cpu.py, tests/test_gpu_train_input.py);
  - roipool3d_cuda.pts_in_boxes3d_cpu (a compiled extension) -> this library's host twin of the same C++ code;
  - np.random.rand / np.random.randint while the method runs -> the table (stream 31 extra_gt_num, 32 easy/hard, 33 index).
The apply-probability draw of get_rpn_sample (:279, stream 30) is the one line restated outside the method.  The tree holds
plane files (read by the reference's get_road_plane) and label files with DontCare, Van and out-of-range objects (read by its
get_label + filtrate_dc_objects); the database is a list of dicts holding the reference's Object3d, deep-copied per call so that
the in-place drift of obj.pos (:461) does not leak between cases.
"""
import copy
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
import train_input_twin as tw          # noqa: E402

SCOPE = (-40.0, 40.0, -1.0, 3.0, 0.0, 70.4)


def make_database(rng):
    """44 objects: 40 clustered in front of the car (x -12..12, z 8..32), 4 with the centre outside PC_AREA_SCOPE; point counts
    from 2 to 260 (easy > 100, hard <= 100, some < 5)"""
    n_in, n_out = 40, 4
    xs = np.concatenate([rng.uniform(-12, 12, n_in), [45.0, -44.0, 5.0, 0.0]])
    zs = np.concatenate([rng.uniform(8, 32, n_in), [20.0, 15.0, 75.0, -2.0]])
    ys = rng.uniform(1.2, 2.0, n_in + n_out)
    dims = np.stack([rng.uniform(1.4, 1.7, n_in + n_out), rng.uniform(1.5, 1.8, n_in + n_out), rng.uniform(3.4, 4.4, n_in + n_out)], 1)
    ry = rng.uniform(-np.pi, np.pi, n_in + n_out)
    npts = rng.choice([2, 4, 30, 60, 90, 120, 180, 260], n_in + n_out)
    lines, pts, inten = [], [], []
    for k in range(n_in + n_out):
        h, w, l = dims[k]
        lines.append("Car 0.00 0 %.2f 100.00 150.00 300.00 250.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f"
                     % (rng.uniform(-3, 3), h, w, l, xs[k], ys[k], zs[k], ry[k]))
        p = np.stack([xs[k] + rng.uniform(-1, 1, npts[k]), ys[k] - rng.uniform(0, h, npts[k]), zs[k] + rng.uniform(-1, 1, npts[k])], 1)
        pts.append(p.astype(np.float32))
        inten.append(rng.uniform(0, 1, npts[k]).astype(np.float32))
    return lines, pts, inten


def label_lines(kind, rng):
    dc = "DontCare -1 -1 -10 500.00 160.00 520.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10"
    if kind == "sparse":
        objs = [("Car", 6.0, 1.6, 40.0, 0.3), ("Van", -8.0, 1.7, 50.0, 1.2), ("Pedestrian", 30.0, 1.5, 5.0, 0.0),
                ("Car", 60.0, 1.7, 20.0, 0.1)]                       # the last one lies outside PC_AREA_SCOPE
        out = [dc]
    elif kind == "cluster":                                           # a few boxes inside the database's cluster
        objs = [("Car", -4.0, 1.6, 14.0, 0.2), ("Van", 5.0, 1.7, 24.0, -1.0), ("Cyclist", 0.0, 1.6, 20.0, 1.5)]
        out = [dc, dc]
    elif kind == "crowded":                                           # large boxes tile the whole cluster: every try collides
        objs = [("Truck", x, 1.6, z, 0.0) for x in np.arange(-14.0, 15.0, 4.0) for z in np.arange(6.0, 35.0, 4.0)]
        out = [dc]
    else:                                                             # only DontCare: the collision list starts empty
        return [dc]
    for cls, x, y, z, ry in objs:
        dims = (4.2, 4.5, 4.5) if cls == "Truck" else (1.5, 1.6, 3.9)
        out.insert(rng.integers(0, len(out) + 1), "%s 0.00 0 0.10 100.00 150.00 300.00 250.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f"
                   % ((cls,) + dims + (x, y, z, ry)))
    return out


# (label kind, GT_EXTRA_NUM, GT_AUG_RAND_NUM, GT_AUG_APPLY_PROB, GT_AUG_HARD_RATIO, use PC_AREA_SCOPE, seed, plane)
CASES = [
    ("sparse", 15, True, 1.0, 0.6, True, 1, (0.0, -1.0, 0.0, 1.65)),
    ("cluster", 15, True, 1.0, 0.6, True, 2, (0.02, -1.0, 0.01, 1.7)),
    ("crowded", 200, False, 1.0, 0.6, True, 3, (0.0, -1.0, 0.0, 1.65)),      # the try budget runs out, nothing accepted
    ("cluster", 3, False, 1.0, 0.6, True, 4, (-0.01, 1.0, 0.02, -1.6)),    # cnt > extra_gt_num with rejected tries counted
    ("sparse", 15, False, 1.0, 0.6, True, 5, (0.0, -1.0, 0.0, 1.65)),      # GT_AUG_RAND_NUM False
    ("sparse", 15, True, 0.5, 0.6, True, 7, (0.0, -1.0, 0.0, 1.65)),      # apply draw fails: nothing accepted
    ("cluster", 12, True, 1.0, 0.0, True, 7, (0.0, -1.0, 0.0, 1.65)),      # no easy/hard split
    ("sparse", 15, True, 1.0, 0.6, False, 8, (0.03, -0.99, -0.02, 1.6)),   # PC_REDUCE_BY_RANGE False
    ("cluster", 15, True, 1.0, 0.6, True, 9, (0.0, -1.0, 0.0, 1.65)),
    ("empty", 15, True, 1.0, 0.6, True, 10, (0.0, -1.0, 0.0, 1.65)),      # the reference raises (max of an empty IoU array)
    ("cluster", 10, True, 1.0, 0.6, True, 11, (0.0, -1.0, 0.0, 1.65)),     # randint(10, 10) raises
]


class _Answers:
    """np.random.rand / randint of one apply_gt_aug_to_one_scene call, answered from the table; counts the tries started"""

    def __init__(self, seed, frame, rand_num, hard):
        self.seed, self.frame, self.first, self.hard, self.t = seed, frame, rand_num, hard, 0

    def rand(self, *shape):
        assert not shape and self.hard
        return tw.u01(tw.rand32(self.seed, tw.STREAM_HARD, self.frame, self.t))

    def randint(self, lo, hi=None):
        if hi <= lo:
            raise ValueError("low >= high")
        if self.first:
            self.first = False
            return lo + tw.below(tw.rand32(self.seed, tw.STREAM_EXTRA, self.frame, 0), hi - lo)
        r = tw.rand32(self.seed, tw.STREAM_INDEX, self.frame, self.t)
        self.t += 1
        return lo + tw.below(r, hi - lo)


def main():
    import pickle
    for p in (os.path.join(TESTS, "compat"), REFERENCE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    rc = sys.modules.setdefault("roipool3d_cuda", types.ModuleType("roipool3d_cuda"))

    def pts_in_boxes3d_cpu(flags, pts, boxes):           # roipool3d.cpp:97-125 through this library's host twin of it
        assert flags.dtype.is_floating_point is False and flags.is_contiguous()
        pts, boxes = pts.contiguous(), boxes.contiguous()
        _cabi.check(lib.prcnn_host_pts_in_boxes3d(pts.data_ptr(), boxes.data_ptr(), pts.shape[0], boxes.shape[0], flags.data_ptr()))
        return 1
    rc.pts_in_boxes3d_cpu = pts_in_boxes3d_cpu
    sys.modules.setdefault("iou3d_cuda", types.ModuleType("iou3d_cuda"))
    import yaml
    _load = yaml.load
    yaml.load = lambda f, Loader=yaml.SafeLoader: _load(f, Loader=Loader)      # lib/config.py predates PyYAML 6
    from lib.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(REFERENCE, "tools/cfgs/default.yaml"))
    yaml.load = _load
    import lib.utils.kitti_utils as kitti_utils
    from lib.utils.object3d import Object3d
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    kitti_utils.get_iou3d = tw.corner_iou3d

    rng = np.random.default_rng(2024)
    root = os.path.join(HERE, "_train_input_tmp")
    shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.join(root, "planes"))
    os.makedirs(os.path.join(root, "label_2"))
    db_lines, db_pts, db_int = make_database(rng)
    database = [{"sample_id": 0, "cls_type": "Car", "gt_box3d": kitti_utils.objs_to_boxes3d([Object3d(ln)])[0],
                 "points": p, "intensity": v, "obj": Object3d(ln)} for ln, p, v in zip(db_lines, db_pts, db_int)]
    with open(os.path.join(root, "gt_database.pkl"), "wb") as f:           # the on-disk form train_rcnn.py loads
        pickle.dump(database, f)
    with open(os.path.join(root, "gt_database.pkl"), "rb") as f:
        database = pickle.load(f)
    out = {"db_boxes": np.stack([d["gt_box3d"] for d in database]).astype(np.float32),
           "db_alpha": np.array([d["obj"].alpha for d in database], np.float32),
           "db_npts": np.array([len(d["points"]) for d in database], np.int32),
           "db_points": np.concatenate(db_pts), "db_intensity": np.concatenate(db_int), "scope": np.asarray(SCOPE),
           "ncases": len(CASES)}
    saved = (np.random.rand, np.random.randint)
    for k, (kind, extra, rand_num, prob, ratio, use_scope, seed, plane) in enumerate(CASES):
        with open(os.path.join(root, "planes", "%06d.txt" % k), "w") as f:
            f.write("# Plane\nWidth 4\nHeight 1\n%s\n" % " ".join("%.6e" % v for v in plane))
        with open(os.path.join(root, "label_2", "%06d.txt" % k), "w") as f:
            f.write("\n".join(label_lines(kind, rng)) + "\n")
        cfg.GT_EXTRA_NUM, cfg.GT_AUG_RAND_NUM, cfg.GT_AUG_APPLY_PROB, cfg.GT_AUG_HARD_RATIO = extra, rand_num, prob, ratio
        cfg.PC_REDUCE_BY_RANGE = use_scope
        ds = KittiRCNNDataset.__new__(KittiRCNNDataset)
        ds.plane_dir, ds.label_dir = os.path.join(root, "planes"), os.path.join(root, "label_2")
        db = copy.deepcopy(database)
        obj_id = {id(d["obj"]): i for i, d in enumerate(db)}
        if ratio > 0:
            ds.gt_database = [[d for d in db if d["points"].shape[0] > 100], [d for d in db if d["points"].shape[0] <= 100]]
        else:
            ds.gt_database = db
        all_gt = kitti_utils.objs_to_boxes3d(ds.filtrate_dc_objects(ds.get_label(k)))
        pts = np.stack([rng.uniform(-30, 30, 3000), rng.uniform(-1, 2.5, 3000), rng.uniform(0, 70, 3000)], 1).astype(np.float32)
        pin = rng.uniform(0, 1, 3000).astype(np.float32)
        applied = int(tw.u01(tw.rand32(seed, tw.STREAM_APPLY, 0, 0)) < prob)       # get_rpn_sample :279
        ans = _Answers(seed, 0, rand_num, ratio > 0)
        ids, boxes, alpha, pasted, status = [], np.zeros((0, 7), np.float32), [], np.zeros((0, 3), np.float32), 0
        if applied:
            np.random.rand, np.random.randint = ans.rand, ans.randint
            try:
                flag, rp, ri, eb, eo = ds.apply_gt_aug_to_one_scene(k, pts, pin, all_gt)
            except ValueError:
                flag, status = False, 1
            finally:
                np.random.rand, np.random.randint = saved
            if flag:
                ids = [obj_id[id(o)] for o in eo]
                boxes = np.asarray(eb, np.float32).reshape(-1, 7)
                alpha = [o.alpha for o in eo]
                pasted = rp[rp.shape[0] - int(sum(len(db[i]["points"]) for i in ids)):]
        out.update({"c%d_gt" % k: all_gt.astype(np.float32), "c%d_plane" % k: ds.get_road_plane(k),
                    "c%d_cfg" % k: np.array([extra, rand_num, prob, ratio, use_scope], np.float64), "c%d_seed" % k: seed,
                    "c%d_applied" % k: applied, "c%d_started" % k: ans.t if applied else 0, "c%d_status" % k: status,
                    "c%d_ids" % k: np.asarray(ids, np.int32), "c%d_boxes" % k: boxes, "c%d_alpha" % k: np.asarray(alpha, np.float32),
                    "c%d_pasted" % k: np.asarray(pasted, np.float32)})
        print("case %d (%s): applied %d, accepted %d, tries %d, status %d" % (k, kind, applied, len(ids), out["c%d_started" % k], status))
    shutil.rmtree(root, ignore_errors=True)
    np.savez_compressed(os.path.join(HERE, "train_input_ref.npz"), **out)


if __name__ == "__main__":
    main()
