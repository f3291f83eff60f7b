"""Run the REFERENCE's own KittiRCNNDataset.get_rpn_sample with mode='TRAIN' (lib/datasets/kitti_rcnn_dataset.py:246-362) on a
throw-away KITTI tree (velodyne, calib, image, label and plane files, a 44-object GT database; npoints = 1024, scans of 3 000 - 9 000
raw points) with its random calls answered from the counter table of csrc/scene.hip.

Only used to GENERATE tests/golden/train_scene_ref.npz (python tests/golden/ref_train_scene.py) in the build container: it needs the
reference tree.  The .npz holds data only: per case the settings, the scan's generator parameters (tests/util.synthetic_scan), the
labels and plane as the reference parsed them, and the reference's outputs.  What is replaced:
  - kitti_utils.get_iou3d -> tests/train_input_twin.py corner_iou3d (shapely is not installed here), as in ref_train_input.py;
  - roipool3d_cuda.pts_in_boxes3d_cpu (a compiled extension) -> this library's host twin of the same C++ code;
  - the hull test is the reference's own (kitti_utils.in_hull, scipy Delaunay), as make_golden.py runs it for labels_ref.npz;
  - np.random.rand / randint / uniform (returning a Python float) / choice / shuffle while get_rpn_sample runs -> the table:
    streams 30-33 as ref_train_input.py, 34 aug_enable, 35 angle, 36 scale, 0 the draw, 1 / 2 the shuffle.  choice and shuffle see
    POSITIONS in the edited cloud; their identities (raw index, or n_raw + j for the j-th pasted point) come from the masks that
    the wrapped get_valid_flag and pts_in_boxes3d_cpu record.
The reference's lidar_to_rect is a BLAS sgemm whose rounding differs from the canonical projection of csrc/scene.hip in the last
ulp (tests/test_oracle_scene.py); `c<k>_rect_ulp` holds, for every raw point, the reference's rect coordinates as a signed distance
in fp32 steps from the canonical ones (oracle.scene_project) and `c<k>_flag` its valid flags, so that a test can feed the reference's
own cloud to everything downstream of the projection.
  - the label boxes of the accepted objects take the y that apply_gt_aug_to_one_scene placed them at (its returned
    extra_gt_boxes3d): obj.pos[1] drifts in place with every try on a database entry (:471), so an entry drawn more than once in a
    frame would otherwise carry another y.  `c<k>_redrawn` names those rows; for all others the two values are
    asserted to be identical.
Asserted per case (another seed is taken when one fails): no output point lies within 1e-4 m of a face of a label box or its
enlarged box (the hull test and the analytic test then agree); every collision test of the sampling loop is decided by more than
rounding (IoU exactly 0 with the new box grown by 0.2 mm, or IoU > 1e-6).  numpy's fp32 arctan2 is not glibc's
atan2f (csrc/ref_trig.h, the contract's): the generator prints on how many rotated box centres the two differ (about half of them, by
one ulp), so no seed makes them agree on a whole case; tests/test_train_scene_cpu.py compares ry through numpy's arctan2 bit for bit
and through the contract's to that ulp.  At least one case has no repeated
database draw.
"""
import logging
import os
import pickle
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
REFERENCE = os.environ.get("PRCNN_REFERENCE", "/root/reference")
for p in (HERE, TESTS, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import train_input_twin as tw          # noqa: E402
import ref_train_input as rti          # noqa: E402
from util import KITTI_CALIB_TXT, synthetic_scan          # noqa: E402

NPOINTS = 1024
SCOPE = rti.SCOPE
ALL = ("rotation", "scaling", "flip")
# label kind, scan (n, fov, far), hw, plane, GT aug (enabled, extra, rand_num, apply_prob, hard_ratio), use scope,
# AUG_DATA, AUG_METHOD_LIST, AUG_METHOD_PROB, seed
CASES = [
    dict(kind="sparse", scan=(8000, 0.5, 0.05), hw=(375, 1242), plane=(0.0, -1.0, 0.0, 1.65), gt_aug=(True, 15, True, 1.0, 0.6),
         scope=True, aug=(True, ALL, (1.0, 1.0, 1.0)), seed=1),                      # n > npoints, far pasted object, everything on
    dict(kind="cluster", scan=(3000, 0.06, 0.1), hw=(370, 1224), plane=(0.02, -1.0, 0.01, 1.7), gt_aug=(True, 3, False, 1.0, 0.6),
         scope=True, aug=(True, ("rotation", "flip"), (1.0, 1.0, 0.0)), seed=2, no_repeat=True, top_up=True),     # top-up branch; no scaling, flip off
    dict(kind="crowded", scan=(5000, 0.5, 0.1), hw=(374, 1238), plane=(0.0, -1.0, 0.0, 1.65), gt_aug=(True, 15, True, 1.0, 0.6),
         scope=True, aug=(True, ALL, (1.0, 1.0, 0.5)), seed=3),                      # nothing accepted, no training label
    dict(kind="sparse", scan=(6000, 0.5, 0.1), hw=(376, 1241), plane=(0.0, -1.0, 0.0, 1.65), gt_aug=(True, 15, True, 0.5, 0.6),
         scope=True, aug=(True, ALL, (0.0, 1.0, 0.5)), seed=7, applied=False),                      # apply draw fails; rotation off by probability
    dict(kind="nocar", scan=(9000, 0.4, 0.05), hw=(375, 1242), plane=(-0.01, 1.0, 0.02, -1.6), gt_aug=(True, 12, True, 1.0, 0.0),
         scope=True, aug=(True, ("scaling",), (1.0, 1.0, 1.0)), seed=5),             # no training label, collision list non-empty
    dict(kind="cluster", scan=(7000, 0.5, 0.1), hw=(375, 1242), plane=(0.0, -1.0, 0.0, 1.65), gt_aug=(True, 15, True, 1.0, 0.6),
         scope=True, aug=(False, ALL, (1.0, 1.0, 1.0)), seed=6),                     # AUG_DATA false
    dict(kind="sparse", scan=(8000, 0.5, 0.05), hw=(370, 1224), plane=(0.03, -0.99, -0.02, 1.6), gt_aug=(True, 15, True, 1.0, 0.6),
         scope=False, aug=(True, ("flip",), (1.0, 1.0, 1.0)), seed=8),               # PC_REDUCE_BY_RANGE false; flip only
    dict(kind="cluster", scan=(4000, 0.5, 0.1), hw=(376, 1241), plane=(0.0, -1.0, 0.0, 1.65), gt_aug=(False, 15, True, 1.0, 0.6),
         scope=True, aug=(True, ("rotation", "scaling"), (1.0, 1.0, 0.5)), seed=9),  # GT_AUG_ENABLED false
]


def make_database(rng):
    """ref_train_input.make_database's 44 objects with six of the in-scope ones moved beyond 40 m (their pasted points are far points)"""
    n = 44
    xs = np.concatenate([rng.uniform(-12, 12, 40), [45.0, -44.0, 5.0, 0.0]])
    zs = np.concatenate([rng.uniform(42, 62, 6), rng.uniform(8, 32, 34), [20.0, 15.0, 75.0, -2.0]])
    ys = rng.uniform(1.2, 2.0, n)
    dims = np.stack([rng.uniform(1.4, 1.7, n), rng.uniform(1.5, 1.8, n), rng.uniform(3.4, 4.4, n)], 1)
    ry = rng.uniform(-np.pi, np.pi, n)
    npts = rng.choice([2, 4, 30, 60, 90, 120, 180, 260], n)
    npts[:6] = [120, 30, 180, 60, 260, 90]
    lines, pts, inten = [], [], []
    for k in range(n):
        h = dims[k, 0]
        lines.append("Car 0.00 0 %.2f 100.00 150.00 300.00 250.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f"
                     % ((rng.uniform(-3, 3),) + tuple(dims[k]) + (xs[k], ys[k], zs[k], ry[k])))
        p = np.stack([xs[k] + rng.uniform(-1, 1, npts[k]), ys[k] - rng.uniform(0, h, npts[k]), zs[k] + rng.uniform(-1, 1, npts[k])], 1)
        pts.append(p.astype(np.float32))
        inten.append(rng.uniform(0, 1, npts[k]).astype(np.float32))
    return lines, pts, inten


def label_lines(kind, rng):
    dc = "DontCare -1 -1 -10 500.00 160.00 520.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10"
    if kind == "crowded":                 # large boxes tile every place a database object can go: every try collides
        return [dc] + ["Truck 0.00 0 0.10 100.00 150.00 300.00 250.00 4.20 4.50 4.50 %.2f 1.60 %.2f 0.00" % (x, z)
                       for x in np.arange(-14.0, 15.0, 4.0) for z in np.arange(6.0, 67.0, 4.0)]
    if kind != "nocar":
        return rti.label_lines(kind, rng)
    objs = [("Pedestrian", 3.0, 1.6, 12.0, 0.3), ("Cyclist", -6.0, 1.7, 25.0, 1.2), ("Truck", 10.0, 1.7, 48.0, 0.1)]
    return [dc] + ["%s 0.00 0 0.10 100.00 150.00 300.00 250.00 1.70 0.80 1.20 %.2f %.2f %.2f %.2f" % o for o in objs]


class Answers(rti._Answers):
    """every np.random call of one get_rpn_sample, answered from the table"""

    def __init__(self, seed, frame, rand_num, hard, gt_aug):
        super().__init__(seed, frame, rand_num, hard)
        self.first_rand = gt_aug                 # the first rand() is get_rpn_sample's apply draw (:279)
        self.n_raw = self.valid = None
        self.removed = None
        self.ident = None

    def rand(self, *shape):
        if shape == (3,):
            return np.array([tw.u01(tw.rand32(self.seed, 34, self.frame, i)) for i in range(3)])
        if self.first_rand:
            self.first_rand = False
            return tw.u01(tw.rand32(self.seed, tw.STREAM_APPLY, self.frame, 0))
        return super().rand()

    def uniform(self, lo, hi):
        stream = 36 if lo == 0.95 else 35
        return float(lo + (hi - lo) * tw.u01(tw.rand32(self.seed, stream, self.frame, 0)))

    def identities(self, n):
        """identity of every position of the edited cloud of n points"""
        if self.ident is None:
            raw = np.nonzero(self.valid)[0]
            if self.removed is not None:
                raw = raw[~self.removed]
            self.ident = np.concatenate([raw, self.n_raw + np.arange(n - len(raw))]).astype(np.int64)
        assert len(self.ident) == n
        return self.ident

    def choice(self, a, size, replace=True):
        assert replace is False
        a = np.asarray(a)
        if size < 0 or size > len(a):
            raise ValueError("cannot take a larger sample than population")
        ident = self.ident[a]
        key = [tw.rand32(self.seed, 0, self.frame, int(i)) >> 2 for i in ident]
        return a[np.lexsort((ident, key))[:size]]

    def shuffle(self, x):
        n = len(self.ident)
        ident = self.ident[x]
        stream = [1 if (n > NPOINTS or j < n) else 2 for j in range(len(x))]
        key = [tw.rand32(self.seed, s, self.frame, int(i)) for s, i in zip(stream, ident)]
        x[:] = x[np.lexsort((ident, key))]


def near_face(pts, boxes, tol=1e-4):
    """True when a point lies within tol of a face of a box or of its 0.2 m enlarged box (and not clearly outside it)"""
    for b in np.asarray(boxes, np.float64).reshape(-1, 7):
        for e in (0.0, 0.2):
            h, w, l = b[3] + 2 * e, b[4] + 2 * e, b[5] + 2 * e
            d = pts.astype(np.float64) - [b[0], b[1] + e - h / 2, b[2]]
            c, s = np.cos(b[6]), np.sin(b[6])
            lx, lz = d[:, 0] * c - d[:, 2] * s, d[:, 0] * s + d[:, 2] * c
            m = np.stack([np.abs(lx) - l / 2, np.abs(d[:, 1]) - h / 2, np.abs(lz) - w / 2], 1)
            if ((np.abs(m) < tol).any(1) & (m < tol).all(1)).any():
                return True
    return False


def main():
    for p in (os.path.join(TESTS, "compat"), REFERENCE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    rc = sys.modules.setdefault("roipool3d_cuda", types.ModuleType("roipool3d_cuda"))
    state = {}

    def pts_in_boxes3d_cpu(flags, pts, boxes):           # roipool3d.cpp:97-125 through this library's host twin of it
        pts, boxes = pts.contiguous(), boxes.contiguous()
        _cabi.check(lib.prcnn_host_pts_in_boxes3d(pts.data_ptr(), boxes.data_ptr(), pts.shape[0], boxes.shape[0], flags.data_ptr()))
        ans = state["ans"]
        m = flags.numpy().reshape(boxes.shape[0], -1)[0] == 1
        ans.removed = m.copy() if ans.removed is None else (ans.removed | m)
        return 1
    rc.pts_in_boxes3d_cpu = pts_in_boxes3d_cpu
    sys.modules.setdefault("iou3d_cuda", types.ModuleType("iou3d_cuda"))
    import yaml
    _load = yaml.load
    yaml.load = lambda f, Loader=yaml.SafeLoader: _load(f, Loader=Loader)      # lib/config.py predates PyYAML 6
    from lib.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(REFERENCE, "tools/cfgs/default.yaml"))
    yaml.load = _load
    from PIL import Image
    import lib.utils.kitti_utils as kitti_utils
    from lib.utils.object3d import Object3d
    import lib.datasets.kitti_rcnn_dataset as krd
    KittiRCNNDataset = krd.KittiRCNNDataset

    def get_iou3d(new_corners, cur_corners):              # the twin's IoU; every pair must be decided by more than rounding
        iou = tw.corner_iou3d(new_corners, cur_corners)
        c = np.asarray(new_corners, np.float32).copy()
        ctr = c.mean(1, keepdims=True)
        grown = ctr + (c - ctr) * np.float32(1.0 + 2e-4)   # half extents >= 1 m: every side moves out by >= 0.2 mm
        grown[:, :, 1] = c[:, :, 1]
        g = tw.corner_iou3d(grown.astype(np.float32), cur_corners)
        if (((iou == 0) & (g != 0)) | ((iou > 0) & (iou < 1e-6))).any():
            state["close"] = True
        return iou
    kitti_utils.get_iou3d = get_iou3d
    orig_valid = KittiRCNNDataset.get_valid_flag

    def get_valid_flag(pts_rect, pts_img, depth, img_shape):
        flag = orig_valid(pts_rect, pts_img, depth, img_shape)
        state["ans"].n_raw, state["ans"].valid = len(flag), flag.copy()
        state["rect"] = np.asarray(pts_rect, np.float32).copy()
        return flag
    KittiRCNNDataset.get_valid_flag = staticmethod(get_valid_flag)
    orig_apply = KittiRCNNDataset.apply_gt_aug_to_one_scene

    def apply_gt_aug(self, sample_id, pts_rect, pts_intensity, all_gt):
        state["applied"] = True
        out = orig_apply(self, sample_id, pts_rect, pts_intensity, all_gt)
        state["extra"] = (out[3], out[4]) if out[0] else None
        return out
    KittiRCNNDataset.apply_gt_aug_to_one_scene = apply_gt_aug
    orig_o2b = kitti_utils.objs_to_boxes3d

    def objs_to_boxes3d(objs):
        boxes = orig_o2b(objs)
        ex = state.get("extra")
        if ex is not None and len(objs) >= len(ex[1]) and all(a is b for a, b in zip(objs[len(objs) - len(ex[1]):], ex[1])):
            k0 = len(objs) - len(ex[1])
            state["redrawn"] = np.nonzero(boxes[k0:, 1] != ex[0][:, 1])[0] + k0
            other = np.ones(len(ex[1]), bool)
            other[state["redrawn"] - k0] = False
            assert np.array_equal(boxes[k0:][other], ex[0][other])
            boxes[k0:, 1] = ex[0][:, 1]
            state["extra_ids"] = [state["obj_id"][id(o)] for o in ex[1]]
        return boxes
    kitti_utils.objs_to_boxes3d = objs_to_boxes3d
    orig_sample = KittiRCNNDataset.get_rpn_sample

    import oracle
    from pointrcnn_amd import kitti_input
    calib24 = kitti_input.Calibration.from_text(KITTI_CALIB_TXT).packed()
    rng = np.random.default_rng(2025)
    root = os.path.join(HERE, "_train_scene_tmp")
    shutil.rmtree(root, ignore_errors=True)
    base = os.path.join(root, "KITTI", "object", "training")
    for d in ("velodyne", "calib", "image_2", "label_2", "planes"):
        os.makedirs(os.path.join(base, d))
    os.makedirs(os.path.join(root, "KITTI", "ImageSets"))
    with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % k for k in range(len(CASES))))
    db_lines, db_pts, db_int = make_database(rng)
    database = [{"sample_id": 0, "cls_type": "Car", "gt_box3d": orig_o2b([Object3d(ln)])[0], "points": p, "intensity": v,
                 "obj": Object3d(ln)} for ln, p, v in zip(db_lines, db_pts, db_int)]
    pkl = os.path.join(root, "gt_database.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(database, f)
    out = {"db_boxes": np.stack([d["gt_box3d"] for d in database]).astype(np.float32),
           "db_alpha": np.array([d["obj"].alpha for d in database], np.float32),
           "db_npts": np.array([len(d["points"]) for d in database], np.int32),
           "db_points": np.concatenate(db_pts), "db_intensity": np.concatenate(db_int), "scope": np.asarray(SCOPE),
           "ncases": len(CASES), "npoints": NPOINTS}
    label_text = [label_lines(c["kind"], rng) for c in CASES]
    for k, c in enumerate(CASES):
        with open(os.path.join(base, "calib", "%06d.txt" % k), "w") as f:
            f.write(KITTI_CALIB_TXT)
        Image.new("RGB", (c["hw"][1], c["hw"][0])).save(os.path.join(base, "image_2", "%06d.png" % k))
        with open(os.path.join(base, "planes", "%06d.txt" % k), "w") as f:
            f.write("# Plane\nWidth 4\nHeight 1\n%s\n" % " ".join("%.6e" % v for v in c["plane"]))
        with open(os.path.join(base, "label_2", "%06d.txt" % k), "w") as f:
            f.write("\n".join(label_text[k]) + "\n")
    saved = (np.random.rand, np.random.randint, np.random.uniform, np.random.choice, np.random.shuffle)
    any_unrepeated = False
    atan_total = [0, 0, 0]
    try:
        for k, c in enumerate(CASES):
            n, fov, far = c["scan"]
            enabled, extra, rand_num, prob, ratio = c["gt_aug"]
            cfg.GT_AUG_ENABLED, cfg.GT_EXTRA_NUM, cfg.GT_AUG_RAND_NUM, cfg.GT_AUG_APPLY_PROB, cfg.GT_AUG_HARD_RATIO = enabled, extra, rand_num, prob, ratio
            cfg.PC_REDUCE_BY_RANGE = c["scope"]
            cfg.AUG_DATA, cfg.AUG_METHOD_LIST, cfg.AUG_METHOD_PROB = c["aug"][0], list(c["aug"][1]), list(c["aug"][2])
            cfg.RPN.ENABLED, cfg.RPN.FIXED, cfg.RPN.USE_INTENSITY = True, False, False
            for attempt in range(20):
                seed, scan_seed = c["seed"] + 100 * attempt, 40 + k + 100 * attempt
                synthetic_scan(n, scan_seed, fov, far).tofile(os.path.join(base, "velodyne", "%06d.bin" % k))
                ds = KittiRCNNDataset(root_dir=root, npoints=NPOINTS, split="train", mode="TRAIN", random_select=True,
                                      logger=logging.getLogger("ref_train_scene"), gt_database_dir=pkl)
                ds.sample_id_list = list(range(len(CASES)))
                flat = ds.gt_database[0] + ds.gt_database[1] if ratio > 0 else ds.gt_database
                state.clear()
                state["obj_id"] = {id(d["obj"]): [np.array_equal(d["gt_box3d"], e["gt_box3d"]) for e in database].index(True) for d in flat}
                ans = state["ans"] = Answers(seed, k, rand_num, ratio > 0, enabled)
                ans.ratio = ratio
                np.random.rand, np.random.randint, np.random.uniform, np.random.choice, np.random.shuffle = \
                    ans.rand, ans.randint, ans.uniform, ans.choice, ans.shuffle
                raised = 0
                try:
                    sample = _run(ds, k, ans, state)
                except ValueError:
                    raised = 1
                finally:
                    np.random.rand, np.random.randint, np.random.uniform, np.random.choice, np.random.shuffle = saved
                assert not raised, "case %d raises" % k
                gt = sample["gt_boxes3d"].astype(np.float32)
                bad = state.get("close", False) or near_face(sample["pts_rect"], gt)
                scan = synthetic_scan(n, scan_seed, fov, far)
                can = oracle.scene_project(scan, calib24, c["hw"][0], c["hw"][1], SCOPE if c["scope"] else None)[0]
                delta = state["rect"].view(np.int32).astype(np.int64) - can.view(np.int32)
                bad = bad or np.abs(delta).max() > 30000
                at = state.get("atan2", (0, 0, 0))
                atan_total[0] += at[0]; atan_total[1] += at[1]; atan_total[2] = max(atan_total[2], at[2])
                bad = bad or state.get("applied", False) != c.get("applied", enabled)
                bad = bad or (c.get("no_repeat", False) and ans.t != len(set(state["tries"])))
                bad = bad or (c.get("top_up", False) and not state["n_edit"] < NPOINTS)
                if not bad:
                    break
                print("case %d: seed %d rejected (close pair %s, edited %d, tries %d, atan2 %s)" % (k, seed, state.get("close", False), state["n_edit"], ans.t, at))
            else:
                raise RuntimeError("case %d: no seed satisfies the fixture's conditions" % k)
            train_objs = ds.filtrate_objects(ds.get_label(k))
            all_objs = ds.filtrate_dc_objects(ds.get_label(k))
            am = sample.get("aug_method", [])
            angle = [m[1] for m in am if isinstance(m, list) and m[0] == "rotation"]
            scale = [m[1] for m in am if isinstance(m, list) and m[0] == "scaling"]
            ids = state.get("extra_ids", [])
            if enabled and len(ids) and ans.t == len(set(state["tries"])):
                any_unrepeated = True
            out.update({
                "c%d_scan" % k: np.array([n, scan_seed, fov, far], np.float64), "c%d_hw" % k: np.array(c["hw"], np.int32),
                "c%d_plane" % k: ds.get_road_plane(k), "c%d_seed" % k: seed, "c%d_frame" % k: k,
                "c%d_gt_aug" % k: np.array([enabled, extra, rand_num, prob, ratio, c["scope"]], np.float64),
                "c%d_aug" % k: np.array([c["aug"][0]] + [m in c["aug"][1] for m in ALL] + list(c["aug"][2]), np.float64),
                "c%d_train_gt" % k: orig_o2b(train_objs).astype(np.float32).reshape(-1, 7),
                "c%d_train_alpha" % k: np.array([o.alpha for o in train_objs], np.float32),
                "c%d_all_gt" % k: orig_o2b(all_objs).astype(np.float32).reshape(-1, 7),
                "c%d_ids" % k: np.asarray(ids, np.int32), "c%d_redrawn" % k: np.asarray(state.get("redrawn", []), np.int32),
                "c%d_pts_rect" % k: sample["pts_rect"].astype(np.float32), "c%d_pts_features" % k: sample["pts_features"].astype(np.float32),
                "c%d_gt_boxes3d" % k: gt.reshape(-1, 7), "c%d_cls" % k: sample["rpn_cls_label"].astype(np.int8),
                "c%d_reg" % k: sample["rpn_reg_label"].astype(np.float32),
                "c%d_method" % k: np.array([angle[0] if angle else np.nan, scale[0] if scale else np.nan, float("flip" in am)], np.float64),
                "c%d_rect_ulp" % k: delta.astype(np.int16), "c%d_flag" % k: np.packbits(ans.valid),
                "c%d_nedit" % k: state["n_edit"], "c%d_nfar" % k: state["n_far"], "c%d_nfar_pasted" % k: state["n_far_pasted"]})
            print("case %d (%s): raw %d, valid %d, edited %d (far %d, pasted far %d), accepted %d (redrawn rows %s), tries %d, aug %s, fg %d"
                  % (k, c["kind"], n, ans.valid.sum(), state["n_edit"], state["n_far"], state["n_far_pasted"], len(ids),
                     list(state.get("redrawn", [])), ans.t, am, (sample["rpn_cls_label"] > 0).sum()))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print("numpy fp32 arctan2 != ref_trig atan2f on %d of %d box centres met (all attempts), at most %d ulp" % tuple(atan_total))
    assert any_unrepeated, "every case repeats a database draw"
    np.savez_compressed(os.path.join(HERE, "train_scene_ref.npz"), **out)
    print("wrote train_scene_ref.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "train_scene_ref.npz")))


def _run(ds, k, ans, state):
    """get_rpn_sample with the edited cloud's size and far counts recorded on the way (np.where is how the reference splits near / far)"""
    import oracle
    tries = state["tries"] = []
    orig_randint = ans.randint
    first = [ans.first]

    def randint(lo, hi=None):
        v = orig_randint(lo, hi)
        if first[0]:
            first[0] = False
        else:
            tries.append((ans.hard_list, v))
        return v
    orig_rand = ans.rand

    def rand(*shape):
        v = orig_rand(*shape)
        if not shape:
            ans.hard_list = bool(v > ans.ratio) if ans.hard else None
        return v
    ans.hard_list = None
    np.random.randint, np.random.rand = randint, rand
    real_where = np.where
    seen = {}

    def where(cond, *a):
        r = real_where(cond, *a)
        if not a and "n" not in seen and getattr(cond, "dtype", None) == bool and cond.ndim == 1:
            seen["n"] = len(cond)          # :289 far_idxs_choice = np.where(pts_near_flag == 0)
            seen["far"] = r[0].copy()
        return r
    orig_choice, orig_shuffle = np.random.choice, np.random.shuffle

    def shuffle(x):
        if ans.ident is None:
            ans.identities(len(x) if len(x) <= NPOINTS and "n" not in seen else seen["n"])
        ans.shuffle(x)
    np.random.shuffle = shuffle
    np.where = where
    real_atan2 = np.arctan2

    def arctan2(y, x):                      # numpy's fp32 arctan2 against csrc/ref_trig.h's atan2f, the contract's
        r = real_atan2(y, x)
        if getattr(r, "dtype", None) == np.float32 and r.ndim == 1 and len(r):
            want = oracle.cpu().ref_trig("atan2f", np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32))
            state["atan2"] = (int((want.view(np.int32) != r.view(np.int32)).sum()), len(r),
                              int(np.abs(want.view(np.int32).astype(np.int64) - r.view(np.int32)).max()))
        return r
    np.arctan2 = arctan2
    try:
        # n > npoints: np.where runs first and tells the size; otherwise choice's population / shuffle's array is arange(n)
        def choice2(a, size, replace=True):
            a = np.asarray(a)
            if ans.ident is None:
                ans.identities(seen["n"] if "n" in seen else len(a))
            return ans.choice(a, size, replace)
        np.random.choice = choice2
        sample = ds.get_rpn_sample(k)
    finally:
        np.where = real_where
        np.arctan2 = real_atan2
        np.random.choice, np.random.shuffle = orig_choice, orig_shuffle
    n_edit = len(ans.ident)
    state["n_edit"] = n_edit
    far = seen.get("far", np.zeros(0, np.int64))
    state["n_far"] = len(far)
    state["n_far_pasted"] = int((ans.ident[far] >= ans.n_raw).sum()) if len(far) else 0
    return sample


if __name__ == "__main__":
    main()
