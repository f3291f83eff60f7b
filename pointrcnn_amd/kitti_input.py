"""KITTI input side of the RPN, on the device.

Host-side mirror of what the reference's dataset class does for one inference sample
(lib/datasets/kitti_rcnn_dataset.py:246-310 get_rpn_sample, lib/datasets/kitti_dataset.py:34-48,
lib/utils/calibration.py:5-70): parse the calibration text, read the velodyne ``.bin``, and hand the raw scans of a whole
batch to ``prcnn_scene_prepare`` (csrc/scene.hip), which does lidar->rect, the image / PC_AREA_SCOPE crop and the
``npoints`` sampling for all frames in two launches.  Same names and argument meaning as the reference where a
counterpart exists; there is no CPU fallback -- the transform runs in the HIP library or not at all.
"""
import os

import numpy as np
import torch

from . import ops

PC_AREA_SCOPE = ((-40.0, 40.0), (-1.0, 3.0), (0.0, 70.4))        # tools/cfgs/default.yaml:18


# the calibration of KITTI training frame 000000 (public dataset values), as the text file the reference parses;
# used by the synthetic-scan generator below (bench.py --input raw, tests)
KITTI_CALIB_TXT = """P0: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 0.000000000000e+00 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00
P1: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 -3.875744000000e+02 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00
P2: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 4.485728000000e+01 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 2.163791000000e-01 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 2.745884000000e-03
P3: 7.215377000000e+02 0.000000000000e+00 6.095593000000e+02 -3.395242000000e+02 0.000000000000e+00 7.215377000000e+02 1.728540000000e+02 2.199936000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 2.729905000000e-03
R0_rect: 9.999239000000e-01 9.837760000000e-03 -7.445048000000e-03 -9.869795000000e-03 9.999421000000e-01 -4.278459000000e-03 7.402527000000e-03 4.351614000000e-03 9.999631000000e-01
Tr_velo_to_cam: 7.533745000000e-03 -9.999714000000e-01 -6.166020000000e-04 -4.069766000000e-03 1.480249000000e-02 7.280733000000e-04 -9.998902000000e-01 -7.631618000000e-02 9.998621000000e-01 7.523790000000e-03 1.480755000000e-02 -2.717806000000e-01
Tr_imu_to_velo: 9.999976000000e-01 7.553071000000e-04 -2.035826000000e-03 -8.086759000000e-01 -7.854027000000e-04 9.998898000000e-01 -1.482298000000e-02 3.195559000000e-01 2.024406000000e-03 1.482454000000e-02 9.998881000000e-01 -7.997231000000e-01
"""


def synthetic_scan(n, seed=0, fov_frac=0.5, far_frac=0.25):
    """(n,4) fp32 velodyne-frame scan [x fwd, y left, z up, intensity]: fov_frac of the points inside the camera frustum /
    PC_AREA_SCOPE region (far_frac of those beyond 40 m), the rest all around the sensor (behind, beside, above)."""
    r = np.random.default_rng(seed)
    nin = int(n * fov_frac)
    nfar = int(nin * far_frac)
    depth = np.concatenate([r.uniform(2.0, 40.0, nin - nfar), r.uniform(40.0, 72.0, nfar)])
    lat = r.uniform(-0.75, 0.75, nin) * depth               # roughly the +-40 deg horizontal field of view
    up = r.uniform(-2.2, 1.2, nin)
    inside = np.stack([depth, lat, up], 1)
    outside = np.stack([r.uniform(-80, 80, n - nin), r.uniform(-80, 80, n - nin), r.uniform(-3, 3, n - nin)], 1)
    pts = np.concatenate([inside, outside])
    out = np.concatenate([pts, r.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    return out[r.permutation(n)]


def get_calib_from_file(calib_file):
    """lib/utils/calibration.py:5-21: lines 2..5 of a KITTI calib txt = P2, P3, R0_rect, Tr_velo_to_cam (fp32)"""
    with open(calib_file) as f:
        return get_calib_from_lines(f.readlines())


def get_calib_from_lines(lines):

    def row(k, shape):
        return np.array(lines[k].strip().split(" ")[1:], dtype=np.float32).reshape(shape)
    return {"P2": row(2, (3, 4)), "P3": row(3, (3, 4)), "R0": row(4, (3, 3)), "Tr_velo2cam": row(5, (3, 4))}


class Calibration:
    """lib/utils/calibration.py:24-42 (the members the input path uses)"""

    def __init__(self, calib_file):
        calib = get_calib_from_file(calib_file) if isinstance(calib_file, str) else calib_file
        self.P2 = np.asarray(calib["P2"], np.float32).reshape(3, 4)
        self.R0 = np.asarray(calib["R0"], np.float32).reshape(3, 3)
        self.V2C = np.asarray(calib["Tr_velo2cam"], np.float32).reshape(3, 4)

    @classmethod
    def from_text(cls, text):
        """the same parse from the file's content"""
        return cls(get_calib_from_lines(text.split("\n")))

    def lidar_to_rect_matrix(self):
        """(4,3) fp32 M with pts_rect = [pts_lidar, 1] . M -- formed exactly as calibration.py:57 forms it"""
        return np.dot(self.V2C.T, self.R0.T)

    def packed(self):
        """(24,) fp32 row of prcnn_scene_prepare's calib argument"""
        return np.concatenate([self.lidar_to_rect_matrix().reshape(-1), self.P2.reshape(-1)]).astype(np.float32)


def get_lidar(lidar_file):
    """lib/datasets/kitti_dataset.py:40-43"""
    assert os.path.exists(lidar_file)
    return np.fromfile(lidar_file, dtype=np.float32).reshape(-1, 4)


def pack_scans(scans, calibs, img_shapes, pin=True):
    """The scan part of a packed batch, shared by ScenePreparer.pack and TrainScenePreparer.pack."""
    sizes = [int(s.shape[0]) for s in scans]
    off = np.zeros(len(scans) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    raw = torch.empty((int(off[-1]), 4), dtype=torch.float32, pin_memory=pin and torch.cuda.is_available())
    for s, a, b in zip(scans, off[:-1], off[1:]):
        raw[a:b] = torch.from_numpy(np.ascontiguousarray(s, np.float32))
    calib = torch.from_numpy(np.stack([c.packed() for c in calibs]))
    hw = torch.tensor([[int(s[0]), int(s[1])] for s in img_shapes], dtype=torch.int32)
    return {"raw": raw, "offsets": torch.from_numpy(off), "calib": calib, "img_hw": hw, "max_points": max(sizes) if sizes else 0}


class ScenePreparer:
    """Batch version of get_rpn_sample's inference branch.  ``npoints`` / ``random_select`` as in KittiRCNNDataset
    (kitti_rcnn_dataset.py:13); area_scope = cfg.PC_AREA_SCOPE or None for cfg.PC_REDUCE_BY_RANGE = False."""

    def __init__(self, npoints=16384, area_scope=PC_AREA_SCOPE, device="cuda"):
        self.npoints = npoints
        self.scope = None if area_scope is None else [float(v) for ax in area_scope for v in ax]
        self.device = torch.device(device)

    def pack(self, scans, calibs, img_shapes, pin=True):
        """host side of one batch: scans = list of (Ni,4) fp32 arrays, calibs = list of Calibration, img_shapes = list of
        (H, W[, 3]).  Returns pinned host tensors ready for one asynchronous copy each."""
        return pack_scans(scans, calibs, img_shapes, pin)

    def __call__(self, packed, seed=0):
        """device side: H2D of the packed batch on the current stream + prcnn_scene_prepare.
        -> dict(pts_input (B,npoints,3), pts_rect (same tensor), pts_features (B,npoints,1), src, nvalid, status)"""
        dev = self.device
        raw, off, calib, hw = (packed[k].to(dev, non_blocking=True) for k in ("raw", "offsets", "calib", "img_hw"))
        xyz, inten, src, nvalid, status = ops.scene_prepare(raw, off, packed["max_points"], calib, hw, self.scope, self.npoints, seed)
        return {"pts_input": xyz, "pts_rect": xyz, "pts_features": inten.unsqueeze(-1), "src": src, "nvalid": nvalid, "status": status}


def gt_aug_edit_scene(pts_rect, pts_intensity, accepted_boxes3d, new_pts_list, new_intensity_list, device="cuda"):
    """The point work of KittiRCNNDataset.apply_gt_aug_to_one_scene (lib/datasets/kitti_rcnn_dataset.py:484-507) for one
    scene, on the device: drop every scene point inside an accepted object's box (h + 2, :484-489), keep the rest in order and
    append the pasted objects' points (:501-507).  numpy in, numpy out (pts_rect (n', 3), pts_intensity (n',)) -- what the
    reference's function returns as its second and third value.  Batches of scenes: ops.gt_aug_edit."""
    pts = torch.as_tensor(np.ascontiguousarray(pts_rect, np.float32), device=device)[None]
    inten = torch.as_tensor(np.ascontiguousarray(pts_intensity, np.float32), device=device)[None]
    boxes = torch.as_tensor(np.ascontiguousarray(accepted_boxes3d, np.float32).reshape(-1, 7), device=device)[None]
    new_pts = np.concatenate(new_pts_list, axis=0).astype(np.float32) if len(new_pts_list) else np.zeros((0, 3), np.float32)
    new_int = np.concatenate(new_intensity_list, axis=0).astype(np.float32) if len(new_intensity_list) else np.zeros((0,), np.float32)
    out_pts, out_int, count = ops.gt_aug_edit(pts, inten, boxes, torch.as_tensor(new_pts, device=device)[None],
                                              torch.as_tensor(new_int, device=device)[None])
    n = int(count[0])
    return out_pts[0, :n].cpu().numpy(), out_int[0, :n].cpu().numpy()


# tools/generate_gt_database.py:22-29: the label classes each --class_name keeps
GT_DATABASE_CLASSES = {"Car": ("Car",), "People": ("Pedestrian", "Cyclist"), "Pedestrian": ("Pedestrian",), "Cyclist": ("Cyclist",)}


def read_label_lines(lines):
    """KITTI training labels (label_2 lines, field order of lib/utils/object3d.py:12-30) as plain arrays, one row per line:
    cls_type (K,) str, truncation / occlusion / alpha (K,) f64, box2d (K,4) f32, boxes3d (K,7) f32 [x, y, z, h, w, l, ry] as
    generate_gt_database.py:63-66 forms its rows (every field rounded from the parsed double), score (K,) f64 (-1 without a 16th
    field) and level (K,) i32: 1 Easy, 2 Moderate, 3 Hard, 4 UnKnown by the rule of object3d.py:31-45 (2-D height from the fp32
    box2d, truncation, occlusion)."""
    rows = [ln.strip().split(" ") for ln in lines if ln.strip()]
    K = len(rows)
    num = np.array([[float(v) for v in r[1:15]] for r in rows], np.float64).reshape(K, 14)
    box2d = num[:, 3:7].astype(np.float32)
    trunc, occ = num[:, 0], num[:, 1]
    height = box2d[:, 3].astype(np.float64) - box2d[:, 1].astype(np.float64) + 1
    level = np.full(K, 4, np.int32)
    level[(height >= 25) & (trunc <= 0.5) & (occ <= 2)] = 3
    level[(height >= 25) & (trunc <= 0.3) & (occ <= 1)] = 2
    level[(height >= 40) & (trunc <= 0.15) & (occ <= 0)] = 1
    return {"cls_type": np.array([r[0] for r in rows], dtype=np.str_).reshape(K), "truncation": trunc.copy(), "occlusion": occ.copy(),
            "alpha": num[:, 2].copy(), "box2d": box2d, "boxes3d": num[:, [10, 11, 12, 7, 8, 9, 13]].astype(np.float32),
            "score": np.array([float(r[15]) if len(r) == 16 else -1.0 for r in rows], np.float64), "level": level}


def lidar_to_rect_host(pts_lidar, M):
    """The canonical lidar -> rect of csrc/scene.hip's contract in numpy: fp32, every operation rounded on its own, left to
    right (elementwise numpy arithmetic does exactly that).  pts_lidar (n, >=3), M (4,3) fp32 -> (n,3) fp32"""
    p = np.ascontiguousarray(pts_lidar, np.float32)
    M = np.asarray(M, np.float32)
    return np.stack([((p[:, 0] * M[0, c] + p[:, 1] * M[1, c]) + p[:, 2] * M[2, c]) + M[3, c] for c in range(3)], 1)


def _gt_objects_host(scan, calib, boxes3d):
    """one frame of the database on the host: lidar_to_rect_host + the library's host twin of pts_in_boxes3d_cpu
    -> per box (rect points, intensity, raw index), in raw order"""
    from . import _cabi
    rect = np.ascontiguousarray(lidar_to_rect_host(scan, calib.lidar_to_rect_matrix()))
    boxes3d = np.ascontiguousarray(boxes3d, np.float32).reshape(-1, 7)
    flags = np.zeros((boxes3d.shape[0], rect.shape[0]), np.int64)
    _cabi.check(_cabi.lib().prcnn_host_pts_in_boxes3d(rect.ctypes.data, boxes3d.ctypes.data, rect.shape[0], boxes3d.shape[0],
                                                      flags.ctypes.data), "prcnn_host_pts_in_boxes3d")
    inten = np.ascontiguousarray(scan[:, 3], np.float32)
    return [(rect[m == 1], inten[m == 1], np.nonzero(m == 1)[0].astype(np.int32)) for m in flags]


class GTDatabase:
    """The GT database of the reference's GT augmentation (generate_gt_database.py:78-84, kitti_rcnn_dataset.py:62-76), packed once
    into device tensors: boxes (D,7), alpha (D,), npts (D,) i32, point offsets (D+1,) i64, points (P,3), intensity (P,); and the
    easy (> 100 points) / hard id lists of GT_AUG_HARD_RATIO > 0 (in database order, as the reference builds its two lists).
    from_kitti builds it from a KITTI tree (csrc/gt_database.hip), save / load keep it in one .npz of plain arrays."""

    def __init__(self, boxes, alpha, points, intensity, hard_ratio=0.6, device="cuda", sample_id=None, cls_type=None):
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 7)
        D = boxes.shape[0]
        if len(points) != D or len(intensity) != D or np.asarray(alpha).reshape(-1).shape[0] != D:
            raise ValueError("GTDatabase: boxes, alpha, points and intensity must describe the same %d objects" % D)
        npts = np.array([np.asarray(p).reshape(-1, 3).shape[0] for p in points], np.int32)
        off = np.zeros(D + 1, np.int64)
        np.cumsum(npts, out=off[1:])
        pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in points]) if D else np.zeros((0, 3), np.float32)
        inten = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in intensity]) if D else np.zeros((0,), np.float32)
        if inten.shape[0] != pts.shape[0]:
            raise ValueError("GTDatabase: every object needs one intensity per point")
        self.hard_ratio = float(hard_ratio)
        easy = np.nonzero(npts > 100)[0].astype(np.int32)
        hard = np.nonzero(npts <= 100)[0].astype(np.int32)
        # the reference raises (np.random.randint on an empty range) when it draws from an empty list
        if self.hard_ratio > 0:
            if len(hard) == 0:
                raise ValueError("GTDatabase: the hard list (<= 100 points) is empty but GT_AUG_HARD_RATIO > 0 draws from it")
            if len(easy) == 0 and self.hard_ratio < 1.0:
                raise ValueError("GTDatabase: the easy list (> 100 points) is empty but GT_AUG_HARD_RATIO < 1 draws from it")
        elif D == 0:
            raise ValueError("GTDatabase: empty database")
        dev = torch.device(device)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        self.size = D
        self.max_points = int(npts.max()) if D else 0
        self.boxes, self.alpha, self.npts = T(boxes), T(np.asarray(alpha, np.float32).reshape(-1)), T(npts)
        self.offsets, self.points, self.intensity = T(off), T(pts), T(inten)
        self.easy_idx, self.hard_idx = T(easy), T(hard)
        # where every object came from (host arrays; -1 / "" when the caller did not say): from_kitti, save / load, entries
        self.sample_id = np.full(D, -1, np.int64) if sample_id is None else np.asarray(sample_id, np.int64).reshape(-1)
        self.cls_type = np.full(D, "", np.str_) if cls_type is None else np.asarray(cls_type, np.str_).reshape(-1)
        self.src = None                     # (P,) i32 raw index of every point in its frame's scan: from_kitti only, not saved
        if self.sample_id.shape[0] != D or self.cls_type.shape[0] != D:
            raise ValueError("GTDatabase: one sample_id and one cls_type per object")

    @classmethod
    def from_arrays(cls, boxes, alpha, points, intensity, hard_ratio=0.6, device="cuda"):
        return cls(boxes, alpha, points, intensity, hard_ratio, device)

    @classmethod
    def from_pickle(cls, path, hard_ratio=0.6, device="cuda"):
        """the reference's *_gt_database_3level_*.pkl: a list of dicts with gt_box3d, points, intensity, obj (its Object3d class
        must be importable by the caller's environment for the unpickling)"""
        import pickle
        with open(path, "rb") as f:
            db = pickle.load(f)
        return cls([d["gt_box3d"] for d in db], [d["obj"].alpha for d in db], [d["points"] for d in db],
                   [d["intensity"] for d in db], hard_ratio, device)

    @classmethod
    def _from_packed(cls, boxes, alpha, npts, points, intensity, sample_id, cls_type, hard_ratio, device, src=None):
        cuts = np.cumsum(np.asarray(npts, np.int64))[:-1]
        D = len(npts)
        db = cls(boxes, alpha, np.split(np.asarray(points, np.float32).reshape(-1, 3), cuts) if D else [],
                 np.split(np.asarray(intensity, np.float32).reshape(-1), cuts) if D else [], hard_ratio, device, sample_id, cls_type)
        if src is not None:
            db.src = torch.from_numpy(np.ascontiguousarray(src, np.int32)).to(db.points.device)
        return db

    @classmethod
    def from_kitti(cls, root_dir, split="train", class_name="Car", hard_ratio=0.6, device="cuda", frames_per_batch=8, backend="device"):
        """tools/generate_gt_database.py on a KITTI tree (<root_dir>/KITTI/ImageSets/<split>.txt, <root_dir>/KITTI/object/training/
        {velodyne, calib, label_2}), with no pickle and no Object3d: per frame the labels whose class belongs to class_name ('Car',
        'People', 'Pedestrian', 'Cyclist'; :22-29) and whose level is Easy, Moderate or Hard (:39-48), and per such object the rect
        points of the whole scan inside its box, in raw order.  Frames with no such object contribute nothing.
        backend 'device': frames_per_batch frames per prcnn_gt_database_count / _fill call; 'host': the same result with no GPU
        (lidar_to_rect_host + the library's host twin of pts_in_boxes3d_cpu)."""
        if class_name not in GT_DATABASE_CLASSES:
            raise ValueError("GTDatabase.from_kitti: class_name %r is not one of %s" % (class_name, sorted(GT_DATABASE_CLASSES)))
        if backend not in ("device", "host"):
            raise ValueError("GTDatabase.from_kitti: backend %r is not 'device' or 'host'" % (backend,))
        split_file = os.path.join(root_dir, "KITTI", "ImageSets", split + ".txt")
        if not os.path.isfile(split_file):
            raise FileNotFoundError("GTDatabase.from_kitti: no split file %s" % split_file)
        base = os.path.join(root_dir, "KITTI", "object", "testing" if split == "test" else "training")
        with open(split_file) as f:
            frames = [x.strip() for x in f.readlines() if x.strip()]
        keep_cls = GT_DATABASE_CLASSES[class_name]
        boxes, alpha, npts, pts, inten, src, sid, ctype = [], [], [], [], [], [], [], []
        batch = []

        def flush():
            if not batch:
                return
            if backend == "host":
                for scan, calib, b3 in batch:
                    for p, v, i in _gt_objects_host(scan, calib, b3):
                        npts.append(len(p)); pts.append(p); inten.append(v); src.append(i)
            else:
                G = max(len(b3) for _, _, b3 in batch)
                packed = pack_scans([s for s, _, _ in batch], [c for _, c, _ in batch], [(0, 0)] * len(batch))
                pad = np.zeros((len(batch), G, 7), np.float32)
                for k, (_, _, b3) in enumerate(batch):
                    pad[k, :len(b3)] = b3
                dev = torch.device(device)
                n, _, p, v, i = ops.gt_database_build(packed["raw"].to(dev), packed["offsets"].to(dev), packed["max_points"], packed["calib"].to(dev),
                                                      torch.from_numpy(pad).to(dev), torch.tensor([len(b3) for _, _, b3 in batch], dtype=torch.int32, device=dev))
                n = n.cpu().numpy()
                for k, (_, _, b3) in enumerate(batch):                    # padded slots hold no point: the rows are in database order
                    npts.extend(int(c) for c in n[k, :len(b3)])
                pts.append(p.cpu().numpy()); inten.append(v.cpu().numpy()); src.append(i.cpu().numpy())
            batch.clear()
        for fid in frames:
            with open(os.path.join(base, "label_2", "%06d.txt" % int(fid))) as f:
                lab = read_label_lines(f.readlines())
            keep = np.isin(lab["cls_type"], keep_cls) & (lab["level"] <= 3)
            if not keep.any():
                continue
            boxes.append(lab["boxes3d"][keep]); alpha.append(lab["alpha"][keep]); ctype.extend(lab["cls_type"][keep])
            sid.extend([int(fid)] * int(keep.sum()))
            batch.append((get_lidar(os.path.join(base, "velodyne", "%06d.bin" % int(fid))),
                          Calibration(os.path.join(base, "calib", "%06d.txt" % int(fid))), lab["boxes3d"][keep]))
            if len(batch) >= max(1, int(frames_per_batch)):
                flush()
        flush()
        cat = lambda rows, shape, dt: np.concatenate(rows).astype(dt) if rows else np.zeros(shape, dt)      # noqa: E731
        return cls._from_packed(cat(boxes, (0, 7), np.float32), cat(alpha, (0,), np.float32), np.asarray(npts, np.int64),
                                cat(pts, (0, 3), np.float32), cat(inten, (0,), np.float32), sid, ctype, hard_ratio, device,
                                cat(src, (0,), np.int32))

    def save(self, path):
        """one .npz of plain arrays (no pickled object): boxes, alpha, npts, points, intensity, sample_id, cls_type"""
        with open(path, "wb") as f:
            np.savez(f, boxes=self.boxes.cpu().numpy(), alpha=self.alpha.cpu().numpy(), npts=self.npts.cpu().numpy(),
                     points=self.points.cpu().numpy(), intensity=self.intensity.cpu().numpy(), sample_id=self.sample_id,
                     cls_type=self.cls_type)

    @classmethod
    def load(cls, path, hard_ratio=0.6, device="cuda"):
        """a file written by save"""
        with np.load(path, allow_pickle=False) as z:
            return cls._from_packed(z["boxes"], z["alpha"], z["npts"], z["points"], z["intensity"], z["sample_id"], z["cls_type"],
                                    hard_ratio, device)

    def entries(self):
        """the database as generate_gt_database.py:78-84 lists it, without its 'obj': one dict per object with sample_id, cls_type,
        gt_box3d (7,), points (n,3), intensity (n,) -- host arrays, for comparison and export"""
        off = self.offsets.cpu().numpy()
        boxes, pts, inten = self.boxes.cpu().numpy(), self.points.cpu().numpy(), self.intensity.cpu().numpy()
        return [{"sample_id": int(self.sample_id[k]), "cls_type": str(self.cls_type[k]), "gt_box3d": boxes[k],
                 "points": pts[off[k]:off[k + 1]], "intensity": inten[off[k]:off[k + 1]]} for k in range(self.size)]

    def sample(self, gt_boxes3d, num_gt, planes, extra_num=15, rand_num=True, apply_prob=1.0, area_scope=PC_AREA_SCOPE,
               try_times=100, max_accept=16, seed=0):
        """prcnn_gt_aug_sample against this database: gt_boxes3d (B,G,7) + num_gt (B) i32 (non-DontCare labels), planes (B,4) f64,
        all on the device.  area_scope = cfg.PC_AREA_SCOPE or None (PC_REDUCE_BY_RANGE false).  -> ops.gt_aug_sample's dict."""
        scope = None if area_scope is None else [float(v) for ax in area_scope for v in ax]
        return ops.gt_aug_sample(gt_boxes3d, num_gt, planes, self.boxes, self.alpha, self.npts, self.easy_idx, self.hard_idx,
                                 extra_num, rand_num, apply_prob, self.hard_ratio, scope, try_times, max_accept, seed)


def filtrate_objects(labels, classes=("Car",), include_similar_type=True, area_scope=PC_AREA_SCOPE):
    """KittiRCNNDataset.filtrate_objects in TRAIN mode (lib/datasets/kitti_rcnn_dataset.py:152-173) on read_label_lines' arrays:
    keep the classes (with INCLUDE_SIMILAR_TYPE: Van with Car, Person_sitting with Pedestrian) whose float32 centre, widened to
    double, lies inside PC_AREA_SCOPE, bounds included (area_scope None: PC_REDUCE_BY_RANGE off) -> the kept rows' indices, in file order"""
    white = list(classes)
    if include_similar_type:
        white += (["Van"] if "Car" in classes else []) + (["Person_sitting"] if "Pedestrian" in classes else [])
    keep = np.isin(labels["cls_type"], white)
    if area_scope is not None:
        c = labels["boxes3d"][:, 0:3].astype(np.float64)      # check_pc_range compares float32 scalars with Python floats: in double
        for k, (lo, hi) in enumerate(area_scope):
            keep &= (lo <= c[:, k]) & (c[:, k] <= hi)
    return np.nonzero(keep)[0]


def load_rcnn_offline_frame(feature_dir, roi_dir, label_lines, sample_id, classes=("Car",), include_similar_type=True,
                            area_scope=PC_AREA_SCOPE):
    """The file side of KittiRCNNDataset.get_rcnn_training_sample_batch (kitti_rcnn_dataset.py:876-888) for one frame of
    `--train_mode rcnn_offline`: the five RPN dumps of kitti_output.save_rpn_features from feature_dir, the proposals
    roi_dir/%06d.txt parsed as the reference's label parser does (get_objects_from_label + objs_to_boxes3d: every field a float32 of
    the parsed double), and the frame's label lines through filtrate_objects.
    -> dict sample_id, rpn_xyz (N,3), rpn_features (N,C), rpn_intensity (N), seg_mask (N), roi_boxes3d (M,7), roi_scores (M) f32,
    gt_boxes3d (G,7) -- host arrays; ops.rcnn_offline_sample takes the boxes of a batch padded to (B,M,7) / (B,G,7) with their counts"""
    from . import kitti_output
    xyz, features, intensity, seg = kitti_output.get_rpn_features(feature_dir, sample_id)
    with open(os.path.join(roi_dir, "%06d.txt" % int(sample_id))) as fh:
        rois = read_label_lines(fh.readlines())
    labels = read_label_lines(label_lines)
    return {"sample_id": int(sample_id), "rpn_xyz": xyz, "rpn_features": features, "rpn_intensity": intensity, "seg_mask": seg,
            "roi_boxes3d": rois["boxes3d"], "roi_scores": rois["score"].astype(np.float32),
            "gt_boxes3d": labels["boxes3d"][filtrate_objects(labels, classes, include_similar_type, area_scope)]}


class RCNNOfflinePreparer:
    """KittiRCNNDataset.get_rcnn_training_sample_batch (kitti_rcnn_dataset.py:876-1022) for a batch of `--train_mode rcnn_offline`
    frames with RCNN.ROI_SAMPLE_JIT False: files in (load_rcnn_offline_frame), device batch out, nothing returns to the host
    between the sampler and the loss.  pack() pads and pins the frames; the call uploads them and runs ops.rcnn_offline_sample,
    prcnn_roipool3d on the sampled RoIs enlarged by POOL_EXTRA_WIDTH and ops.rcnn_offline_finish.  cfg: the RCNN section
    (pointrcnn_amd.rcnn.RCNNConfig) plus AUG_DATA / AUG_ROT_RANGE; AUG_METHOD_LIST / AUG_METHOD_PROB default to default.yaml's."""

    def __init__(self, cfg=None, device="cuda", aug_method_list=("rotation", "scaling", "flip"), aug_method_prob=(1.0, 1.0, 0.5)):
        if cfg is None:
            from .rcnn import RCNNConfig as cfg
        if cfg.REG_AUG_METHOD not in ("multiple", "single"):
            raise ValueError("RCNNOfflinePreparer: REG_AUG_METHOD %r is not supported ('multiple' or 'single')" % (cfg.REG_AUG_METHOD,))
        self.cfg, self.device = cfg, torch.device(device)
        self.aug_methods = tuple(getattr(cfg, "AUG_METHOD_LIST", aug_method_list)) if cfg.AUG_DATA else ()
        self.flip_prob = float(getattr(cfg, "AUG_METHOD_PROB", aug_method_prob)[2])

    def pack(self, frames, pin=True):
        """frames: load_rcnn_offline_frame's dicts, all with the same point count (the RPN's 16384) -> host batch: rpn_xyz (B,N,3),
        rpn_features (B,N,C), rpn_intensity, seg_mask, pts_depth (B,N; norm / 70 - 0.5 of the unaugmented point), roi_boxes3d (B,M,7) + num_roi, roi_scores (B,M), gt_boxes3d (B,G,7) +
        num_gt, frame_ids (B) = the sample ids, which key the random table"""
        if len({f["rpn_xyz"].shape[0] for f in frames}) != 1:
            raise ValueError("RCNNOfflinePreparer.pack: every frame must hold the same number of points")
        B = len(frames)
        M, G = max(max(len(f["roi_boxes3d"]) for f in frames), 1), max(max(len(f["gt_boxes3d"]) for f in frames), 1)
        roi, gt, sc = np.zeros((B, M, 7), np.float32), np.zeros((B, G, 7), np.float32), np.zeros((B, M), np.float32)
        for b, f in enumerate(frames):
            roi[b, :len(f["roi_boxes3d"])], gt[b, :len(f["gt_boxes3d"])] = f["roi_boxes3d"], f["gt_boxes3d"]
            sc[b, :len(f["roi_boxes3d"])] = f["roi_scores"]
        stack = lambda k: np.stack([np.ascontiguousarray(f[k], np.float32) for f in frames])      # noqa: E731
        out = {"rpn_xyz": stack("rpn_xyz"), "rpn_features": stack("rpn_features"), "rpn_intensity": stack("rpn_intensity"),
               "seg_mask": stack("seg_mask"), "roi_boxes3d": roi,
               # :966 / :838-839 in numpy's own float32 arithmetic, on the host where the reference forms it: the unaugmented point's depth
               "pts_depth": np.stack([(np.linalg.norm(f["rpn_xyz"].astype(np.float32), ord=2, axis=1) / 70.0 - 0.5).astype(np.float32)
                                      for f in frames]), "roi_scores": sc, "gt_boxes3d": gt,
               "num_roi": np.array([len(f["roi_boxes3d"]) for f in frames], np.int32),
               "num_gt": np.array([len(f["gt_boxes3d"]) for f in frames], np.int32),
               "frame_ids": np.array([f["sample_id"] for f in frames], np.int32)}
        out = {k: torch.from_numpy(v) for k, v in out.items()}
        return {k: v.pin_memory() for k, v in out.items()} if pin else out

    def _upload(self, packed):
        return {k: v.to(self.device, non_blocking=True) for k, v in packed.items()}

    def _point_features(self, d):
        cfg = self.cfg
        extras = ([d["rpn_intensity"].unsqueeze(2)] if cfg.USE_INTENSITY else []) + [d["seg_mask"].unsqueeze(2)]
        if cfg.USE_DEPTH:
            extras.append(d["pts_depth"].unsqueeze(2))
        return len(extras), torch.cat(extras + [d["rpn_features"]], dim=2)

    def __call__(self, packed, seed=0):
        """-> the reference's sample_info on the device, flattened over (B, R): pts_input (B*R,S,3+extras), pts_features (B*R,S,C),
        cls_label, reg_valid_mask (B*R) i32, gt_boxes3d_ct, roi_boxes3d, gt_boxes3d (B*R,7), roi_size (B*R,3), plus gt_iou (B*R) the
        noise loop's IoU, src (B*R) i32, status (B) i32 (ops.rcnn_offline_sample: 1 / 2 = a frame the reference raises on, cleared)"""
        from . import rcnn
        cfg, d = self.cfg, self._upload(packed)
        s = ops.rcnn_offline_sample(d["roi_boxes3d"], d["num_roi"], d["gt_boxes3d"], d["num_gt"], cfg.ROI_PER_IMAGE,
                                    (cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH, cfg.CLS_BG_THRESH, cfg.CLS_BG_THRESH_LO), cfg.FG_RATIO,
                                    cfg.HARD_BG_RATIO, aug_method=cfg.REG_AUG_METHOD, seed=seed, frame_ids=d["frame_ids"])
        E, feat = self._point_features(d)
        pooled, empty = rcnn.roipool3d_gpu(d["rpn_xyz"], feat, s["rois"], cfg.POOL_EXTRA_WIDTH, cfg.NUM_POINTS)
        f = ops.rcnn_offline_finish(pooled, s, empty, (cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH, cfg.CLS_BG_THRESH), self.aug_methods,
                                    self.flip_prob, cfg.AUG_ROT_RANGE, seed, d["frame_ids"])
        rows = pooled.view((-1,) + tuple(pooled.shape[2:]))
        return {"pts_input": rows[:, :, :3 + E], "pts_features": rows[:, :, 3 + E:], "cls_label": f["cls_label"].view(-1),
                "reg_valid_mask": f["reg_valid_mask"].view(-1), "gt_boxes3d_ct": f["gt_boxes3d_ct"].view(-1, 7),
                "roi_boxes3d": f["roi_boxes3d"].view(-1, 7), "roi_size": f["roi_boxes3d"].view(-1, 7)[:, 3:6],
                "gt_boxes3d": f["gt_boxes3d"].view(-1, 7), "gt_iou": s["roi_iou"].view(-1), "src": s["src"].view(-1),
                "status": s["status"], "pooled_empty_flag": empty.view(-1)}

    def eval_batch(self, packed):
        """The non-JIT branch of get_proposal_from_file (:832-852): every RoI of every frame pooled and moved into its canonical frame
        by ops.roipool3d_canonical.  -> pts_input (B*M,S,3+extras), pts_features (B*M,S,C), roi_boxes3d (B*M,7), roi_scores (B*M),
        roi_size (B*M,3), pooled_empty_flag (B*M), num_roi (B): rows past a frame's num_roi belong to zero boxes"""
        from . import rcnn
        cfg, d = self.cfg, self._upload(packed)
        extras = ([d["rpn_intensity"]] if cfg.USE_INTENSITY else []) + [d["seg_mask"]]
        if cfg.USE_DEPTH:
            extras.append(d["pts_depth"])
        if len(extras) > 2:
            raise NotImplementedError("RCNNOfflinePreparer.eval_batch: USE_INTENSITY with USE_DEPTH needs three scalar channels; "
                                      "ops.roipool3d_canonical takes two")
        rois = d["roi_boxes3d"].contiguous()
        B, M = rois.shape[:2]
        pool_boxes = rcnn.enlarge_box3d(rois.view(-1, 7), cfg.POOL_EXTRA_WIDTH).view(B, M, 7)
        pts, feat, empty = ops.roipool3d_canonical(d["rpn_xyz"].contiguous(), pool_boxes, rois, extras, d["rpn_features"].contiguous(),
                                                   cfg.NUM_POINTS)
        return {"pts_input": pts, "pts_features": feat.view(B * M, cfg.NUM_POINTS, -1), "roi_boxes3d": rois.view(-1, 7),
                "roi_scores": d["roi_scores"].view(-1), "roi_size": rois.view(-1, 7)[:, 3:6], "pooled_empty_flag": empty.view(-1),
                "num_roi": d["num_roi"]}


def road_plane_from_lines(lines):
    """kitti_dataset.get_road_plane (lib/datasets/kitti_dataset.py:55-68) on the plane file's lines: normal facing up, unit length"""
    plane = np.asarray([float(v) for v in lines[3].split()])
    if plane[1] > 0:
        plane = -plane
    return plane / np.linalg.norm(plane[0:3])


class TrainScenePreparer:
    """Batch version of get_rpn_sample's TRAIN path (lib/datasets/kitti_rcnn_dataset.py:246-362, RPN.FIXED false): raw scans, labels,
    road planes and the packed GT database in, the dictionary collate_batch would return out, on the device.  Settings carry their
    cfg names: GT_AUG_ENABLED (with gt_database), GT_EXTRA_NUM, GT_AUG_RAND_NUM, GT_AUG_APPLY_PROB (GT_AUG_HARD_RATIO belongs to the
    database), AUG_DATA, AUG_METHOD_LIST, AUG_METHOD_PROB, AUG_ROT_RANGE, RPN.USE_INTENSITY as use_intensity; area_scope =
    cfg.PC_AREA_SCOPE or None for cfg.PC_REDUCE_BY_RANGE false; max_accept bounds the accepted objects per frame (K <= 64)."""

    def __init__(self, npoints=16384, area_scope=PC_AREA_SCOPE, gt_database=None, GT_AUG_ENABLED=True, GT_EXTRA_NUM=15,
                 GT_AUG_RAND_NUM=True, GT_AUG_APPLY_PROB=1.0, AUG_DATA=True, AUG_METHOD_LIST=("rotation", "scaling", "flip"),
                 AUG_METHOD_PROB=(1.0, 1.0, 0.5), AUG_ROT_RANGE=18, use_intensity=False, max_accept=16, try_times=100, device="cuda"):
        self.npoints = npoints
        self.scope = None if area_scope is None else [float(v) for ax in area_scope for v in ax]
        self.db = gt_database if GT_AUG_ENABLED else None
        if GT_AUG_ENABLED and gt_database is None:
            raise ValueError("TrainScenePreparer: GT_AUG_ENABLED needs the GTDatabase")
        self.extra_num, self.rand_num, self.apply_prob = int(GT_EXTRA_NUM), bool(GT_AUG_RAND_NUM), float(GT_AUG_APPLY_PROB)
        self.methods = tuple(AUG_METHOD_LIST) if AUG_DATA else ()
        self.prob, self.rot_range = tuple(float(p) for p in AUG_METHOD_PROB), AUG_ROT_RANGE
        self.use_intensity, self.max_accept, self.try_times = bool(use_intensity), int(max_accept), int(try_times)
        self.device = torch.device(device)

    def pack(self, scans, calibs, img_shapes, gt_boxes3d, gt_alpha, all_gt_boxes3d, planes, pin=True):
        """ScenePreparer.pack plus, per frame: gt_boxes3d (ni,7) / gt_alpha (ni,) the training labels (filtrate_objects),
        all_gt_boxes3d (mi,7) the non-DontCare labels the pasted objects must not collide with (filtrate_dc_objects), planes (4,)
        the road plane (get_road_plane / road_plane_from_lines).  Ragged lists are zero-padded to the batch maximum; with pin every
        tensor is pinned, so each of __call__'s copies is asynchronous."""
        packed = pack_scans(scans, calibs, img_shapes, pin)
        B = len(scans)

        def pad(rows, width):
            rows = [np.asarray(r, np.float32).reshape((-1,) + width) for r in rows]
            out = np.zeros((B, max([len(r) for r in rows] + [0])) + width, np.float32)
            for k, r in enumerate(rows):
                out[k, :len(r)] = r
            return torch.from_numpy(out), torch.tensor([len(r) for r in rows], dtype=torch.int32)
        packed["gt_boxes3d"], packed["num_gt"] = pad(gt_boxes3d, (7,))
        packed["gt_alpha"], n_alpha = pad(gt_alpha, ())
        if not torch.equal(n_alpha, packed["num_gt"]):
            raise ValueError("TrainScenePreparer.pack: one alpha per training label")
        packed["all_gt_boxes3d"], packed["num_all_gt"] = pad(all_gt_boxes3d, (7,))
        packed["planes"] = torch.from_numpy(np.asarray(planes, np.float64).reshape(B, 4).copy())
        if pin and torch.cuda.is_available():
            packed = {k: v.pin_memory() if isinstance(v, torch.Tensor) and not v.is_pinned() else v for k, v in packed.items()}
        return packed

    def __call__(self, packed, seed=0):
        """device side: H2D of the packed batch, prcnn_gt_aug_sample, prcnn_train_scene_prepare and prcnn_rpn_labels on the current
        stream, no host synchronisation.  -> dict(pts_input, pts_rect, pts_features, rpn_cls_label, rpn_reg_label, gt_boxes3d, num_gt,
        src, nvalid, status, gt_aug_status, count, db_id, stats, aug)"""
        dev = self.device
        t = {k: v.to(dev, non_blocking=True) for k, v in packed.items() if isinstance(v, torch.Tensor)}
        B = t["calib"].shape[0]
        acc = None
        if self.db is not None:
            acc = self.db.sample(t["all_gt_boxes3d"], t["num_all_gt"], t["planes"], self.extra_num, self.rand_num, self.apply_prob,
                                 None if self.scope is None else [self.scope[0:2], self.scope[2:4], self.scope[4:6]],
                                 self.try_times, self.max_accept, seed)
        out = ops.train_scene_prepare(t["raw"], t["offsets"], packed["max_points"], t["calib"], t["img_hw"], self.scope, self.npoints, seed,
                                      t["gt_boxes3d"], t["gt_alpha"], t["num_gt"], acc, self.db, self.methods, self.prob, self.rot_range,
                                      self.use_intensity)
        out["rpn_cls_label"], out["rpn_reg_label"] = ops.rpn_labels(out["pts_rect"], out["gt_boxes3d"], out["num_gt"])
        if acc is not None:
            out.update(gt_aug_status=acc["status"], count=acc["count"], db_id=acc["db_id"], stats=acc["stats"])
        else:
            out.update(gt_aug_status=torch.zeros((B,), dtype=torch.int32, device=dev), count=torch.zeros((B,), dtype=torch.int32, device=dev),
                       db_id=torch.zeros((B, 0), dtype=torch.int32, device=dev), stats=torch.zeros((B, 4), dtype=torch.int32, device=dev))
        return out
