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
        self.rect_input = False             # load_aug_frame sets it for a train_aug frame: its points are already rect coordinates

    @classmethod
    def from_text(cls, text):
        """the same parse from the file's content"""
        return cls(get_calib_from_lines(text.split("\n")))

    def lidar_to_rect_matrix(self):
        """(4,3) fp32 M with pts_rect = [pts_lidar, 1] . M -- formed exactly as calibration.py:57 forms it"""
        return np.dot(self.V2C.T, self.R0.T)

    def packed(self, rect_input=None):
        """(24,) fp32 row of prcnn_scene_prepare's calib argument.  rect_input (default: self.rect_input): the points are rect
        coordinates already (a train_aug frame's rectified_data): the lidar -> rect part is the identity, and the canonical
        ((x * 1 + y * 0) + z * 0) + 0 reproduces every coordinate (only the sign of a zero may change)"""
        if self.rect_input if rect_input is None else rect_input:
            M = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((1, 3), np.float32)])
        else:
            M = self.lidar_to_rect_matrix()
        return np.concatenate([M.reshape(-1), self.P2.reshape(-1)]).astype(np.float32)


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
    (kitti_rcnn_dataset.py:13); area_scope = cfg.PC_AREA_SCOPE or None for cfg.PC_REDUCE_BY_RANGE = False.  npoints up to 65536:
    above 16384 ops.scene_prepare takes the large export (the shuffle sorted through HBM) on its own."""

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
    cfg.PC_AREA_SCOPE or None for cfg.PC_REDUCE_BY_RANGE false; max_accept bounds the accepted objects per frame (K <= 64).
    large_clouds: False (the default) calls prcnn_train_scene_prepare, which refuses npoints > 16384; True calls
    prcnn_train_scene_prepare_large, which takes 1..65536 and writes the same bytes up to 16384.  ScenePreparer switches on npoints by
    itself; this class does not, because its refusal of 16385 points is asserted behaviour (tests/test_gpu_train_scene.py) that a
    default must not change: a dense training batch is asked for by name."""

    def __init__(self, npoints=16384, area_scope=PC_AREA_SCOPE, gt_database=None, GT_AUG_ENABLED=True, GT_EXTRA_NUM=15,
                 GT_AUG_RAND_NUM=True, GT_AUG_APPLY_PROB=1.0, AUG_DATA=True, AUG_METHOD_LIST=("rotation", "scaling", "flip"),
                 AUG_METHOD_PROB=(1.0, 1.0, 0.5), AUG_ROT_RANGE=18, use_intensity=False, max_accept=16, try_times=100, device="cuda",
                 large_clouds=False):
        self.npoints = npoints
        self.large_clouds = bool(large_clouds)
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
                                      self.use_intensity, large=self.large_clouds)
        out["rpn_cls_label"], out["rpn_reg_label"] = ops.rpn_labels(out["pts_rect"], out["gt_boxes3d"], out["num_gt"])
        if acc is not None:
            out.update(gt_aug_status=acc["status"], count=acc["count"], db_id=acc["db_id"], stats=acc["stats"])
        else:
            out.update(gt_aug_status=torch.zeros((B,), dtype=torch.int32, device=dev), count=torch.zeros((B,), dtype=torch.int32, device=dev),
                       db_id=torch.zeros((B, 0), dtype=torch.int32, device=dev), stats=torch.zeros((B, 4), dtype=torch.int32, device=dev))
        return out


# ---------------------------------------------------------------------------------------------------------
# The offline GT-augmented scenes, the `train_aug` split (tools/generate_aug_scene.py; csrc/aug_scene.hip)
# ---------------------------------------------------------------------------------------------------------
AUG_SCENE_TRIES = 50


def aug_scene_scope(class_name):
    """PC_AREA_SCOPE of tools/generate_aug_scene.py:26-29 as 6 floats [x0 x1 y0 y1 z0 z1]"""
    return [-40.0, 40.0, -1.0, 3.0, 0.0, 70.4] if class_name == "Car" else [-30.0, 30.0, -1.0, 3.0, 0.0, 50.0]


def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    return x ^ (x >> 16)


def counter_rand(seed, stream, frame, i):
    """csrc/counter_rand.h's r(stream, frame, i) on the host"""
    return _mix32(i ^ _mix32(frame * 0x9E3779B9 + _mix32(seed + stream * 0x85EBCA6B)))


def get_image_shape(img_file):
    """kitti_dataset.get_image_shape (lib/datasets/kitti_dataset.py:33-38): (height, width, 3), from the PNG header alone"""
    with open(img_file, "rb") as f:
        head = f.read(24)
    if head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError("get_image_shape: %s is not a PNG file" % img_file)
    return int.from_bytes(head[20:24], "big"), int.from_bytes(head[16:20], "big"), 3


def valid_flag_host(pts_rect, P2, img_shape, scope):
    """rect_to_img + get_valid_flag under the canonical contract of csrc/scene.hip (scene_project) in numpy: fp32, every operation
    rounded on its own, left to right; the PC_AREA_SCOPE comparisons in double.  pts_rect (n,3) f32, scope 6 floats or None -> (n,) bool"""
    r = np.ascontiguousarray(pts_rect, np.float32)
    P = np.asarray(P2, np.float32).reshape(3, 4)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    h = [((x * P[k, 0] + y * P[k, 1]) + z * P[k, 2]) + P[k, 3] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = h[0] / z, h[1] / z
    depth = h[2] - P[2, 3]
    ok = (u >= 0) & (u < np.float32(img_shape[1])) & (v >= 0) & (v < np.float32(img_shape[0])) & (depth >= 0)
    if scope is not None:
        d = r.astype(np.float64)
        for k in range(3):
            ok &= (d[:, k] >= scope[2 * k]) & (d[:, k] <= scope[2 * k + 1])
    return ok


def aug_scene_sample_host(all_gt_boxes3d, plane, db_boxes, db_npts, scope, seed, frame, iou3d):
    """One frame of prcnn_aug_scene_sample on the host (csrc/aug_scene_math.h restated): AugSceneGenerator.aug_one_scene's sampling
    loop, tools/generate_aug_scene.py:157-219.  iou3d(a (1,7), b (M,7)) -> (1,M) float32 stands for boxes_iou3d_gpu: this package has
    no host build of it, the caller brings one.  -> dict ids, boxes (n,7), y_shift (n,) f64, stats (extra_gt_num, cnt, spent), status"""
    cur = np.array(all_gt_boxes3d, np.float32).reshape(-1, 7)
    cur[:, 4] += np.float32(0.5)
    cur[:, 5] += np.float32(0.5)
    db_boxes = np.asarray(db_boxes, np.float32).reshape(-1, 7)
    a, b, c, d = (np.float64(v) for v in plane)
    D = db_boxes.shape[0]
    extra = 10 + ((counter_rand(seed, 60, frame, 0) * 5) >> 32)
    ids, boxes, shifts, status, cnt, spent = [], [], [], 0, 0, 0
    for t in range(AUG_SCENE_TRIES):
        spent = t + 1
        if D <= 1:
            status = 1
            break
        i = (counter_rand(seed, 61, frame, t) * (D - 1)) >> 32
        box = db_boxes[i].copy()
        x, y, z = (np.float64(v) for v in box[:3])
        if not (scope[0] <= x <= scope[1] and scope[2] <= y <= scope[3] and scope[4] <= z <= scope[5]):
            continue
        if cnt > extra:
            break
        if db_npts[i] < 5:
            continue
        with np.errstate(all="ignore"):
            move = y - ((-d - a * x) - c * z) / b
            box[1] = np.float32(y - move)
        cnt += 1
        if cur.shape[0] == 0:
            status = 1
            break
        v = np.asarray(iou3d(box.reshape(1, 7), cur), np.float32).reshape(-1)
        if not bool((v < np.float32(1e-8)).all()):
            continue
        enl = box.copy()
        enl[4] += np.float32(0.5)
        enl[5] += np.float32(0.5)
        cur = np.concatenate([cur, enl[None]])
        ids.append(int(i)); boxes.append(box); shifts.append(float(move))
    return {"ids": np.asarray(ids, np.int32), "boxes": np.asarray(boxes, np.float32).reshape(-1, 7),
            "y_shift": np.asarray(shifts, np.float64), "stats": (int(extra), cnt, spent), "status": status}


def aug_scene_build_host(scan, calib, img_shape, scope, boxes, ids, y_shift, db_points, db_intensity, db_offsets):
    """One frame of prcnn_aug_scene_count / _fill on the host: lidar_to_rect_host, valid_flag_host, the library's host twin of
    pts_in_boxes3d_cpu on the accepted boxes with h + 2, then the pasted objects with y - y_shift -> (n,4) f32, src (n,) i32"""
    from . import _cabi
    rect = np.ascontiguousarray(lidar_to_rect_host(scan, calib.packed()[:12].reshape(4, 3)))
    keep = valid_flag_host(rect, calib.P2, img_shape, scope)
    boxes = np.array(boxes, np.float32).reshape(-1, 7)
    if boxes.shape[0]:
        boxes[:, 3] += np.float32(2)
        flags = np.zeros((boxes.shape[0], rect.shape[0]), np.int64)
        _cabi.check(_cabi.lib().prcnn_host_pts_in_boxes3d(rect.ctypes.data, boxes.ctypes.data, rect.shape[0], boxes.shape[0],
                                                          flags.ctypes.data), "prcnn_host_pts_in_boxes3d")
        keep &= ~(flags == 1).any(axis=0)
    rows = [np.concatenate([rect[keep], np.ascontiguousarray(scan[:, 3:4], np.float32)[keep]], 1)]
    src = [np.nonzero(keep)[0].astype(np.int32)]
    for i, move in zip(ids, y_shift):
        o, e = int(db_offsets[i]), int(db_offsets[i + 1])
        p = np.array(db_points[o:e], np.float32)
        p[:, 1] = (p[:, 1].astype(np.float64) - np.float64(move)).astype(np.float32)
        rows.append(np.concatenate([p, np.asarray(db_intensity[o:e], np.float32).reshape(-1, 1)], 1))
        src.append((-1 - np.arange(o, e)).astype(np.int32))
    return np.concatenate(rows).astype(np.float32), np.concatenate(src)


def reprint_label_line(line):
    """Object3d(line).to_kitti_format() (lib/utils/object3d.py:12-30, :97-102): every field parsed as a double, the 2-D box and the
    position rounded to float32 before they are printed"""
    f = line.strip().split(" ")
    v = [float(t) for t in f[1:15]]
    box2d, pos = np.array(v[3:7], np.float32), np.array(v[10:13], np.float32)
    return "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
        f[0], v[0], int(v[1]), v[2], box2d[0], box2d[1], box2d[2], box2d[3], v[7], v[8], v[9], pos[0], pos[1], pos[2], v[13])


def aug_object_lines(boxes3d, truncation, occlusion, P2, img_shape, class_name):
    """save_kitti_format of tools/generate_aug_scene.py:38-63 for the accepted objects of one frame: the image box from the box
    corners, clipped; boxes wider / taller than 0.8 of the image dropped; class, truncation %.2f, int(occlusion), then the 12 %.4f fields alpha, image box, h w l, x y z, ry"""
    from . import kitti_output
    b = np.asarray(boxes3d, np.float32).reshape(-1, 7)
    if b.shape[0] == 0:
        return []
    H, W = int(img_shape[0]), int(img_shape[1])
    ib = kitti_output.corners_to_image_boxes(kitti_output.box_corners(b), P2)
    ib[:, 0::2] = np.clip(ib[:, 0::2], 0, W - 1)
    ib[:, 1::2] = np.clip(ib[:, 1::2], 0, H - 1)
    keep = ((ib[:, 2] - ib[:, 0]) < W * 0.8) & ((ib[:, 3] - ib[:, 1]) < H * 0.8)
    alpha = kitti_output.observation_angle(b)
    cols = np.column_stack([alpha.astype(np.float64), ib, b[:, 3:6].astype(np.float64), b[:, 0:3].astype(np.float64), b[:, 6].astype(np.float64)])
    return ["%s %.2f %d" % (class_name, float(truncation[k]), int(occlusion[k])) + (" %.4f" * 12) % tuple(cols[k].tolist())
            for k in range(b.shape[0]) if keep[k]]


class AugSceneGenerator:
    """tools/generate_aug_scene.py on a KITTI tree: for every epoch and frame of <split>, objects of the GT database pasted onto the road
    plane where they collide with no label and no earlier paste, written as the `train_aug` split that step 2 (eval_rcnn.py
    --save_rpn_feature) and step 3 (train_rcnn.py --train_mode rcnn_offline) of the reference's offline recipe read.
    backend 'device': frames_per_batch frames per prcnn_aug_scene_sample / _count / _fill call; 'host': the same files with no GPU
    (aug_scene_sample_host, aug_scene_build_host), which needs iou3d=, a host boxes_iou3d_gpu ((1,7), (M,7)) -> (1,M).
    The truncation / occlusion an accepted object's label line carries are looked up in label_2/<gt_database.sample_id>.txt by exact
    float32 box match, or given as truncation= / occlusion= arrays (D,)."""

    def __init__(self, root_dir, gt_database, class_name="Car", split="train", include_similar=False, device="cuda", backend="device",
                 truncation=None, occlusion=None, iou3d=None):
        if class_name not in GT_DATABASE_CLASSES:
            raise ValueError("AugSceneGenerator: class_name %r is not one of %s" % (class_name, sorted(GT_DATABASE_CLASSES)))
        if backend not in ("device", "host"):
            raise ValueError("AugSceneGenerator: backend %r is not 'device' or 'host'" % (backend,))
        if backend == "host" and iou3d is None:
            raise ValueError("AugSceneGenerator: backend 'host' needs iou3d=, a host boxes_iou3d_gpu")
        split_file = os.path.join(root_dir, "KITTI", "ImageSets", split + ".txt")
        if not os.path.isfile(split_file):
            raise FileNotFoundError("AugSceneGenerator: no split file %s" % split_file)
        with open(split_file) as f:
            self.frames = [x.strip() for x in f.readlines() if x.strip()]
        self.base = os.path.join(root_dir, "KITTI", "object", "testing" if split == "test" else "training")
        self.db, self.class_name, self.split, self.backend, self.iou3d = gt_database, class_name, split, backend, iou3d
        self.device = torch.device(device)
        self.scope = aug_scene_scope(class_name)
        white = list(GT_DATABASE_CLASSES[class_name])                       # generate_aug_scene.py:70-77, :98-111
        if include_similar:
            white += (["Van"] if "Car" in white else []) + (["Person_sitting"] if ("Pedestrian" in white or "Cyclist" in white) else [])
        self.whitelist = white
        if (truncation is None) != (occlusion is None):
            raise ValueError("AugSceneGenerator: truncation and occlusion go together")
        if truncation is not None:
            self.truncation, self.occlusion = np.asarray(truncation, np.float64).reshape(-1), np.asarray(occlusion, np.float64).reshape(-1)
            if self.truncation.shape[0] != gt_database.size or self.occlusion.shape[0] != gt_database.size:
                raise ValueError("AugSceneGenerator: one truncation and one occlusion per database object (%d)" % gt_database.size)
        else:
            self.truncation, self.occlusion = self._lookup_trunc_occl()

    def _lookup_trunc_occl(self):
        db, boxes = self.db, self.db.boxes.cpu().numpy()
        trunc, occl, cache = np.zeros(db.size), np.zeros(db.size), {}
        for k in range(db.size):
            sid = int(db.sample_id[k])
            if sid < 0:
                raise ValueError("AugSceneGenerator: database object %d does not say which frame it came from (sample_id -1): "
                                 "pass truncation= and occlusion=" % k)
            if sid not in cache:
                with open(os.path.join(self.base, "label_2", "%06d.txt" % sid)) as f:
                    cache[sid] = read_label_lines(f.readlines())
            lab = cache[sid]
            hit = np.nonzero((lab["boxes3d"] == boxes[k]).all(axis=1))[0]
            if len(hit) == 0:
                raise ValueError("AugSceneGenerator: no label of frame %06d has the box of database object %d" % (sid, k))
            trunc[k], occl[k] = lab["truncation"][hit[0]], lab["occlusion"][hit[0]]
        return trunc, occl

    def _read_frame(self, fid):
        with open(os.path.join(self.base, "label_2", "%06d.txt" % fid)) as f:
            lines = [ln for ln in f.readlines() if ln.strip()]
        lab = read_label_lines(lines)
        with open(os.path.join(self.base, "planes", "%06d.txt" % fid)) as f:
            plane = road_plane_from_lines(f.readlines())
        return {"id": fid, "scan": get_lidar(os.path.join(self.base, "velodyne", "%06d.bin" % fid)),
                "calib": Calibration(os.path.join(self.base, "calib", "%06d.txt" % fid)),
                "img_shape": get_image_shape(os.path.join(self.base, "image_2", "%06d.png" % fid)), "plane": plane,
                "all_gt": lab["boxes3d"][lab["cls_type"] != "DontCare"],                             # filtrate_dc_objects :89-96
                "kept_lines": [ln for ln, c in zip(lines, lab["cls_type"]) if c in self.whitelist]}   # filtrate_objects :98-111

    def _host_batch(self, batch, base_id, seed):
        db = self.db
        dbb, dbn, dbo = db.boxes.cpu().numpy(), db.npts.cpu().numpy(), db.offsets.cpu().numpy()
        dbp, dbi = db.points.cpu().numpy(), db.intensity.cpu().numpy()
        out = []
        for fr in batch:
            s = aug_scene_sample_host(fr["all_gt"], fr["plane"], dbb, dbn, self.scope, seed, base_id + fr["id"], self.iou3d)
            use = s["status"] != 1
            cloud, _ = aug_scene_build_host(fr["scan"], fr["calib"], fr["img_shape"], self.scope, s["boxes"] if use else s["boxes"][:0],
                                            s["ids"] if use else [], s["y_shift"], dbp, dbi, dbo)
            out.append((s["status"], s["ids"], s["boxes"], cloud))
        return out

    def _device_batch(self, batch, base_id, seed):
        from . import ops
        dev, db, B = self.device, self.db, len(batch)
        packed = pack_scans([fr["scan"] for fr in batch], [fr["calib"] for fr in batch], [fr["img_shape"] for fr in batch])
        G = max(max(len(fr["all_gt"]) for fr in batch), 1)
        gt = np.zeros((B, G, 7), np.float32)
        for k, fr in enumerate(batch):
            gt[k, :len(fr["all_gt"])] = fr["all_gt"]
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        acc = ops.aug_scene_sample(T(gt), T(np.array([len(fr["all_gt"]) for fr in batch], np.int32)),
                                   T(np.stack([fr["plane"] for fr in batch]).astype(np.float64)),
                                   T(np.array([base_id + fr["id"] for fr in batch], np.int32)), db.boxes, db.npts, self.scope, seed)
        rows, off, cloud, _ = ops.aug_scene_build(packed["raw"].to(dev), packed["offsets"].to(dev), packed["max_points"], packed["calib"].to(dev),
                                                  packed["img_hw"].to(dev), self.scope, acc, db.points, db.intensity, db.offsets)
        status, count, ids, boxes = (acc[k].cpu().numpy() for k in ("status", "count", "db_id", "boxes3d"))
        off, cloud = off.cpu().numpy(), cloud.cpu().numpy()
        return [(int(status[k]), ids[k, :count[k]], boxes[k, :count[k]], cloud[off[k]:off[k + 1]]) for k in range(B)]

    def generate(self, save_dir, aug_times=4, seed=0, frames_per_batch=8, image_sets_dir=None):
        """generate_aug_scene (:285-305): <save_dir>/rectified_data/%06d.bin (float32 (n,4) rect x y z intensity) and
        <save_dir>/aug_label/%06d.txt (the frame's kept labels re-printed, then one line per accepted object) for the new ids
        (epoch + 1) * 10000 + sample_id, and <save_dir>/<split>_aug.txt: the original ids, then the new ones, no trailing newline
        (copied to image_sets_dir when given).  The new id keys the random table, so the epochs of one frame differ.
        -> one dict per written frame: sample_id (the new id), status, count.  A status-1 frame (fewer than two database objects, or a
        try that reaches the collision test with no label to test against) is written unaugmented and reported here; the reference
        would crash there."""
        data_dir, label_dir = os.path.join(save_dir, "rectified_data"), os.path.join(save_dir, "aug_label")
        os.makedirs(data_dir, exist_ok=True)
        os.makedirs(label_dir, exist_ok=True)
        split_list, report = list(self.frames), []
        run = self._host_batch if self.backend == "host" else self._device_batch
        for epoch in range(int(aug_times)):
            base_id, batch = (epoch + 1) * 10000, []

            def flush():
                for fr, (status, ids, boxes, cloud) in zip(batch, run(batch, base_id, int(seed)) if batch else []):
                    new_id = base_id + fr["id"]
                    np.ascontiguousarray(cloud, np.float32).tofile(os.path.join(data_dir, "%06d.bin" % new_id))
                    lines = [reprint_label_line(ln) for ln in fr["kept_lines"]]
                    if status != 1 and len(ids):
                        lines += aug_object_lines(boxes, self.truncation[ids], self.occlusion[ids], fr["calib"].P2, fr["img_shape"], self.class_name)
                    with open(os.path.join(label_dir, "%06d.txt" % new_id), "w") as f:
                        f.write("".join(ln + "\n" for ln in lines))
                    split_list.append("%06d" % new_id)
                    report.append({"sample_id": new_id, "status": int(status), "count": int(len(ids)) if status != 1 else 0})
                batch.clear()
            for fid in self.frames:
                fr = self._read_frame(int(fid))
                if self.class_name != "Car" and not fr["kept_lines"]:       # :259-260
                    continue
                batch.append(fr)
                if len(batch) >= max(1, int(frames_per_batch)):
                    flush()
            flush()
        split_file = os.path.join(save_dir, "%s_aug.txt" % self.split)
        with open(split_file, "w") as f:
            f.write("\n".join(split_list))
        if image_sets_dir is not None:
            os.makedirs(image_sets_dir, exist_ok=True)
            with open(os.path.join(image_sets_dir, "%s_aug.txt" % self.split), "w") as f:
                f.write("\n".join(split_list))
        return report


def load_aug_frame(root_dir, aug_root, sample_id):
    """One frame of the train_aug split as kitti_dataset.py / kitti_rcnn_dataset.py read it: id < 10000 the original files (velodyne
    scan in lidar coordinates), id >= 10000 <aug_root>/rectified_data/%06d.bin (rect coordinates already) and <aug_root>/aug_label/%06d.txt,
    with the calibration, image shape and road plane of id % 10000.  -> dict sample_id, pts (n,4) f32, rect_input, label_lines, calib
    (its packed() row carries the identity lidar -> rect for a rect_input frame: ScenePreparer / TrainScenePreparer take the frame as it
    is), img_shape, plane (None without a planes folder)"""
    sample_id = int(sample_id)
    base = os.path.join(root_dir, "KITTI", "object", "training")
    src = sample_id % 10000
    aug = sample_id >= 10000
    calib = Calibration(os.path.join(base, "calib", "%06d.txt" % src))
    calib.rect_input = aug
    pts_file = os.path.join(aug_root, "rectified_data", "%06d.bin" % sample_id) if aug else os.path.join(base, "velodyne", "%06d.bin" % src)
    label_file = os.path.join(aug_root, "aug_label", "%06d.txt" % sample_id) if aug else os.path.join(base, "label_2", "%06d.txt" % src)
    with open(label_file) as f:
        lines = [ln for ln in f.readlines() if ln.strip()]
    plane_file, plane = os.path.join(base, "planes", "%06d.txt" % src), None
    if os.path.isfile(plane_file):
        with open(plane_file) as f:
            plane = road_plane_from_lines(f.readlines())
    return {"sample_id": sample_id, "pts": get_lidar(pts_file), "rect_input": aug, "label_lines": lines, "calib": calib,
            "img_shape": get_image_shape(os.path.join(base, "image_2", "%06d.png" % src)), "plane": plane}
