"""The GT-augmentation database built on the device (csrc/gt_database.hip, ops.gt_database_build, GTDatabase.from_kitti) against
the oracle's canonical lidar -> rect followed by the reference's own pts_in_boxes3d_cpu (its source compiled for the host where the
build had it, the oracle's restatement with the host libm otherwise) and boolean masks in raw order -- every output bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kitti_tree
import oracle
from util import GOLDEN

pytestmark = pytest.mark.gpu
G = 6
SIZES = (0, 1, 1025, 3137, 2500)                  # empty, one point, one past a tile, several tiles + a ragged tail, > 2 tiles
INF = np.float32(np.inf)


def _calib24():
    """identity-like calibration: rect == lidar xyz exactly (M = [I; 0]); P2 is not read by the builder"""
    from pointrcnn_amd import kitti_input
    M = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((1, 3), np.float32)])
    return np.concatenate([M.reshape(-1), kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT).P2.reshape(-1)]).astype(np.float32)


def _local_to_world(box, loc):
    c, s = np.cos(np.float64(box[6])), np.sin(np.float64(box[6]))
    cy = np.float64(box[1]) - np.float64(box[3]) / 2
    return np.array([box[0] + loc[0] * c + loc[2] * s, cy + loc[1], box[2] - loc[0] * s + loc[2] * c], np.float32)


def _face_points(box, rng, per_face=4):
    """points on every face of the box (as exactly as fp32 allows; exactly for the y faces and for ry = 0) and one ulp either side"""
    h, w, l = (np.float64(v) for v in box[3:6])
    out = []
    for axis, half, moved in ((0, l / 2, (0, 2)), (2, w / 2, (0, 2)), (1, h / 2, (1,))):
        for sign in (-1.0, 1.0):
            for _ in range(per_face):
                loc = [rng.uniform(-0.45, 0.45) * l, rng.uniform(-0.45, 0.45) * h, rng.uniform(-0.45, 0.45) * w]
                loc[axis] = sign * half
                p = _local_to_world(box, loc)
                out.append(p)
                for k in moved:
                    for d in (-INF, INF):
                        q = p.copy()
                        q[k] = np.nextafter(q[k], d)
                        out.append(q)
    return np.stack(out)


def _case():
    rng = np.random.default_rng(20261018)
    boxes = np.zeros((len(SIZES), G, 7), np.float32)
    num = np.array([3, 0, 6, 5, 2], np.int32)
    scans = []
    # frame 0: boxes, no point
    boxes[0, :3] = [[0, 2, 10, 1.5, 1.6, 3.9, 0.1], [3, 2, 12, 1.5, 1.6, 3.9, 1.1], [-3, 2, 8, 1.5, 1.6, 3.9, -2.0]]
    scans.append(np.zeros((0, 4), np.float32))
    # frame 1: one point inside a box that num_boxes = 0 hides
    boxes[1, 0] = [0, 2, 10, 1.5, 1.6, 3.9, 0.0]
    scans.append(np.array([[0.0, 1.0, 10.0, 0.5]], np.float32))
    # frame 2 (1025 points): two overlapping boxes, a box nothing hits, two 24 m boxes (the 10 m gate decides, along x and along z),
    # a generic one; NaN points; the point alone in the second tile lies in box 0
    boxes[2] = [[0, 2, 10, 1.5, 2, 4, 0.3], [1, 2, 10.5, 1.5, 2, 4, -0.4], [50, 2, 50, 1.5, 1.6, 3.9, 1.0],
                [0, 2, 40, 1.5, 1.6, 24, 0.0], [-30, 2, 40, 1.5, 1.6, 24, np.pi / 2], [20, 2, 10, 1.5, 1.6, 3.9, 2.5]]
    p = [np.stack([rng.uniform(-3, 4, 300), rng.uniform(0.3, 2.2, 300), rng.uniform(7.5, 13, 300)], 1),
         np.stack([rng.uniform(-12.5, 12.5, 190), rng.uniform(0.6, 1.9, 190), rng.uniform(39.3, 40.7, 190)], 1),
         np.stack([rng.uniform(-30.7, -29.3, 190), rng.uniform(0.6, 1.9, 190), rng.uniform(27.5, 52.5, 190)], 1),
         np.stack([rng.uniform(17, 23, 100), rng.uniform(0.3, 2.2, 100), rng.uniform(7, 13, 100)], 1),
         np.stack([rng.uniform(-60, 60, 224), rng.uniform(-2, 3, 224), rng.uniform(-10, 70, 224)], 1)]
    gate = np.float32(10.0)
    edge = [[gate, 1.0, 40.0], [np.nextafter(gate, INF), 1.0, 40.0], [np.nextafter(gate, -INF), 1.0, 40.0],
            [-gate, 1.0, 40.0], [np.nextafter(-gate, -INF), 1.0, 40.0], [11.9, 1.0, 40.0],
            [-30.0, 1.0, 50.0], [-30.0, 1.0, np.nextafter(np.float32(50.0), INF)], [-30.0, 1.0, np.nextafter(np.float32(50.0), -INF)],
            [-30.0, 1.0, 30.0], [-30.0, 1.0, np.nextafter(np.float32(30.0), -INF)], [-30.0, 1.0, 51.9]]
    nan = np.array([[np.nan, 1.0, 10.0], [0.0, np.nan, 10.0], [0.0, 1.0, np.nan], [np.nan, np.nan, np.nan],
                    [np.nan, 1.0, 40.0], [1.0, np.nan, 10.5], [-30.0, 1.0, np.nan], [0.5, np.nan, np.nan]], np.float32)
    xyz = np.concatenate(p + [np.asarray(edge, np.float32), nan]).astype(np.float32)
    assert len(xyz) == 1024
    xyz = np.concatenate([xyz[rng.permutation(1024)], [[0.2, 1.2, 10.1]]]).astype(np.float32)
    scans.append(np.concatenate([xyz, rng.uniform(0, 1, (1025, 1)).astype(np.float32)], 1))
    # frame 3 (3137 points): ry = 0, +-pi/2, pi and a generic angle, with points on every face and one ulp either side; the sixth
    # slot holds a box over everything that num_boxes = 5 hides
    ang = [0.0, np.pi / 2, -np.pi / 2, np.pi, 0.7]
    boxes[3, :5] = [[-16 + 8 * k, 2.0, 20.0, 1.5, 2.0, 4.0, a] for k, a in enumerate(ang)]
    boxes[3, 5] = [0, 3, 20, 4, 9.9, 9.9, 0]
    face = np.concatenate([_face_points(boxes[3, k], rng) for k in range(5)])
    fill = np.stack([rng.uniform(-20, 20, 3137 - len(face)), rng.uniform(0.2, 2.3, 3137 - len(face)), rng.uniform(16, 24, 3137 - len(face))], 1)
    xyz = np.concatenate([face, fill]).astype(np.float32)[rng.permutation(3137)]
    scans.append(np.concatenate([xyz, rng.uniform(0, 1, (3137, 1)).astype(np.float32)], 1))
    # frame 4 (2500 points): box 0 holds every point (hits cross wave and tile boundaries), box 1 some of them
    boxes[4, :2] = [[0, 2, 10, 1.5, 4, 4, 0.2], [0.5, 2, 10, 1.5, 1, 1, 0.0]]
    xyz = np.stack([rng.uniform(-1, 1, 2500), rng.uniform(0.6, 1.9, 2500), rng.uniform(9, 11, 2500)], 1).astype(np.float32)
    scans.append(np.concatenate([xyz, rng.uniform(0, 1, (2500, 1)).astype(np.float32)], 1))
    assert tuple(len(s) for s in scans) == SIZES
    return scans, boxes, num, _calib24()


def _in_boxes(rect, boxes):
    r = oracle.ref()
    return r.pts_in_boxes3d_cpu(rect, boxes) if r is not None else oracle.cpu().pts_in_boxes3d(rect, boxes, 0)


def _expected(scans, boxes, num, calib24):
    """oracle.scene_project -> the reference's pts_in_boxes3d_cpu -> boolean masks in raw order"""
    npts = np.zeros(boxes.shape[:2], np.int32)
    pts, inten, src = [np.zeros((0, 3), np.float32)], [np.zeros(0, np.float32)], [np.zeros(0, np.int32)]
    for b, scan in enumerate(scans):
        if len(scan) == 0 or num[b] == 0:
            continue
        rect = oracle.scene_project(scan, calib24, 375, 1242, None)[0]
        for g, row in enumerate(_in_boxes(rect, boxes[b, :num[b]])):
            m = row == 1
            npts[b, g] = m.sum()
            pts.append(rect[m]); inten.append(scan[m, 3]); src.append(np.nonzero(m)[0].astype(np.int32))
    off = np.concatenate([[0], np.cumsum(npts.reshape(-1))]).astype(np.int64)
    return npts, off, np.concatenate(pts), np.concatenate(inten), np.concatenate(src)


def _device_args(scans, boxes, num, calib24):
    from pointrcnn_amd import kitti_input
    B = len(scans)
    raw = torch.from_numpy(np.concatenate(scans)).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)).cuda()
    assert kitti_input is not None
    return (raw, off, max(len(s) for s in scans), torch.from_numpy(np.tile(calib24, (B, 1))).cuda(), torch.from_numpy(boxes).cuda(),
            torch.from_numpy(num).cuda())


@pytest.fixture(scope="module")
def case():
    scans, boxes, num, calib24 = _case()
    return scans, boxes, num, calib24, _expected(scans, boxes, num, calib24)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_the_case_holds_what_it_claims(case):
    """the expected values themselves: every situation the case was built for occurs in it"""
    scans, boxes, num, calib24, (npts, off, pts, inten, src) = case
    assert not npts[0].any() and not npts[1].any()                            # no point / num_boxes 0
    f2 = npts[2]
    assert f2[0] > 0 and f2[1] > 0 and f2[2] == 0 and f2[3] > 0 and f2[4] > 0 and f2[5] > 0
    o = off[2 * G:3 * G + 1]
    a, b = set(src[o[0]:o[1]]), set(src[o[1]:o[2]])
    assert len(a & b) > 0 and 1024 in a                                       # shared points; the lone point of the second tile
    x = scans[2][:, 0]
    gx = set(src[o[3]:o[4]])
    on = lambda v: set(np.nonzero((x == np.float32(v)) & (scans[2][:, 2] == 40.0))[0])      # noqa: E731
    assert on(10.0) <= gx and on(-10.0) <= gx and not (on(np.nextafter(np.float32(10.0), INF)) & gx) and not (on(11.9) & gx)
    assert ((np.abs(x[list(gx)]) <= 10.0).all()) and (np.abs(x) > 10.0)[(np.abs(x) < 12) & (np.abs(scans[2][:, 2] - 40) < 0.7)].any()
    nan_rows = set(np.nonzero(np.isnan(scans[2][:, :3]).any(1))[0])
    assert len(nan_rows) == 8 and not (nan_rows & set(src[o[0]:o[6]]))
    assert (npts[3, :5] > 50).all() and npts[3, 5] == 0                      # the hidden sixth box
    assert npts[4, 0] == 2500 and 0 < npts[4, 1] < 2500
    assert np.array_equal(src[off[4 * G]:off[4 * G + 1]], np.arange(2500))
    # the face points split: some of every face family are in, some out
    rect3 = scans[3][:, :3]
    flags = _in_boxes(rect3, boxes[3, :5])
    assert np.array_equal(flags.sum(1), npts[3, :5])


def test_build_matches_the_reference_bit_for_bit(case):
    from pointrcnn_amd import ops
    scans, boxes, num, calib24, want = case
    got = ops.gt_database_build(*_device_args(scans, boxes, num, calib24))
    torch.cuda.synchronize()
    for name, g, w in zip(("npts", "offsets", "points", "intensity", "src"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), name


def test_two_builds_give_identical_bytes(case):
    from pointrcnn_amd import ops
    scans, boxes, num, calib24, _ = case
    args = _device_args(scans, boxes, num, calib24)
    a = [t.cpu().numpy().tobytes() for t in ops.gt_database_build(*args)]
    b = [t.cpu().numpy().tobytes() for t in ops.gt_database_build(*args)]
    assert a == b


def _abi_call(case, G_=None, null_boxes=False, short_ws=False, extra_rows=16):
    """count and fill through the C ABI with caller-owned buffers; -> (rc_count, rc_fill, npts, src buffer, P)"""
    from pointrcnn_amd import _cabi
    scans, boxes, num, calib24, _ = case
    raw, off, mp, calib, bx, nb = _device_args(scans, boxes, num, calib24)
    L = _cabi.lib()
    B, Gn = len(scans), boxes.shape[1] if G_ is None else G_
    need = int(L.prcnn_gt_database_workspace_bytes(mp, B, min(Gn, 128)))
    ws = torch.zeros((need - 64 if short_ws else need,), dtype=torch.uint8, device="cuda")
    npts = torch.zeros((B, Gn), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    bp = None if null_boxes else bx.data_ptr()
    rc = L.prcnn_gt_database_count(raw.data_ptr(), off.data_ptr(), B, raw.shape[0], mp, calib.data_ptr(), bp, nb.data_ptr(), Gn, npts.data_ptr(),
                                   ws.data_ptr(), ws.numel(), s)
    if rc != 0:
        return rc, None, None, None, None
    o = torch.zeros((B * Gn + 1,), dtype=torch.int64, device="cuda")
    o[1:] = torch.cumsum(npts.reshape(-1), 0, dtype=torch.int64)
    P = int(o[-1])
    pts = torch.full((P + extra_rows, 3), -7.0, device="cuda")
    inten = torch.full((P + extra_rows,), -7.0, device="cuda")
    src = torch.full((P + extra_rows,), -7, dtype=torch.int32, device="cuda")
    rc2 = L.prcnn_gt_database_fill(raw.data_ptr(), off.data_ptr(), B, raw.shape[0], mp, calib.data_ptr(), bp, nb.data_ptr(), Gn, o.data_ptr(), P,
                                   pts.data_ptr(), inten.data_ptr(), src.data_ptr(), ws.data_ptr(), ws.numel(), s)
    torch.cuda.synchronize()
    return rc, rc2, npts.cpu().numpy(), (pts.cpu().numpy(), inten.cpu().numpy(), src.cpu().numpy()), P


def test_count_and_fill_agree_on_the_rows(case):
    want = case[4]
    rc, rc2, npts, (pts, inten, src), P = _abi_call(case)
    assert rc == 0 and rc2 == 0
    assert P == int(npts.sum()) == len(want[4])
    assert (src[:P] >= 0).all() and (src[P:] == -7).all()                     # every counted row written, nothing beyond
    assert (pts[P:] == -7.0).all() and (inten[P:] == -7.0).all()
    assert np.array_equal(src[:P], want[4]) and np.array_equal(_bits(pts[:P]), _bits(want[2]))


def test_status_paths_return_errors_without_a_launch(case):
    from pointrcnn_amd import _cabi, ops
    L = _cabi.lib()
    scans, boxes, num, calib24, _ = case
    raw, off, mp, calib, bx, nb = _device_args(scans, boxes, num, calib24)
    with pytest.raises(_cabi.PointOpsError, match="G=129"):
        ops.gt_database_build(raw, off, mp, calib, torch.zeros((len(scans), 129, 7), device="cuda"), nb)
    assert _abi_call(case, G_=129)[0] == -1 and b"G=129" in L.prcnn_last_error()
    assert _abi_call(case, null_boxes=True)[0] == -1 and b"null pointer" in L.prcnn_last_error()
    assert _abi_call(case, short_ws=True)[0] == -1 and b"workspace too small" in L.prcnn_last_error()
    torch.cuda.synchronize()
    assert ctypes.c_int(L.prcnn_abi_version()).value == 12


# ---------------------------------------------------------------------------------------------------------------------------
# GTDatabase.from_kitti on a 3-frame tree (the first three frames of the CPU fixture's tree: its scans and label text)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    gold = np.load(os.path.join(GOLDEN, "gt_database_ref.npz"))
    root = str(tmp_path_factory.mktemp("gt_database_gpu_tree"))
    frames = [int(f) for f in gold["frames"][:3]]
    base = kitti_tree.write_tree(root, frames, seed0=int(gold["seed0"]), n_scan=int(gold["n_scan"]))
    for k, f in enumerate(frames):
        with open(os.path.join(base, "label_2", "%06d.txt" % f), "w") as fh:
            fh.write("".join(str(ln) + "\n" for ln in gold["f%d_labels" % k]))
    return root, base, frames


@pytest.fixture(scope="module")
def databases(tree):
    from pointrcnn_amd import kitti_input
    root = tree[0]
    dev = kitti_input.GTDatabase.from_kitti(root, "train", "Car", hard_ratio=0.6, device="cuda", frames_per_batch=2, backend="device")
    host = kitti_input.GTDatabase.from_kitti(root, "train", "Car", hard_ratio=0.6, device="cuda", backend="host")
    return dev, host


def test_from_kitti_device_equals_host(databases, tree):
    from pointrcnn_amd import kitti_input
    dev, host = databases
    assert dev.size == host.size > 0 and dev.max_points == host.max_points
    for k in ("boxes", "alpha", "npts", "offsets", "points", "intensity", "easy_idx", "hard_idx", "src"):
        a, b = getattr(dev, k), getattr(host, k)
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), k
    assert len(dev.easy_idx) and len(dev.hard_idx)
    assert np.array_equal(dev.sample_id, host.sample_id) and np.array_equal(dev.cls_type, host.cls_type)
    people = [kitti_input.GTDatabase.from_kitti(tree[0], class_name="People", backend=bk) for bk in ("device", "host")]
    assert set(people[0].cls_type) == {"Pedestrian", "Cyclist"}
    for k in ("boxes", "npts", "points", "intensity", "src"):
        assert torch.equal(getattr(people[0], k), getattr(people[1], k)), k


def test_database_drives_the_train_scene_preparer(databases, tree):
    """the device-built database and from_arrays of the host result give TrainScenePreparer the same batch"""
    from pointrcnn_amd import kitti_input
    dev, host = databases
    root, base, frames = tree
    e = host.entries()
    twin = kitti_input.GTDatabase.from_arrays(np.stack([d["gt_box3d"] for d in e]), host.alpha.cpu().numpy(), [d["points"] for d in e],
                                              [d["intensity"] for d in e], hard_ratio=0.6)
    scans, calibs, gt, alpha, all_gt = [], [], [], [], []
    for f in frames:
        scans.append(kitti_input.get_lidar(os.path.join(base, "velodyne", "%06d.bin" % f)))
        calibs.append(kitti_input.Calibration(os.path.join(base, "calib", "%06d.txt" % f)))
        with open(os.path.join(base, "label_2", "%06d.txt" % f)) as fh:
            lab = kitti_input.read_label_lines(fh.readlines())
        car = lab["cls_type"] == "Car"
        gt.append(lab["boxes3d"][car]); alpha.append(lab["alpha"][car].astype(np.float32))
        all_gt.append(lab["boxes3d"][lab["cls_type"] != "DontCare"])
    outs = []
    for db in (dev, twin):
        prep = kitti_input.TrainScenePreparer(npoints=1024, gt_database=db)
        packed = prep.pack(scans, calibs, [kitti_tree.image_shape(f) for f in frames], gt, alpha, all_gt, [[0.0, -1.0, 0.0, 1.65]] * len(frames), pin=False)
        out = prep(packed, 11)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
    assert outs[0]["count"].sum() > 0                                       # objects were pasted
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=outs[0][k].dtype.kind == "f"), k
