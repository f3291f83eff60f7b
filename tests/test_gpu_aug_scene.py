"""GPU: the offline GT-augmented scenes on the device (csrc/aug_scene.hip: prcnn_aug_scene_sample, prcnn_aug_scene_count / _fill;
kitti_input.AugSceneGenerator) against the numpy twin (tests/aug_scene_twin.py, itself held to the reference's own tool by
tests/test_aug_scene_cpu.py), bit for bit.  Inputs are chosen so that the reference's loop, which the twin restates, has the outcome
each case names; the case asserts that outcome on the twin before it compares."""
import ctypes
import os

import numpy as np
import pytest
import torch

import aug_scene_twin as tw
import kitti_tree

pytestmark = pytest.mark.gpu
F32 = np.float32
PLANE = (0.0, -1.0, 0.0, 1.65)
CAR = (1.5, 1.6, 3.9)
JUNK = np.array([0, 1.65, 35, 9, 90, 90, 0], F32)           # a padding row: it would collide with everything if it were read


def grid_db(npts=20):
    """224 cars on a 5 m grid over the whole scope, heading 0: enlarged they are 4.4 x 2.1 m, so no two of them collide"""
    db = np.array([[x, 1.6, z] + list(CAR) + [0.0] for x in np.arange(-37.5, 38, 5.0) for z in np.arange(2.5, 70, 5.0)], F32)
    return db, np.full(len(db), npts, np.int32)


_twin = {}


def twin_sample(key, gt, plane, db, npts, seed, frame):
    if key not in _twin:
        _twin[key] = tw.sample(gt, plane, db, npts, seed, frame)
    return _twin[key]


def run_sampler(dev, gts, planes, frame_ids, db, npts, seed, G=None, K=15):
    from pointrcnn_amd import ops
    B = len(gts)
    G = max(len(g) for g in gts) if G is None else G
    gt = np.tile(JUNK, (B, G, 1)).astype(F32)
    for b, g in enumerate(gts):
        gt[b, :len(g)] = g
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    acc = ops.aug_scene_sample(T(gt), T(np.array([len(g) for g in gts], np.int32)), T(np.asarray(planes, np.float64).reshape(B, 4)),
                               T(np.asarray(frame_ids, np.int32)), T(db), T(npts), tw.SCOPE, seed, K)
    return {k: v.cpu().numpy() for k, v in acc.items()}


def assert_frame(acc, b, t, tag):
    n = len(t["ids"])
    assert acc["status"][b] == t["status"] and acc["count"][b] == n, (tag, acc["status"][b], acc["count"][b], t["status"], n)
    assert tuple(acc["stats"][b]) == tuple(t["stats"]), (tag, acc["stats"][b], t["stats"])
    assert np.array_equal(acc["db_id"][b, :n], t["ids"]) and (acc["db_id"][b, n:] == -1).all(), tag
    assert np.array_equal(acc["boxes3d"][b, :n].view(np.int32), t["boxes"].view(np.int32)) and not acc["boxes3d"][b, n:].any(), tag
    assert np.array_equal(acc["y_shift"][b, :n].view(np.int64), t["y_shift"].view(np.int64)) and not acc["y_shift"][b, n:].any(), tag


def test_sampler_outcomes_of_the_reference_loop(dev):
    db, npts = grid_db()
    far_label = np.array([[0, 1.6, -30] + list(CAR) + [0]], F32)
    none = np.zeros((0, 7), F32)
    # empty road: the accepted count reaches extra_gt_num + 1, for extra_gt_num 10, 12 and 14
    for seed, extra in ((0, 10), (3, 12), (23, 14)):
        t = twin_sample(("full", seed), far_label, PLANE, db, npts, seed, 10000)
        assert t["stats"][0] == extra and len(t["ids"]) == extra + 1 == t["stats"][1] and t["status"] == 0
        assert_frame(run_sampler(dev, [far_label], [PLANE], [10000], db, npts, seed), 0, t, ("full", seed))
    # no non-DontCare label: the first try that reaches the collision test raises; with G = 0, and with only padding rows
    t = twin_sample("nolabel", none, PLANE, db, npts, 1, 10002)
    assert t["status"] == 1 and len(t["ids"]) == 0 and t["stats"][1] == 1
    assert_frame(run_sampler(dev, [none], [PLANE], [10002], db, npts, 1, G=0), 0, t, "G=0")
    assert_frame(run_sampler(dev, [none], [PLANE], [10002], db, npts, 1, G=3), 0, t, "num_gt=0")
    # D = 1: randint(0, 0) raises at the first try; D = 2: only id 0 is ever drawn
    t = twin_sample("D1", far_label, PLANE, db[:1], npts[:1], 1, 10000)
    assert t["status"] == 1 and t["stats"][1:] == (0, 1)
    assert_frame(run_sampler(dev, [far_label], [PLANE], [10000], db[:1], npts[:1], 1), 0, t, "D=1")
    t = twin_sample("D2", far_label, PLANE, db[:2], npts[:2], 1, 10000)
    assert list(t["ids"]) == [0] and t["status"] == 0 and t["stats"][1] == t["stats"][0] + 1       # accepted once, then it collides with itself
    assert_frame(run_sampler(dev, [far_label], [PLANE], [10000], db[:2], npts[:2], 1), 0, t, "D=2")
    # all centres out of scope: 50 tries spent, nothing counted -- and nothing raised, even without a label
    out = db.copy()
    out[:, 0] += F32(100)
    for gt in (far_label, none):
        t = twin_sample(("out", len(gt)), gt, PLANE, out, npts, 2, 10001)
        assert t["stats"][1:] == (0, 50) and t["status"] == 0 and len(t["ids"]) == 0
        assert_frame(run_sampler(dev, [gt], [PLANE], [10001], out, npts, 2), 0, t, "out of scope")
    # entries with 4 points spend tries and are never accepted
    few = npts.copy()
    few[::2] = 4
    t = twin_sample("few", far_label, PLANE, db, few, 4, 10003)
    assert len(t["ids"]) > 3 and (few[t["ids"]] == 20).all() and t["stats"][2] > t["stats"][1] + 5
    assert_frame(run_sampler(dev, [far_label], [PLANE], [10003], db, few, 4), 0, t, "4 points")
    # every candidate that reaches the test collides, and few enough reach it: count 0, all 50 tries spent
    cover = np.array([[x, 1.65, 35, 4, 81, 41, 0] for x in (-20, 20)], F32)
    rare = out.copy()
    rare[::20] = db[::20]
    t = twin_sample("collide", cover, PLANE, rare, npts, 7, 10004)
    assert len(t["ids"]) == 0 and t["stats"][2] == 50 and 0 < t["stats"][1] <= t["stats"][0] and t["status"] == 0
    assert_frame(run_sampler(dev, [cover], [PLANE], [10004], rare, npts, 7), 0, t, "all collide")


def test_sampler_touching_boxes_pass_and_a_sliver_collides(dev):
    """the new box against a label enlarged to x in [-2, 2], z in [19, 21]: touching at x = 2 gives IoU 0 and is accepted, one float32
    step of overlap gives IoU 3e-8 >= 1e-8 and is not.  D = 2: the candidate is the only entry ever drawn."""
    import oracle
    label = np.array([[0, 1.65, 20, 1.5, 1.5, 3.5, 0]], F32)
    enl = label + np.array([0, 0, 0, 0, 0.5, 0.5, 0], F32)
    for x, accepted in ((F32(4.0), True), (np.nextafter(F32(4.0), F32(0)), False)):
        cand = np.array([[x, 0.9, 20, 1.5, 2.0, 4.0, 0], [0, 0, 0, 1, 1, 1, 0]], F32)
        t = twin_sample(("touch", accepted), label, PLANE, cand, np.array([9, 9], np.int32), 5, 10000)
        iou = oracle.cpu().boxes_iou3d(np.array([[x, 1.65, 20, 1.5, 2.0, 4.0, 0]], F32), enl)[0, 0]
        assert (iou == 0 and list(t["ids"]) == [0]) if accepted else (1e-8 < iou < 1e-7 and len(t["ids"]) == 0), (x, iou, t["ids"])
        if accepted:
            assert t["boxes"][0, 1] == F32(1.65) and t["y_shift"][0] == float(F32(0.9)) - 1.65
        assert_frame(run_sampler(dev, [label], [PLANE], [10000], cand, np.array([9, 9], np.int32), 5), 0, t, ("touch", accepted))


def test_sampler_batches_padding_and_many_labels(dev):
    """B = 5 against B = 1, G = 1 and G = 128 with padding rows present, tilted planes: a frame's result does not depend on its batch"""
    db, npts = grid_db()
    rng = np.random.default_rng(3)
    many = np.array([[x, 1.6, z] + list(CAR) + [rng.uniform(-3, 3)] for x in np.arange(-36, 37, 8.0) for z in np.arange(4, 68, 5.0)], F32)[:128]
    assert len(many) == 128
    gts = [many, many[:1], many[5:40], np.zeros((0, 7), F32), many[::3]]
    planes = [PLANE, (0.02, -1.0, 0.01, 1.7), (0.01, -1.0, -0.02, 1.6), PLANE, (-0.03, -0.99, 0.02, 1.5)]
    ids = [10000, 10001, 20001, 30007, 47480]
    want = [twin_sample(("batch", b), gts[b], planes[b], db, npts, 9, ids[b]) for b in range(5)]
    assert [t["status"] for t in want] == [0, 0, 0, 1, 0] and 0 < len(want[0]["ids"]) < len(want[1]["ids"])
    assert len({tuple(t["ids"]) for t in want}) == 5
    acc = run_sampler(dev, gts, planes, ids, db, npts, 9, G=128)
    for b in range(5):
        assert_frame(acc, b, want[b], ("B=5", b))
    for b, G in ((0, 128), (1, 1), (2, 64), (4, 241)):
        one = run_sampler(dev, [gts[b]], [planes[b]], [ids[b]], db, npts, 9, G=G, K=15 if b else 64)
        assert_frame(one, 0, want[b], ("B=1", b))


# ------------------------------------------------------------------------------------------------------------------ builder
def builder_case():
    """13 frames of rect points under the identity lidar -> rect (the valid flag still decides): sizes on the tile and wave edges,
    no valid point, every valid point inside an accepted box, count 0, status 1, two accepted boxes sharing points"""
    from pointrcnn_amd import kitti_input
    rng = np.random.default_rng(12)
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    calib.rect_input = True
    db_n = np.array([7, 0, 33, 120, 5], np.int64)
    db_off = np.concatenate([[0], np.cumsum(db_n)])
    db_pts = rng.uniform(-3, 3, (int(db_off[-1]), 3)).astype(F32)
    db_int = rng.uniform(0, 1, int(db_off[-1])).astype(F32)

    def cloud(n, inside=None):
        p = np.stack([rng.uniform(-8, 8, n), rng.uniform(-0.5, 1.7, n), rng.uniform(8, 40, n), rng.uniform(0, 1, n)], 1).astype(F32)
        p[::5, 2] *= F32(-1)                                               # behind the camera: not valid
        if inside is not None:
            p[:, :3] = inside[:3] + rng.uniform(-0.4, 0.4, (n, 3)) - [0, 0.7, 0]
        return p
    box_a, box_b = np.array([0, 1.65, 20, 1.5, 1.8, 4.2, 0.4], F32), np.array([1.0, 1.6, 21, 1.6, 1.7, 4.0, -0.9], F32)
    acc2 = dict(ids=np.array([3, 0], np.int32), boxes=np.stack([box_a, box_b]), y_shift=np.array([0.25, -0.125]), status=0)
    acc3 = dict(ids=np.array([4, 1, 2], np.int32), boxes=np.stack([box_b, box_a + F32(5), box_a]), y_shift=np.array([1e-3, 0.0, -0.7]), status=0)
    none = dict(ids=np.zeros(0, np.int32), boxes=np.zeros((0, 7), F32), y_shift=np.zeros(0), status=0)
    frames = [(cloud(n), acc2 if k % 2 else acc3) for k, n in enumerate((0, 1, 63, 64, 65, 1024, 1025))]
    behind = cloud(300)
    behind[:, 2] = -np.abs(behind[:, 2])
    frames += [(behind, acc2), (cloud(500, box_a), acc2), (cloud(700), none), (cloud(700), dict(acc2, status=1)),
               (np.concatenate([cloud(200, box_a), cloud(200, (box_a + box_b) / 2), cloud(2100)]), acc2), (cloud(1500), dict(acc3, status=2))]
    return calib, frames, db_pts, db_int, db_off


def run_builder(dev, calib, frames, db_pts, db_int, db_off, guard_rows=0):
    from pointrcnn_amd import kitti_input, ops
    B, K = len(frames), 15
    packed = kitti_input.pack_scans([s for s, _ in frames], [calib] * B, [(375, 1242)] * B, pin=False)
    acc = {"count": np.zeros(B, np.int32), "db_id": np.full((B, K), -1, np.int32), "boxes3d": np.zeros((B, K, 7), F32),
           "y_shift": np.zeros((B, K)), "status": np.zeros(B, np.int32)}
    for b, (_, a) in enumerate(frames):
        n = len(a["ids"])
        acc["count"][b], acc["status"][b] = n, a["status"]
        acc["db_id"][b, :n], acc["boxes3d"][b, :n], acc["y_shift"][b, :n] = a["ids"], a["boxes"], a["y_shift"]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    rows, off, out, src = ops.aug_scene_build(packed["raw"].to(dev), packed["offsets"].to(dev), packed["max_points"], packed["calib"].to(dev),
                                              packed["img_hw"].to(dev), tw.SCOPE, {k: T(v) for k, v in acc.items()}, T(db_pts), T(db_int),
                                              T(db_off), guard_rows)
    return rows.cpu().numpy(), off.cpu().numpy(), out.cpu().numpy(), src.cpu().numpy()


def test_builder_equals_the_twin_on_tile_and_wave_edges(dev):
    calib, frames, db_pts, db_int, db_off = builder_case()
    if "build" not in _twin:
        _twin["build"] = [tw.build(s, calib.packed(), (375, 1242), a, db_pts, db_int, db_off) for s, a in frames]
    want = _twin["build"]
    kept = [w[2] for w in want]
    # what the frames were built to show
    assert [len(s) for s, _ in frames[:7]] == [0, 1, 63, 64, 65, 1024, 1025]
    assert kept[7] == 0 and kept[8] == 0 and len(want[8][0]) == 127 and int((want[7][1] < 0).sum()) == 127       # no valid point; all valid points removed
    assert (want[9][1] >= 0).all() and (want[10][1] >= 0).all() and kept[9] > 400 and kept[10] > 400            # count 0 / status 1: the valid cloud
    assert kept[11] < 2100 and len(want[12][0]) == kept[12] + 5 + 0 + 33                                       # status 2 still pastes
    rows, off, out, src = run_builder(dev, calib, frames, db_pts, db_int, db_off, guard_rows=16)
    assert list(rows) == [len(w[0]) for w in want] and list(off) == list(np.concatenate([[0], np.cumsum(rows)]))
    n = int(off[-1])
    for b, w in enumerate(want):
        assert np.array_equal(out[off[b]:off[b + 1]].view(np.int32), w[0].view(np.int32)), b
        assert np.array_equal(src[off[b]:off[b + 1]], w[1]), b
    assert (out[n:] == -12345.0).all() and (src[n:] == -12345).all() and len(out) == n + 16                    # the guard rows are untouched
    again = run_builder(dev, calib, frames, db_pts, db_int, db_off, guard_rows=16)
    assert out.tobytes() == again[2].tobytes() and src.tobytes() == again[3].tobytes()
    # a frame's rows do not depend on its batch
    one = run_builder(dev, calib, frames[11:12], db_pts, db_int, db_off)
    assert np.array_equal(one[2].view(np.int32), want[11][0].view(np.int32)) and np.array_equal(one[3], want[11][1])


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_generate_on_the_device_writes_the_host_backends_files(dev, tmp_path, cpu):
    import oracle
    from pointrcnn_amd import kitti_input
    root = str(tmp_path / "tree")
    tw.write_aug_tree(root)
    outs = {}
    for backend in ("device", "host"):
        gen = kitti_input.AugSceneGenerator(root, tw.database(dev if backend == "device" else "cpu"), device=dev if backend == "device" else "cpu",
                                            backend=backend, iou3d=cpu.boxes_iou3d)
        outs[backend] = str(tmp_path / backend)
        report = gen.generate(outs[backend], aug_times=2, seed=11, frames_per_batch=3)
        assert [(r["sample_id"], r["status"]) for r in report] == [(e * 10000 + f, int(f == 2)) for e in (1, 2) for f in tw.FRAMES]
        assert sum(r["count"] for r in report) > 20
    for sub, names in (("rectified_data", ["%06d.bin" % r["sample_id"] for r in report]), ("aug_label", ["%06d.txt" % r["sample_id"] for r in report]),
                       ("", ["train_aug.txt"])):
        for name in names:
            with open(os.path.join(outs["device"], sub, name), "rb") as a, open(os.path.join(outs["host"], sub, name), "rb") as b:
                assert a.read() == b.read(), (sub, name)
    # a written train_aug frame through the reader and ScenePreparer == the oracle on the stored rect cloud with the identity matrix
    frames = [kitti_input.load_aug_frame(root, outs["device"], i) for i in (10000, 20001)]
    prep = kitti_input.ScenePreparer(npoints=1024, device=dev)
    pk = prep.pack([f["pts"] for f in frames], [f["calib"] for f in frames], [f["img_shape"] for f in frames], pin=False)
    got = prep(pk, seed=5)
    eye = np.stack([f["calib"].packed(rect_input=True) for f in frames])
    assert np.array_equal(pk["calib"].numpy(), eye) and np.array_equal(eye[0, :12].reshape(4, 3), np.eye(4, 3, dtype=F32))
    want = oracle.scene_prepare(pk["raw"].numpy(), pk["offsets"].numpy(), eye, pk["img_hw"].numpy(), prep.scope, 1024, 5)
    assert np.array_equal(got["pts_input"].cpu().numpy(), want[0]) and np.array_equal(got["src"].cpu().numpy(), want[2])
    assert np.array_equal(got["nvalid"].cpu().numpy(), want[3]) and (got["status"].cpu().numpy() == 0).all()
    assert all(0 < v <= len(f["pts"]) for v, f in zip(want[3], frames))


def test_argument_errors_are_refused_without_a_launch(dev):
    from pointrcnn_amd import _cabi, ops
    lib = _cabi.lib()
    db, npts = grid_db()
    gt = np.zeros((1, 7), F32)
    with pytest.raises(_cabi.PointOpsError, match="K=14"):
        run_sampler(dev, [gt], [PLANE], [10000], db, npts, 1, K=14)
    with pytest.raises(_cabi.PointOpsError, match=r"G \+ 15 = 257 > 256"):
        run_sampler(dev, [gt], [PLANE], [10000], db, npts, 1, G=242)
    t = torch.zeros(64, dtype=torch.float32, device=dev)
    p, scope = t.data_ptr(), (ctypes.c_double * 6)(*tw.SCOPE)
    assert lib.prcnn_aug_scene_sample(p, None, p, p, 1, 1, p, p, 2, scope, 15, 0, p, p, None, p, p, p, None) == -1
    assert b"null pointer" in lib.prcnn_last_error()
    need = lib.prcnn_aug_scene_workspace_bytes(4, 1)
    assert lib.prcnn_aug_scene_count(p, p, 1, 4, 4, p, p, scope, p, p, p, p, 15, p, 1, 4, p, p, need - 1, None) == -1
    assert b"workspace too small" in lib.prcnn_last_error()
    torch.cuda.synchronize()
    assert not t.any()
