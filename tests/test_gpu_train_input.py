"""GT-augmentation sampling on the device: prcnn_corner_iou3d against the double restatement (tests/train_input_twin.py) and
prcnn_gt_aug_sample against the reference's own sampling loop (tests/golden/train_input_ref.npz) and the restatement, on single
frames, ragged batches, the accepted-object bound and repeated seeds.  Reads only the fixture and the package."""
import os

import numpy as np
import pytest
import torch

import train_input_twin as tw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "train_input_ref.npz")
DEV = torch.device("cuda")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case_cfg(z, k):
    extra, rand_num, prob, ratio, use_scope = z["c%d_cfg" % k]
    return {"GT_EXTRA_NUM": int(extra), "GT_AUG_RAND_NUM": bool(rand_num), "GT_AUG_APPLY_PROB": float(prob),
            "GT_AUG_HARD_RATIO": float(ratio), "PC_AREA_SCOPE": tuple(z["scope"]) if use_scope else None, "TRY_TIMES": 100}


def _db(z, ratio):
    from pointrcnn_amd.kitti_input import GTDatabase
    off = np.concatenate([[0], np.cumsum(z["db_npts"])])
    pts = [z["db_points"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    inten = [z["db_intensity"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return GTDatabase.from_arrays(z["db_boxes"], z["db_alpha"], pts, inten, hard_ratio=ratio, device=DEV)


def _run(db, gts, planes, cfg, seed, K=16):
    B = len(gts)
    G = max(1, max(len(g) for g in gts))
    gt = np.zeros((B, G, 7), np.float32)
    for b, g in enumerate(gts):
        gt[b, :len(g)] = g
    ng = np.array([len(g) for g in gts], np.int32)
    scope = cfg["PC_AREA_SCOPE"]
    area = None if scope is None else ((scope[0], scope[1]), (scope[2], scope[3]), (scope[4], scope[5]))
    r = db.sample(T(gt), T(ng), T(np.asarray(planes, np.float64).reshape(B, 4)), cfg["GT_EXTRA_NUM"], cfg["GT_AUG_RAND_NUM"],
                  cfg["GT_AUG_APPLY_PROB"], area, cfg["TRY_TIMES"], K, seed)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _boxes(n, rng, spread=6.0):
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = rng.uniform(-spread, spread, n)
    b[:, 1] = rng.uniform(0.5, 2.0, n)
    b[:, 2] = rng.uniform(5, 5 + 2 * spread, n)
    b[:, 3] = rng.uniform(1.0, 2.0, n)
    b[:, 4] = rng.uniform(0.5, 2.0, n)
    b[:, 5] = rng.uniform(1.0, 5.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def test_corner_iou3d_matches_restatement():
    from pointrcnn_amd import ops
    rng = np.random.default_rng(5)
    a = _boxes(48, rng)
    nested = a[:8].copy(); nested[:, 3:6] *= 0.5; nested[:, 1] -= 0.2          # inside a's boxes
    disjoint = a[:8].copy(); disjoint[:, 0] += 40.0
    identical = a[:8].copy()
    edge = a[:8].copy(); edge[:, 0] += edge[:, 5] * np.cos(edge[:, 6]) * 1.0001    # shifted by about one length: near-touching
    b = np.concatenate([_boxes(40, rng), nested, disjoint, identical, edge]).astype(np.float32)
    ca, cb = tw.corners3d(a), tw.corners3d(b)
    degenerate = cb[:2].copy(); degenerate[0, [1, 2, 5, 6]] = degenerate[0, [0, 3, 4, 7]]    # zero-area quad
    cb = np.concatenate([cb, degenerate])
    want3, wantb = tw.corner_iou3d(ca, cb, need_bev=True)
    got3, gotb = (t.cpu().numpy() for t in ops.corner_iou3d(T(ca), T(cb), need_bev=True))
    assert np.array_equal(got3 < np.float32(1e-8), want3 < np.float32(1e-8))
    assert np.allclose(got3, want3, rtol=1e-6, atol=0) and np.allclose(gotb, wantb, rtol=1e-6, atol=0)
    assert (want3 > 0.1).any() and (want3 == 0).any()
    only3 = ops.corner_iou3d(T(ca), T(cb)).cpu().numpy()
    assert np.array_equal(only3, got3)


def test_gt_aug_sample_matches_reference_fixture():
    z = np.load(GOLD)
    for k in range(int(z["ncases"])):
        cfg = _case_cfg(z, k)
        r = _run(_db(z, cfg["GT_AUG_HARD_RATIO"]), [z["c%d_gt" % k]], [z["c%d_plane" % k]], cfg, int(z["c%d_seed" % k]))
        n = int(r["count"][0])
        assert r["status"][0] == int(z["c%d_status" % k]), k
        assert r["stats"][0, 0] == int(z["c%d_applied" % k]), k
        if r["status"][0] == 0:
            assert r["stats"][0, 3] == int(z["c%d_started" % k]), k
        assert np.array_equal(r["db_id"][0, :n], z["c%d_ids" % k]), k
        assert np.array_equal(r["boxes3d"][0, :n].view(np.uint32), z["c%d_boxes" % k].view(np.uint32)), k
        assert np.array_equal(r["alpha"][0, :n], z["c%d_alpha" % k]), k
        assert (r["db_id"][0, n:] == -1).all() and (r["boxes3d"][0, n:] == 0).all()
        want = tw.gt_aug_sample(z["c%d_gt" % k], z["c%d_plane" % k], z["db_boxes"], z["db_alpha"], z["db_npts"], cfg,
                                int(z["c%d_seed" % k]), 0)
        assert np.array_equal(r["y_shift"][0, :n], want["y_shift"]) and tuple(r["stats"][0]) == tuple(want["stats"]), k


def test_gt_aug_sample_ragged_batch_matches_restatement():
    z = np.load(GOLD)
    rng = np.random.default_rng(9)
    cfg = _case_cfg(z, 0)
    gts = [z["c%d_gt" % k] for k in range(int(z["ncases"])) if len(z["c%d_gt" % k])] + [_boxes(int(n), rng) for n in (0, 3, 30, 7)]
    gts[-4] = np.zeros((0, 7), np.float32)
    planes = [(0.0, -1.0, 0.0, 1.65 + 0.01 * b) for b in range(len(gts))]
    db = _db(z, 0.6)
    for seed in (0, 17):
        r = _run(db, gts, planes, cfg, seed)
        for b, g in enumerate(gts):
            want = tw.gt_aug_sample(g, planes[b], z["db_boxes"], z["db_alpha"], z["db_npts"], cfg, seed, b)
            n = int(r["count"][b])
            assert r["status"][b] == want["status"] and tuple(r["stats"][b]) == tuple(want["stats"]), b
            assert np.array_equal(r["db_id"][b, :n], want["ids"]), b
            assert np.array_equal(r["boxes3d"][b, :n], want["boxes"]) and np.array_equal(r["y_shift"][b, :n], want["y_shift"]), b


def test_gt_aug_sample_bound_and_status():
    z = np.load(GOLD)
    cfg = _case_cfg(z, 7)                      # 9 objects accepted in the fixture
    r = _run(_db(z, 0.6), [z["c7_gt"]], [z["c7_plane"]], cfg, int(z["c7_seed"]), K=2)
    assert r["status"][0] == 2 and r["count"][0] == 2
    assert np.array_equal(r["db_id"][0], z["c7_ids"][:2])
    with pytest.raises(ValueError):
        _run(_db(z, 0.6), [np.zeros((250, 7), np.float32)], [z["c0_plane"]], cfg, 0, K=16)      # G + K > 256


def test_gt_aug_sample_seed_determinism():
    z = np.load(GOLD)
    cfg = _case_cfg(z, 1)
    db = _db(z, 0.6)
    gts = [z["c1_gt"]] * 6
    planes = [z["c1_plane"]] * 6
    a, b, c = _run(db, gts, planes, cfg, 3), _run(db, gts, planes, cfg, 3), _run(db, gts, planes, cfg, 4)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not all(np.array_equal(a[k], c[k]) for k in ("db_id", "boxes3d"))
    assert len({tuple(a["db_id"][i]) for i in range(6)}) > 1          # frames draw independently


def test_gt_database_split_and_rejects_empty_lists():
    from pointrcnn_amd.kitti_input import GTDatabase
    z = np.load(GOLD)
    db = _db(z, 0.6)
    npts = z["db_npts"]
    assert np.array_equal(db.easy_idx.cpu().numpy(), np.nonzero(npts > 100)[0])
    assert np.array_equal(db.hard_idx.cpu().numpy(), np.nonzero(npts <= 100)[0])
    assert int(db.offsets[-1]) == db.points.shape[0] == npts.sum()
    big = [np.zeros((150, 3), np.float32)]
    with pytest.raises(ValueError):
        GTDatabase.from_arrays(np.zeros((1, 7), np.float32), [0.0], big, [np.zeros(150, np.float32)], hard_ratio=0.6, device=DEV)
    GTDatabase.from_arrays(np.zeros((1, 7), np.float32), [0.0], big, [np.zeros(150, np.float32)], hard_ratio=0.0, device=DEV)


def test_corner_iou3d_device_matches_analytic_rectangles_and_rejects_bad_quads():
    """the device clip itself against closed-form overlaps: axis-aligned pairs and the same rectangles written as boxes turned by
    90 degrees (corner order permuted, extents swapped); degenerate (zero-width) and bow-tie quads give 0 on either side"""
    from pointrcnn_amd import ops
    rng = np.random.default_rng(21)
    A, B, want3, wantb = [], [], [], []
    for _ in range(400):
        cx, cz, qx, qz = rng.uniform(-5, 5, 4)
        hx, hz, gx, gz = rng.uniform(0.2, 3, 4)
        a = tw.rect_corners(cx, cz, hx, hz, y0=1.0, h=2.0)
        if rng.random() < 0.5:
            b = tw.rect_corners(qx, qz, gz, gx, y0=1.5, h=2.0)[[1, 2, 3, 0, 5, 6, 7, 4]]
        else:
            b = tw.rect_corners(qx, qz, gx, gz, y0=1.5, h=2.0)
        fa, fb = a.astype(np.float64), b.astype(np.float64)
        ox = max(0.0, min(fa[:4, 0].max(), fb[:4, 0].max()) - max(fa[:4, 0].min(), fb[:4, 0].min()))
        oz = max(0.0, min(fa[:4, 2].max(), fb[:4, 2].max()) - max(fa[:4, 2].min(), fb[:4, 2].min()))
        area_a = (fa[:4, 0].max() - fa[:4, 0].min()) * (fa[:4, 2].max() - fa[:4, 2].min())
        area_b = (fb[:4, 0].max() - fb[:4, 0].min()) * (fb[:4, 2].max() - fb[:4, 2].min())
        o = ox * oz
        A.append(a); B.append(b)
        want3.append(o * 1.5 / (area_a * 2.0 + area_b * 2.0 - o * 1.5))      # heights [-1, 1] and [-1.5, 0.5]: overlap 1.5
        wantb.append(o / (area_a + area_b - o))
    A, B = np.stack(A), np.stack(B)
    got3, gotb = ops.corner_iou3d(T(A), T(B), need_bev=True)
    d3 = torch.diagonal(got3).cpu().numpy().astype(np.float64)
    db = torch.diagonal(gotb).cpu().numpy().astype(np.float64)
    want3, wantb = np.asarray(want3), np.asarray(wantb)
    assert np.array_equal(d3 == 0, want3 == 0) and (want3 == 0).any() and (want3 > 0).any()
    assert np.allclose(d3, want3, rtol=1e-6, atol=0) and np.allclose(db, wantb, rtol=1e-6, atol=0)

    sq = tw.rect_corners(0, 0, 1, 1)
    flat = tw.rect_corners(0, 0, 1, 0)                       # zero width
    bow = sq[[0, 2, 1, 3, 4, 6, 5, 7]]                        # self-intersecting corner order
    stacked = tw.rect_corners(0, 0, 1, 1, y0=-1.0, h=1.0)    # touching faces: no height overlap
    bad = np.stack([flat, bow, stacked])
    g3, gb = ops.corner_iou3d(T(np.stack([sq])), T(bad), need_bev=True)
    r3, rb = ops.corner_iou3d(T(bad), T(np.stack([sq])), need_bev=True)
    for t in (g3, gb, r3, rb):
        assert (t == 0).all()
    assert float(ops.corner_iou3d(T(sq[None]), T(sq[None]))[0, 0]) == 1.0


def test_gt_aug_sample_list_outside_database_reports_status():
    from pointrcnn_amd import ops
    z = np.load(GOLD)
    db = _db(z, 0.6)
    D = db.size
    bad_easy = torch.full_like(db.easy_idx, D + 5)           # a list built for another database
    r = ops.gt_aug_sample(T(z["c1_gt"][None]), None, T(np.asarray(z["c1_plane"], np.float64)[None]), db.boxes, db.alpha, db.npts,
                          bad_easy, db.hard_idx, hard_ratio=0.0001, apply_prob=1.0, seed=1)
    assert int(r["status"][0]) == 3 and int(r["count"][0]) == 0
    with pytest.raises(RuntimeError):                       # a database tensor off the device is refused before the launch
        ops.gt_aug_sample(T(z["c1_gt"][None]), None, T(np.asarray(z["c1_plane"], np.float64)[None]), db.boxes.cpu(), db.alpha, db.npts,
                          db.easy_idx, db.hard_idx)
