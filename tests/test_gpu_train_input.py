"""GT-augmentation sampling on the device: prcnn_corner_iou3d against the double restatement (tests/train_input_twin.py) and
prcnn_gt_aug_sample against the reference's own sampling loop (tests/golden/train_input_ref.npz) and the restatement, on single
frames, ragged batches, the accepted-object bound and repeated seeds; both kernels against the exact rational reference
(tests/exact_quad.py) on the adversarial families, car parks and rows of tests/quad_families.py, and the sampler's collision list
at its capacity.  Reads only the fixture and the package."""
import os
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import torch

import exact_quad as xq
import quad_families as qf
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
    fams = qf.families()                                  # exact contact (the `edge` rows above leave a 0.4 mm gap)
    for name in ["parking_rows"] + [w + k for w in ("near_", "far_") for k in qf.TOUCHING]:
        f = fams[name]
        want3, wantb = tw.corner_iou3d(f.ca, f.cb, need_bev=True)
        got3, gotb = (t.cpu().numpy() for t in ops.corner_iou3d(T(f.ca), T(f.cb), need_bev=True))
        assert np.array_equal(got3 < np.float32(1e-8), want3 < np.float32(1e-8)), name
        _close_to_twin(got3, want3, name)
        _close_to_twin(gotb, wantb, name)


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


# ------------------------------------------------------------------------------------------------ against the exact reference
THR = np.float32(1e-8)
PLANE = (0.0, -1.0, 0.0, 1.65)


def _close_to_twin(got, want, what):
    """kernel and twin are each within 2^-23 * exact + 1e-12 of the exact value (tests/test_quad_exact_cpu.py derives that bar), so
    they are within twice that of each other; the twin stands for the exact value in the bound at a relative cost of 2^-23"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.abs(got - want) > 2.0 * (want * (2.0 ** -23) * (1 + 2.0 ** -22) + 1e-12)
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _check_exact(name, got, want):
    """got fp32 values, want Fractions, same order: prints the worst errors, then |got - exact| <= 2^-23 * exact + 1e-12"""
    worst_rel = worst_abs = 0.0
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        d = abs(Fraction(float(g)) - w)
        worst_abs = max(worst_abs, float(d))
        if w > 0:
            worst_rel = max(worst_rel, float(d / w))
        if d > w / 2 ** 23 + Fraction(1, 10 ** 12):
            bad.append((i, float(g), float(w)))
    print("%-28s worst rel %.2e abs %.2e" % (name, worst_rel, worst_abs))
    assert not bad, (name, bad[:5])


def _same_decisions(name, got3, want3):
    flips = [i for i, (g, w) in enumerate(zip(got3, want3)) if (np.float32(g) < THR) != (np.float32(float(w)) < THR)]
    assert not flips, (name, flips[:5])


@lru_cache(maxsize=None)
def _family_cross_exact():
    """{family: (ca (n,8,3), cb (n+5,8,3), [[(iou3d, bev)]] exact for every pair)}: cb is the family's b side plus five of its a side"""
    qf.check_liveness()
    out = {}
    for name, f in qf.families().items():
        cb = np.concatenate([f.cb, f.ca[:5]])
        out[name] = (f.ca, cb, [[xq.exact_iou(a, b) for b in cb] for a in f.ca])
    return out


def test_corner_iou3d_matches_exact_on_every_family():
    from pointrcnn_amd import ops
    for name, (ca, cb, want) in _family_cross_exact().items():
        assert ca.shape[0] != cb.shape[0]
        got3, gotb = (t.cpu().numpy() for t in ops.corner_iou3d(T(ca), T(cb), need_bev=True))
        flat = [w for row in want for w in row]
        _check_exact(name + " iou3d", got3.ravel(), [w[0] for w in flat])
        _check_exact(name + " bev", gotb.ravel(), [w[1] for w in flat])
        _same_decisions(name, got3.ravel(), [w[0] for w in flat])


@lru_cache(maxsize=None)
def _tiled_pool():
    """62 corner sets per side drawn from every family (every ninth pair), the twin's IoUs of all 62 x 62 pairs, and the row and
    column index of each of 1500 x 1500 tiled entries"""
    fams = qf.families()
    pick = np.arange(0, sum(len(f.ca) for f in fams.values()), 9)
    pa = np.concatenate([f.ca for f in fams.values()])[pick]
    pb = np.concatenate([f.cb for f in fams.values()])[pick]
    t3, tb = tw.corner_iou3d(pa, pb, need_bev=True)
    rng = np.random.default_rng(77)
    ia, ib = rng.integers(0, len(pick), 1500), rng.integers(0, len(pick), 1500)
    ia[:len(pick)], ib[:len(pick)] = np.arange(len(pick)), np.arange(len(pick))      # the families' own pairs are on the diagonal
    sample = np.stack([rng.integers(0, 1500, 5000), rng.integers(0, 1500, 5000)], 1)
    sample[:len(pick)] = np.arange(len(pick))[:, None]
    memo = {}
    want = []
    for i, j in sample:
        key = (int(ia[i]), int(ib[j]))
        if key not in memo:
            memo[key] = xq.exact_iou(pa[key[0]], pb[key[1]])
        want.append(memo[key])
    return pa, pb, t3, tb, ia, ib, sample, want


def test_corner_iou3d_grid_stride_on_1500_by_1500():
    """N * M = 2 250 000 > 8192 * 256 threads: the grid-stride loop takes a second step; every entry against the twin, a seeded
    sample of 5 000 against the exact reference"""
    from pointrcnn_amd import ops
    pa, pb, t3, tb, ia, ib, sample, want = _tiled_pool()
    assert 1500 * 1500 > 8192 * 256
    got3, gotb = (t.cpu().numpy() for t in ops.corner_iou3d(T(pa[ia]), T(pb[ib]), need_bev=True))
    full3, fullb = t3[ia][:, ib], tb[ia][:, ib]
    assert np.array_equal(got3 < THR, full3 < THR)
    _close_to_twin(got3, full3, "iou3d")
    _close_to_twin(gotb, fullb, "bev")
    assert (full3 > 0.1).mean() > 0.02 and (full3 == 0).mean() > 0.2
    s3, sb = got3[sample[:, 0], sample[:, 1]], gotb[sample[:, 0], sample[:, 1]]
    _check_exact("1500x1500 sample iou3d", s3, [w[0] for w in want])
    _check_exact("1500x1500 sample bev", sb, [w[1] for w in want])
    _same_decisions("1500x1500 sample", s3, [w[0] for w in want])
    assert sum(w[0] > 0 for w in want) >= 500


def _cfg(extra, tries):
    return {"GT_EXTRA_NUM": extra, "GT_AUG_RAND_NUM": False, "GT_AUG_APPLY_PROB": 1.0, "GT_AUG_HARD_RATIO": 0.0, "PC_AREA_SCOPE": None,
            "TRY_TIMES": tries}


class _ExactIou:
    """the sampler twin's iou= callable: the exact iou3d rounded to fp32; remembers what it was asked"""

    def __init__(self):
        self.values, self.near_misses, self.touching = [], 0, 0

    def __call__(self, a, b):
        v = xq.exact_iou(a, b)[0]
        self.values.append(v)
        if v == 0 and xq.near_miss(a, b, 1e-4):
            self.near_misses += 1
            self.touching += xq.quad_gap(a, b) == 0.0
        return np.float32(float(v))


def _sample(gt, num_gt, db, cfg, seed, K):
    """ops.gt_aug_sample on (B,G,7) scene boxes with a plain database (no easy / hard split, every object has 50 points)"""
    from pointrcnn_amd import ops
    B = gt.shape[0]
    r = ops.gt_aug_sample(T(gt), None if num_gt is None else T(np.asarray(num_gt, np.int32)), T(np.tile(np.asarray(PLANE, np.float64), (B, 1))),
                          T(db), T(np.zeros(len(db), np.float32)), T(np.full(len(db), 50, np.int32)), None, None,
                          extra_num=cfg["GT_EXTRA_NUM"], rand_num=False, apply_prob=1.0, hard_ratio=0.0, area_scope=None,
                          try_times=cfg["TRY_TIMES"], max_accept=K, seed=seed)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _exact_twin(scene, db, cfg, seed, frame, K):
    rec = _ExactIou()
    want = tw.gt_aug_sample(scene, PLANE, db, np.zeros(len(db), np.float32), np.full(len(db), 50), cfg, seed, frame, max_accept=K, iou=rec)
    return want, rec


def _assert_frame(r, b, want, what=None):
    what = (what, b)
    n = int(r["count"][b])
    assert r["status"][b] == want["status"] and tuple(r["stats"][b]) == tuple(want["stats"]), what
    assert np.array_equal(r["db_id"][b, :n], want["ids"]), what
    assert np.array_equal(r["boxes3d"][b, :n].view(np.uint32), want["boxes"].view(np.uint32)), what
    assert np.array_equal(r["y_shift"][b, :n], want["y_shift"]), what
    assert (r["db_id"][b, n:] == -1).all(), what


@lru_cache(maxsize=None)
def _parking_case():
    scene, db = qf.parking_scene(11, 120, 240)
    cfg = _cfg(60, 150)
    return scene, db, cfg, [_exact_twin(scene, db, cfg, 5, b, 64) for b in range(6)]


def test_gt_aug_sample_parking_rows_match_exact_twin():
    """ry = 0: no cosine anywhere.  A candidate either touches its neighbours exactly (exact IoU 0: accept) or overlaps one by
    2^-10 m or more (reject); everything equal to the twin that decides by the exact IoU, bit for bit"""
    scene, db, cfg, wants = _parking_case()
    r = _sample(np.tile(scene[None], (6, 1, 1)), None, db, cfg, 5, 64)
    accepted = rejected = touching = slight = 0
    for b, (want, rec) in enumerate(wants):
        _assert_frame(r, b, want, "parking")
        accepted += len(want["ids"])
        rejected += want["stats"][2] - len(want["ids"])
        touching += rec.touching
        slight += sum(0 < v < Fraction(1, 1000) for v in rec.values)
    assert accepted >= 60 and rejected >= 60 and touching >= 100 and slight >= 10, (accepted, rejected, touching, slight)


ROWS_SEED = 2          # the first seed tried after 1 whose region stays inside x <= 38.6; seeds 1..7 all meet the input condition


@lru_cache(maxsize=None)
def _rows_case():
    scenes, db, theta = qf.rows_scene(ROWS_SEED)
    cfg = _cfg(90, 100)
    return scenes, db, cfg, [_exact_twin(sc, db, cfg, ROWS_SEED, b, 64) for b, sc in enumerate(scenes)]


def test_gt_aug_sample_rotated_rows_at_the_far_corner_match_exact_twin():
    """Input condition (asserted): no pair the exact twin evaluates has an exact IoU in [1e-10, 1e-6], nor a gap under 0.1 mm.
    Inside that band, and for such gaps, the verdict hangs on the last bit of cosf / sinf in the corners, which numpy builds do
    not share; outside it the device must decide every pair as the exact IoU does, none left out"""
    scenes, db, cfg, wants = _rows_case()
    lo, hi = Fraction(1, 10 ** 10), Fraction(1, 10 ** 6)
    accepted = rejected = 0
    for want, rec in wants:
        assert not any(lo <= v <= hi for v in rec.values) and rec.near_misses == 0
        accepted += len(want["ids"])
        rejected += want["stats"][2] - len(want["ids"])
    assert accepted >= 10 * len(scenes) and rejected >= 30 * len(scenes), (accepted, rejected)
    assert max(np.abs(sc[:, 0]).max() for sc in scenes) > 36 and max(sc[:, 2].max() for sc in scenes) > 66
    r = _sample(np.stack(scenes), None, db, cfg, ROWS_SEED, 64)
    for b, (want, _) in enumerate(wants):
        _assert_frame(r, b, want, "rows")


@pytest.mark.parametrize("at", [0, 63, 64, 127, 191])
def test_gt_aug_sample_collision_at_list_index(at):
    """G = 192, K = 64: the list fills the LDS, a lane walks it in up to four steps.  The only entry the candidate overlaps (by
    2^-10 m; its other neighbours touch it exactly) sits at index `at`: every try must be rejected"""
    scene, free, nudged, _ = qf.capacity_scene(1, at)
    cfg = _cfg(10, 3)
    r = _sample(scene[None], None, nudged[None], cfg, 9, 64)
    want, rec = _exact_twin(scene, nudged[None], cfg, 9, 0, 64)
    assert len(want["ids"]) == 0 and want["stats"][2] == 3
    assert len(rec.values) == 3 * (at + 1)                  # the twin stops at the hit: the entries before it are all clear
    assert [i for i, v in enumerate(rec.values[:at + 1]) if v > 0] == [at]
    _assert_frame(r, 0, want, "list index")
    assert r["count"][0] == 0


def test_gt_aug_sample_most_recent_slot_rejects():
    """the same scene, the candidate exactly on the free slot: accepted once, into list entry 192, and from then on rejected by
    that entry alone; then several free slots in turn, each rejected by its own entry (192, 193, ...)"""
    scene, free, _, spare = qf.capacity_scene(1, 0)
    cfg = _cfg(10, 4)
    r = _sample(scene[None], None, free[None], cfg, 9, 64)
    want, _ = _exact_twin(scene, free[None], cfg, 9, 0, 64)
    assert len(want["ids"]) == 1 and want["stats"][2] == 4
    _assert_frame(r, 0, want, "own slot")
    db = np.concatenate([free[None], spare[:5]])
    cfg = _cfg(60, 40)
    r = _sample(scene[None], None, db, cfg, 3, 64)
    want, _ = _exact_twin(scene, db, cfg, 3, 0, 64)
    assert len(want["ids"]) == 6 and want["stats"][2] == 40
    _assert_frame(r, 0, want, "own slots")


def test_gt_aug_sample_fills_64_slots_then_reports_status_2():
    scene, free, _, spare = qf.capacity_scene(2, 17)
    db = np.concatenate([free[None], spare[:99]])
    cfg = _cfg(2000, 1000)
    want, _ = _exact_twin(scene, db, cfg, 21, 0, 64)
    assert want["status"] == 2 and len(want["ids"]) == 64 and want["stats"][2] > 65
    r = _sample(scene[None], None, db, cfg, 21, 64)
    _assert_frame(r, 0, want, "full")
    assert r["count"][0] == 64 and r["status"][0] == 2
    with pytest.raises(ValueError):                         # G + K = 257
        _sample(np.concatenate([scene, scene[:1]])[None], None, db, cfg, 21, 64)


def test_gt_aug_sample_ragged_num_gt_is_clamped():
    scene, db = qf.parking_scene(12, 192, 200)
    cfg = _cfg(40, 60)
    num_gt = [0, 1, 100, 192, 500, -3]
    r = _sample(np.tile(scene[None], (len(num_gt), 1, 1)), num_gt, db, cfg, 2, 64)
    for b, n in enumerate(num_gt):
        want, _ = _exact_twin(scene[:min(max(n, 0), 192)], db, cfg, 2, b, 64)
        _assert_frame(r, b, want, "ragged")
    assert r["status"][0] == 1 and r["status"][5] == 1 and r["count"][2] > r["count"][3] > 0


@lru_cache(maxsize=None)
def _batch_case():
    scene, db = qf.parking_scene(13, 40, 120)
    cfg = _cfg(25, 30)
    return scene, db, cfg, [_exact_twin(scene, db, cfg, 8, b, 16)[0] for b in range(64)]


def test_gt_aug_sample_64_frames_equal_one_frame_at_a_time():
    """A frame's draws are keyed by its index in the launch, so "one frame at a time" is a launch of b + 1 frames of which only the
    last has a scene (the others raise at once, status 1): frame b must not depend on what its neighbours do"""
    scene, db, cfg, wants = _batch_case()
    gt = np.tile(scene[None], (64, 1, 1))
    r = _sample(gt, None, db, cfg, 8, 16)
    for b in range(64):
        _assert_frame(r, b, wants[b], "batch")
        one = _sample(gt[:b + 1], [0] * b + [len(scene)], db, cfg, 8, 16)
        for k in r:
            assert np.array_equal(one[k][b], r[k][b]), (k, b)
        assert (one["status"][:b] == 1).all()
    assert len({tuple(r["db_id"][b]) for b in range(64)}) > 32


@lru_cache(maxsize=None)
def _shortcut_frames():
    """2 000 (candidate, scene box) pairs from the touching / collinear families and the parking rows.  Not generated: pairs with an
    exact IoU in [1e-10, 1e-6], and turned pairs (ry != 0) that miss each other by less than 0.1 mm -- for both the verdict hangs on
    the last bit of cosf / sinf in the corners (the device's cosf is not numpy's for about one angle in ten).
    Exact contact stays in through the parking rows (ry = 0: no cosine), near contact through overlaps and gaps of 1 mm .. 10 cm.
    Frame b of a launch with this seed tries candidate pick[b] first, so its scene is that candidate's partner"""
    fams = qf.families(seed=4, n=400)
    names = [w + k for w in ("near_", "far_") for k in qf.TOUCHING] + ["parking_rows"]
    a = np.concatenate([fams[k].a for k in names])
    b = np.concatenate([fams[k].b for k in names])
    a[:, 1] = b[:, 1] = np.float32(1.65)
    cfg = _cfg(10, 1)
    lo, hi = Fraction(1, 10 ** 10), Fraction(1, 10 ** 6)
    keep, value, contact = [], [], 0
    for i in np.random.default_rng(4).permutation(len(a)):
        want, rec = _exact_twin(qf.sampler_boxes(b[i:i + 1]), qf.sampler_boxes(a[i:i + 1]), cfg, 0, 0, 1)
        v = rec.values[0]
        assert (len(want["ids"]) == 1) == (np.float32(float(v)) < THR)
        if lo <= v <= hi or (rec.near_misses and not (a[i, 6] == 0 and b[i, 6] == 0)):
            continue
        keep.append(i)
        value.append(v)
        contact += rec.touching
        if len(keep) == 2000:
            break
    assert len(keep) == 2000 and contact >= 50
    db, partner = qf.sampler_boxes(a[keep]), qf.sampler_boxes(b[keep])
    pick = np.array([tw.below(tw.rand32(6, tw.STREAM_INDEX, f, 0), 2000) for f in range(2000)])
    return db, partner[pick], [value[p] for p in pick]


def test_gt_aug_sample_shortcut_never_overrules_the_exact_iou():
    """the separating-axis shortcut through the public surface: one scene box, one try; accepted iff the exact IoU < 1e-8"""
    db, scene, value = _shortcut_frames()
    want = np.array([np.float32(float(v)) < THR for v in value])
    assert want.sum() >= 300 and (~want).sum() >= 300
    assert sum(v == 0 for v in value) >= 200 and sum(Fraction(1, 10 ** 6) < v < Fraction(1, 100) for v in value) >= 200
    r = _sample(scene[:, None, :], None, db, _cfg(10, 1), 6, 1)
    assert (r["status"] == 0).all() and (r["stats"][:, 2] == 1).all()
    wrong = np.nonzero((r["count"] == 1) != want)[0]
    assert len(wrong) == 0, [(int(f), float(value[f])) for f in wrong[:10]]
