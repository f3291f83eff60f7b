"""iou3d_geom.h: cannot_exceed -- the overlap bound that lets a rotated-NMS threshold decision skip the polygon clip (round 6), and
far_apart, the circumscribed-circle test that skips pairs of exactly zero overlap.

Both are restated in numpy float32, operation for operation, with the kernels' cos / sin (tests/collinear_boxes.py), and held against
the ORACLE's overlaps (the reference's clip restated in C, pinned to the reference's own sources compiled for the host): the bound must
never decide a pair the clip would decide the other way, and it must never fall below the clip's overlap by more than rounding -- on
continuous random boxes, and on the families with collinear edges where the clip is NOT the true overlap.  The GPU tests
(tests/test_gpu_nms_degenerate.py, test_gpu_proposal.py, test_gpu_roipool_iou.py, test_gpu_parity_residuals.py) hold the kernels that
USE it to the oracle's keep lists."""
import numpy as np
import pytest

from collinear_boxes import (FAR, FLIP_SETS, HEADING_DELTAS, JITTERS, KINDS, SEED_PAIR, cannot_exceed, family_bev, family_boxes3d,
                             far_apart, flip_set, greedy_nms_with_skip, overlap_bound)
from rcnn_bev import bev

f = np.float32
THRESHOLDS = (0.85, 0.8, 0.7, 0.3, 0.1)


def _boxes(rng, n, spread, clusters, shift=(0.0, 0.0)):
    ctr = rng.uniform([-spread, 0], [spread, 2 * spread], (n, 2))
    l = rng.uniform(3.2, 4.6, n) * rng.choice([1, 1, 1, 0.3], n)
    w = rng.uniform(1.4, 1.9, n) * rng.choice([1, 1, 1, 2.0], n)
    ang = rng.uniform(-np.pi, np.pi, n)
    if clusters:          # eight near-copies of every box, as an RPN emits around one object (incl. heading flips)
        k = n // 8
        base = np.concatenate([ctr[:k], l[:k, None], w[:k, None], ang[:k, None]], 1)
        rep = np.repeat(base, 8, 0) + rng.normal(0, 1, (8 * k, 5)) * np.array([0.3, 0.3, 0.2, 0.1, 0.08])
        rep[::5, 4] += np.pi
        ctr, l, w, ang = rep[:, :2], np.abs(rep[:, 2]) + 0.1, np.abs(rep[:, 3]) + 0.1, rep[:, 4]
    out = np.stack([ctr[:, 0] - l / 2, ctr[:, 1] - w / 2, ctr[:, 0] + l / 2, ctr[:, 1] + w / 2, ang], 1).astype(f)
    out[:, [0, 2]] += f(shift[0]); out[:, [1, 3]] += f(shift[1])
    return out


def _above_bound(ov, u):
    return ov > u * f(1.0001) + f(1e-4)


@pytest.mark.parametrize("name,n,spread,clusters,shift", [("scattered", 400, 20, False, (0, 0)), ("dense", 400, 4, False, (0, 0)),
                                                        ("clusters", 400, 15, True, (0, 0)), ("far from the origin", 400, 4, False, (70, 35))])
def test_bound_never_decides_against_the_clip(cpu, name, n, spread, clusters, shift):
    rng = np.random.default_rng(7)
    B = _boxes(rng, n, spread, clusters, shift)
    ov, iou = cpu.boxes_overlap_bev(B, B), cpu.boxes_iou_bev(B, B)
    u, sa, sb, ok = overlap_bound(B, B, cpu=cpu)
    assert not _above_bound(ov, u).any(), "the bound fell below the clip's overlap by more than rounding"
    decided = 0
    for thr in THRESHOLDS:
        skip = cannot_exceed(u, sa, sb, ok, thr)
        assert not (skip & (iou > thr)).any(), (name, thr)
        assert iou[skip].max(initial=0.0) < 0.9 * thr + 1e-3       # what is skipped is below the threshold with the margin the comment states
        decided = max(decided, (skip & (ov > 0)).sum() / max(1, (ov > 0).sum()))
    assert decided > 0.5                                        # and it does decide most overlapping pairs (else it is dead code)
    assert not (far_apart(B, B, cpu=cpu) & (ov != 0)).any()


@pytest.mark.parametrize("shift", [(0.0, 0.0), FAR], ids=["origin", "far"])
@pytest.mark.parametrize("kind", KINDS)
def test_bound_on_collinear_families(cpu, kind, shift):
    """(a) wherever the guarded bound may decide a pair, the clip's overlap is at most the bound (+ rounding); (b) no pair it skips has a
    clip IoU above the threshold; (c) far_apart implies a clip overlap of exactly 0 (proposal_target.hip and the NMS kernels skip the clip
    there); over every perturbation from exact alignment and two seeds.  The next test shows (a) is not vacuous."""
    for jit in JITTERS:
        for dth in HEADING_DELTAS:
            for seed in range(2):
                B = family_bev(kind, seed, jit, dth, shift)
                ov, iou = cpu.boxes_overlap_bev(B, B), cpu.boxes_iou_bev(B, B)
                u, sa, sb, ok = overlap_bound(B, B, cpu=cpu)
                where = (kind, jit, dth, seed)
                assert not (ok & _above_bound(ov, u)).any(), where                                       # (a)
                for thr in THRESHOLDS:
                    skip = cannot_exceed(u, sa, sb, ok, thr) | far_apart(B, B, cpu=cpu)
                    assert not (skip & (iou > thr)).any(), where + (thr,)                                  # (b)
                assert not (far_apart(B, B, cpu=cpu) & (ov != 0)).any(), where                             # (c)


def test_the_unguarded_bound_fails_on_the_families(cpu):
    """(d) liveness: the round-6 bound (no collinearity guard) does fall below the clip's overlap on these families -- (a) above is not
    vacuous -- and on the seed pair it decides against the clip at RCNN.NMS_THRESH"""
    bad = {}
    for kind in KINDS:
        for shift in ((0.0, 0.0), FAR):
            for jit in JITTERS:
                for dth in HEADING_DELTAS:
                    for seed in range(2):
                        B = family_bev(kind, seed, jit, dth, shift)
                        u, sa, sb, ok = overlap_bound(B, B, guard=None, cpu=cpu)
                        bad[kind] = bad.get(kind, 0) + int((ok & _above_bound(cpu.boxes_overlap_bev(B, B), u)).sum())
    assert sum(bad.values()) > 0 and sum(v > 0 for v in bad.values()) >= 4, bad
    X = SEED_PAIR
    iou = cpu.boxes_iou_bev(X, X)
    u, sa, sb, ok = overlap_bound(X, X, guard=None, cpu=cpu)
    assert cannot_exceed(u, sa, sb, ok, 0.1)[0, 1] and iou[0, 1] > 0.1
    u, sa, sb, ok = overlap_bound(X, X, cpu=cpu)
    assert not ok[0, 1] and not cannot_exceed(u, sa, sb, ok, 0.1)[0, 1]


def test_flip_sets_change_the_keep_list_without_the_guard(cpu):
    """the GPU test's sets are sensitive: the greedy keep list at 0.1 with the unguarded bound's skips differs from the reference's
    (for the 3-D sets, on the BEV the kernels compute), and with the guard it is the reference's"""
    for kind, seed, shift, form in FLIP_SETS:
        B = flip_set(kind, seed, shift, form)
        X = B if form == "bev" else bev(B)
        iou, want = cpu.boxes_iou_bev(X, X), cpu.nms(X, 0.1)
        for guard, same in ((None, False), ("default", True)):
            u, sa, sb, ok = overlap_bound(X, X, cpu=cpu) if guard else overlap_bound(X, X, guard=None, cpu=cpu)
            got = greedy_nms_with_skip(iou, cannot_exceed(u, sa, sb, ok, 0.1), 0.1)
            assert np.array_equal(got, want) == same, (kind, seed, form, guard)


def test_3d_families_keep_their_collinear_bev(cpu):
    """nms_batched and the proposal layer take (x, y, z, h, w, l, ry) boxes: the families built in 3-D keep collinear edges in the BEV
    the kernels derive (kitti_utils.boxes3d_to_bev), where the unguarded bound again falls below the clip"""
    bad = 0
    for kind in KINDS:
        for seed, jit in ((0, 0.0), (1, 0.0), (2, 0.0), (3, 1e-6), (4, 1e-6), (5, 1e-3)):
            X = bev(family_boxes3d(kind, seed, jit, shift=FAR if seed % 2 else (0.0, 0.0)))
            u, sa, sb, ok = overlap_bound(X, X, guard=None, cpu=cpu)
            ov = cpu.boxes_overlap_bev(X, X)
            bad += int((ok & _above_bound(ov, u)).sum())
            u, sa, sb, ok = overlap_bound(X, X, cpu=cpu)
            assert not (ok & _above_bound(ov, u)).any(), (kind, seed)
    assert bad > 0
