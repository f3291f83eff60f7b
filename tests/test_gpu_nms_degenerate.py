"""Every rotated-NMS entry point against the oracle on boxes with collinear edges (tests/collinear_boxes.py), where the reference's clip
is NOT the true overlap and an overlap bound that trusts it (iou3d_geom.h: cannot_exceed) would skip pairs the reference suppresses;
and the LDS boundaries of the batched NMS (proposal.hip: which kernel runs, and where a request is refused)."""
import numpy as np
import pytest
import torch

from collinear_boxes import (FAR, FLIP_SETS, SEED_PAIR, SEED_PAIR_3D_OF, cannot_exceed, family_bev, family_boxes3d, greedy_nms_with_skip,
                             overlap_bound)
from rcnn_bev import bev

pytestmark = pytest.mark.gpu

f = np.float32


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _unguarded_keep(cpu, X, thresh):
    """the greedy keep list of a kernel whose bound skips collinear pairs (the round-6 cannot_exceed)"""
    u, sa, sb, ok = overlap_bound(X, X, guard=None, cpu=cpu)
    return greedy_nms_with_skip(cpu.boxes_iou_bev(X, X), cannot_exceed(u, sa, sb, ok, thresh), thresh)


def _nms_sorted(X, thresh, dev):
    from pointrcnn_amd import ops
    keep, num = ops.nms_sorted(_t(X, dev), thresh)
    return keep.cpu().numpy()[:int(num.cpu()[0])]


def _nms_batched_both(boxes3d, sc, thresh, max_keep=0, rotated=True):
    from pointrcnn_amd import _cabi, ops
    out = {}
    for flag in ("1", "0"):
        with _cabi.switches(PRCNN_NMS_PREFILTER=flag):
            k, n = ops.nms_batched(boxes3d, sc, None, thresh, rotated, max_keep=max_keep)
            out[flag] = (k.cpu().numpy(), n.cpu().numpy())
    return out


def test_seed_pair_through_nms_sorted_and_the_dropin(dev, cpu):
    import iou3d_cuda
    import oracle
    X = SEED_PAIR
    assert np.array_equal(cpu.nms(X, 0.1), [0])
    if oracle.ref() is not None:
        assert np.array_equal(oracle.ref().nms(X, 0.1), [0])
    assert np.array_equal(_unguarded_keep(cpu, X, 0.1), [0, 1])           # what the unguarded bound keeps
    assert np.array_equal(_nms_sorted(X, 0.1, dev), [0])
    keep = torch.zeros((2,), dtype=torch.int64)
    n = iou3d_cuda.nms_gpu(_t(X, dev), keep, 0.1)
    assert n == 1 and int(keep[0]) == 0


def test_seed_pair_through_nms_batched(dev, cpu):
    kind, seed, (i, j) = SEED_PAIR_3D_OF
    P = family_boxes3d(kind, seed)[[i, j]][None]
    sc = np.array([[1.0, 0.5]], f)
    assert np.array_equal(_unguarded_keep(cpu, bev(P[0]), 0.1), [0, 1])   # the BEV the kernel computes is collinear (checked, not assumed)
    ok, on = cpu.nms_batched(P, sc, None, 0.1)
    assert on.tolist() == [1] and ok.tolist() == [[0, -1]]
    for flag, (k, n) in _nms_batched_both(_t(P, dev), _t(sc, dev), 0.1).items():
        assert np.array_equal(n, on) and np.array_equal(k, ok), flag


# the flip sets (tests/test_overlap_bound.py: without the guard their keep lists at 0.1 differ) and a handful of the other families, as BEV boxes (nms_sorted) and as 3-D boxes (nms_batched, the proposal layer)
CASES = [("flip", k, s, sh) for k, s, sh, _ in FLIP_SETS] + [
    ("along", 0, 0.0, 0.0, (0.0, 0.0)), ("along", 1, 1e-6, 0.0, FAR), ("end_to_end", 1, 1e-3, 0.0, FAR),
    ("side_by_side", 0, 1e-6, 1e-6, (0.0, 0.0)), ("perpendicular", 0, 0.0, 0.0, FAR), ("grid", 0, 0.0, 0.0, (0.0, 0.0)),
    ("grid", 1, 1e-7, 1e-4, FAR), ("duplicates", 0, 0.0, 0.0, (0.0, 0.0))]


def _case(c):
    if c[0] == "flip":
        return family_bev(c[1], c[2], shift=c[3]), family_boxes3d(c[1], c[2], shift=c[3])
    kind, seed, jit, dth, shift = c
    return family_bev(kind, seed, jit, dth, shift), family_boxes3d(kind, seed, jit, dth, shift)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_family_sets_every_entry_point_equals_the_oracle(dev, cpu, case):
    import oracle
    from pointrcnn_amd import _cabi, ops
    X, B3 = _case(case)
    n = X.shape[0]
    sc = np.linspace(1.0, 0.0, n, dtype=f)[None]              # sorted order == row order (no ties)
    for thresh in (0.1, 0.3, 0.8, 0.85, -1.0):
        assert np.array_equal(_nms_sorted(X, thresh, dev), cpu.nms(X, thresh)), thresh
        ok, on = cpu.nms_batched(B3[None], sc, None, thresh)
        for flag, (k, nk) in _nms_batched_both(_t(B3[None], dev), _t(sc, dev), thresh).items():
            assert np.array_equal(nk, on) and np.array_equal(k, ok), (thresh, flag)
        for flag in ("1", "0"):
            with _cabi.switches(PRCNN_NMS_PREFILTER=flag):
                rois, scores, cnt = ops.proposal_layer(_t(sc, dev), _t(B3[None], dev), (6300, 2700), (70, 30), thresh, rotated=True)
                o = cpu.proposal_layer(sc, B3[None], (6300, 2700), (70, 30), thresh, "rotated")
                assert np.array_equal(cnt.cpu().numpy(), o[2]) and np.array_equal(rois.cpu().numpy(), o[0]), (thresh, flag)
                assert np.array_equal(scores.cpu().numpy(), o[1]), (thresh, flag)
    # the pair kernels: bit for bit
    Xd, Bd = _t(X, dev), _t(B3, dev)
    ov, iou = ops.boxes_overlap_bev(Xd, Xd).cpu().numpy(), ops.boxes_iou_bev(Xd, Xd).cpu().numpy()
    assert np.array_equal(ov, cpu.boxes_overlap_bev(X, X)) and np.array_equal(iou, cpu.boxes_iou_bev(X, X))
    assert np.array_equal(ops.boxes_iou3d(Bd, Bd).cpu().numpy(), cpu.boxes_iou3d(B3, B3))
    ref = oracle.ref()
    if ref is not None:
        assert np.array_equal(ov, ref.boxes_overlap_bev(X, X)) and np.array_equal(iou, ref.boxes_iou_bev(X, X))


# ---- LDS boundaries of the batched NMS (proposal.hip: *_lds_bytes, LDS_BUDGET) ----
# the dynamic LDS of each kernel, restated from its struct sizes: RBox is 21 floats (x1, y1, x2, y2, cx, cy, c, s, cn, sn, p[5] as
# (x, y), rad), NBox 5; NMS_RT threads (and candidates per batch) of the prefiltered kernels, PAIR_CAP pair-list entries (rotated)
RBOX, NBOX, NMS_RT, PAIR_CAP, LDS_BUDGET = 21 * 4, 5 * 4, 1024, 4096, 150 * 1024
LDS = {
    ("rotated", "prefilter"): lambda mk: 64 * 8 + 4 * 8 + 32 * 4 + PAIR_CAP * 4 + NMS_RT * 4 + (64 + NMS_RT + mk) * RBOX,
    ("rotated", "chunk"): lambda mk: 64 * 8 + 4 * 8 + 4 * 4 + PAIR_CAP * 4 + (64 + mk) * RBOX,
    ("normal", "prefilter"): lambda mk: 64 * 8 + 4 * 8 + 32 * 4 + NMS_RT * 4 + (64 + NMS_RT + mk) * NBOX,
    ("normal", "chunk"): lambda mk: 64 * 8 + 4 * 8 + 4 * 4 + (64 + mk) * NBOX,
}


def _largest_max_keep(key):
    fn = LDS[key]
    mk = 0
    while fn(mk + 1) <= LDS_BUDGET:
        mk += 1
    return mk


def test_lds_boundaries_as_documented():
    got = {k: _largest_max_keep(k) for k in LDS}
    assert got == {("rotated", "prefilter"): 488, ("rotated", "chunk"): 1562, ("normal", "prefilter"): 6353, ("normal", "chunk"): 7588}


def _scattered(M, seed):
    """M boxes on a lattice 7 m apart (all kept) except every eighth, a near copy of its predecessor (suppressed at any threshold here)"""
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(M)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:M] * 7.0
    boxes = np.stack([g[:, 0] - 150, np.ones(M), g[:, 1] + 2, r.uniform(1.4, 1.7, M), r.uniform(1.5, 1.8, M), r.uniform(3.4, 4.4, M),
                      r.uniform(-np.pi, np.pi, M)], 1)
    boxes[8::8] = boxes[7::8][:len(boxes[8::8])] + np.array([0.05, 0, 0.05, 0, 0, 0, 0.02])
    return boxes.astype(f)[None], r.permutation(M).astype(f)[None]


@pytest.mark.parametrize("kind,edge", [("rotated", "prefilter"), ("rotated", "chunk"), ("normal", "prefilter"), ("normal", "chunk")])
def test_nms_batched_on_both_sides_of_each_lds_boundary(dev, cpu, kind, edge):
    """max_keep at the boundary and one above: the prefiltered kernels fall back to the chunk kernel (same keep lists), the chunk
    kernels refuse with PRCNN_EUNSUPPORTED"""
    from pointrcnn_amd import _cabi, ops
    from pointrcnn_amd._cabi import PointOpsError
    mk = _largest_max_keep((kind, edge))
    M = mk + mk // 6 + 64
    boxes, sc = _scattered(M, seed=mk)
    ok_at, on_at = cpu.nms_batched(boxes, sc, None, 0.1, kind, max_keep=mk)
    assert on_at[0] == mk                                       # the kept list really fills up to max_keep
    for flag, (k, n) in _nms_batched_both(_t(boxes, dev), _t(sc, dev), 0.1, mk, kind == "rotated").items():
        assert np.array_equal(n, on_at) and np.array_equal(k, ok_at), flag
    if edge == "prefilter":
        ok, on = cpu.nms_batched(boxes, sc, None, 0.1, kind, max_keep=mk + 1)
        for flag, (k, n) in _nms_batched_both(_t(boxes, dev), _t(sc, dev), 0.1, mk + 1, kind == "rotated").items():
            assert np.array_equal(n, on) and np.array_equal(k, ok), flag
    else:
        for flag in ("1", "0"):
            with _cabi.switches(PRCNN_NMS_PREFILTER=flag):
                with pytest.raises(PointOpsError, match=r"code -3\).*LDS"):
                    ops.nms_batched(_t(boxes, dev), _t(sc, dev), None, 0.1, kind == "rotated", max_keep=mk + 1)
