"""GPU: the evaluation statistics counted on the device (csrc/eval_stats.hip, pointrcnn_amd/eval_stats.py).

Per-ground-truth maximum IoU: bit-equal (NaN == NaN) to the oracle's boxes_iou3d(...).max(0), the -1 fill and num_gt included, over
M in {1, 63, 64, 65, 130} x G in {1, 15, 16, 17, 128} (around the 64-lane stride and pt_overlaps_kernel's 16), both trim modes, gt_cols 7
and 8, on random boxes, near-duplicates of the ground truth, the collinear / grid families of tests/collinear_boxes.py, a frame without a
live box, an all-zero row in the middle, and predicted boxes with NaN and +-inf coordinates.
The accumulated dictionaries of all three modes over the fixture's two batches EQUAL the dictionaries the reference's own
eval_one_epoch_rpn / _rcnn / _joint returned (tests/golden/eval_stats_ref.npz): integers exact, ratios float32 bit-equal, double sums in
the reference's order.  Determinism, reset, graph capture, the device loop eval_one_epoch_joint on a synthetic KITTI tree, argument errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import collinear_boxes as cb
import eval_stats_cases as ec
import kitti_tree

pytestmark = pytest.mark.gpu
F32 = np.float32
MS, GS = (1, 63, 64, 65, 130), (1, 15, 16, 17, 128)
_cases = {}


def _scene(M, G):
    """(rois (3,M,7), gt7 (3,G,7) before trimming, the oracle's full column maxima (3,G)) -- computed once per shape, shared by every test"""
    if (M, G) in _cases:
        return _cases[(M, G)]
    import oracle
    from util import rand_boxes3d
    cpu = oracle.cpu()
    seed = M * 1000 + G
    rng = np.random.default_rng(seed)
    pts = rng.uniform([-20, 0, 5], [20, 2, 45], (500, 3)).astype(F32)
    gt = np.zeros((3, G, 7), F32)
    rois = np.zeros((3, M, 7), F32)
    # frame 0: random ground truth; RoIs random, jittered copies and exact duplicates of ground-truth boxes
    gt[0] = rand_boxes3d(pts, G, seed=seed)
    r = rand_boxes3d(pts, M, seed=seed + 1)
    pick = rng.integers(0, G, M)
    near = gt[0][pick] + (rng.normal(0, 1, (M, 7)) * np.array([0.3, 0.1, 0.3, 0.05, 0.05, 0.1, 0.05]) * rng.choice([0.03, 0.3, 1.0], (M, 1))).astype(F32)
    kind = rng.integers(0, 3, M)
    rois[0] = np.where((kind == 0)[:, None], r, np.where((kind == 1)[:, None], near, gt[0][pick]))
    if M == 65:
        rois[0, 7, 0] = rois[0, 7, 4] = np.nan                        # NaN centre and width: every column of the frame is NaN (torch.max)
    if M == 130:
        rois[0, 3, 0], rois[0, 9, 2] = np.inf, -np.inf
    # frame 1: one collinear / grid family for both sets (shared heading and sizes), duplicates among them
    fam = cb.KINDS[(M + G) % len(cb.KINDS)]
    up4 = lambda n: -(-n // 4) * 4                                    # noqa: E731  (the families come in groups of four)
    gt[1] = cb.family_boxes3d(fam, seed % 50, jitter=cb.JITTERS[(M * G) % len(cb.JITTERS)], n=up4(G))[:G]
    rois[1] = cb.family_boxes3d(fam, seed % 50, n=up4(M + G))[G:G + M] if M > 1 else gt[1][:1]
    # frame 2: nothing live (G == 16 | M == 63), else a zero row in the middle and zero rows at the end
    rois[2] = rand_boxes3d(pts, M, seed=seed + 2)
    if not (G == 16 or M == 63):
        live = max(1, G - G // 3)
        gt[2, :live] = rois[2][rng.integers(0, M, live)] + rng.normal(0, 0.15, (live, 7)).astype(F32)
        if live > 2:
            gt[2, live // 2] = 0
    with np.errstate(invalid="ignore"):
        full = np.stack([cpu.boxes_iou3d(rois[b], gt[b]).max(0) for b in range(3)])
    _cases[(M, G)] = (rois, gt, full)
    return _cases[(M, G)]


@pytest.mark.parametrize("gt_cols", [7, 8])
@pytest.mark.parametrize("trim_mode", [0, 1])
def test_gt_max_iou_equals_the_oracle_bit_for_bit(dev, trim_mode, gt_cols):
    from pointrcnn_amd import ops
    seen_nan = seen_dead = seen_mid = 0
    for M in MS:
        for G in GS:
            rois, gt7, full = _scene(M, G)
            gt = np.zeros((3, G, gt_cols), F32)
            gt[:, :, :7] = gt7
            if gt_cols == 8:
                gt[:, :, 7] = (np.abs(gt7).sum(2) != 0)               # a class column: 1 on a box, 0 on a padding row
            num = np.array([ec.live_rows(gt[b], trim_mode) for b in range(3)], np.int32)
            want = np.full((2, 3, G), -1, F32)
            for b in range(3):
                want[:, b, :num[b]] = full[b, :num[b]]
            other = rois[:, ::-1].copy()                          # the second set: the same boxes in another order -> the same maxima
            got, got_num = ops.eval_gt_max_iou([torch.from_numpy(rois).to(dev), torch.from_numpy(other).to(dev)],
                                               torch.from_numpy(gt).to(dev), trim_mode)
            got, got_num = got.cpu().numpy(), got_num.cpu().numpy()
            assert np.array_equal(got_num, num), (M, G, got_num, num)
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), (M, G, np.argwhere(~same)[:5], got[~same][:5], want[~same][:5])
            one, _ = ops.eval_gt_max_iou(torch.from_numpy(rois).to(dev), torch.from_numpy(gt).to(dev), trim_mode)
            assert np.array_equal(one.cpu().numpy()[0], got[0], equal_nan=True)
            seen_nan += int(np.isnan(want).any())
            seen_dead += int(num[2] == 0) + int(trim_mode == 1 and num[2] == 1 and not gt[2, 0].any())
            seen_mid += int(any(not gt[2, j].any() for j in range(1, max(num[2] - 1, 1))))
            if M < 65:
                assert not np.isnan(want).any()
    assert seen_nan >= 5 and seen_dead >= 5 and seen_mid >= 5        # the families are present


def _to(dev, batch):
    return {k: v.to(dev) for k, v in batch.items()}


def _run(dev, mode, times=1):
    from pointrcnn_amd.eval_stats import EvalStats
    st = EvalStats(mode, dev)
    for _ in range(times):
        for b in ec.batches(mode):
            st.update(**_to(dev, b))
    return st


@pytest.mark.parametrize("mode", ec.MODES)
def test_result_equals_the_dictionary_of_the_reference_loop(dev, mode):
    st = _run(dev, mode)
    got = st.result()
    want = ec.ref_dict(mode)
    want.pop("empty_cnt", None)
    assert len(want) >= 7 and set(want) <= set(got)
    for k, v in want.items():
        print(mode, k, got[k], v)
        assert got[k] == v, (mode, k, got[k], v)
    c, s = st.raw()
    assert c[12] == 6 and c[13] == 2 and c[10] == (24 if mode == "rpn" else 23) and not c[14:].any() and s[3] == 0
    # determinism: a second fresh run gives the same bytes; reset gives zeros
    again = _run(dev, mode)
    assert torch.equal(st.state, again.state)
    st.reset()
    assert not st.state.any() and all(v == 0 for v in st.result().values())


def test_update_is_captured_in_a_graph_and_replays(dev):
    from pointrcnn_amd.eval_stats import EvalStats
    for mode in ("joint", "rcnn"):
        batch = _to(dev, ec.batches(mode)[0])
        st = EvalStats(mode, dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st.update(**batch)                                        # warm-up outside the capture: the workspace is allocated here
        torch.cuda.current_stream().wait_stream(side)
        st.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                 # a hidden synchronisation or host read would fail the capture
            st.update(**batch)
        assert not st.state.any()                                     # capturing runs nothing
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        eager = EvalStats(mode, dev)
        for _ in range(3):
            eager.update(**batch)
        assert torch.equal(st.state, eager.state) and eager.raw()[0][13] == 3


def test_eval_one_epoch_joint_on_a_synthetic_tree(dev, cpu, tmp_path):
    from pointrcnn_amd import eval_stats, kitti_eval, kitti_input
    from pointrcnn_amd.point_rcnn import PointRCNN
    from pointrcnn_amd.rpn import randomize_bn_stats, synthetic_clouds
    frames = [0, 1, 2, 3]                                             # frame 3 is in the split but in no batch: its file is dumped empty
    training = kitti_tree.write_tree(tmp_path, frames, n_scan=2000)
    split_file = os.path.join(str(tmp_path), "KITTI", "ImageSets", "val.txt")
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    torch.manual_seed(0)
    model = randomize_bn_stats(PointRCNN(mode="TEST")).to(dev).eval()
    pts = synthetic_clouds(3, 16384, device=dev)
    with torch.no_grad():
        first = model({"pts_input": pts})
        pred0 = model.detections(first, score_thresh=0.3)[0].cpu().numpy()
    G = 6
    gt = np.zeros((3, G, 7), F32)
    rng = np.random.default_rng(3)
    for b in range(3):                                                # labels: refined boxes of the model itself, some of them jittered
        n = 3 + b
        gt[b, :n] = pred0[b, :n] + (rng.normal(0, 1, (n, 7)) * np.array([0.2, 0.05, 0.2, 0.03, 0.03, 0.08, 0.04]) * (np.arange(n) % 3)[:, None]).astype(F32)
        kitti_tree.write_labels(training, b, gt[b, :n], calib.P2)
    gt[1] = 0                                                         # the batch's ground truth of frame 1 is empty (its label file is not)
    seen = []
    detections = model.detections

    def recording(ret, **kw):
        out = detections(ret, **kw)
        seen.append((ret["rois"].cpu().numpy(), out[0].cpu().numpy(), out[3].cpu().numpy()))
        return out
    model.detections = recording
    batches = [{"sample_id": np.array([0, 1]), "pts_input": pts[:2], "gt_boxes3d": gt[:2]},
               {"sample_id": np.array([2]), "pts_input": pts[2:].cpu().numpy(), "gt_boxes3d": torch.from_numpy(gt[2:])}]
    result_dir = str(tmp_path / "out")
    ret = eval_stats.eval_one_epoch_joint(model, batches, result_dir, lambda i: calib, kitti_tree.image_shape, split_file=split_file,
                                          label_dir=os.path.join(training, "label_2"))
    out_dir = os.path.join(result_dir, "final_result", "data")
    # recall: an oracle-side recount from the model's own rois, refined boxes and detection counts
    counts, total, dets = np.zeros((2, 5), np.int64), 0, 0
    for (rois, pred, num), data in zip(seen, batches):
        g = np.asarray(data["gt_boxes3d"], F32)
        gmax, ng = ec.oracle_gt_max([rois, pred], g, 0)
        for b in range(len(ng)):
            for s in range(2):
                for t, th in enumerate(ec.THRESH):
                    counts[s, t] += int((torch.from_numpy(gmax[s, b, :ng[b]]) > th).sum())
        total += int(ng.sum())
        dets += int(num.sum())
    assert total == 3 + 5
    for t, th in enumerate(ec.THRESH):
        assert ret["rpn_recall(thresh=%.2f)" % th] == counts[0, t] / max(total, 1.0)
        assert ret["rcnn_recall(thresh=%.2f)" % th] == counts[1, t] / max(total, 1.0)
    assert ret["rcnn_avg_num"] == dets / 3.0 and ret["rpn_iou"] == 0.0 and ret["rcnn_cls_acc"] == 0.0
    assert counts[1, 0] > 0                                           # the labels are refined boxes of the model: some are recalled
    # files: one per frame of the split; those without a detection were dumped empty and counted
    assert sorted(os.listdir(out_dir)) == ["%06d.txt" % f for f in frames]
    nums = np.concatenate([s[2] for s in seen])
    assert ret["empty_cnt"] == 1 + int((nums == 0).sum())
    assert os.path.getsize(os.path.join(out_dir, "000003.txt")) == 0
    # AP keys: the evaluator called directly on the written files
    _, ap = kitti_eval.evaluate(os.path.join(training, "label_2"), out_dir, split_file, current_class=0)
    assert len(ap) == 9
    for k, v in ap.items():
        assert ret[k] == v or (np.isnan(ret[k]) and np.isnan(v)), k


def test_argument_errors_return_a_status_and_a_message(dev):
    from pointrcnn_amd import _cabi, ops
    L = _cabi.lib()
    boxes = torch.zeros((1, 4, 7), device=dev)
    gt = torch.zeros((1, 200, 8), device=dev)
    gt_max, num_gt = ops.eval_stats_workspace(1, 1, 200, dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def gt_max_iou(M, G, cols):
        return L.prcnn_eval_gt_max_iou(p(boxes), None, 1, 1, M, p(gt), G, cols, 0, p(gt_max), p(num_gt), None)
    for args, word in (((0, 4, 7), "M=0"), ((4, 129, 7), "G=129"), ((4, 4, 6), "gt_cols=6")):
        assert gt_max_iou(*args) == -1
        assert word in L.prcnn_last_error().decode(), L.prcnn_last_error()
    state = torch.zeros((ops.EVAL_STATS_STATE_BYTES,), dtype=torch.uint8, device=dev)
    seg = torch.zeros((1, 8), device=dev)

    def accumulate(seg_t, label_t, state_t):
        return L.prcnn_eval_stats_accumulate(None, None, 0, 1, 0, None, None if seg_t is None else p(seg_t), None if label_t is None else p(label_t),
                                             0, 8, 0, None, None, 0, 0.6, 0.45, 0.7, None if state_t is None else p(state_t), None)
    assert accumulate(None, None, None) == -1 and "null state" in L.prcnn_last_error().decode()
    assert accumulate(seg, None, state) == -1 and "cls_label null" in L.prcnn_last_error().decode()
    with pytest.raises(_cabi.PointOpsError, match="cls_label"):
        ops.eval_stats_accumulate(state, None, None, 1, seg=seg)
    torch.cuda.synchronize()
    assert not state.any()                                            # a refused call adds nothing
    assert L.prcnn_eval_stats_workspace_bytes(2, 3, 5) == (2 * 3 * 5 + 3) * 4 + 4 and L.prcnn_abi_version() == 12
