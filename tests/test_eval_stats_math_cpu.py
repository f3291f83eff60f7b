"""CPU: the arithmetic header of the evaluation statistics (pointrcnn_amd/csrc/eval_stats_math.h), compiled for the host by
tests/eval_stats_math_host.cpp -- once plain, once with -fsanitize=address,undefined -- and run as a program.

Thresholds: es_recalled against `torch.tensor(x) > t` on the CPU for the five Python doubles: float32(t) itself is not recalled at t, the
next float32 above it is; NaN, -1, +-inf.  Segmentation ratio and the two accuracies: bit-equal to the torch CPU float32 expressions of
tools/eval_rcnn.py:198-202 and :355-364 on random masks, with union == 0, sum(valid) == 0 and R = 1, and the double sums added in the
reference's order (per frame; the batch's ratio B times in seg_mode 1).  The whole accumulate step over the fixture's two batches per mode
(tests/golden/eval_stats_ref.npz: the dictionaries the reference's own eval_one_epoch_* returned), with the per-ground-truth maxima taken
from the oracle's boxes_iou3d(...).max(0): every entry equal, no tolerance."""
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_stats_cases as ec
from pointrcnn_amd import eval_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
F32 = np.float32


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eval_stats_math") / "eval_stats_math_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "eval_stats_math_host.cpp"),
                    "-o", exe], check=True)
    work = os.path.dirname(exe)

    def run(mode, blob):
        with open(os.path.join(work, "in.bin"), "wb") as f:
            f.write(blob)
        r = subprocess.run([exe, mode, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        with open(os.path.join(work, "out.bin"), "rb") as f:
            return f.read()
    return run


def test_thresholds_compare_in_float32_as_torch_does(host):
    rng = np.random.default_rng(5)
    vals = [np.nan, -1.0, 0.0, 1.0, np.inf, -np.inf]
    for t in ec.THRESH:
        vals += [F32(t), np.nextafter(F32(t), F32(1)), np.nextafter(F32(t), F32(0)), t + 1e-9, t - 1e-9]
    x = np.concatenate([np.array(vals, F32), rng.uniform(0, 1, 2000).astype(F32)])
    got = np.frombuffer(host("thresh", x.tobytes()), F32).reshape(len(x), 5)
    for k, t in enumerate(ec.THRESH):
        want = (torch.from_numpy(x) > t).numpy()
        assert np.array_equal(got[:, k] == 1, want), (t, x[(got[:, k] == 1) != want])
        i = int(np.flatnonzero(x == F32(t))[0])
        assert got[i, k] == 0 and got[i + 1, k] == 1                        # float32(t) is not recalled at t, its upper neighbour is
    assert not got[:2].any()                                                # NaN and the -1 fill: never recalled


def _seg_torch(seg, label):
    """eval_rcnn.py:198-201, torch CPU"""
    seg, label = torch.from_numpy(seg).long(), torch.from_numpy(label).long()
    fg_mask = label > 0
    correct = ((seg == label) & fg_mask).sum().float()
    union = fg_mask.sum().float() + (seg > 0).sum().float() - correct
    return (correct / torch.clamp(union, min=1.0)).item()


def _acc_torch(pred, gt_iou, fg, bg, thr):
    """eval_rcnn.py:355-364, torch CPU"""
    pred_classes, gt_iou = torch.from_numpy(pred).long(), torch.from_numpy(gt_iou)
    cls_label = (gt_iou > fg).float()
    cls_valid_mask = ((gt_iou >= fg) | (gt_iou <= bg)).float()
    cls_acc = ((pred_classes == cls_label.long()).float() * cls_valid_mask).sum() / max(cls_valid_mask.sum(), 1.0)
    cls_label_refined = (gt_iou >= thr).float()
    cls_acc_refined = (pred_classes == cls_label_refined.long()).float().sum() / max(cls_label_refined.shape[0], 1.0)
    return cls_acc.item(), cls_acc_refined.item()


@pytest.mark.parametrize("label_dtype", [np.int32, np.int64], ids=["i32", "i64"])
def test_segmentation_ratio_equals_torch_cpu_and_sums_in_the_reference_order(host, label_dtype):
    rng = np.random.default_rng(11)
    cases = []
    for n in (1, 7, 64, 1000, 4097):
        for p in (0.0, 0.05, 0.5, 1.0):
            seg = (rng.random((3, n)) < p).astype(F32)
            lab = rng.choice([-1, 0, 1], (3, n), p=[0.1, 0.9 - 0.8 * p, 0.8 * p]).astype(label_dtype)
            cases.append((seg, lab))
    cases.append((np.zeros((3, 33), F32), np.zeros((3, 33), label_dtype)))                 # union == 0
    cases.append((np.zeros((3, 33), F32), np.full((3, 33), -1, label_dtype)))              # only ignored labels
    for mode in (0, 1):
        blob = b"".join(ec.pack(B=3, seg=s, label=l, seg_mode=mode) for s, l in cases)
        states = ec.unpack_states(host("each", blob))
        assert len(states) == len(cases)
        for (seg, lab), (c, s) in zip(cases, states):
            want = 0.0
            if mode == 0:
                for b in range(3):
                    want += _seg_torch(seg[b], lab[b])
            else:
                for b in range(3):                                                          # :568-573 inside `for k in range(batch_size)`
                    want += _seg_torch(seg, lab)
            assert s[0] == want, (mode, seg.shape, s[0], want)
            assert c[12] == 3 and c[13] == 1 and not c[:12].any() and not s[1:].any()
    one = ec.unpack_states(host("each", ec.pack(B=1, seg=cases[-2][0][:1], label=cases[-2][1][:1])))[0]
    assert one[1][0] == 0.0


def test_classification_accuracies_equal_torch_cpu(host):
    rng = np.random.default_rng(13)
    fg, bg, thr = ec.CLS_FG, ec.CLS_BG, ec.REFINE
    cases = []
    for R in (1, 2, 63, 64, 500):
        for _ in range(4):
            iou = rng.uniform(0, 1, (2, R)).astype(F32)
            iou[:, 0] = rng.choice([F32(fg), F32(bg), F32(thr), np.nextafter(F32(fg), F32(1)), np.nextafter(F32(bg), F32(0))])
            cases.append(((rng.random((2, R)) < 0.5).astype(np.uint8), iou))
    cases.append((np.ones((2, 9), np.uint8), np.full((2, 9), 0.5, F32)))                   # sum(valid) == 0
    cases.append((np.zeros((2, 1), np.uint8), np.full((2, 1), np.nan, F32)))               # NaN IoU: label 0, not valid
    for refine in (0.7, 0.5):
        blob = b"".join(ec.pack(B=2, pred=p, gt_iou=i, thr=(fg, bg, refine)) for p, i in cases)
        states = ec.unpack_states(host("each", blob))
        for (pred, iou), (c, s) in zip(cases, states):
            a = r = 0.0
            for b in range(2):
                ta, tr = _acc_torch(pred[b], iou[b], fg, bg, refine)
                a += ta
                r += tr
            assert s[1] == a and s[2] == r, (pred.shape, s, a, r)
            assert s[0] == 0.0 and c[12] == 2 and c[13] == 1


@pytest.mark.parametrize("mode", ec.MODES)
def test_fixture_dictionaries_of_the_reference_loops(host, mode):
    blob = b""
    for b in ec.batches(mode):
        sets = [b["rois"].numpy()] + ([b["pred_boxes3d"].numpy()] if mode != "rpn" else [])
        gt_max, num_gt = ec.oracle_gt_max(sets, b["gt_boxes3d"].numpy(), ec.TRIM[mode])
        np_ = lambda k: b[k].numpy() if k in b else None      # noqa: E731
        blob += ec.pack(gt_max, num_gt, B=gt_max.shape[1], det_num=np_("det_num"), seg=np_("seg_result"), label=np_("rpn_cls_label"),
                        seg_mode=ec.SEG_MODE[mode], pred=np_("pred_class"), gt_iou=np_("gt_iou"))
    (c, s), = ec.unpack_states(host("accumulate", blob))
    got = eval_stats.result_from_state(mode, c, s)
    want = ec.ref_dict(mode)
    want.pop("empty_cnt", None)                               # the file dump of the loop, not a statistic
    assert want and set(want) <= set(got)
    for k, v in want.items():
        assert got[k] == v, (mode, k, got[k], v)
    assert c[12] == 6 and c[13] == 2 and c[10] == (24 if mode == "rpn" else 23)            # rpn keeps the all-zero row 0 as a box
    assert 0 < c[4] < c[0] < c[10]
