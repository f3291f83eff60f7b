"""VERDICT r04 item 3 / `north_star`: "... so lib/net AND tools/eval_rcnn.py call it unchanged".

The reference's `tools/eval_rcnn.py` is run AS A SCRIPT, unchanged, end to end on the MI355X, with the command line of README.md:84-87
(`--eval_mode rcnn`, checkpoint through `--ckpt`), in the environment INTEGRATION.md section 1 describes (PYTHONPATH = the drop-in
modules + the environment shims of tests/compat: easydict, tensorboardX, fire, numba incl. a numba.cuda launch emulator for the
evaluator's one CUDA kernel, skimage, yaml.load / collections.Iterable adapters -- nothing of the reference is edited):

  dataset     lib/datasets/kitti_rcnn_dataset.py on a synthetic KITTI tree in the real on-disk formats (tests/kitti_tree.py)
  checkpoint  a seeded reference model saved by the reference's own checkpoint_state / save_checkpoint (train_utils.py:60-76) and
              loaded by its load_checkpoint (:79-94) through `--ckpt`
  model       lib/net/point_rcnn.py on pointrcnn_amd/dropin -> libprcnn_pointops.so
  post        decode_bbox_target, score threshold, iou3d_utils.nms_gpu, save_kitti_format (eval_rcnn.py:505-620)
  AP          tools/kitti_object_eval_python (eval_rcnn.py:676-681)

Checked against this package's own route on the SAME inputs (the mirror detector + `PointRCNN.detections` + kitti_output.py, fed by
the reference's dataset class with the script's seeds -- tests/eval_rcnn_helpers.py) and evaluator (pointrcnn_amd/kitti_eval.py):
  * one result file per frame, the same detections in the same order; every printed field within 2e-3 (the files carry 4 decimals;
    the two routes differ by fp32 rounding -- fused heads, device proposal stage, fused canonical transform -- i.e. <= 1e-5 * scale
    upstream of the printing), scores within 1e-3;  [string equality is reported, not required: a 1e-6 difference flips a fourth
    decimal once per few hundred numbers]
  * the AP table the reference's evaluator logs for ITS files == kitti_eval.get_official_eval_result on the same files, as strings;
  * the AP of the mirror's files == the AP of the reference's files (ground truth is placed 4 % of the footprint / 0.02 rad off detections, far
    from the 0.7 IoU threshold, plus boxes nothing detects).
Ground truth: derived from the mirror's detections of a first pass (labels do not influence the inputs: eval mode draws the same
points whatever the label files hold), so the AP numbers are not all zero with an untrained network."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kitti_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = list(range(50))          # the reference evaluator splits the examples into 50 parts and fails on an empty one (eval.py:334-356)


def _env(mlp_mode):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests", "compat"), os.path.join(ROOT, "pointrcnn_amd", "dropin"), ROOT,
                                         os.path.join(ROOT, "tests")])
    env["PRCNN_MLP_SPLIT"] = "6" if mlp_mode == "split6" else "0"
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    return env


def _run(cmd, cwd, env, log):
    with open(log, "w") as fh:
        p = subprocess.run(cmd, cwd=cwd, env=env, stdout=fh, stderr=subprocess.STDOUT, timeout=1500)
    if p.returncode != 0:
        with open(log) as fh:
            raise AssertionError("%s failed (rc %d):\n%s" % (" ".join(cmd), p.returncode, fh.read()[-6000:]))


def _ground_truth_from(det_dir, training_dir, P2):
    """per frame: the three best-scored detections moved by 4 % of their footprint / 0.02 rad (IoU3D ~0.85 with the detection) + two
    boxes nothing detects; returns the number of boxes written"""
    total = 0
    for f in FRAMES:
        det = kitti_tree.read_result_file(os.path.join(det_dir, "%06d.txt" % f))
        rows = sorted((r[1] for r in det), key=lambda v: -v[14])[:3]
        # x y z h w l ry; the shift is 4 % of the box's smaller footprint side (an untrained network emits boxes of any size)
        boxes = [[v[10] + 0.04 * min(v[8], v[9]), v[11], v[12] - 0.04 * min(v[8], v[9]), v[7], v[8], v[9], v[13] + 0.02] for v in rows]
        r = np.random.default_rng(90 + f)
        for _ in range(2):
            boxes.append([r.uniform(-8, 8), 1.6, r.uniform(12, 30), 1.5, 1.6, 3.9, r.uniform(-3, 3)])
        kitti_tree.write_labels(training_dir, f, np.array(boxes), P2)
        total += len(boxes)
    return total


def test_reference_eval_rcnn_script_runs_unchanged_end_to_end(dev, mlp_mode, tmp_path):
    from oracle import stage_reference
    from pointrcnn_amd import kitti_eval, kitti_input
    where = stage_reference.writable_copy(tmp_path / "PointRCNN")
    if where is None:
        pytest.skip("no reference tree: neither /root/reference nor oracle/_ref/reference_py.tar.gz on this box")
    tools = os.path.join(where, "tools")
    with open(os.path.join(tools, "eval_rcnn.py"), "rb") as fh:
        script_bytes = fh.read()
    training = kitti_tree.write_tree(os.path.join(where, "data"), FRAMES)
    env = _env(mlp_mode)
    helpers = os.path.join(ROOT, "tests", "eval_rcnn_helpers.py")
    ckpt = os.path.join(where, "ckpt", "checkpoint_epoch_7.pth")
    _run([sys.executable, helpers, "ckpt", ckpt, "11"], tools, env, str(tmp_path / "ckpt.log"))

    # pass 1: this package's route; its detections place the ground truth
    mirror_dir = str(tmp_path / "mirror")
    _run([sys.executable, helpers, "mirror", ckpt, mirror_dir, "4"], tools, env, str(tmp_path / "mirror.log"))
    P2 = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT).P2
    assert _ground_truth_from(mirror_dir, training, P2) >= 2 * len(FRAMES)

    # pass 2: the reference's script, unchanged (README.md:84-87 with the synthetic tree's checkpoint; --workers 0 keeps the numpy
    # draw of the 16384 points in the main process, where the script's own np.random.seed(666) fixes it), run as __main__ by the
    # helper, which applies the compat adapters first (`site` skips usercustomize while the user site directory is disabled)
    out_dir = os.path.join(where, "output", "e2e")
    _run([sys.executable, helpers, "script", "eval_rcnn.py", "--cfg_file", "cfgs/default.yaml", "--ckpt", ckpt, "--batch_size", "4", "--eval_mode", "rcnn",
          "--workers", "0", "--output_dir", out_dir], tools, env, str(tmp_path / "eval_rcnn.log"))
    with open(os.path.join(tools, "eval_rcnn.py"), "rb") as fh:
        assert fh.read() == script_bytes
    res_dir = os.path.join(out_dir, "eval", "epoch_7", "val", "final_result", "data")
    assert sorted(os.listdir(res_dir)) == ["%06d.txt" % f for f in FRAMES]

    # (1) the same detections from both routes
    n_lines = n_same = 0
    for f in FRAMES:
        ref = kitti_tree.read_result_file(os.path.join(res_dir, "%06d.txt" % f))
        mine = kitti_tree.read_result_file(os.path.join(mirror_dir, "%06d.txt" % f))
        assert len(ref) == len(mine), (f, len(ref), len(mine))
        with open(os.path.join(res_dir, "%06d.txt" % f)) as a, open(os.path.join(mirror_dir, "%06d.txt" % f)) as b:
            n_same += sum(x == y for x, y in zip(a.readlines(), b.readlines()))
        for (cr, vr), (cm, vm) in zip(ref, mine):
            assert cr == cm == "Car"
            d = np.abs(np.array(vr) - np.array(vm))
            # (2e-3 absolute on metres / radians, plus 1e-5 of the value for the image-plane corners: a pixel coordinate of 600-1200 carries the
            #  1e-5 contract of the network outputs times the focal length -- the two routes may send a grouped layer to different kernel
            #  families, e.g. the mirror's hoisted grouped layers run on the split-bf16 kernel since round 5)
            assert (d[:14] <= 2e-3 + 1e-5 * np.abs(np.array(vr[:14]))).all() and d[14] <= 1e-3 * max(1.0, abs(vr[14])), (f, vr, vm)
        n_lines += len(ref)
    assert n_lines >= 3 * len(FRAMES), "an untrained detector should still emit detections: %d" % n_lines
    print("\n[eval_rcnn.py unchanged] %d detections in %d frames, %d lines string-identical between the two routes" % (n_lines, len(FRAMES), n_same))

    # (2) the AP table the reference's evaluator logged for its files == this package's evaluator on the same files
    with open(os.path.join(out_dir, "eval", "epoch_7", "val", "log_eval_one.txt")) as fh:
        log = fh.read()
    assert "==> Loading from checkpoint" in log and "==> Done" in log                  # train_utils.load_checkpoint ran
    split_file = os.path.join(where, "data", "KITTI", "ImageSets", "val.txt")
    mine_on_ref, _ = kitti_eval.evaluate(os.path.join(training, "label_2"), res_dir, split_file, current_class=0)    # eval_rcnn.py:678-679
    assert mine_on_ref.strip() and mine_on_ref.strip() in log, (mine_on_ref, log[-3000:])
    aps = [float(v) for v in re.findall(r"3d\s+AP:([\d.]+)", mine_on_ref)]
    assert aps and max(aps) > 0.0, mine_on_ref                                         # not the all-zero table
    # (3) the mirror's files score the same AP
    mine_on_mine, _ = kitti_eval.evaluate(os.path.join(training, "label_2"), mirror_dir, split_file, current_class=0)
    assert mine_on_mine == mine_on_ref
