"""CPU: the RCNN offline RoI sampler's arithmetic header (pointrcnn_amd/csrc/rcnn_offline_math.h) compiled for the host by
tests/rcnn_offline_math_host.cpp -- once plain, once with -fsanitize=address,undefined -- and run as a program, against the numpy
twin (tests/rcnn_offline_twin.py), BIT FOR BIT: every pair IoU of the synthetic frames, every sampled slot of those frames and
10 000 random slots (both noise methods, one and ten attempts).  The header applies a separating-axis test before the clip and the
twin does not: equality shows that the test changes no result.

The twin itself is held to what each synthetic frame is built to be (tests/rcnn_offline_cases.py) and to the properties of
get_rcnn_training_sample_batch that do not need its arithmetic: list order, duplicates, slot quotas, the cases it raises on."""
import os
import subprocess

import numpy as np
import pytest

import rcnn_offline_cases as rc
import rcnn_offline_twin as ot
import train_input_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
F32 = np.float32


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rcnn_offline_math") / "rcnn_offline_math_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "rcnn_offline_math_host.cpp"),
                    "-o", exe], check=True)
    work = os.path.dirname(exe)

    def run(mode, records):
        records = np.ascontiguousarray(records, dtype=F32)
        records.tofile(os.path.join(work, "in.bin"))
        r = subprocess.run([exe, mode, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(os.path.join(work, "out.bin"), F32).reshape(len(records), -1)
    return run


def slot_records(box, gt, times, method, seed, frame, slot):
    n = len(box)
    ints = np.stack([np.broadcast_to(np.asarray(v, np.int32), (n,)) for v in (times, method, seed, frame, slot)], 1).astype(np.int32)
    return np.concatenate([np.asarray(box, F32), np.asarray(gt, F32), ints.view(F32)], 1)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_the_twin_reports_what_each_frame_is_built_to_be(name):
    t = rc.twin_result(name, 3)
    roi, gt = rc.CASES[name][0]()
    R, want = rc.CASES[name][1], rc.CASES[name][2]
    got = dict(status=t["status"], nfg=t["counts"][0], nhard=t["counts"][1], neasy=t["counts"][2], fs=t["counts"][3])
    for k, v in want.items():
        assert got[k] == v, (name, k, got)
    mo, ga = t["max_overlaps"], t["gt_assignment"]
    assert same_bits(mo, t["iou3d"][np.arange(len(roi)), ga])
    if t["status"]:
        assert (t["src"] == -1).all() and not t["rois"].any() and not t["gt_of_rois"].any() and not t["roi_iou"].any()
        return
    fs, src = got["fs"], t["src"]
    assert len(src) == R and (src >= 0).all() and same_bits(t["gt_of_rois"], gt[ga[src]])
    thr = np.nonzero(mo >= F32(0.55))[0]
    best = [int(np.argmax(t["iou3d"][:, j])) for j in range(len(gt)) if t["iou3d"][:, j].max() > 0]
    assert got["nfg"] == len(thr) + len(best)
    pool = sorted(list(thr) + best)
    assert all(pool.count(i) >= list(src[:fs]).count(i) for i in set(src[:fs]))          # without replacement, duplicates kept
    if fs == got["nfg"]:
        assert sorted(src[:fs]) == pool
    bg = src[fs:]
    nh = int((R - fs) * 0.8) if got["nhard"] and got["neasy"] else (R - fs if got["nhard"] else 0)
    assert ((mo[bg[:nh]] >= F32(0.05)) & (mo[bg[:nh]] < F32(0.45))).all() and (mo[bg[nh:]] < F32(0.05)).all()
    # a background slot draws once and its IoU is the loop's, never the matrix entry: even where the draw kept the original box the loop
    # measures it in the one-box corner form (one float32 step of a coordinate below 64 m, 4e-6 m, against a 1.5 m wide box: the IoU
    # moves by a few 1e-6)
    moved = (t["rois"][fs:] != roi[bg]).any(1)
    assert moved.any() and np.abs(t["roi_iou"][fs:][~moved] - mo[bg][~moved]).max(initial=0) <= 1e-4


def test_case_specifics():
    t = rc.twin_result("shared best", 3)
    assert sorted(t["src"][:3]) == [1, 1, 1]                                   # over the threshold and the best RoI of both labels
    t = rc.twin_result("identical RoIs", 3)
    assert sorted(t["src"][:3])[0] == 0 and 3 not in t["src"][:3] and 9 not in t["src"][:3]      # the first of the identical RoIs
    t = rc.twin_result("M 2 G 1", 3)
    assert list(t["src"][:2]) == [0, 0] and (t["src"][2:] == 1).all()
    t = rc.twin_result("odd quota", 3)
    assert t["counts"][3] == 4                                                  # np.round(0.5 * 7) = 4, to even
    assert ot.sample_frame(np.zeros((3, 7), F32), np.zeros((0, 7), F32), 1, 0)["status"] == 2
    assert ot.sample_frame(np.zeros((0, 7), F32), np.ones((2, 7), F32), 1, 0)["status"] == 1
    with pytest.raises(NotImplementedError):
        ot.noise_box(np.ones(7, F32), 1, 0, 0, "normal")
    a, b = rc.twin_result("all three lists", 3), rc.twin_result("all three lists", 4)
    assert not np.array_equal(a["src"], b["src"])                               # the frame id keys the table


def test_pair_iou_of_every_frame_bit_for_bit(host):
    for name in rc.CASES:
        roi, gt = rc.CASES[name][0]()
        rec = np.concatenate([np.repeat(roi, len(gt), 0), np.tile(gt, (len(roi), 1))], 1)
        got = host("iou", rec).reshape(len(roi), len(gt))
        assert same_bits(got, rc.twin_result(name, 3)["iou3d"]), name


def test_sampled_slots_of_every_frame_bit_for_bit(host):
    for name in rc.CASES:
        t = rc.twin_result(name, 3)
        if t["status"]:
            continue
        roi, gt = rc.CASES[name][0]()
        R, fs = rc.CASES[name][1], t["counts"][3]
        times = np.where(np.arange(R) < fs, 10, 1)
        method = ("multiple", "single").index(rc.METHOD.get(name, "multiple"))
        got = host("slot", slot_records(roi[t["src"]], t["gt_of_rois"], times, method, rc.SEED, 3, np.arange(R)))
        assert same_bits(got[:, :7], t["rois"]) and same_bits(got[:, 7], t["roi_iou"]), name


def random_slots(n):
    rng = np.random.default_rng(5)
    gt = rc.labels(rng, n)
    gt[:, 0] += rng.uniform(-30, 30, n).astype(F32)
    kinds = rng.choice(["near", "near", "hard", "graze", "far"], n)
    box = np.stack([rc.moved(rng, gt[i], kinds[i]) for i in range(n)])
    return box, gt, rng.choice([1, 10], n), rng.integers(0, 2, n), rng.integers(0, 2 ** 31 - 1, n), rng.integers(0, 8000, n), rng.integers(0, 64, n)


_random = {}


def random_expected():
    if not _random:
        box, gt, times, method, seed, frame, slot = random_slots(10000)
        trig = ot.ref_trig()
        res = [ot.noise_slot(box[i], gt[i], int(times[i]), 0.55, int(seed[i]), int(frame[i]), int(slot[i]), ("multiple", "single")[method[i]], trig)
               for i in range(len(box))]
        _random["v"] = (np.stack([r[0] for r in res]), np.array([r[1] for r in res], F32), np.array([r[2] for r in res], np.int32))
    return _random["v"]


def test_ten_thousand_random_slots_bit_for_bit(host):
    box, gt, times, method, seed, frame, slot = random_slots(10000)
    rois, iou, cnt = random_expected()
    got = host("slot", slot_records(box, gt, times, method, seed, frame, slot))
    assert same_bits(got[:, :7], rois) and same_bits(got[:, 7], iou) and np.array_equal(got[:, 8].view(np.int32), cnt)
    assert cnt.min() == 1 and cnt.max() == 10 and ((cnt > 1) & (cnt < 10)).any()          # early exits, full loops and single draws all occur
    assert (iou >= F32(0.55)).any() and (iou == 0).any()


def test_corner_twins_agree_with_train_input_twin_where_they_must():
    rng = np.random.default_rng(9)
    b = rc.labels(rng, 64)
    b[:8, 6] = 0                                               # cos 1, sin 0 under any libm
    assert same_bits(ot.corners_f32(b[:8]), tw.corners3d(b[:8]))
    assert same_bits(ot.corners_f32(b, (np.cos, np.sin)), tw.corners3d(b))
    # a float64 box whose entries are float32 values: the float64 path agrees with the float32 path to one float32 step of the largest coordinate
    c64 = np.stack([ot.corners_f64(v.astype(np.float64)) for v in b])
    c32 = ot.corners_f32(b)
    assert np.abs(c64.astype(np.float64) - c32).max() <= 2 * np.spacing(F32(np.abs(c32).max()))


def test_offline_entry_takes_both_layouts_and_copies_the_targets_through():
    """RCNNNet's ROI_SAMPLE_JIT False entry up to the network trunk (rcnn_net.py:155-163; the trunk is HIP only): pts_features appended
    as train_functions.py:31-33 does, a frame axis in front of the RoI axis flattened, the targets copied through in training only"""
    import torch
    from pointrcnn_amd import rcnn

    class Cfg(rcnn.RCNNConfig):
        ROI_SAMPLE_JIT = False
    net = rcnn.RCNNNet(cfg=Cfg)
    B, R, S, C = 2, 3, 4, 128
    g = torch.Generator().manual_seed(1)
    batch = {"pts_input": torch.randn(B, R, S, 5, generator=g), "pts_features": torch.randn(B, R, S, C, generator=g),
             "cls_label": torch.randint(-1, 2, (B, R), generator=g, dtype=torch.int32), "reg_valid_mask": torch.ones(B, R, dtype=torch.int32),
             "gt_boxes3d_ct": torch.randn(B, R, 7, generator=g), "roi_boxes3d": torch.randn(B, R, 7, generator=g)}
    net.train()
    pts, tgt = net._offline_input(batch)
    assert pts.shape == (B * R, S, 5 + C) and tgt["pts_input"] is pts
    assert torch.equal(pts[..., :5], batch["pts_input"].view(-1, S, 5)) and torch.equal(pts[..., 5:], batch["pts_features"].view(-1, S, C))
    assert set(tgt) == {"pts_input", "roi_boxes3d", "cls_label", "reg_valid_mask", "gt_of_rois"}
    assert tgt["cls_label"].shape == (B * R,) and tgt["cls_label"].dtype == torch.int32 and tgt["gt_of_rois"].shape == (B * R, 7)
    assert torch.equal(tgt["gt_of_rois"], batch["gt_boxes3d_ct"].view(-1, 7)) and torch.equal(tgt["roi_boxes3d"], batch["roi_boxes3d"].view(-1, 7))
    flat = {k: v.reshape((-1,) + tuple(v.shape[2:])) for k, v in batch.items()}
    pts2, tgt2 = net._offline_input(flat)
    assert torch.equal(pts2, pts) and all(torch.equal(tgt2[k], tgt[k]) for k in tgt)
    net.eval()
    assert set(net._offline_input({"pts_input": pts, "roi_boxes3d": flat["roi_boxes3d"]})[1]) == {"pts_input", "roi_boxes3d"}
    with pytest.raises(ValueError, match="rows"):
        net._offline_input({"pts_input": pts, "roi_boxes3d": flat["roi_boxes3d"][:2]})
    assert rcnn.RCNNConfig.ROI_SAMPLE_JIT is True                      # the default stays the online route


# ------------------------------------------------------------------------------------------------ the reference's own method
def test_twin_equals_the_reference_method_bit_for_bit():
    """tests/golden/rcnn_offline_ref.npz: KittiRCNNDataset.get_rcnn_training_sample_batch itself on every frame of
    tests/rcnn_offline_cases.py (tests/golden/ref_rcnn_offline.py; boxes as its own parser reads them from text).  The twin with
    numpy's float32 sine / cosine -- what the reference's boxes3d_to_corners3d calls -- must return the same source boxes, the same
    boxes after the noise loop, the same IoUs and labels, slot for slot, bit for bit; the labels and masks of sample_info follow
    from those IoUs.  The reference raised on the foreground-only frame and on no other."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "rcnn_offline_ref.npz"))
    names = list(z["names"])
    assert names == list(rc.CASES)
    raised = [n for k, n in enumerate(names) if str(z["c%d_raised" % k])]
    assert raised == ["foreground only"] and str(z["c%d_raised" % names.index("foreground only")]).startswith(("TypeError", "AttributeError"))
    for k, n in enumerate(names):
        roi, gt = z["c%d_roi" % k], z["c%d_gt" % k]
        m, g = rc.CASES[n][0]()
        assert roi.shape == m.shape and gt.shape == g.shape and np.abs(roi - m).max() <= 1e-4      # text with four decimals
        t = ot.sample_frame(roi, gt, int(z["seed"]), k, dict(ROI_PER_IMAGE=int(z["c%d_R" % k]), REG_AUG_METHOD=str(z["c%d_method" % k])),
                            trig=(np.cos, np.sin))
        if n in raised:
            assert t["status"] == 1
            continue
        assert t["status"] == 0 and t["counts"][3] == int(z["c%d_fs" % k]), n
        assert same_bits(roi[t["src"]], z["c%d_src_boxes" % k]), n
        assert same_bits(t["rois"], z["c%d_rois" % k]), n
        assert same_bits(t["roi_iou"], z["c%d_roi_iou" % k]), n
        assert same_bits(t["gt_of_rois"], z["c%d_gt_of_rois" % k]), n
        iou = t["roi_iou"]
        label = (iou > 0.6).astype(np.int32)
        label[(iou > 0.45) & (iou < 0.6)] = -1
        empty = z["c%d_empty" % k] != 0                                # the recorded pooled_empty_flag explains every other -1
        label[empty] = -1
        assert np.array_equal(label, z["c%d_cls_label" % k]), n
        assert np.array_equal(((iou > 0.55) & ~empty).astype(np.int32), z["c%d_reg_valid_mask" % k]), n


def test_load_rcnn_offline_frame_reads_what_the_reference_reads(tmp_path):
    """kitti_input.load_rcnn_offline_frame on a synthetic tree -- the five dumps of kitti_output.save_rpn_features, a proposals file and
    label lines, written as tests/golden/ref_rcnn_offline.py writes them: the RoIs and the filtered labels are the arrays the
    reference's own parser and filtrate_objects returned (the fixture), bit for bit; the dumps come back as saved"""
    from pointrcnn_amd import kitti_input, kitti_output
    z = np.load(os.path.join(ROOT, "tests", "golden", "rcnn_offline_ref.npz"))
    rng = np.random.default_rng(3)
    feat_dir, roi_dir = str(tmp_path / "features"), str(tmp_path / "rois")
    os.makedirs(feat_dir), os.makedirs(roi_dir)
    for k, name in enumerate(rc.CASES):
        if name not in ("all three lists", "M 2 G 1", "shared best"):
            continue
        roi, gt = rc.CASES[name][0]()
        n = 50 + k
        seg, raw, inten = (rng.random(n) > 0.5).astype(F32), rng.normal(0, 2, n).astype(F32), rng.random((n, 1)).astype(F32)
        xyz, feat = rng.normal(0, 9, (n, 3)).astype(F32), rng.normal(0, 1, (n, 8)).astype(F32)
        kitti_output.save_rpn_features(seg, raw, inten, xyz, feat, feat_dir, 7000 + k)
        with open(os.path.join(roi_dir, "%06d.txt" % (7000 + k)), "w") as f:
            f.write("".join(ln + "\n" for ln in rc.roi_text(roi)))
        fr = kitti_input.load_rcnn_offline_frame(feat_dir, roi_dir, rc.label_text(gt), 7000 + k)
        assert fr["sample_id"] == 7000 + k
        assert same_bits(fr["roi_boxes3d"], z["c%d_roi" % k]) and same_bits(fr["gt_boxes3d"], z["c%d_gt" % k]), name
        assert fr["roi_scores"].dtype == F32 and same_bits(fr["roi_scores"], (1.0 - 0.001 * np.arange(len(roi))).round(4).astype(F32))
        assert np.array_equal(fr["rpn_xyz"], xyz) and np.array_equal(fr["rpn_features"], feat)
        assert np.array_equal(fr["rpn_intensity"], inten[:, 0]) and np.array_equal(fr["seg_mask"], seg)
    # INCLUDE_SIMILAR_TYPE (default.yaml: on) keeps a Van with Car; off, or for another class list, it goes; bounds of the scope are inside
    van = rc.box_line([3.0, 1.6, 30.0, 1.9, 1.9, 5.0, 0.1], cls="Van")
    edge = rc.box_line([40.0, 3.0, 70.375, 1.5, 1.6, 3.9, 0.0])
    past = rc.box_line([0.0, 1.6, 70.4, 1.5, 1.6, 3.9, 0.0])      # float32(70.4) = 70.40000153 > 70.4: check_pc_range compares in double
    lab = kitti_input.read_label_lines(rc.label_text(gt) + [van, edge, past])
    g = len(gt)
    assert g + 5 not in kitti_input.filtrate_objects(lab) and g + 5 in kitti_input.filtrate_objects(lab, area_scope=None)
    lab = kitti_input.read_label_lines(rc.label_text(gt) + [van, edge])
    assert list(kitti_input.filtrate_objects(lab)) == list(range(1, g + 1)) + [g + 3, g + 4]
    assert list(kitti_input.filtrate_objects(lab, include_similar_type=False)) == list(range(1, g + 1)) + [g + 4]
    assert list(kitti_input.filtrate_objects(lab, area_scope=None)) == list(range(1, g + 1)) + [g + 2, g + 3, g + 4]
    assert list(kitti_input.filtrate_objects(lab, classes=("Pedestrian",))) == [g + 1]


# ------------------------------------------------------------------------------------------------ the whole method
def _fixture_frame(z, k):
    gt = z["c%d_gt" % k]
    return dict(rc.frame_points(k, rc.CASES[list(rc.CASES)[k]][0]()[1]), roi_boxes3d=z["c%d_roi" % k], gt_boxes3d=gt)


def _twin_frame(z, k, **kw):
    aug, ui = rc.frame_config(k)
    return ot.offline_frame(_fixture_frame(z, k), int(z["seed"]), k, dict(ROI_PER_IMAGE=int(z["c%d_R" % k]), REG_AUG_METHOD=str(z["c%d_method" % k])),
                            S=rc.S_POINTS, use_intensity=ui, methods=("rotation", "scaling", "flip") if aug else (), **kw)


def test_whole_method_twin_against_the_reference():
    """sample_info of the reference's get_rcnn_training_sample_batch, AUG_DATA and USE_INTENSITY on and off.  Formed in integers or
    rounded once -- pooled points and features, extras, empty flags, labels, masks: bit for bit.  Through torch's float32 product or
    numpy's float32 arctan2 -- point xyz, gt_boxes3d_ct, the ry of the augmented boxes: the twin in the contract's arithmetic
    (csrc/ref_trig.h) stays within the distance measured when the fixture was made (stored there, in float32 steps of the frame's
    largest coordinate: xyz 3.5, gt_boxes3d_ct 3.5, ry 2.0 steps of 2 pi) plus one step; with numpy's arctan2 ry is bit for bit."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "rcnn_offline_ref.npz"))
    seen = dict(empty=0, wrapped=0, full=0, aug=set(), ui=set())
    for k, n in enumerate(z["names"]):
        if str(z["c%d_raised" % k]):
            assert _twin_frame(z, k)["status"] == 1
            continue
        t = _twin_frame(z, k, sample_trig=(np.cos, np.sin))
        ref_in, step = z["c%d_pts_input" % k], float(z["c%d_step" % k])
        assert np.array_equal(t["empty"], z["c%d_empty" % k]), n
        assert same_bits(t["pooled_xyz"], z["c%d_pooled_xyz" % k]) and same_bits(t["pts_features"], z["c%d_pts_features" % k]), n
        assert same_bits(t["pts_input"][:, :, 3:], ref_in[:, :, 3:]), n
        assert np.array_equal(t["cls_label"], z["c%d_cls_label" % k]) and np.array_equal(t["reg_valid_mask"], z["c%d_reg_valid_mask" % k]), n
        assert np.abs(t["pts_input"][:, :, :3].astype(np.float64) - ref_in[:, :, :3]).max() <= (float(z["steps_xyz"]) + 1) * step, n
        assert np.abs(t["gt_boxes3d_ct"][:, :6].astype(np.float64) - z["c%d_gt_ct" % k][:, :6]).max() <= (float(z["steps_ct"]) + 1) * step, n
        assert same_bits(t["roi_boxes3d"][:, 3:6], z["c%d_info_rois" % k][:, 3:6]) and same_bits(t["gt_boxes3d"][:, 3:6], z["c%d_info_gt" % k][:, 3:6]), n
        ry_step = float(np.spacing(F32(2 * np.pi)))
        for a, b in ((t["roi_boxes3d"], z["c%d_info_rois" % k]), (t["gt_boxes3d"], z["c%d_info_gt" % k]), (t["gt_boxes3d_ct"], z["c%d_gt_ct" % k])):
            assert np.abs(a[:, 6].astype(np.float64) - b[:, 6]).max() <= (float(z["steps_ry"]) + 1) * ry_step, n
        u = _twin_frame(z, k, sample_trig=(np.cos, np.sin), atan2=np.arctan2)
        for a, b in ((u["roi_boxes3d"], z["c%d_info_rois" % k]), (u["gt_boxes3d"], z["c%d_info_gt" % k]), (u["gt_boxes3d_ct"], z["c%d_gt_ct" % k])):
            assert same_bits(a[:, 6], b[:, 6]), n
        for r in range(len(t["empty"])):
            distinct = len(np.unique(t["pooled_xyz"][r], axis=0))
            if t["empty"][r]:
                seen["empty"] += 1
                assert t["cls_label"][r] == -1 and t["reg_valid_mask"][r] == 0 and not t["pts_features"][r].any() and not t["pooled_xyz"][r].any()
            elif distinct < rc.S_POINTS:
                seen["wrapped"] += 1                                # fewer than S points: wrap-around copies
                assert same_bits(t["pooled_xyz"][r, distinct:2 * distinct], t["pooled_xyz"][r, :min(distinct, rc.S_POINTS - distinct)])
            else:
                seen["full"] += 1                                   # S or more points: the first S
        aug, ui = rc.frame_config(k)
        seen["aug"].add(aug), seen["ui"].add(ui)
    assert seen["empty"] and seen["wrapped"] and seen["full"] and seen["aug"] == {True, False} and seen["ui"] == {True, False}, seen
    assert float(z["steps_xyz"]) <= 4 and float(z["steps_ct"]) <= 4 and float(z["steps_ry"]) <= 3        # what was measured, not a bar chosen here


def _finish_records(roi, gt, pt, methods, seed, frame, slot):
    n = len(roi)
    ints = np.stack([np.broadcast_to(np.asarray(v, np.int32), (n,)) for v in (methods, seed, frame, slot)], 1).astype(np.int32)
    return np.concatenate([np.asarray(roi, F32), np.asarray(gt, F32), np.asarray(pt, F32), ints.view(F32)], 1)


def _finish_twin(roi, gt, pt, methods, seed, frame, slot):
    out = []
    for i in range(len(roi)):
        names = tuple(m for m, bit in ot.METHOD_BITS.items() if int(methods[i]) & bit)
        a = ot.aug_draw(int(seed[i]), int(frame[i]), int(slot[i]), names, 0.5, 18)
        p, r, g, ct = ot.finish_slot(pt[i:i + 1], roi[i], gt[i], a)
        out.append(np.concatenate([r, g, ct, p[0]]))
    return np.stack(out).astype(F32)


def test_finish_arithmetic_of_the_header_equals_the_twin_bit_for_bit(host):
    """rotate / scale / flip of a point and of both boxes, gt_boxes3d_ct and the canonical transform: the fixture's slots (their
    first pooled point) and 10 000 random slots with every combination of methods"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "rcnn_offline_ref.npz"))
    for k, n in enumerate(z["names"]):
        if str(z["c%d_raised" % k]):
            continue
        R = int(z["c%d_R" % k])
        args = (z["c%d_rois" % k], z["c%d_gt_of_rois" % k], z["c%d_pooled_xyz" % k][:, 0], np.full(R, 7 if rc.frame_config(k)[0] else 0),
                np.full(R, int(z["seed"])), np.full(R, k), np.arange(R))
        assert same_bits(host("finish", _finish_records(*args)), _finish_twin(*args)), n
    rng = np.random.default_rng(17)
    m = 10000
    gt = rc.labels(rng, m)
    gt[:, 0] += rng.uniform(-30, 30, m).astype(F32)
    roi = np.stack([rc.moved(rng, gt[i], "near" if i % 2 else "hard") for i in range(m)])
    roi[:, 6] += rng.choice([0, 2 * np.pi, -2 * np.pi, 7.0], m).astype(F32)             # ry outside one turn: the float32 remainder
    pt = (gt[:, :3] + rng.normal(0, 2, (m, 3))).astype(F32)
    args = (roi, gt, pt, rng.integers(0, 8, m), rng.integers(0, 2 ** 31 - 1, m), rng.integers(0, 8000, m), rng.integers(0, 64, m))
    got, want = host("finish", _finish_records(*args)), _finish_twin(*args)
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), "%d values differ, first at %s" % ((~same).sum(), np.argwhere(~same)[0])
