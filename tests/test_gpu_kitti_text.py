"""GPU: the KITTI result text formatted on the device (csrc/kitti_text.hip) against the host build of the same header
(tests/kitti_text_host.cpp): byte-identical text, lengths, statuses, rows and flags; kitti_output.DeviceResultWriter's files; the three
evaluation loops of pointrcnn_amd/eval_stats.py on a tiny synthetic tree.  The bounds against the host route's files are those of
tests/test_kitti_text_cpu.py: same lines in the same order, a field may move by one unit of the fourth decimal (numpy's trigonometry
against the host libm's, which the device restates), at most 1 field in 100 moves."""
import os

import numpy as np
import pytest
import torch

import kitti_text_cases as kc
import kitti_tree
from test_kitti_text_cpu import compare_with_recorded

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    work = tmp_path_factory.mktemp("kitti_text_host_gpu")
    return kc.build_host(work, False), work


def device_lines(dev, batch):
    from pointrcnn_amd import ops
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)      # noqa: E731
    keep, num = batch.get("keep"), batch.get("num")
    text, text_len, status, rows, valid = ops.kitti_result_text(
        t(batch["boxes"], F32), t(batch["scores"], F32), t(batch["P2"], np.float64), t(batch["img_hw"], np.int32),
        keep=None if keep is None else t(keep, np.int32), num=None if num is None else t(num, np.int32),
        class_name=batch.get("class_name", "Car"), want_rows=True)
    return {"text": text.cpu().numpy(), "text_len": text_len.cpu().numpy(), "status": status.cpu().numpy(), "rows": rows.cpu().numpy(),
            "valid": valid.cpu().numpy()}


def assert_same(got, want):
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["text_len"], want["text_len"])
    assert np.array_equal(got["valid"], want["valid"])
    assert np.array_equal(got["rows"].view(np.uint64), want["rows"].view(np.uint64))
    for b in range(len(want["status"])):                                          # bytes past text_len mean nothing
        n = int(want["text_len"][b])
        assert np.array_equal(got["text"][b, :n], want["text"][b, :n]), b


def _shuffled_subset(M, n, seed):
    keep = np.full((M,), -1, np.int32)
    keep[:n] = np.random.default_rng(seed).permutation(M)[:n]
    return keep


def _cases():
    out = {}
    M = 40
    keep = np.stack([_shuffled_subset(M, 17, 0), np.arange(M, dtype=np.int32), np.arange(M, dtype=np.int32)])
    out["B3_M40_keep_num"] = kc.make_batch((1, 2, 5), keep=keep, num=[17, 0, 40])
    out["B3_M40_all"] = kc.make_batch((1, 2, 5))
    out["B3_M40_num_only_pedestrian"] = kc.make_batch((1, 2, 5), num=[0, 17, 40], class_name="Pedestrian")
    one = kc.make_batch((3,))
    j = int(np.flatnonzero(kc.numpy_valid(one, 0))[0])
    out["B1_M1"] = {k: (v[:, j:j + 1].copy() if k in ("boxes", "scores") else v) for k, v in one.items()}
    out["B2_M130"] = kc.make_batch((4, 6), n=130)
    out["B1_M512"] = kc.make_batch((8,), n=512)
    out["B2_M512_keep"] = kc.make_batch((9, 10), n=512, keep=np.stack([_shuffled_subset(512, 300, 1), _shuffled_subset(512, 512, 2)]), num=[300, 512])
    # the formatter's edge values in boxes the size test keeps: ties (2j+1)/32, signed zeros, values that round to zero, in h w l
    # (positive, small: the box stays kept), ry and y (either sign); everything up to the top of the float32 domain in the score
    edge = kc.make_batch((1, 2))
    kept = np.flatnonzero(kc.numpy_valid(edge, 0))[:24]
    ties = [(2 * j + 1) / 32 for j in (0, 1, 2, 7, 15, 40)]
    small = ties + [0.0, 1e-5, 0.00005, 0.99995, 0.00015, 1.00005]
    for k, i in enumerate(kept):
        edge["boxes"][0, i, 3 + k % 3] = F32(small[k % len(small)])
        edge["boxes"][0, i, 6] = F32([1, -1][k % 2] * small[(k + 5) % len(small)]) if k % 3 else F32(-0.0)
        edge["boxes"][0, i, 1] = F32([-1, 1][k % 2] * small[(k + 2) % len(small)])
    big = [v for v in kc.EDGE_VALUES if abs(float(F32(v))) < 2.0 ** 31] + [2147483520.0, -2147483520.0, 1241.0] + ties + [-t for t in ties]
    big += [(2 * j + 1) / 32 for j in (1000, 12345, 2 ** 20 + 1)]
    edge["scores"][0, kept] = np.resize(np.array(big, np.float64).astype(F32), len(kept))
    edge["scores"][1, :len(big)] = np.array(big, np.float64).astype(F32)
    edge["_kept"] = kept
    out["edge_values"] = edge
    bad = kc.make_batch((1, 2, 5, 6))
    first_kept = [int(np.flatnonzero(kc.numpy_valid(bad, b))[2]) for b in range(4)]
    bad["scores"][0, first_kept[0]] = np.inf                                      # frame 0: +inf in a kept box -> 1
    bad["scores"][1, first_kept[1]] = F32(3e9)                                    # frame 1: finite, 2^31 and above, in a kept box -> 1
    bad["keep"] = np.tile(np.arange(40, dtype=np.int32), (4, 1))
    bad["keep"][2, 3] = 40                                                        # frame 2: an index outside the frame -> 2
    bad["boxes"][3, first_kept[3], 6] = np.nan                                    # frame 3: a NaN angle drops the box -> 0
    bad["scores"][3, 0] = np.nan                                                  # ... and so does a NaN score in a box the size test drops
    bad["num"] = np.array([40, 40, 40, 40], np.int32)
    bad["_nan_box"] = first_kept[3]
    out["out_of_domain"] = bad
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_is_byte_identical_to_the_host_program(dev, host, name):
    exe, work = host
    batch = CASES[name]
    want = kc.run_lines(exe, work, batch)
    got = device_lines(dev, batch)
    assert_same(got, want)
    B, M = batch["scores"].shape
    if name == "out_of_domain":
        assert want["status"].tolist() == [1, 1, 2, 0] and want["valid"][3, batch["_nan_box"]] == 0 and want["valid"][3, 0] == 0
        assert kc.frame_lines(got, 3) == kc.python_lines(got["rows"][3], got["valid"][3]) and len(kc.frame_lines(got, 3)) > 10
    else:
        assert not want["status"].any()
        for b in range(B):
            lines = kc.frame_lines(got, b)
            assert lines == kc.python_lines(got["rows"][b], got["valid"][b], batch.get("class_name", "Car"))
        assert sum(len(kc.frame_lines(got, b)) for b in range(B)) > 0
    if name == "edge_values":
        assert want["valid"][0, batch["_kept"]].all()
        text = got["text"][0, :got["text_len"][0]].tobytes()
        for s in (b" -0.0000", b" 2147483520.0000", b" -2147483520.0000", b" 1241.0000", b" 0.0312", b" 0.0938", b" 0.4688"):
            assert s in text, s
    if name == "B1_M512":
        assert int(got["valid"].sum()) > 400 and int(got["text_len"][0]) > 400 * 90


def test_nothing_to_do_and_argument_errors(dev):
    from pointrcnn_amd import _cabi, ops
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)         # noqa: E731
    text, text_len, status = ops.kitti_result_text(z(2, 0, 7), z(2, 0), z(2, 12, dt=torch.float64), z(2, 2, dt=torch.int32))
    assert text.shape == (2, 0) and not text_len.any().item() and not status.any().item()
    with pytest.raises(_cabi.PointOpsError, match="class name"):
        ops.kitti_result_text(z(1, 4, 7), z(1, 4), z(1, 12, dt=torch.float64), z(1, 2, dt=torch.int32), class_name="")
    with pytest.raises(_cabi.PointOpsError, match="class name"):
        ops.kitti_result_text(z(1, 4, 7), z(1, 4), z(1, 12, dt=torch.float64), z(1, 2, dt=torch.int32), class_name="x" * 16)
    with pytest.raises(ValueError, match="P2"):
        ops.kitti_result_text(z(1, 4, 7), z(1, 4), z(2, 12, dt=torch.float64), z(1, 2, dt=torch.int32))
    L = _cabi.lib()
    assert L.prcnn_kitti_result_text(None, None, None, None, 1, 4, None, None, b"Car", None, None, None, None, None, None) == -1
    assert b"null pointer" in L.prcnn_last_error()
    assert L.prcnn_kitti_result_text(None, None, None, None, 0, 4, None, None, b"Car", None, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- the writer
class _Calib:
    def __init__(self, P2):
        self.P2 = np.asarray(P2, np.float64).reshape(3, 4)


def _writer_inputs(dev, batch):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)      # noqa: E731
    keep, num = batch.get("keep"), batch.get("num")
    return (t(batch["boxes"], F32), t(batch["scores"], F32), None if keep is None else t(keep, np.int32), None if num is None else t(num, np.int32),
            [_Calib(p) for p in batch["P2"]], [tuple(hw) for hw in batch["img_hw"]])


def test_writer_files_parse_back_and_declined_frames_take_the_host_route(dev, host, tmp_path):
    from pointrcnn_amd import kitti_eval, kitti_output
    exe, work = host
    batch = kc.make_batch((1, 2, 5, 6), keep=np.tile(np.arange(40, dtype=np.int32), (4, 1)), num=[40, 0, 40, 23])
    batch["scores"][2, :] = np.where(np.arange(40) % 7 == 0, np.nan, batch["scores"][2])          # frame 2: NaN scores in kept boxes
    want = kc.run_lines(exe, work, batch)
    assert want["status"].tolist() == [0, 0, 1, 0]
    writer = kitti_output.DeviceResultWriter(dev)
    args = _writer_inputs(dev, batch)
    ids = [11, 12, 13, 14]
    h = writer.format(*args, class_name="Car")
    assert writer.lines(h) == writer.lines(h)
    out_dir, skip_dir, host_dir = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    blobs = writer.write(h, ids, out_dir)
    writer.write(h, ids, skip_dir, skip_empty=True)
    assert sorted(os.listdir(out_dir)) == ["%06d.txt" % i for i in ids] and os.path.getsize(os.path.join(out_dir, "000012.txt")) == 0
    assert sorted(os.listdir(skip_dir)) == ["%06d.txt" % i for i in (11, 13, 14)]                  # num = 0: left to the empty-file dump
    os.makedirs(host_dir)
    for b, sid in enumerate(ids):
        n = int(batch["num"][b])
        data = open(os.path.join(out_dir, "%06d.txt" % sid), "rb").read()
        assert data == blobs[b]
        if want["status"][b] == 0:
            assert data == want["text"][b, :want["text_len"][b]].tobytes()
            anno = kitti_eval.get_label_anno(os.path.join(out_dir, "%06d.txt" % sid))
            rows = want["rows"][b][want["valid"][b].astype(bool)]
            printed = np.array([[float("%.4f" % v) for v in r] for r in rows.tolist()]).reshape(-1, 13)
            assert len(anno["name"]) == len(rows) and (n == 0 or set(anno["name"]) == {"Car"})
            if len(rows):
                assert np.array_equal(anno["alpha"], printed[:, 0]) and np.array_equal(anno["bbox"], printed[:, 1:5])
                assert np.array_equal(anno["dimensions"], printed[:, [7, 5, 6]])                   # the evaluator's l, h, w order
                assert np.array_equal(anno["location"], printed[:, 8:11]) and np.array_equal(anno["rotation_y"], printed[:, 11])
                assert np.array_equal(anno["score"], printed[:, 12])
        else:                                                                                      # the host route, byte for byte
            kitti_output.save_kitti_format(sid, args[4][b], batch["boxes"][b][:n], host_dir, batch["scores"][b][:n], batch["img_hw"][b])
            assert data == open(os.path.join(host_dir, "%06d.txt" % sid), "rb").read() and b"nan" in data
    bad = dict(batch, keep=batch["keep"].copy())
    bad["keep"][0, 0] = -1
    with pytest.raises(ValueError, match="outside"):
        writer.lines(writer.format(*_writer_inputs(dev, bad)))
    # buffers are reused in turn: a handle older than `depth` batches says so instead of returning another batch's text
    h0 = writer.format(*args)
    writer.format(*args), writer.format(*args)
    with pytest.raises(RuntimeError, match="later batch"):
        writer.lines(h0)


# ---------------------------------------------------------------------------------------------- the loops
def _tree(tmp_path, frames):
    from pointrcnn_amd import kitti_input
    training = kitti_tree.write_tree(tmp_path, frames, n_scan=2000)
    return training, os.path.join(str(tmp_path), "KITTI", "ImageSets", "val.txt"), kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)


def _check_files_against_host_route(dir_dev, dir_host, names):
    differ = total = 0
    for n in names:
        a, b = open(os.path.join(dir_dev, n)).read().splitlines(), open(os.path.join(dir_host, n)).read().splitlines()
        d, t = compare_with_recorded(a, b)
        differ, total = differ + d, total + t
    print("fields that differ from the host route", differ, "of", total)
    assert differ * 100 <= total
    return total


def _host_text(host, boxes, scores, keep, num, calib, shapes, class_name="Car"):
    exe, work = host
    B = boxes.shape[0]
    batch = {"boxes": boxes, "scores": scores, "P2": np.tile(np.asarray(calib.P2, np.float64).reshape(1, 12), (B, 1)),
             "img_hw": np.array([s[:2] for s in shapes], np.int32), "class_name": class_name}
    if keep is not None:
        batch["keep"], batch["num"] = keep, num
    out = kc.run_lines(exe, work, batch)
    assert not out["status"].any()
    return [out["text"][b, :out["text_len"][b]].tobytes() for b in range(B)]


def test_joint_loop_with_the_device_writer(dev, host, tmp_path):
    from pointrcnn_amd import eval_stats, kitti_output
    from pointrcnn_amd.point_rcnn import PointRCNN
    from pointrcnn_amd.rpn import randomize_bn_stats, synthetic_clouds
    frames = [0, 1, 2, 3, 4]                                          # frame 4 is in the split but in no batch
    training, split_file, calib = _tree(tmp_path, frames)
    torch.manual_seed(0)
    model = randomize_bn_stats(PointRCNN(mode="TEST")).to(dev).eval()
    pts = synthetic_clouds(4, 16384, device=dev)
    with torch.no_grad():
        pred0 = model.detections(model({"pts_input": pts}), score_thresh=0.3)[0].cpu().numpy()
    gt = np.zeros((4, 5, 7), F32)
    for b in range(4):
        gt[b, :2 + b % 3] = pred0[b, :2 + b % 3]
    seen = []
    detections = model.detections

    def recording(ret, **kw):
        out = detections(ret, **kw)
        seen.append([t.cpu().numpy() for t in out])
        return out
    model.detections = recording
    batches = [{"sample_id": np.array([0, 1]), "pts_input": pts[:2], "gt_boxes3d": gt[:2]},
               {"sample_id": np.array([2, 3]), "pts_input": pts[2:], "gt_boxes3d": gt[2:]}]
    dirs = [str(tmp_path / "host"), str(tmp_path / "device")]
    rets = [eval_stats.eval_one_epoch_joint(model, batches, d, lambda i: calib, kitti_tree.image_shape, split_file=split_file, writer=w)
            for d, w in zip(dirs, (None, kitti_output.DeviceResultWriter(dev)))]
    assert rets[0] == rets[1] and rets[0]["rcnn_avg_num"] > 0
    out = [os.path.join(d, "final_result", "data") for d in dirs]
    names = ["%06d.txt" % f for f in frames]
    assert sorted(os.listdir(out[0])) == sorted(os.listdir(out[1])) == names
    assert _check_files_against_host_route(out[1], out[0], names) > 0
    for k, (pred, raw, keep, num) in enumerate(seen[2:]):            # the second run's batches: the files are the host program's bytes
        ids = [2 * k, 2 * k + 1]
        want = _host_text(host, pred, raw, keep, num, calib, [kitti_tree.image_shape(i) for i in ids])
        for sid, w in zip(ids, want):
            assert open(os.path.join(out[1], "%06d.txt" % sid), "rb").read() == w


def _rpn_batches(pts, dev, with_labels=True):
    rng = np.random.default_rng(5)
    B, N = pts.shape[:2]
    out = []
    for k in range(0, B, 2):
        d = {"sample_id": np.array([k, k + 1]), "pts_input": pts[k:k + 2], "pts_rect": pts[k:k + 2].cpu().numpy(),
             "pts_features": rng.uniform(0, 1, (2, N, 1)).astype(F32)}
        if with_labels:
            d["rpn_cls_label"] = rng.integers(-1, 2, (2, N)).astype(np.int32)
            d["gt_boxes3d"] = np.zeros((2, 3, 7), F32)
        out.append(d)
    return out


def _run_rpn_loop(dev, tmp_path, with_labels=True):
    from pointrcnn_amd import eval_stats
    from pointrcnn_amd.point_rcnn import PointRCNN
    from pointrcnn_amd.rpn import randomize_bn_stats, synthetic_clouds
    training, split_file, calib = _tree(tmp_path, [0, 1, 2, 3])
    torch.manual_seed(0)
    model = randomize_bn_stats(PointRCNN(mode="TEST")).to(dev).eval()
    pts = synthetic_clouds(4, 16384, device=dev)
    batches = _rpn_batches(pts, dev, with_labels)
    with torch.no_grad():
        first = model.rpn({"pts_input": pts})
        rois0 = model.rpn.proposal_layer(first["rpn_cls"][:, :, 0].contiguous(), first["rpn_reg"], first["backbone_xyz"])[0].cpu().numpy()
    if with_labels:
        for d in batches:
            for b, sid in enumerate(d["sample_id"]):
                d["gt_boxes3d"][b, :2] = rois0[sid, :2] + F32(0.05)
    result_dir = str(tmp_path / "rpn_out")
    ret = eval_stats.eval_one_epoch_rpn(model, batches, result_dir, lambda i: calib, kitti_tree.image_shape, save_rpn_feature=True)
    return model, batches, calib, training, split_file, result_dir, ret


def test_rpn_loop_dumps_what_the_model_computed(dev, host, tmp_path):
    from pointrcnn_amd import eval_stats, kitti_input, kitti_output
    model, batches, calib, training, split_file, result_dir, ret = _run_rpn_loop(dev, tmp_path)
    stats = eval_stats.EvalStats("rpn", dev)
    for d in batches:
        with torch.no_grad():
            r = model.rpn({"pts_input": d["pts_input"]})
            raw = r["rpn_cls"][:, :, 0].contiguous()
            seg = (torch.sigmoid(raw) > 0.3).float()
            rois, scores = model.rpn.proposal_layer(raw, r["rpn_reg"], r["backbone_xyz"])
        label = torch.from_numpy(d["rpn_cls_label"]).to(dev).long()
        stats.update(rois.contiguous(), torch.from_numpy(d["gt_boxes3d"]).to(dev), seg_result=seg, rpn_cls_label=label)
        ids = [int(i) for i in d["sample_id"]]
        want = _host_text(host, rois.cpu().numpy(), scores.cpu().numpy(), None, None, calib, [kitti_tree.image_shape(i) for i in ids])
        for b, sid in enumerate(ids):
            f = {k: np.load(p) for k, p in kitti_output.rpn_feature_files(os.path.join(result_dir, "features"), sid).items()}
            assert f["features"].dtype == f["xyz"].dtype == f["seg"].dtype == f["rawscore"].dtype == f["intensity"].dtype == F32
            assert np.array_equal(f["features"], r["backbone_features"][b].cpu().numpy().T) and f["features"].shape == (16384, 128)
            assert np.array_equal(f["xyz"], r["backbone_xyz"][b].cpu().numpy()) and np.array_equal(f["seg"], seg[b].cpu().numpy())
            assert np.array_equal(f["rawscore"], raw[b].cpu().numpy()) and np.array_equal(f["intensity"], d["pts_features"][b][:, 0])
            packed = np.load(os.path.join(result_dir, "seg_result", "%06d.npy" % sid))
            numpy_way = np.concatenate((d["pts_rect"][b].reshape(-1, 3), d["rpn_cls_label"][b].astype(np.int64).reshape(-1, 1),
                                        seg[b].long().cpu().numpy().reshape(-1, 1)), axis=1).astype(np.float16)
            assert packed.dtype == np.float16 and np.array_equal(packed.view(np.uint16), numpy_way.view(np.uint16))
            assert open(os.path.join(result_dir, "detections", "data", "%06d.txt" % sid), "rb").read() == want[b]
            fr = kitti_input.load_rcnn_offline_frame(os.path.join(result_dir, "features"), os.path.join(result_dir, "detections", "data"),
                                                     kitti_tree.label_lines(d["gt_boxes3d"][b, :2], calib.P2, kitti_tree.image_shape(sid)), sid)
            assert fr["rpn_xyz"].shape == (16384, 3) and fr["rpn_features"].shape == (16384, 128) and fr["gt_boxes3d"].shape[1] == 7
            kept = want[b].count(b"\n")
            assert fr["roi_boxes3d"].shape == (kept, 7) and 0 < kept <= 100
    assert ret == stats.result() and set(ret) == {"max_obj_num", "rpn_iou"} | {"rpn_recall(thresh=%.2f)" % t for t in eval_stats.THRESH_LIST}
    assert ret["rpn_recall(thresh=0.50)"] > 0


def test_rpn_loop_without_labels_packs_two_columns_less(dev, tmp_path):
    model, batches, calib, training, split_file, result_dir, ret = _run_rpn_loop(dev, tmp_path, with_labels=False)
    packed = np.load(os.path.join(result_dir, "seg_result", "000003.npy"))
    assert packed.shape == (16384, 4) and packed.dtype == np.float16
    assert np.array_equal(packed[:, :3], batches[1]["pts_rect"][1].astype(np.float16)) and set(np.unique(packed[:, 3])) <= {0.0, 1.0}


def test_rcnn_loop_on_the_rpn_dumps(dev, host, tmp_path):
    from pointrcnn_amd import eval_stats, kitti_input, kitti_output, ops
    from pointrcnn_amd.proposal_layer import CLS_MEAN_SIZE, _anchor3
    from pointrcnn_amd.rcnn import RCNNConfig, RCNNNet
    from pointrcnn_amd.rpn import randomize_bn_stats
    model, batches, calib, training, split_file, rpn_dir, _ = _run_rpn_loop(dev, tmp_path)
    cfg = type("Cfg", (RCNNConfig,), dict(ROI_SAMPLE_JIT=False))
    frames = []
    for d in batches:
        for b, sid in enumerate(int(i) for i in d["sample_id"]):
            frames.append(kitti_input.load_rcnn_offline_frame(
                os.path.join(rpn_dir, "features"), os.path.join(rpn_dir, "detections", "data"),
                kitti_tree.label_lines(d["gt_boxes3d"][b, :2], calib.P2, kitti_tree.image_shape(sid)), sid))
    assert any(len(f["gt_boxes3d"]) for f in frames)
    torch.manual_seed(1)
    net = randomize_bn_stats(RCNNNet(cfg=cfg)).to(dev).eval()
    prep = kitti_input.RCNNOfflinePreparer(cfg, dev)
    result_dir = str(tmp_path / "rcnn_out")
    ret = eval_stats.eval_one_epoch_rcnn(net, prep, [frames[:2], frames[2:]], result_dir, lambda i: calib, kitti_tree.image_shape,
                                         split_file=split_file, save_result=True, score_thresh=0.3)
    keys = {"empty_cnt", "rcnn_cls_acc", "rcnn_cls_acc_refined", "rcnn_avg_num"}
    keys |= {"%s_recall(thresh=%.2f)" % (s, t) for s in ("rpn", "rcnn") for t in eval_stats.THRESH_LIST}
    assert set(ret) == keys
    # the same numbers frame by frame, composed from the existing operators
    stats = eval_stats.EvalStats("rcnn", dev, cls_fg=cfg.CLS_FG_THRESH, cls_bg=cfg.CLS_BG_THRESH)
    empty = 0
    for f in frames:
        sid, shape = f["sample_id"], kitti_tree.image_shape(f["sample_id"])
        with torch.no_grad():
            d = prep.eval_batch(prep.pack([f]))
            out = net({"pts_input": d["pts_input"], "pts_features": d["pts_features"], "roi_boxes3d": d["roi_boxes3d"]})
            pred = ops.decode_bbox_target(d["roi_boxes3d"].contiguous(), out["rcnn_reg"].contiguous(), cfg.LOC_SCOPE, cfg.LOC_BIN_SIZE,
                                          cfg.NUM_HEAD_BIN, _anchor3(CLS_MEAN_SIZE[0]), True, cfg.LOC_Y_BY_BIN, cfg.LOC_Y_SCOPE,
                                          cfg.LOC_Y_BIN_SIZE, True)
            raw = out["rcnn_cls"].reshape(1, -1).contiguous()
            pred_class = torch.sigmoid(raw) > 0.3
            keep, num = ops.nms_batched(pred[None], raw, pred_class, cfg.NMS_THRESH, True)
            if len(f["gt_boxes3d"]):                                                # what the reference's dataset attaches as gt_iou
                corners = [torch.from_numpy(kitti_output.box_corners(x)).to(dev) for x in (f["roi_boxes3d"], f["gt_boxes3d"])]
                gt_iou = ops.corner_iou3d(*corners).max(dim=1)[0].view(1, -1).contiguous()
            else:
                gt_iou = torch.zeros((1, len(f["roi_boxes3d"])), device=dev)
            stats.update(d["roi_boxes3d"][None].contiguous(), torch.from_numpy(f["gt_boxes3d"][None]).to(dev), pred_boxes3d=pred[None].contiguous(),
                         det_num=num, pred_class=pred_class, gt_iou=gt_iou)
        n = len(f["roi_boxes3d"])
        rows = np.arange(n, dtype=np.int32)[None]
        for sub, boxes, scores, kp, nm in (("final_result", pred, raw, keep, num), ("refine_result", pred, raw, rows, [n]),
                                           ("roi_result", d["roi_boxes3d"], d["roi_scores"], rows, [n])):
            to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)      # noqa: E731
            want = _host_text(host, to_np(boxes).reshape(1, n, 7), to_np(scores).reshape(1, n), to_np(kp).astype(np.int32).reshape(1, -1),
                              np.asarray(to_np(nm), np.int32).reshape(1), calib, [shape])[0]
            path = os.path.join(result_dir, sub, "data", "%06d.txt" % sid)
            if sub == "final_result" and int(num[0]) == 0:
                empty += 1
                assert os.path.getsize(path) == 0
            else:
                assert open(path, "rb").read() == want, (sub, sid)
    want_ret = stats.result()
    want_ret.pop("rpn_iou")
    assert ret["empty_cnt"] == empty
    for k, v in want_ret.items():
        assert ret[k] == v, k
    # SIZE_RES_ON_ROI: the RoI's own size is the anchor of the size residual (eval_rcnn.py:306-308)
    cfg_roi = type("CfgRoi", (cfg,), dict(SIZE_RES_ON_ROI=True))
    prep_roi = kitti_input.RCNNOfflinePreparer(cfg_roi, dev)
    f = frames[0]
    eval_stats.eval_one_epoch_rcnn(net, prep_roi, [[f]], str(tmp_path / "rcnn_roi"), lambda i: calib, kitti_tree.image_shape, save_result=True)
    with torch.no_grad():
        d = prep_roi.eval_batch(prep_roi.pack([f]))
        out = net({"pts_input": d["pts_input"], "pts_features": d["pts_features"], "roi_boxes3d": d["roi_boxes3d"]})
        pred = ops.decode_bbox_target(d["roi_boxes3d"].contiguous(), out["rcnn_reg"].contiguous(), cfg.LOC_SCOPE, cfg.LOC_BIN_SIZE,
                                      cfg.NUM_HEAD_BIN, _anchor3(CLS_MEAN_SIZE[0]), True, cfg.LOC_Y_BY_BIN, cfg.LOC_Y_SCOPE, cfg.LOC_Y_BIN_SIZE, True)
        anchored = pred.clone()
        pred[:, 3:6] = out["rcnn_reg"][:, -3:] * d["roi_boxes3d"][:, 3:6] + d["roi_boxes3d"][:, 3:6]
    assert not torch.equal(pred, anchored)
    n = len(f["roi_boxes3d"])
    want = _host_text(host, pred.cpu().numpy().reshape(1, n, 7), out["rcnn_cls"].reshape(1, n).cpu().numpy(), np.arange(n, dtype=np.int32)[None],
                      np.array([n], np.int32), calib, [kitti_tree.image_shape(f["sample_id"])])[0]
    assert open(os.path.join(str(tmp_path / "rcnn_roi"), "refine_result", "data", "%06d.txt" % f["sample_id"]), "rb").read() == want
    multi = type("Net", (torch.nn.Module,), {"forward": lambda self, x: {"rcnn_cls": torch.zeros((x["roi_boxes3d"].shape[0], 2), device=dev),
                                                                          "rcnn_reg": torch.zeros((x["roi_boxes3d"].shape[0], 46), device=dev)}})()
    multi.p = torch.nn.Parameter(torch.zeros(1, device=dev))
    with pytest.raises(NotImplementedError, match="multi-class"):
        eval_stats.eval_one_epoch_rcnn(multi, prep, [frames[:1]], str(tmp_path / "multi"), lambda i: calib, kitti_tree.image_shape)
