"""Offline GT-augmented scenes (the train_aug split), host side, no GPU: the numpy twin (tests/aug_scene_twin.py) against the reference's
own tools/generate_aug_scene.py (fixture tests/golden/aug_scene_ref.npz, made by tests/golden/ref_aug_scene.py), the generator's host
backend against the twin, the readers, the truncation / occlusion lookup, csrc/aug_scene_math.h compiled for the host (plain and with
-fsanitize=address,undefined, run as a program) and the C ABI's four new entry points."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import aug_scene_twin as tw
from util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
RTOL, ATOL = 2e-6, 2e-5              # tests/test_gt_database_cpu.py: the reference's BLAS sgemm against the canonical transform
EXPORTS = ("prcnn_aug_scene_sample", "prcnn_aug_scene_workspace_bytes", "prcnn_aug_scene_count", "prcnn_aug_scene_fill")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "aug_scene_ref.npz")))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("aug_scene_tree"))
    tw.write_aug_tree(root)
    return root


@pytest.fixture(scope="module")
def twin(gold, tree):
    return tw.generate(tree, int(gold["aug_times"]), int(gold["seed"]))


def test_twin_sampler_equals_the_reference_tool(gold, twin):
    want, _ = twin
    assert sorted(want) == [int(i) for i in gold["ids"]] == [e * 10000 + f for e in (1, 2) for f in tw.FRAMES]
    accepted = set()
    for i in want:
        t = want[i]
        assert t["status"] == int(gold["f%d_status" % i]), i
        assert np.array_equal(t["ids"], gold["f%d_ids" % i]), i
        assert t["boxes"].dtype == np.float32 and np.array_equal(t["boxes"], gold["f%d_boxes" % i]), i
        assert np.array_equal(t["y_shift"], gold["f%d_y_shift" % i]), i
        assert (t["stats"][0], t["stats"][2]) == tuple(int(v) for v in gold["f%d_stats" % i]), i          # extra_gt_num, tries spent
        assert len(t["ids"]) <= t["stats"][1] <= t["stats"][0] + 1 <= 15
        accepted |= set(int(v) for v in t["ids"])
    # what the tree was built to show
    assert [want[10000 + f]["status"] for f in tw.FRAMES] == [0, 0, 1, 0]
    assert len(want[10003]["ids"]) == 0 and want[10003]["stats"][1] == want[10003]["stats"][0] + 1       # every candidate collides
    assert len(want[10000]["ids"]) >= 5 and not np.array_equal(want[10000]["ids"], want[20000]["ids"])   # the epochs of one frame differ
    d = tw.database_arrays()
    assert len(d["boxes"]) - 1 not in accepted and all(len(d["points"][k]) >= 5 for k in accepted)


def test_twin_clouds_labels_and_split_equal_the_reference_tool(gold, twin):
    want, split = twin
    assert "\n".join(split) == str(gold["split"]) and not str(gold["split"]).endswith("\n")
    pasted = dropped = 0
    for i in want:
        t, ref = want[i], gold["f%d_cloud" % i]
        assert t["labels"] == [str(s) for s in gold["f%d_labels" % i]], i
        assert t["cloud"].dtype == np.float32 and t["cloud"].shape == ref.shape, i
        raw = t["src"] >= 0
        assert (np.diff(t["src"][raw]) > 0).all() and not raw[int(raw.sum()):].any()                 # survivors in raw order, then the pasted
        print("frame %d: max |raw rows - reference| = %g" % (i, np.abs(t["cloud"][raw] - ref[raw]).max()))
        assert (np.abs(t["cloud"][raw, :3] - ref[raw, :3]) <= ATOL + RTOL * np.abs(ref[raw, :3])).all(), i
        assert np.array_equal(t["cloud"][raw, 3], ref[raw, 3]), i
        assert np.array_equal(t["cloud"][~raw], ref[~raw]), i                                         # pasted rows bit for bit
        pasted += int((~raw).sum())
        none = tw.build(np.zeros((0, 4), np.float32), np.zeros(24, np.float32), (1, 1), dict(t, status=1), None, None, None)
        assert none[0].shape == (0, 4)
        dropped += int(t["status"] == 0 and len(t["ids"]) > 0)
    assert pasted > 500 and dropped >= 4
    assert any(len(str(s).split(" ")) == 15 and str(s).split(" ")[1:3] == ["0.35", "2"] for i in want for s in gold["f%d_labels" % i])


def test_accepted_boxes_remove_scan_points(twin, tree):
    """the drop is exercised: some valid point of the tree lies inside an accepted box with h + 2"""
    from pointrcnn_amd import kitti_input
    want, _ = twin
    base = os.path.join(tree, "KITTI", "object", "training")
    removed = 0
    for i in want:
        scan = kitti_input.get_lidar(os.path.join(base, "velodyne", "%06d.bin" % (i % 10000)))
        calib = kitti_input.Calibration(os.path.join(base, "calib", "%06d.txt" % (i % 10000)))
        import kitti_tree
        plain = tw.build(scan, calib.packed(), kitti_tree.image_shape(i % 10000), dict(want[i], status=1), None, None, None)
        removed += plain[2] - int((want[i]["src"] >= 0).sum())
    assert removed > 0


@pytest.fixture(scope="module")
def host_files(gold, tree, tmp_path_factory, cpu):
    from pointrcnn_amd import kitti_input
    out = str(tmp_path_factory.mktemp("aug_scene_host"))
    gen = kitti_input.AugSceneGenerator(tree, tw.database("cpu"), device="cpu", backend="host", iou3d=cpu.boxes_iou3d)
    report = gen.generate(out, aug_times=int(gold["aug_times"]), seed=int(gold["seed"]), frames_per_batch=3,
                          image_sets_dir=os.path.join(out, "ImageSets"))
    return out, report, gen


def test_host_backend_writes_the_twins_files(host_files, twin):
    out, report, _ = host_files
    want, split = twin
    assert [r["sample_id"] for r in report] == sorted(want)
    for r in report:
        t = want[r["sample_id"]]
        assert r["status"] == t["status"] and r["count"] == len(t["ids"])
        with open(os.path.join(out, "rectified_data", "%06d.bin" % r["sample_id"]), "rb") as f:
            assert f.read() == t["cloud"].tobytes(), r
        with open(os.path.join(out, "aug_label", "%06d.txt" % r["sample_id"])) as f:
            assert f.read() == "".join(ln + "\n" for ln in t["labels"]), r
    with open(os.path.join(out, "train_aug.txt")) as f:
        assert f.read() == "\n".join(split)
    assert filecmp.cmp(os.path.join(out, "train_aug.txt"), os.path.join(out, "ImageSets", "train_aug.txt"), shallow=False)


def test_load_aug_frame_and_the_identity_calibration(host_files, tree, twin):
    from pointrcnn_amd import kitti_input
    out, _, _ = host_files
    want, _ = twin
    fr = kitti_input.load_aug_frame(tree, out, 10001)
    assert fr["rect_input"] and fr["sample_id"] == 10001 and fr["pts"].dtype == np.float32
    assert np.array_equal(fr["pts"], want[10001]["cloud"]) and fr["label_lines"] == [ln + "\n" for ln in want[10001]["labels"]]
    import kitti_tree
    assert fr["img_shape"] == kitti_tree.image_shape(1) + (3,) and np.allclose(fr["plane"], np.array([0.02, -1.0, 0.01, 1.7]) / np.linalg.norm([0.02, 1, 0.01]))
    row = fr["calib"].packed()
    assert np.array_equal(row, fr["calib"].packed(rect_input=True)) and np.array_equal(row[12:], fr["calib"].P2.reshape(-1))
    assert np.array_equal(kitti_input.lidar_to_rect_host(fr["pts"], row[:12].reshape(4, 3)), fr["pts"][:, :3])
    orig = kitti_input.load_aug_frame(tree, out, 1)
    assert not orig["rect_input"] and orig["pts"].shape == (tw.N_SCAN + 137, 4)
    assert np.array_equal(orig["calib"].packed(), kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT).packed())
    assert not np.array_equal(orig["calib"].packed(), row) and orig["label_lines"] == [ln + "\n" for ln in tw.frame_labels(1)]
    # a train_aug frame's labels are what load_rcnn_offline_frame's parser takes
    lab = kitti_input.read_label_lines(fr["label_lines"])
    assert len(lab["cls_type"]) == 1 + len(want[10001]["ids"]) and set(lab["cls_type"]) == {"Car"}


def test_truncation_and_occlusion_lookup(host_files, tree):
    from pointrcnn_amd import kitti_input
    _, _, gen = host_files
    d = tw.database_arrays()
    assert np.array_equal(gen.truncation, d["truncation"]) and np.array_equal(gen.occlusion, d["occlusion"])
    assert len(set(gen.occlusion)) == 4 and len(set(gen.truncation)) == 4
    anon = kitti_input.GTDatabase(d["boxes"], d["alpha"], d["points"], d["intensity"], 0.0, "cpu")
    with pytest.raises(ValueError, match="sample_id -1.*truncation= and occlusion="):
        kitti_input.AugSceneGenerator(tree, anon, device="cpu", backend="host", iou3d=lambda a, b: None)
    given = kitti_input.AugSceneGenerator(tree, anon, device="cpu", backend="host", iou3d=lambda a, b: None,
                                          truncation=d["truncation"], occlusion=d["occlusion"])
    assert np.array_equal(given.truncation, d["truncation"])
    moved = d["boxes"].copy()
    moved[3, 0] += np.float32(0.01)
    other = kitti_input.GTDatabase(moved, d["alpha"], d["points"], d["intensity"], 0.0, "cpu", d["sample_id"], d["cls_type"])
    with pytest.raises(ValueError, match="no label of frame 000007 has the box of database object 3"):
        kitti_input.AugSceneGenerator(tree, other, device="cpu", backend="host", iou3d=lambda a, b: None)
    with pytest.raises(ValueError, match="backend 'host' needs iou3d"):
        kitti_input.AugSceneGenerator(tree, anon, device="cpu", backend="host")
    with pytest.raises(ValueError, match="go together"):
        kitti_input.AugSceneGenerator(tree, anon, device="cpu", truncation=d["truncation"])


def test_other_classes_skip_frames_without_kept_labels(tree, tmp_path, cpu):
    from pointrcnn_amd import kitti_input
    d = tw.database_arrays()
    gen = kitti_input.AugSceneGenerator(tree, tw.database("cpu"), class_name="Cyclist", device="cpu", backend="host", iou3d=cpu.boxes_iou3d)
    assert gen.scope == [-30.0, 30.0, -1.0, 3.0, 0.0, 50.0] and len(d["boxes"]) == gen.db.size
    report = gen.generate(str(tmp_path), aug_times=1, seed=3)
    assert [r["sample_id"] for r in report] == [10001]                         # only frame 1 holds a Cyclist (:259-260)
    with open(os.path.join(str(tmp_path), "train_aug.txt")) as f:
        assert f.read() == "000000\n000001\n000002\n000003\n010001"
    with open(os.path.join(str(tmp_path), "aug_label", "010001.txt")) as f:
        lines = f.read().split("\n")
    assert lines[0].startswith("Cyclist 0.00 0 0.30 ") and all(ln.startswith("Cyclist ") for ln in lines[1:-1]) and lines[-1] == ""
    sim = kitti_input.AugSceneGenerator(tree, tw.database("cpu"), include_similar=True, device="cpu", backend="host", iou3d=cpu.boxes_iou3d)
    assert sim.whitelist == ["Car", "Van"]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aug_scene_math") / "aug_scene_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "aug_scene_host.cpp"), "-o", exe], check=True)
    return exe


def test_header_arithmetic_equals_the_twin(host):
    rng = np.random.default_rng(9)
    n = 64
    boxes = np.concatenate([rng.uniform([-45, -2, -3], [45, 4, 75], (n, 3)), rng.uniform(0.5, 5, (n, 3)), rng.uniform(-4, 4, (n, 1))], 1).astype(np.float32)
    boxes[:6, :3] = [[-40, -1, 0], [40, 3, 70.375], [40.000004, 0, 1], [0, 3.0000002, 1], [0, 0, 70.4], [0, -1.0000001, 5]]     # on and just past the bounds: float32(70.4) > 70.4
    planes = np.concatenate([rng.normal(0, 0.03, (n, 1)), -1 + rng.normal(0, 0.01, (n, 1)), rng.normal(0, 0.03, (n, 1)), rng.uniform(1.4, 1.9, (n, 1))], 1)
    planes[7] = [0.0, 0.0, 0.0, 1.65]                                             # b == 0: inf / nan, no trap
    work = os.path.dirname(host)
    for seed, D in ((0, 2), (11, 31), (0xFFFFFFFF, 100000)):
        frames = [10000, 10001, 47999, 2 ** 31 - 1]
        want = tw.host_table(os.path.join(work, "in.bin"), seed if seed < 2 ** 31 else seed - 2 ** 32, frames, D, boxes, planes)
        r = subprocess.run([host, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(os.path.join(work, "out.bin"), np.int32)
        assert np.array_equal(got, want), (seed, D, np.nonzero(got != want)[0][:8])
        draws = got[:len(frames) * 51].reshape(len(frames), 51)
        assert (draws[:, 0] >= 10).all() and (draws[:, 0] <= 14).all() and (draws[:, 1:] >= 0).all() and (draws[:, 1:] <= D - 2).all()
    assert list(got[len(frames) * 51:].reshape(n, 7)[:6, 0]) == [1, 1, 0, 0, 0, 0]
    assert list(got[len(frames) * 51:].reshape(n, 7)[:7, 6]) == [0, 1, 0, 1, 1, 0, 1]      # 0, 1e-8f, just below, just above, nan, -0, 1


def test_header_binding_and_library_agree_on_the_new_exports():
    from pointrcnn_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "prcnn_pointops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.library_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (prcnn_\w+)", out))
    lib = _cabi.lib()
    for name in EXPORTS:
        m = re.search(r"^(?:int|size_t)\s+%s\s*\((.*?)\);" % name, code, flags=re.S | re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_cabi.SIGNATURES[name][1]), name
        assert name in exported and hasattr(lib, name)
        assert name in hdr[:hdr.index("const char* prcnn_last_error")], "the version comment names %s" % name
    assert lib.prcnn_abi_version() == _cabi.REQUIRED_ABI == 12
    # pure host query: two (frame, tile) tables of 1024-point tiles and the per-frame survivors
    assert lib.prcnn_aug_scene_workspace_bytes(-1, 4) == 0 and lib.prcnn_aug_scene_workspace_bytes(0, 0) == 64
    assert lib.prcnn_aug_scene_workspace_bytes(1025, 5) >= (2 * 5 * 2 + 5) * 4
    scene = open(os.path.join(CSRC, "scene.hip")).read()
    table = scene[scene.index("Stream ids in use"):scene.index("#include")]
    assert re.search(r"//\s+60\s", table) and re.search(r"//\s+61\s", table)
    assert "aug_scene" not in open(os.path.join(CSRC, "switches.h")).read()


def test_argument_checks_run_on_the_host_before_any_launch():
    """K < 15, G + 15 > 256, a null pointer and a short workspace: PRCNN_EINVAL with a message; no device is needed to be told so"""
    import ctypes
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    p = ctypes.c_void_p(64)
    scope = (ctypes.c_double * 6)(*tw.SCOPE)
    sample = lambda G, K, ptr=p, sc=scope, B=1: lib.prcnn_aug_scene_sample(ptr, None, ptr, ptr, B, G, ptr, ptr, 5, sc, K, 0, ptr, ptr, ptr, ptr, ptr, ptr, None)   # noqa: E731
    assert sample(4, 14) == -1 and b"K=14" in lib.prcnn_last_error()
    assert sample(242, 15) == -1 and b"G + 15 = 257 > 256" in lib.prcnn_last_error()
    assert sample(4, 15, None) == -1 and b"null pointer" in lib.prcnn_last_error()
    assert sample(4, 15, p, None) == -1 and b"null scope" in lib.prcnn_last_error()
    assert sample(4, 15, None, scope, 0) == 0                                    # no frame: nothing to do
    count = lambda ws, nbytes, K=15, rows=p: lib.prcnn_aug_scene_count(p, p, 1, 2048, 2048, p, p, scope, p, p, p, p, K, p, 5, 100, rows, ws, nbytes, None)   # noqa: E731
    need = lib.prcnn_aug_scene_workspace_bytes(2048, 1)
    assert count(p, need - 1) == -1 and b"workspace too small" in lib.prcnn_last_error()
    assert count(None, need) == -1 and b"workspace too small" in lib.prcnn_last_error()
    assert count(p, need, 65) == -1 and b"K=65" in lib.prcnn_last_error()
    assert count(p, need, 15, None) == -1 and b"null pointer" in lib.prcnn_last_error()
    fill = lambda out, ws_bytes: lib.prcnn_aug_scene_fill(p, p, 1, 2048, 2048, p, p, scope, p, p, p, p, p, 15, p, p, p, 5, 100, p, 10, out, p, p, ws_bytes, None)   # noqa: E731
    assert fill(p, need - 1) == -1 and b"workspace too small" in lib.prcnn_last_error()
    assert fill(None, need) == -1 and b"null pointer" in lib.prcnn_last_error()
    assert fill(ctypes.c_void_p(68), need) == -1 and b"16-byte aligned" in lib.prcnn_last_error()
