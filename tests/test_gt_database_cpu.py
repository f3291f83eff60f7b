"""GT-augmentation database from a KITTI tree, host side (no GPU): the label reader and GTDatabase.from_kitti(backend="host") against
the reference's own tools/generate_gt_database.py (fixture tests/golden/gt_database_ref.npz, made by tests/golden/ref_gt_database.py
with the reference's KittiDataset / Object3d / lidar_to_rect / pts_in_boxes3d_cpu), the .npz file format, and the C ABI's three new
entry points."""
import os
import re
import subprocess
import zipfile

import numpy as np
import pytest

import kitti_tree
from util import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-6, 2e-5              # tests/test_oracle_scene.py: the reference's BLAS sgemm against the canonical transform
EXPORTS = ("prcnn_gt_database_workspace_bytes", "prcnn_gt_database_count", "prcnn_gt_database_fill")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "gt_database_ref.npz")))


@pytest.fixture(scope="module")
def tree(gold, tmp_path_factory):
    """the fixture's tree, regenerated: write_tree's scans from the stored seeds, the label text as stored"""
    root = str(tmp_path_factory.mktemp("gt_database_tree"))
    frames = [int(f) for f in gold["frames"]]
    base = kitti_tree.write_tree(root, frames, seed0=int(gold["seed0"]), n_scan=int(gold["n_scan"]))
    for k, f in enumerate(frames):
        with open(os.path.join(base, "label_2", "%06d.txt" % f), "w") as fh:
            fh.write("".join(str(ln) + "\n" for ln in gold["f%d_labels" % k]))
    return root


def test_label_reader_matches_the_reference_parse(gold):
    from pointrcnn_amd import kitti_input
    levels = set()
    for k in range(len(gold["frames"])):
        lab = kitti_input.read_label_lines([str(ln) + "\n" for ln in gold["f%d_labels" % k]])
        f = gold["f%d_fields" % k]                       # truncation occlusion alpha h w l ry score, as Object3d holds them (double)
        assert list(lab["cls_type"]) == [str(c) for c in gold["f%d_cls" % k]]
        assert np.array_equal(lab["truncation"], f[:, 0]) and np.array_equal(lab["occlusion"], f[:, 1]) and np.array_equal(lab["alpha"], f[:, 2])
        assert np.array_equal(lab["score"], f[:, 7])
        assert lab["box2d"].dtype == np.float32 and np.array_equal(lab["box2d"], gold["f%d_box2d" % k])
        want = np.concatenate([gold["f%d_pos" % k], f[:, 3:7].astype(np.float32)], 1)      # generate_gt_database.py:63-66
        assert lab["boxes3d"].dtype == np.float32 and np.array_equal(lab["boxes3d"], want)
        assert lab["level"].dtype == np.int32 and np.array_equal(lab["level"], gold["f%d_level" % k])
        levels |= set(int(v) for v in lab["level"])
    assert levels == {1, 2, 3, 4}
    empty = kitti_input.read_label_lines([])
    assert empty["boxes3d"].shape == (0, 7) and empty["level"].shape == (0,)


@pytest.mark.parametrize("name", ["Car", "People"])
def test_from_kitti_host_matches_the_reference_database(gold, tree, name):
    from pointrcnn_amd import kitti_input
    db = kitti_input.GTDatabase.from_kitti(tree, "train", name, hard_ratio=0.6, device="cpu", frames_per_batch=3, backend="host")
    assert db.size == len(gold[name + "_npts"]) > 0
    assert np.array_equal(db.sample_id, gold[name + "_sample_id"]) and [str(c) for c in db.cls_type] == [str(c) for c in gold[name + "_cls_type"]]
    assert set(db.cls_type) == ({"Car"} if name == "Car" else {"Pedestrian", "Cyclist"})
    assert int(gold["frames"][-1]) not in set(db.sample_id)                       # the frame with no kept object
    assert np.array_equal(db.boxes.numpy(), gold[name + "_gt_box3d"])
    assert np.array_equal(db.alpha.numpy(), gold[name + "_alpha"].astype(np.float32))
    assert np.array_equal(db.npts.numpy(), gold[name + "_npts"])
    assert np.array_equal(db.offsets.numpy(), np.concatenate([[0], np.cumsum(gold[name + "_npts"])]))
    assert np.array_equal(db.src.numpy(), gold[name + "_src"])                    # every object's raw-index list, in order
    ref_pts = gold[name + "_points"]
    print("max |points - reference| = %g" % np.abs(db.points.numpy() - ref_pts).max())
    assert (np.abs(db.points.numpy() - ref_pts) <= ATOL + RTOL * np.abs(ref_pts)).all()
    assert np.array_equal(db.intensity.numpy(), gold[name + "_intensity"])
    n = gold[name + "_npts"]
    assert np.array_equal(db.easy_idx.numpy(), np.nonzero(n > 100)[0]) and np.array_equal(db.hard_idx.numpy(), np.nonzero(n <= 100)[0])
    assert len(db.easy_idx) and len(db.hard_idx)
    # entries(): the reference's list of dicts without 'obj'
    ent = db.entries()
    off = db.offsets.numpy()
    assert len(ent) == db.size and set(ent[0]) == {"sample_id", "cls_type", "gt_box3d", "points", "intensity"}
    for k in (0, db.size - 1):
        assert ent[k]["sample_id"] == gold[name + "_sample_id"][k] and ent[k]["cls_type"] == str(gold[name + "_cls_type"][k])
        assert np.array_equal(ent[k]["gt_box3d"], gold[name + "_gt_box3d"][k]) and ent[k]["points"].shape == (n[k], 3)
        assert np.array_equal(ent[k]["intensity"], gold[name + "_intensity"][off[k]:off[k + 1]])


def test_host_transform_is_the_canonical_one_and_near_the_reference(gold, tree):
    import oracle
    from pointrcnn_amd import kitti_input
    base = os.path.join(tree, "KITTI", "object", "training")
    for k, f in enumerate(int(f) for f in gold["frames"][:-1]):
        scan = kitti_input.get_lidar(os.path.join(base, "velodyne", "%06d.bin" % f))
        calib = kitti_input.Calibration(os.path.join(base, "calib", "%06d.txt" % f))
        rect = kitti_input.lidar_to_rect_host(scan, calib.lidar_to_rect_matrix())
        assert rect.dtype == np.float32 and np.array_equal(rect, oracle.scene_project(scan, calib.packed(), 375, 1242, None)[0])
        ref = gold["f%d_pts_rect" % k]
        assert (np.abs(rect - ref) <= ATOL + RTOL * np.abs(ref)).all()


def test_save_load_round_trip_holds_no_pickled_object(tree, tmp_path):
    from pointrcnn_amd import kitti_input
    db = kitti_input.GTDatabase.from_kitti(tree, class_name="People", device="cpu", backend="host")
    path = str(tmp_path / "people_db.npz")
    db.save(path)
    with zipfile.ZipFile(path) as z:
        assert sorted(z.namelist()) == sorted(k + ".npy" for k in ("boxes", "alpha", "npts", "points", "intensity", "sample_id", "cls_type"))
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    back = kitti_input.GTDatabase.load(path, hard_ratio=0.6, device="cpu")
    assert back.size == db.size and back.max_points == db.max_points and back.hard_ratio == db.hard_ratio
    for k in ("boxes", "alpha", "npts", "offsets", "points", "intensity", "easy_idx", "hard_idx"):
        a, b = getattr(db, k), getattr(back, k)
        assert a.dtype == b.dtype and a.device == b.device and np.array_equal(a.numpy(), b.numpy()), k
    assert np.array_equal(db.sample_id, back.sample_id) and np.array_equal(db.cls_type, back.cls_type)
    assert back.src is None


def test_from_arrays_is_unchanged_and_carries_empty_provenance():
    from pointrcnn_amd import kitti_input
    r = np.random.default_rng(0)
    pts = [r.random((n, 3)).astype(np.float32) for n in (3, 150)]
    db = kitti_input.GTDatabase.from_arrays(r.random((2, 7)).astype(np.float32), np.zeros(2, np.float32), pts, [p[:, 0] for p in pts], device="cpu")
    assert db.size == 2 and list(db.sample_id) == [-1, -1] and list(db.cls_type) == ["", ""] and db.src is None
    assert list(db.easy_idx.numpy()) == [1] and list(db.hard_idx.numpy()) == [0]


def test_from_kitti_rejects_a_missing_split_and_an_unknown_class(tree):
    from pointrcnn_amd import kitti_input
    with pytest.raises(FileNotFoundError, match="no split file .*nosuch.txt"):
        kitti_input.GTDatabase.from_kitti(tree, split="nosuch", device="cpu", backend="host")
    with pytest.raises(ValueError, match="class_name 'Truck' is not one of"):
        kitti_input.GTDatabase.from_kitti(tree, class_name="Truck", device="cpu", backend="host")
    with pytest.raises(ValueError, match="backend"):
        kitti_input.GTDatabase.from_kitti(tree, device="cpu", backend="numpy")


def test_header_binding_and_library_agree_on_the_new_exports():
    from pointrcnn_amd import _cabi
    hdr = open(os.path.join(REPO, "include", "prcnn_pointops.h")).read()
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
    # pure host queries: two (frame, box, tile) tables of 1024-point tiles
    assert lib.prcnn_gt_database_workspace_bytes(0, 4, 6) == 64 and lib.prcnn_gt_database_workspace_bytes(-1, 4, 6) == 0
    assert lib.prcnn_gt_database_workspace_bytes(1025, 5, 6) >= 2 * 5 * 6 * 2 * 4


def test_argument_checks_run_on_the_host_before_any_launch():
    """limits and null pointers are refused from the host code, with prcnn_last_error set; no device is needed to be told so"""
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    assert lib.prcnn_gt_database_count(None, None, 1, 0, 0, None, None, None, 129, None, None, 0, None) == -1
    assert b"G=129" in lib.prcnn_last_error()
    assert lib.prcnn_gt_database_fill(None, None, 1, 0, 0, None, None, None, 4, None, 0, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.prcnn_last_error()
    assert lib.prcnn_gt_database_count(None, None, 0, 0, 0, None, None, None, 4, None, None, 0, None) == 0          # no frame: nothing to do
