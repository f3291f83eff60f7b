"""Run the REFERENCE's own tools/generate_aug_scene.py (AugSceneGenerator.generate_aug_scene: aug_one_epoch_scene, aug_one_scene,
save_kitti_format; KittiDataset, Object3d, Calibration) on the synthetic tree of tests/aug_scene_twin.py, for --class_name Car and two
epochs.

Only used to GENERATE tests/golden/aug_scene_ref.npz (python tests/golden/ref_aug_scene.py) where the reference tree exists.  The .npz
holds data only: per written frame the accepted database ids, the placed boxes, extra_gt_num and the tries spent, the written cloud,
the written label lines; and the split list.  What is replaced:
  - np.random.randint while aug_one_scene runs -> the counter table (stream 60: randint(10, 15), stream 61: the index draw of try t),
    keyed by the new sample id;
  - iou3d_cuda.boxes_overlap_bev_gpu (a compiled extension) -> the same source compiled for the host by oracle/build_ref.py
    (oracle.ref()); the reference's own boxes_iou3d_gpu runs around it on CPU tensors (Tensor.cuda and torch.cuda.FloatTensor are
    pointed at their CPU counterparts for the run);
  - roipool3d_cuda.pts_in_boxes3d_cpu -> the same C++ source compiled for the host (oracle.ref());
  - os.system (the tool's `cp` of the split file) -> nothing.
aug_one_scene is wrapped to record what it returns, and to turn the ValueError the reference raises on a frame without a label to test
against into the unaugmented result (status 1) so that the run goes on.  y_shift is not a value the tool exposes: it is restated here
from the tool's own get_road_plane and the database box (:191-192) in float64.
Asserted: the tool's clouds hold the same rows as the twin's (the reference's BLAS sgemm differs from the canonical transform in the last
ulp; a point sitting on a boundary of the valid flag or of a box would change the row set: another scan seed is the remedy).
"""
import importlib
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
REFERENCE = os.environ.get("PRCNN_REFERENCE", "/root/reference")
for p in (HERE, TESTS, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import aug_scene_twin as tw          # noqa: E402

AUG_TIMES, SEED = 2, 11
RTOL, ATOL = 2e-6, 2e-5                  # tests/test_oracle_scene.py: the reference's sgemm against the canonical transform


def main():
    import torch
    import oracle
    for p in (os.path.join(TESTS, "compat"), REFERENCE, os.path.join(REFERENCE, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    ref = oracle.ref()
    assert ref is not None, "oracle/_ref is not built"
    rc = sys.modules.setdefault("roipool3d_cuda", types.ModuleType("roipool3d_cuda"))
    rc.pts_in_boxes3d_cpu = lambda flags, pts, boxes: flags.copy_(torch.from_numpy(ref.pts_in_boxes3d_cpu(pts.numpy(), boxes.numpy()))) is None or 1
    ic = sys.modules.setdefault("iou3d_cuda", types.ModuleType("iou3d_cuda"))
    ic.boxes_overlap_bev_gpu = lambda a, b, out: out.copy_(torch.from_numpy(ref.boxes_overlap_bev(a.numpy(), b.numpy()))) is None or 1
    root = os.path.join(HERE, "_aug_scene_tmp")
    save_dir = os.path.join(root, "aug_scene", "training")
    shutil.rmtree(root, ignore_errors=True)
    tw.write_aug_tree(root)
    argv, sys.argv = sys.argv, ["generate_aug_scene.py", "--class_name", "Car", "--split", "train", "--save_dir", save_dir]
    try:
        tool = importlib.import_module("generate_aug_scene")           # the reference's tool itself
    finally:
        sys.argv = argv
    from lib.utils.object3d import Object3d
    d = tw.database_arrays()
    lines = [ln for f in tw.DB_FRAMES for ln in tw.frame_labels(f)]
    db = [{"sample_id": int(d["sample_id"][k]), "cls_type": "Car", "gt_box3d": d["boxes"][k].copy(), "points": d["points"][k].copy(),
           "intensity": d["intensity"][k].copy(), "obj": Object3d(lines[k])} for k in range(len(lines))]
    assert all(np.array_equal(np.concatenate([e["obj"].pos, np.array([e["obj"].h, e["obj"].w, e["obj"].l, e["obj"].ry], np.float32)]), e["gt_box3d"])
               for e in db)
    obj_id = {id(e["obj"]): k for k, e in enumerate(db)}
    gen = tool.AugSceneGenerator(root_dir=root, gt_database=db, split="train")
    state, rec = {"base": 0, "frame": 0, "first": True, "t": 0}, {}

    def randint(lo, hi=None):
        if hi <= lo:
            raise ValueError("low >= high")
        if state["first"]:
            state["first"] = False
            return lo + tw.below(tw.rand32(SEED, tw.STREAM_EXTRA, state["frame"], 0), hi - lo)
        r = tw.rand32(SEED, tw.STREAM_INDEX, state["frame"], state["t"])
        state["t"] += 1
        return lo + tw.below(r, hi - lo)
    one_scene, one_epoch = gen.aug_one_scene, gen.aug_one_epoch_scene

    def aug_one_scene(sample_id, pts_rect, pts_intensity, all_gt_boxes3d):
        state.update(frame=state["base"] + sample_id, first=True, t=0)
        extra = 10 + tw.below(tw.rand32(SEED, tw.STREAM_EXTRA, state["frame"], 0), 5)
        status = 0
        try:
            res = one_scene(sample_id, pts_rect, pts_intensity, all_gt_boxes3d)
        except ValueError:
            res, status = (False, pts_rect, pts_intensity, None, None), 1
        ids = [obj_id[id(o)] for o in res[4]] if res[0] else []
        a, b, c, dd = gen.get_road_plane(sample_id)
        shift = [float(db[i]["gt_box3d"][1] - (-dd - a * db[i]["gt_box3d"][0] - c * db[i]["gt_box3d"][2]) / b) for i in ids]
        rec[state["frame"]] = {"ids": np.asarray(ids, np.int32), "boxes": np.asarray(res[3], np.float32).reshape(-1, 7) if res[0] else np.zeros((0, 7), np.float32),
                               "y_shift": np.asarray(shift, np.float64), "stats": np.array([extra, state["t"]], np.int32), "status": status,
                               "nvalid": len(pts_rect)}
        return res

    def aug_one_epoch_scene(base_id, *a, **k):
        state["base"] = base_id
        return one_epoch(base_id, *a, **k)
    gen.aug_one_scene, gen.aug_one_epoch_scene = aug_one_scene, aug_one_epoch_scene
    saved = (np.random.randint, torch.Tensor.cuda, torch.cuda.FloatTensor, os.system)
    np.random.randint, torch.Tensor.cuda, torch.cuda.FloatTensor, os.system = randint, (lambda self, *a, **k: self), torch.FloatTensor, (lambda cmd: 0)
    try:
        gen.generate_aug_scene(aug_times=AUG_TIMES)
    finally:
        np.random.randint, torch.Tensor.cuda, torch.cuda.FloatTensor, os.system = saved
    want, split = tw.generate(root, AUG_TIMES, SEED)
    with open(os.path.join(save_dir, "train_aug.txt")) as f:
        ref_split = f.read()
    out = {"aug_times": AUG_TIMES, "seed": SEED, "split": np.array(ref_split), "ids": np.array(sorted(rec), np.int64)}
    for new_id in sorted(rec):
        r = rec[new_id]
        cloud = np.fromfile(os.path.join(save_dir, "rectified_data", "%06d.bin" % new_id), np.float32).reshape(-1, 4)
        with open(os.path.join(save_dir, "aug_label", "%06d.txt" % new_id)) as f:
            labels = f.read().split("\n")[:-1]
        t = want[new_id]
        assert cloud.shape == t["cloud"].shape, "frame %d: the tool keeps %d rows, the twin %d: take another SEED0" % (new_id, len(cloud), len(t["cloud"]))
        assert (np.abs(cloud - t["cloud"]) <= ATOL + RTOL * np.abs(t["cloud"])).all(), "frame %d: rows differ: take another SEED0" % new_id
        out.update({"f%d_ids" % new_id: r["ids"], "f%d_boxes" % new_id: r["boxes"], "f%d_y_shift" % new_id: r["y_shift"],
                    "f%d_stats" % new_id: r["stats"], "f%d_status" % new_id: r["status"], "f%d_cloud" % new_id: cloud,
                    "f%d_labels" % new_id: np.array(labels, np.str_)})
        print("frame %06d: status %d, accepted %d of extra %d, %d tries, %d rows (%d pasted), %d label lines"
              % (new_id, r["status"], len(r["ids"]), r["stats"][0], r["stats"][1], len(cloud), len(cloud) - int((t["src"] >= 0).sum()), len(labels)))
    shutil.rmtree(root, ignore_errors=True)
    path = os.path.join(HERE, "aug_scene_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote aug_scene_ref.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
