#!/usr/bin/env python3
"""Generate tests/golden/kitti_stats_ref.npz: what the REFERENCE'S OWN evaluator (tools/kitti_object_eval_python, numba stubbed
to identity by ref_kitti_eval.py) returns on the crowded and adversarial inputs of tests/kitti_stats_cases.py.

    <case>_crc                      CRC of the regenerated inputs of one statistics case
    <case>_s<k>_res   (F, T, 4)     compute_statistics_jit(..., compute_fp=True) per frame and threshold: tp, fp, fn, similarity
    <case>_s<k>_p1res (F, 4)        ... pass 1 (thresh 0, compute_fp=False)
    <case>_s<k>_p1thr, _p1cnt       the `thresholds` pass 1 returns, concatenated, and how many each frame contributes
    ov_m<metric>, ov_flag, ov_crc   image_box_overlap / bev_box_overlap / d3_box_overlap per pair of the overlap frames, flat;
                                    ov_flag marks the rotated pairs on which the reference's Python raises IndexError (its point
                                    list holds 8 points): they carry no reference value
    ec_*                            eval_class on the crowded annotation set

Only CRCs, flags and outputs are stored.  Needs the reference checkout; re-running reproduces the arrays.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import kitti_stats_cases as K  # noqa: E402
import ref_kitti_eval  # noqa: E402

MAX_FLAGGED_SHARE = 0.05


def ref_statistics(ev, c, metric, min_overlap, compute_aos):
    """the reference's compute_statistics_jit on every frame of a case: -> res (F, T, 4), p1res (F, 4), p1thr, p1cnt"""
    thr = c["thresholds"]
    res = np.zeros((len(c["frames"]), len(thr), 4))
    p1res, p1thr, p1cnt = np.zeros((len(c["frames"]), 4)), [], []
    for f, fr in enumerate(c["frames"]):
        a = (fr["ov"], fr["gt"], fr["dt"], fr["ign_gt"], fr["ign_det"], fr["dc"], metric, min_overlap)
        *p1res[f], th = ev.compute_statistics_jit(*a, thresh=0.0, compute_fp=False)
        p1thr.append(np.asarray(th, np.float64))
        p1cnt.append(len(th))
        for t, v in enumerate(thr):
            res[f, t] = ev.compute_statistics_jit(*a, thresh=v, compute_fp=True, compute_aos=compute_aos)[:4]
    return res, p1res, np.concatenate(p1thr) if p1thr else np.zeros(0), np.array(p1cnt, np.int64)


def ref_overlaps(ev, frames):
    """per pair, so that a pair the reference cannot compute does not take its frame along"""
    out, flags = {0: [], 1: [], 2: []}, []
    for dt7, gt7, dtb, gtb in frames:
        out[0].append(ev.image_box_overlap(dtb, gtb).reshape(-1))
        for n in range(len(dt7)):
            for k in range(len(gt7)):
                try:
                    bev = ev.bev_box_overlap(dt7[n:n + 1][:, [0, 2, 3, 5, 6]], gt7[k:k + 1][:, [0, 2, 3, 5, 6]])[0, 0]
                    d3 = ev.d3_box_overlap(dt7[n:n + 1], gt7[k:k + 1])[0, 0]
                    flags.append(False)
                except IndexError:
                    bev = d3 = np.nan
                    flags.append(True)
                out[1].append(np.float64(bev).reshape(1))
                out[2].append(np.float64(d3).reshape(1))
    cat = lambda parts: np.concatenate(parts).astype(np.float64) if parts else np.zeros(0)      # noqa: E731
    return cat(out[0]), cat(out[1]), cat(out[2]), np.array(flags, bool)


def check_hand_cases(ev):
    for name, fr, metric, mo, thr, compute_fp, want in K.hand_cases():
        tp, fp, fn, sim, th = ev.compute_statistics_jit(fr["ov"], fr["gt"], fr["dt"], fr["ign_gt"], fr["ign_det"], fr["dc"], metric, mo,
                                                        thresh=thr, compute_fp=compute_fp, compute_aos=compute_fp)
        if compute_fp:
            assert (tp, fp, fn) == tuple(want[:3]), (name, tp, fp, fn)
            assert len(want) == 3 or abs(sim - want[3]) < 1e-9, (name, sim)
        else:
            assert list(th) == [w for w in want if w == w], (name, th)


def main():
    ev, _ = ref_kitti_eval.load()
    check_hand_cases(ev)
    out = {}
    for name, c in K.families().items():
        out[name + "_crc"] = K.case_crc(c)
        for k, (metric, mo, aos) in enumerate(c["settings"]):
            for key, v in zip(("res", "p1res", "p1thr", "p1cnt"), ref_statistics(ev, c, metric, mo, aos)):
                out["%s_s%d_%s" % (name, k, key)] = v
        print(name, "frames", len(c["frames"]), "settings", len(c["settings"]))
    frames = K.overlap_frames()
    out["ov_m0"], out["ov_m1"], out["ov_m2"], out["ov_flag"] = ref_overlaps(ev, frames)
    out["ov_crc"] = K.overlap_crc(frames)
    share = out["ov_flag"].mean()
    print("rotated pairs without a reference value: %d of %d (%.2f %%)" % (out["ov_flag"].sum(), len(out["ov_flag"]), 100 * share))
    if share > MAX_FLAGGED_SHARE:
        raise SystemExit("too many overlap pairs on which the reference raises")
    sys.path.insert(0, HERE)
    from kitti_cases import MIN_OVERLAPS, annos_crc
    gt, dt = K.crowded_annos()
    out["ec_crc"] = np.array([annos_crc(gt), annos_crc(dt)])
    for metric in (0, 1, 2):
        r = ev.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], metric, MIN_OVERLAPS, compute_aos=(metric == 0), num_parts=len(gt))
        for key in ("recall", "precision", "orientation"):
            out["ec_m%d_%s" % (metric, key)] = r[key]
    np.savez_compressed(os.path.join(HERE, "kitti_stats_ref.npz"), **out)
    print("wrote kitti_stats_ref.npz", os.path.getsize(os.path.join(HERE, "kitti_stats_ref.npz")), "bytes")


if __name__ == "__main__":
    main()
