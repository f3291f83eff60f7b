"""KITTI evaluator kernels (csrc/kitti_eval.hip) through the C ABI: identical to the CPU oracle and to the golden
vectors from the reference's own Python."""
import numpy as np
import pytest
import torch

from kitti_cases import MIN_OVERLAPS, check_against_golden, golden, kitti_eval_inputs

pytestmark = pytest.mark.gpu


def test_hip_backend_equals_golden_and_oracle(dev):
    import oracle
    from pointrcnn_amd import kitti_eval
    hip, cpu_be = kitti_eval.HipBackend(), oracle.KittiBackend()
    check_against_golden(kitti_eval, hip, golden())
    gt, dt = kitti_eval_inputs()
    for metric in (0, 1, 2):
        a = kitti_eval.calculate_iou_partly(dt, gt, metric, hip)[1]
        b = kitti_eval.calculate_iou_partly(dt, gt, metric, cpu_be)[1]
        assert np.array_equal(a, b), metric                                      # same arithmetic, bit for bit

    class Recorder:                                                              # every statistics() call: HIP == oracle
        def __init__(self):
            self.calls = 0

        def overlaps(self, *a):
            return hip.overlaps(*a)

        def statistics(self, *a):
            r1, m1 = hip.statistics(*a)
            r2, m2 = cpu_be.statistics(*a)
            assert np.array_equal(r1[..., :3], r2[..., :3]) and np.array_equal(m1, m2, equal_nan=True)
            np.testing.assert_allclose(r1[..., 3], r2[..., 3], rtol=1e-13, atol=1e-13)
            self.calls += 1
            return r1, m1

    rec = Recorder()
    kitti_eval.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], 0, MIN_OVERLAPS, compute_aos=True, backend=rec)
    assert rec.calls == 2 * 3 * 3 * 2


def test_rotate_iou_eval_kernel(dev, cpu):
    import oracle
    from pointrcnn_amd import ops
    g = golden()
    be = oracle.KittiBackend()
    b, q = torch.from_numpy(g["riou_boxes"]).to(dev), torch.from_numpy(g["riou_query"]).to(dev)
    for c in (-1, 0, 1, 2):
        got = ops.rotate_iou_eval(b, q, c).cpu().numpy()
        assert np.array_equal(got, be.rotate_iou_eval(g["riou_boxes"], g["riou_query"], c))
        np.testing.assert_allclose(got, g["riou_c%d" % c], rtol=0, atol=2e-6)
    assert ops.rotate_iou_eval(b[:0], q, -1).shape == (0, 30)


def test_full_split_size_runs(dev):
    """3 769 frames (the KITTI val split size) of synthetic annotations: shapes, finiteness, monotone precision envelope"""
    from util import kitti_annos
    from pointrcnn_amd import kitti_eval
    gt = kitti_annos(3769, seed=11)
    dt = kitti_annos(3769, seed=12, with_score=True, gt=gt)
    res, d = kitti_eval.get_official_eval_result(gt, dt, 0)
    assert all(np.isfinite(v) and 0 <= v <= 100 for v in d.values())
    r = kitti_eval.eval_class(gt, dt, [0], [0, 1, 2], 2, np.full((1, 3, 1), 0.7))
    assert (np.diff(r["precision"], axis=-1) <= 1e-12).all()                     # the running max makes it non-increasing


# ---------------------------------------------------------------------------------------------------------------------
# crowded and adversarial frames (kitti_stats_cases.py) against tests/golden/kitti_stats_ref.npz, which holds what the reference's
# own compute_statistics_jit / *_box_overlap / eval_class return on them.  The oracle keeps one byte per detection where the
# kernel keeps 1024-bit bitmaps, so agreement with the oracle on frames of more than 64 detections is a real second opinion.
# ---------------------------------------------------------------------------------------------------------------------
import kitti_stats_cases as K  # noqa: E402


@pytest.fixture(scope="module")
def backends(dev):
    import oracle
    from pointrcnn_amd import kitti_eval
    return kitti_eval.HipBackend(), oracle.KittiBackend()


@pytest.fixture(scope="module")
def stats_golden():
    return K.golden()


def assert_same_statistics(a, b, what):
    """HIP against the oracle: counts and matched scores bit for bit, the similarity sum to the project's 1e-13"""
    (r1, m1), (r2, m2) = a, b
    assert np.array_equal(r1[..., :3], r2[..., :3]), what
    assert np.array_equal(m1, m2, equal_nan=True), what
    np.testing.assert_allclose(r1[..., 3], r2[..., 3], rtol=1e-13, atol=1e-13, err_msg=str(what))


@pytest.mark.parametrize("name", sorted(K.families()))
def test_statistics_family_equals_reference_and_oracle(backends, stats_golden, name):
    """tp / fp / fn and the matched scores exact; similarity within 1e-9 of the reference, which adds the n <= 40 terms in another
    order and with another cos: the bound is (4 n + n^2) 2^-53 = 2e-13 at n = 40, the largest difference measured on an MI355X is
    3.6e-15 (words and aos families; printed below); the same calls bit for bit against the oracle"""
    hip, cpu_be = backends
    c = K.families()[name]
    worst = K.check_case(hip, stats_golden, c)
    print("%s: largest |similarity - reference| = %.3g" % (name, worst))
    for k, (metric, mo, aos) in enumerate(c["settings"]):
        for thr, fp in ((np.zeros(1), False), (c["thresholds"], True)):
            a = c["args"] + (metric, mo, thr, fp, aos and fp)
            assert_same_statistics(hip.statistics(*a), cpu_be.statistics(*a), (name, metric, mo, fp))


def test_statistics_hand_cases(backends):
    K.check_hand_cases(backends[0])


def test_statistics_frames_are_independent(backends):
    """permuting the frames of a call permutes res and matched; a frame evaluated alone equals its rows in the batch"""
    hip, _ = backends
    fam = K.families()
    frames = fam["shapes_ragged"]["frames"] + fam["words"]["frames"][:5] + fam["dontcare"]["frames"] + fam["aos"]["frames"][:2]
    thr = K.THRESHOLDS
    order = np.random.default_rng(7).permutation(len(frames))
    for metric, mo, fp in ((0, 0.5, True), (0, 0.7, False)):
        res, matched = hip.statistics(*K.pack(frames), metric, mo, thr, fp, fp)
        res_p, matched_p = hip.statistics(*K.pack(K.permuted(frames, order)), metric, mo, thr, fp, fp)
        res, res_p = res.reshape(len(frames), len(thr), 4), res_p.reshape(len(frames), len(thr), 4)
        goff = K.off([len(f["gt"]) for f in frames])
        goff_p = K.off([len(frames[i]["gt"]) for i in order])
        for pos, i in enumerate(order):
            assert np.array_equal(res_p[pos], res[i]), (i, metric)
            assert np.array_equal(matched_p[goff_p[pos]:goff_p[pos + 1]], matched[goff[i]:goff[i + 1]], equal_nan=True), (i, metric)
        for i in (1, 3, 4, 8, 12):                                               # 1024 and 65 detections, an empty frame, ...
            r1, m1 = hip.statistics(*K.pack([frames[i]]), metric, mo, thr, fp, fp)
            assert np.array_equal(r1.reshape(len(thr), 4), res[i]), (i, metric)
            assert np.array_equal(m1, matched[goff[i]:goff[i + 1]], equal_nan=True), (i, metric)


def test_statistics_detection_limit(backends, dev):
    """a frame of 1024 detections is computed (the words family holds four); one of 1025 is refused with an error and no result
    is written"""
    from pointrcnn_amd import _cabi, ops
    hip, _ = backends
    frames = K.over_limit_frames()
    assert max(len(f["dt"]) for f in frames) == K.KS_MAX_DET + 1
    with pytest.raises(_cabi.PointOpsError, match="1025 detections"):
        hip.statistics(*K.pack(frames), 0, 0.5, K.THRESHOLDS, True, True)
    dtypes = (np.float64, np.int64, np.float64, np.int32, np.float64, np.int32, np.int32, np.int32, np.float64, np.int32)
    t = [hip._t(a, d) for a, d in zip(K.pack(frames), dtypes)]
    thr = hip._t(K.THRESHOLDS, np.float64)
    res = torch.zeros((len(frames), len(thr), 4), dtype=torch.float64, device=dev)
    matched = torch.full((int(t[3][-1]),), float("nan"), dtype=torch.float64, device=dev)
    rc = _cabi.lib().prcnn_kitti_statistics(*[ops._p(x) for x in t], len(frames), K.KS_MAX_DET + 1, 0, 0.5, ops._p(thr), len(thr), 1, 1,
                                            ops._p(res), ops._p(matched), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert not res.any() and torch.isnan(matched).all()


def test_overlap_cases_equal_reference_and_oracle(backends, stats_golden):
    hip, cpu_be = backends
    K.check_overlaps(hip, stats_golden, other=cpu_be)


def test_eval_class_on_crowded_annotations(backends, stats_golden):
    K.check_eval_class(backends[0], stats_golden)
