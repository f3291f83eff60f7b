"""GPU parity of the RPN input builder above 16384 points per frame (prcnn_scene_prepare_large: the draw written to HBM, the shuffle
sorted there in 16384-key chunks, the rows written by a launch of their own) against the CPU oracle, bit for bit on every output,
as tests/test_gpu_scene.py holds the one-workgroup form."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from test_gpu_scene import SCOPE, _assert_same, _calibs, _run_both
from util import scene_invariants, synthetic_scan

pytestmark = pytest.mark.gpu
HWS = [(375, 1242), (370, 1224), (375, 1242), (376, 1241), (375, 1242), (374, 1238)]


def _behind():
    behind = synthetic_scan(700, seed=1, fov_frac=0.0)
    behind[:, 0] = -np.abs(behind[:, 0]) - 1.0
    return behind


@pytest.mark.parametrize("npoints", [16385, 40000, 65536])
def test_scene_prepare_large_matches_oracle_ragged_batch(dev, npoints):
    """16385: one key in the second chunk; 40000: a partly filled third chunk and an all-padding fourth; 65536: four full chunks.
    A plain draw, a top-up from itself, an empty scan, more far points than npoints, a scan behind the camera, a cyclic repeat."""
    scans = [synthetic_scan(240000, 31, 0.5, 0.02), synthetic_scan(int(0.9 * npoints), 32, 0.9), np.zeros((0, 4), np.float32),
             synthetic_scan(240000, 33, 0.6, 0.95), _behind(), synthetic_scan(3000, 35, 0.5)]
    got, ref, packed = _run_both(scans, HWS, npoints, 1234, SCOPE, dev)
    print("status", list(ref[4]), "nvalid", list(ref[3]))
    assert list(ref[4]) == [0, 0, 2, 1, 2, 1]
    _assert_same(got, ref)
    for b in (0, 1):                                          # the status-0 frames obey what kitti_rcnn_dataset.py:285-306 guarantees
        o0, o1 = int(packed["offsets"][b]), int(packed["offsets"][b + 1])
        scan = packed["raw"].numpy()[o0:o1]
        rect, _, _, flag = oracle.scene_project(scan, packed["calib"].numpy()[b], HWS[b][0], HWS[b][1], SCOPE)
        scene_invariants(got["pts_input"][b].cpu().numpy(), got["pts_features"][b, :, 0].cpu().numpy(), rect[flag],
                         scan[flag, 3] - np.float32(0.5), npoints)


def test_scene_prepare_large_exactly_npoints_valid(dev):
    """k == 0: the frame holds exactly npoints valid points, nothing is drawn and nothing topped up"""
    from pointrcnn_amd import kitti_input
    npoints = 20000
    scan = synthetic_scan(240000, 31, 0.5, 0.02)
    calib24 = kitti_input.pack_scans([scan], _calibs(1), HWS[:1], False)["calib"].numpy()[0]
    flag = oracle.scene_project(scan, calib24, HWS[0][0], HWS[0][1], SCOPE)[3]
    scan = scan[:np.nonzero(flag)[0][npoints - 1] + 1]
    got, ref, _ = _run_both([scan], HWS[:1], npoints, 1234, SCOPE, dev)
    assert list(ref[3]) == [npoints] and list(ref[4]) == [0]
    _assert_same(got, ref)
    assert sorted(got["src"][0].cpu().numpy()) == sorted(np.nonzero(flag[:len(scan)])[0])


@pytest.mark.parametrize("seed,expect_need", [(4550, 1), (6235, 2)])
def test_scene_prepare_large_draw_ties(dev, seed, expect_need):
    """seeds found offline (the search of test_scene_prepare_draw_ties, at npoints 40000) for which the draw's threshold key is
    shared by two candidates: only the lower raw index (need 1) or both (need 2) belong to the sample"""
    npoints = 40000
    scan = synthetic_scan(220000, seed=21, fov_frac=1.0, far_frac=0.0)
    got, ref, packed = _run_both([scan], [(375, 1242)], npoints, seed, SCOPE, dev)
    _assert_same(got, ref)
    assert list(ref[4]) == [0]
    flag = oracle.scene_project(scan, packed["calib"].numpy()[0], 375, 1242, SCOPE)[3]         # the premise, on the oracle side
    cand = np.nonzero(flag)[0].astype(np.uint32)

    def mix(x):
        x = x.astype(np.uint32); x ^= x >> np.uint32(16); x = (x * np.uint32(0x7feb352d)).astype(np.uint32)
        x ^= x >> np.uint32(15); x = (x * np.uint32(0x846ca68b)).astype(np.uint32); x ^= x >> np.uint32(16)
        return x
    keys = mix(cand ^ mix(mix(np.array([seed], np.uint32)))) >> np.uint32(2)
    kth = np.partition(keys, npoints - 1)[npoints - 1]
    print("keys at the threshold", int((keys == kth).sum()), "need", int(npoints - (keys < kth).sum()))
    assert (keys == kth).sum() == 2 and npoints - (keys < kth).sum() == expect_need


def test_scene_prepare_large_without_range_crop(dev):
    """cfg.PC_REDUCE_BY_RANGE = False (scope None) at 65536 points: the first frame has more far points than npoints"""
    scans = [synthetic_scan(240000, seed=41, fov_frac=0.5, far_frac=0.95), synthetic_scan(240000, seed=43, fov_frac=0.5, far_frac=0.1)]
    got, ref, _ = _run_both(scans, [(375, 1242)] * 2, 65536, 7, None, dev)
    assert list(ref[4]) == [1, 0]
    _assert_same(got, ref)


def test_scene_prepare_large_is_order_independent_and_seeded(dev):
    """the same batch three times = the same bytes (the order in which the atomics append must not leak through the HBM sort);
    another seed = another sample"""
    scans = [synthetic_scan(150000, seed=51, fov_frac=0.5, far_frac=0.1), synthetic_scan(120000, seed=52, fov_frac=0.5)]
    hws = [(375, 1242)] * 2
    a, ref, _ = _run_both(scans, hws, 40000, 99, SCOPE, dev)
    _assert_same(a, ref)
    for _ in range(2):
        b, _, _ = _run_both(scans, hws, 40000, 99, SCOPE, dev)
        for key in ("src", "pts_input", "pts_features", "nvalid", "status"):
            assert torch.equal(a[key], b[key]), key
    c, _, _ = _run_both(scans, hws, 40000, 100, SCOPE, dev)
    assert not torch.equal(a["src"], c["src"])


def _device_batch(scans, dev):
    from pointrcnn_amd import kitti_input
    packed = kitti_input.pack_scans(scans, _calibs(len(scans)), HWS[:len(scans)], False)
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in packed.items()}


@pytest.mark.parametrize("npoints", [16384, 1000])
def test_large_export_on_small_sizes_is_the_old_export(dev, npoints):
    from pointrcnn_amd import _cabi, ops
    scans = [synthetic_scan(115000, 31, 0.4, 0.1), synthetic_scan(npoints + npoints // 3, 32, 0.6), np.zeros((0, 4), np.float32),
             synthetic_scan(300, 35, 0.5)]
    t = _device_batch(scans, dev)
    args = (t["raw"], t["offsets"], t["max_points"], t["calib"], t["img_hw"], SCOPE, npoints, 1234)
    old = ops.scene_prepare(*args, large=False)
    new = ops.scene_prepare(*args, large=True)
    for a, b in zip(old, new):
        assert torch.equal(a, b)
    lib = _cabi.lib()
    total, B = t["raw"].shape[0], len(scans)
    assert lib.prcnn_scene_large_workspace_bytes(total, B, npoints) == lib.prcnn_scene_workspace_bytes(total, B)
    ws = torch.empty(int(lib.prcnn_scene_workspace_bytes(total, B)), dtype=torch.uint8, device=dev)      # the old size is enough
    for a, b in zip(old, ops.scene_prepare(*args, large=True, workspace=ws)):
        assert torch.equal(a, b)


def test_large_export_domain(dev):
    from pointrcnn_amd import _cabi, ops
    t = _device_batch([synthetic_scan(5000, 31, 0.5)], dev)
    args = (t["raw"], t["offsets"], t["max_points"], t["calib"], t["img_hw"], SCOPE)
    for npoints in (65537, 0):
        with pytest.raises(_cabi.PointOpsError, match=r"1\.\.65536"):
            ops.scene_prepare(*args, npoints, 1, large=True)
    # the library itself: refused with the range in the message, and a sentinel-filled output stays untouched
    lib = _cabi.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())          # noqa: E731
    ws = torch.empty(int(lib.prcnn_scene_large_workspace_bytes(5000, 1, 65536)), dtype=torch.uint8, device=dev)
    scope = (ctypes.c_double * 6)(*[float(v) for v in SCOPE])
    for npoints in (65537, 0):
        rows = max(npoints, 16)
        xyz = torch.full((1, rows, 3), -77.0, device=dev)
        inten = torch.full((1, rows), -77.0, device=dev)
        src, nvalid, status = (torch.full(s, -77, dtype=torch.int32, device=dev) for s in ((1, rows), (1,), (1,)))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.prcnn_scene_prepare_large(p(t["raw"]), p(t["offsets"]), 1, 5000, 5000, p(t["calib"]), p(t["img_hw"]), scope, npoints, 1,
                                           p(xyz), p(inten), p(src), p(nvalid), p(status), p(ws), ws.numel(), stream)
        assert rc == -1 and b"1..65536" in lib.prcnn_last_error()
        torch.cuda.synchronize()
        for out in (xyz, inten, src, nvalid, status):
            assert bool((out == -77).all())
    with pytest.raises(_cabi.PointOpsError, match="workspace too small"):
        ops.scene_prepare(*args, 40000, 1, workspace=torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(_cabi.PointOpsError, match="workspace too small"):                # the small form's size is short above 16384
        ops.scene_prepare(*args, 40000, 1, workspace=torch.empty(int(lib.prcnn_scene_workspace_bytes(5000, 1)), dtype=torch.uint8, device=dev))
