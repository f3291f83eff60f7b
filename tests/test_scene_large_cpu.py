"""CPU: the large forms of the two input builders (prcnn_scene_prepare_large, prcnn_train_scene_prepare_large; npoints up to
65536) as far as they can be held without a device: the workspace arithmetic, the exports, and the refusal of an npoints
outside 1..65536 before anything is allocated or launched."""
import re
import subprocess

import pytest
import torch

from test_cabi_and_host import header_decls

NEW = ("prcnn_scene_prepare_large", "prcnn_scene_large_workspace_bytes", "prcnn_train_scene_prepare_large",
       "prcnn_train_scene_large_workspace_bytes")
SHAPES = [(0, 0), (1, 1), (115000, 1), (8 * 400000, 8), (123457, 6)]


def test_workspace_equals_the_small_form_up_to_16384():
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    for total, B in SHAPES:
        for npoints in (1, 1000, 16383, 16384):
            assert lib.prcnn_scene_large_workspace_bytes(total, B, npoints) == lib.prcnn_scene_workspace_bytes(total, B)
            for K, dbm in ((0, 0), (16, 1500), (64, 4000)):
                assert lib.prcnn_train_scene_large_workspace_bytes(total, B, K, dbm, npoints) == \
                    lib.prcnn_train_scene_workspace_bytes(total, B, K, dbm)


def test_workspace_grows_monotonically_above_16384():
    """above the one-workgroup form the need grows by B key arrays of NP = npoints rounded up to a power of two, 8 bytes a key,
    and one 4-byte record per frame, placed on a 256-byte boundary"""
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    sizes = (16384, 16385, 20000, 32768, 32769, 40000, 65535, 65536)
    for total, B in SHAPES[1:]:
        small = lib.prcnn_scene_workspace_bytes(total, B)
        got = [lib.prcnn_scene_large_workspace_bytes(total, B, n) for n in sizes]
        assert got == sorted(got) and got[1] > got[0] == small and got[4] > got[3]
        tsmall = lib.prcnn_train_scene_workspace_bytes(total, B, 16, 1500)
        tgot = [lib.prcnn_train_scene_large_workspace_bytes(total, B, 16, 1500, n) for n in sizes]
        assert tgot == sorted(tgot) and tgot[1] > tgot[0] == tsmall and tgot[4] > tgot[3]
        for n, g, tg in zip(sizes[1:], got[1:], tgot[1:]):
            NP = 32768 if n <= 32768 else 65536
            assert small + B * NP * 8 + B * 4 <= g < small + B * NP * 8 + B * 4 + 256
            assert tsmall + B * NP * 8 + B * 4 <= tg < tsmall + B * NP * 8 + B * 4 + 256


def test_workspace_is_zero_on_negative_arguments():
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    assert lib.prcnn_scene_large_workspace_bytes(-1, 2, 40000) == 0
    assert lib.prcnn_scene_large_workspace_bytes(10, -2, 40000) == 0
    assert lib.prcnn_scene_large_workspace_bytes(10, 2, -1) == 0
    for args in ((-1, 2, 1, 1, 40000), (10, -1, 1, 1, 40000), (10, 2, -1, 1, 40000), (10, 2, 1, -1, 40000), (10, 2, 1, 1, -5)):
        assert lib.prcnn_train_scene_large_workspace_bytes(*args) == 0


def test_new_exports_in_header_signatures_and_library():
    from pointrcnn_amd import _cabi
    decls = header_decls()
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (prcnn_\w+)", out))
    for name in NEW:
        assert name in decls and name in _cabi.SIGNATURES and name in exported, name
    # the large exports take the argument lists of the originals
    assert _cabi.SIGNATURES["prcnn_scene_prepare_large"] == _cabi.SIGNATURES["prcnn_scene_prepare"]
    assert _cabi.SIGNATURES["prcnn_train_scene_prepare_large"] == _cabi.SIGNATURES["prcnn_train_scene_prepare"]


def test_library_refuses_npoints_outside_the_domain_without_a_device():
    """the domain check comes first: with B = 0 nothing else of the arguments is looked at"""
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    null18 = [None, None, 0, 0, 0, None, None, None]
    for npoints in (0, 65537, -3):
        assert lib.prcnn_scene_prepare_large(*null18, npoints, 1, None, None, None, None, None, None, 0, None) == -1
        assert b"1..65536" in lib.prcnn_last_error() and b"prcnn_scene_prepare_large" in lib.prcnn_last_error()
    assert lib.prcnn_scene_prepare_large(*null18, 65536, 1, None, None, None, None, None, None, 0, None) == 0      # B = 0: nothing to do
    # the old export keeps its domain and its message
    assert lib.prcnn_scene_prepare(*null18, 16385, 1, None, None, None, None, None, None, 0, None) == -1
    assert b"1..16384: the shuffle is one LDS-resident sort per frame" in lib.prcnn_last_error()


@pytest.mark.parametrize("npoints", [65537, 0])
def test_ops_refuse_npoints_before_any_launch(npoints):
    """CPU tensors: had the check come after the allocation or the launch, the error would be another one"""
    from pointrcnn_amd import _cabi, ops
    raw = torch.zeros((10, 4))
    off = torch.tensor([0, 10], dtype=torch.int64)
    calib = torch.zeros((1, 24))
    hw = torch.tensor([[375, 1242]], dtype=torch.int32)
    with pytest.raises(_cabi.PointOpsError, match=r"1\.\.65536"):
        ops.scene_prepare(raw, off, 10, calib, hw, None, npoints, 1, large=True)
    with pytest.raises(_cabi.PointOpsError, match=r"1\.\.65536"):
        ops.train_scene_prepare(raw, off, 10, calib, hw, None, npoints, 1, torch.zeros((1, 0, 7)), torch.zeros((1, 0)), large=True)
    if npoints > 16384:
        with pytest.raises(_cabi.PointOpsError, match=r"1\.\.65536"):
            ops.scene_prepare(raw, off, 10, calib, hw, None, npoints, 1)                # large=None follows npoints
