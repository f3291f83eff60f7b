"""What ops.scene_prepare, ops.train_scene_prepare and ops.gt_database_build require of the arguments they share -- raw, offsets,
calib and (the first two) img_hw: every malformed one is refused in Python, before the library is called, with the exception type
the wrappers raised for it before they took these checks from one helper (ops._frames)."""
import pytest
import torch

from util import synthetic_scan

pytestmark = pytest.mark.gpu
NPOINTS, G = 128, 2
WRAPPERS = ("scene_prepare", "train_scene_prepare", "gt_database_build")

# case -> (the argument it replaces, how, the exception type each wrapper's own check raised before the helper existed)
CASES = {
    "offsets_int32": ("offsets", lambda t: t.to(torch.int32), RuntimeError),
    "offsets_non_contiguous": ("offsets", lambda t: torch.stack([t, t], 1)[:, 0], RuntimeError),
    "offsets_on_cpu": ("offsets", lambda t: t.cpu(), RuntimeError),
    "raw_total_by_3": ("raw", lambda t: t[:, :3].contiguous(), RuntimeError),
    "calib_b_by_23": ("calib", lambda t: t[:, :23].contiguous(), RuntimeError),
    "calib_b_plus_1_rows": ("calib", lambda t: torch.cat([t, t[:1]]), RuntimeError),
    "img_hw_b_by_3": ("img_hw", lambda t: torch.cat([t, t[:, :1]], 1), RuntimeError),
}


@pytest.fixture(scope="module")
def frames(dev):
    from pointrcnn_amd import kitti_input
    calib = kitti_input.Calibration.from_text(kitti_input.KITTI_CALIB_TXT)
    pk = kitti_input.pack_scans([synthetic_scan(256, seed=1), synthetic_scan(300, seed=2)], [calib] * 2, [(375, 1242)] * 2, pin=False)
    a = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in pk.items()}
    a["boxes3d"] = torch.tensor([0.0, 1.0, 20.0, 1.5, 1.6, 3.9, 0.3], device=dev).repeat(2, G, 1)
    a["alpha"] = torch.zeros((2, G), device=dev)
    a["num"] = torch.full((2,), G, dtype=torch.int32, device=dev)
    return a


def _call(name, a):
    from pointrcnn_amd import ops
    if name == "scene_prepare":
        return ops.scene_prepare(a["raw"], a["offsets"], a["max_points"], a["calib"], a["img_hw"], None, NPOINTS, 1)
    if name == "train_scene_prepare":
        return ops.train_scene_prepare(a["raw"], a["offsets"], a["max_points"], a["calib"], a["img_hw"], None, NPOINTS, 1, a["boxes3d"],
                                       a["alpha"], a["num"])
    return ops.gt_database_build(a["raw"], a["offsets"], a["max_points"], a["calib"], a["boxes3d"], a["num"])


@pytest.mark.parametrize("name", WRAPPERS)
def test_well_formed_arguments_are_accepted(frames, name):
    _call(name, frames)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,case", [(n, c) for n in WRAPPERS for c in sorted(CASES)
                                       if not (n == "gt_database_build" and CASES[c][0] == "img_hw")])      # it takes no img_hw
def test_malformed_shared_argument_is_refused(frames, name, case):
    key, change, exc = CASES[case]
    bad = dict(frames)
    bad[key] = change(frames[key])
    with pytest.raises(exc) as info:
        _call(name, bad)
    assert type(info.value) is exc                          # the type itself, not a subclass (PointOpsError is a RuntimeError)
