"""Nested FPS levels answered from the parent's sample order (prcnn_fps_nested, ops.FPS_NESTED).

A cloud that gather_rows made from the indices furthest_point_sample returned IS that cloud's FPS order, so the next level's
samples are positions 0, 1, 2, ... unless the parent ran out of distinct points or a coordinate is non-finite / huge; a device
pass decides per frame, the rest run the plain kernels.  Every case here compares indices bit for bit with the oracle run level by
level, with the nested path on and off (off == PRCNN_FPS_NESTED=0): pass and fallback in one launch through the fps_reg sizes
("mixed", "odd"; "large" has the issue's sizes, whose nested levels are fps_reg too) and through sort + fps_pruned<4> with skip words
("pruned": a nested level of 4 096 points), a stale hint, the upstream order, inference tensors, the call routing, and the RPN in
inference and in training mode.
"""
import functools

import numpy as np
import pytest
import torch

from util import kitti_cloud

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the cached clouds are read-only


def lattice(dims, seed):
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3) * 0.5
    return g[np.random.default_rng(seed).permutation(len(g))].astype(np.float32)


def take(cloud, idx):
    return np.take_along_axis(cloud, idx[:, :, None].astype(np.int64), axis=1)


@functools.lru_cache(maxsize=None)
def case(name):
    """(level-0 cloud (B,N,3), the npoint of every level); computed once, never written to"""
    rng = np.random.default_rng(21)
    if name == "mixed":            # 512 -> 128 -> 32 -> 8: uniform | 37 distinct points wrapped | one NaN point | all points identical
        c = kitti_cloud(4, 512, seed=31)
        c[1] = rng.uniform(-10, 10, (37, 3)).astype(np.float32)[np.arange(512) % 37]
        c[2, 200, 1] = np.nan
        c[3] = c[3, 0]
        levels = (128, 32, 8)
    elif name == "large":          # 4 096 -> 1 024 -> 256 -> 64: sort + fps_pruned<4> (no hint), then nested fps_reg<64,16>, fps_reg<64,4>; frame 1 is a lattice
        c = kitti_cloud(2, 4096, seed=32)
        c[1] = lattice((16, 16, 16), 3)
        levels = (1024, 256, 64)
    elif name == "pruned":         # 8 192 -> 4 096 -> 1 024: the NESTED level runs fps_sort + fps_pruned<4> under skip words: frame 0 is accepted,
        c = kitti_cloud(2, 8192, seed=34)          # frame 1 (600 distinct points, wrapped) runs out of them before 1 024 samples: rejected
        c[1] = rng.uniform(-20, 20, (600, 3)).astype(np.float32)[np.arange(8192) % 600]
        levels = (4096, 1024)
    else:                          # odd sizes, 300 -> 150 -> 75: the wrapped frame runs out of distinct points INSIDE the nested levels
        assert name == "odd"
        c = kitti_cloud(3, 300, seed=33)
        c[1] = rng.uniform(-10, 10, (37, 3)).astype(np.float32)[np.arange(300) % 37]
        c[2, 1:] = c[2, :1] + np.float32(0.25) * rng.integers(0, 3, (299, 3)).astype(np.float32)       # 27 lattice sites
        levels = (150, 75)
    c.setflags(write=False)
    return c, levels


@functools.lru_cache(maxsize=None)
def oracle_levels(name):
    import oracle
    cpu = oracle.cpu()
    cloud, levels = case(name)
    out = []
    for n in levels:
        idx = cpu.fps(cloud, n)
        out.append(idx)
        cloud = take(cloud, idx)
    return out


class CallCounter:
    """stands in for the ctypes library (as bench.py's EventProfiler does) and counts the prcnn_* calls"""

    def __init__(self, lib):
        self._lib = lib
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("prcnn_"):
            return fn

        def wrapped(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return wrapped


@pytest.fixture
def counted(dev):
    from pointrcnn_amd import _cabi
    real = _cabi.lib()
    counter = CallCounter(real)
    _cabi._lib = counter
    try:
        yield counter.calls
    finally:
        _cabi._lib = real


@pytest.fixture(params=[True, False], ids=["nested", "plain"])
def nested(request, monkeypatch):
    from pointrcnn_amd import ops
    monkeypatch.setattr(ops, "FPS_NESTED", request.param)
    return request.param


def run_levels(x, levels):
    from pointrcnn_amd import ops
    out = []
    for n in levels:
        idx = ops.furthest_point_sample(x, n)
        out.append(idx)
        x = ops.gather_rows(x, idx).contiguous()            # (as the SA modules do: the same object for a contiguous tensor)
    return out


@pytest.mark.parametrize("name", ["mixed", "large", "odd", "pruned"])
def test_levels_match_the_oracle(dev, counted, nested, name):
    cloud, levels = case(name)
    got = run_levels(T(cloud, dev), levels)
    for lvl, (g, w) in enumerate(zip(got, oracle_levels(name))):
        g = g.cpu().numpy()
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert len(bad) == 0, "level %d (npoint %d): frames %s differ from the oracle" % (lvl, levels[lvl], bad.tolist())
    assert counted.get("prcnn_fps_nested", 0) == (len(levels) - 1 if nested else 0)
    assert counted.get("prcnn_fps", 0) == (1 if nested else len(levels))


@pytest.mark.parametrize("name,want_skip", [("mixed", [1, 1, 0, 0]), ("pruned", [1, 0])])
def test_the_device_pass_accepts_and_rejects_per_frame(dev, name, want_skip):
    """prcnn_fps_nested's skip words on the first nested level.  mixed (128 -> 32, fps_reg): the uniform frame and the wrapped frame
    (37 distinct points >= 32 samples) are answered with positions, the NaN frame and the all-identical frame run the kernels.
    pruned (4 096 -> 1 024, fps_sort + fps_pruned<4> through the (B,N) scratch): uniform accepted, 600 distinct points rejected."""
    from pointrcnn_amd import _cabi, ops
    cloud, levels = case(name)
    B = cloud.shape[0]
    x = T(cloud, dev)
    prev = ops.furthest_point_sample(x, levels[0])
    x1 = ops.gather_rows(x, prev)
    idx = torch.full((B, levels[1]), -7, dtype=torch.int32, device=dev)
    skip = torch.full((B,), -7, dtype=torch.int32, device=dev)
    tmp = torch.empty((B, levels[0]), dtype=torch.float32, device=dev) if levels[0] > 2048 else None
    _cabi.check(_cabi.lib().prcnn_fps_nested(x1.data_ptr(), prev.data_ptr(), B, levels[0], levels[1], None if tmp is None else tmp.data_ptr(),
                                             idx.data_ptr(), skip.data_ptr(), torch.cuda.current_stream().cuda_stream), "prcnn_fps_nested")
    assert skip.cpu().tolist() == want_skip
    assert np.array_equal(idx.cpu().numpy(), oracle_levels(name)[1])
    if name != "mixed":
        return
    L = _cabi.lib()
    assert L.prcnn_fps_nested(x1.data_ptr(), prev.data_ptr(), 4, 16, 32, None, idx.data_ptr(), skip.data_ptr(), None) == -1          # npoint > N
    assert L.prcnn_fps_nested(x1.data_ptr(), None, 4, 128, 32, None, idx.data_ptr(), skip.data_ptr(), None) == -1                     # null prev_idx
    assert L.prcnn_fps_nested(x1.data_ptr(), prev.data_ptr(), 1, 20000, 32, x1.data_ptr(), idx.data_ptr(), skip.data_ptr(), None) == -1   # N > 16384
    assert L.prcnn_fps_nested(None, None, 0, 128, 32, None, None, None, None) == 0                                                   # empty problem


def test_stale_hint_falls_back(dev, cpu, counted, nested):
    """rows of the sample set overwritten in place after sampling: the tensor's version moved, the hint is void"""
    from pointrcnn_amd import ops
    cloud, levels = case("mixed")
    x = T(cloud[:2], dev)
    new_xyz = ops.gather_rows(x, ops.furthest_point_sample(x, 128))
    assert (getattr(new_xyz, "_prcnn_fps_parent", None) is not None) == nested          # (with the switch off no hint is made at all)
    new_xyz[:, 1:12] = new_xyz[:, :1]               # positions 1..11 now duplicate position 0: FPS must not return them early
    before = dict(counted)
    got = ops.furthest_point_sample(new_xyz, 32).cpu().numpy()
    assert np.array_equal(got, cpu.fps(new_xyz.cpu().numpy(), 32))
    assert not np.array_equal(got[0], np.arange(32))
    assert counted.get("prcnn_fps_nested", 0) == before.get("prcnn_fps_nested", 0)
    assert counted["prcnn_fps"] == before["prcnn_fps"] + 1


def test_upstream_order_takes_no_hint(dev, cpu, counted):
    from pointrcnn_amd import ops
    x = T(lattice((16, 8, 16), 5)[None], dev)
    new_xyz = ops.gather_rows(x, ops.furthest_point_sample(x, 1536))
    assert getattr(new_xyz, "_prcnn_fps_parent", None) is not None
    got = ops.furthest_point_sample(new_xyz, 384, order="upstream").cpu().numpy()
    assert np.array_equal(got, cpu.fps_upstream(new_xyz.cpu().numpy(), 384))
    assert not np.array_equal(got[0], np.arange(384))           # (1 536 points, T = 1 024: the tie orders differ on this lattice)
    assert counted.get("prcnn_fps_nested", 0) == 0 and counted["prcnn_fps_order"] == 1


def test_inference_tensors_carry_no_hint(dev, counted):
    """tensors made under torch.inference_mode() track no version counter (reading it raises; an in-place write leaves no trace):
    sample, gather, sample there works as before, on plain prcnn_fps, whether the cloud itself is an inference tensor or not"""
    from pointrcnn_amd import ops
    cloud, levels = case("mixed")
    outside = T(cloud, dev)
    with torch.inference_mode():
        for x in (outside, T(cloud, dev)):
            counted.clear()
            got = run_levels(x, levels)
            assert counted == {"prcnn_fps": len(levels), "prcnn_gather_rows": len(levels)}
            for g, w in zip(got, oracle_levels("mixed")):
                assert np.array_equal(g.cpu().numpy(), w)
        # a sample set tagged OUTSIDE inference mode keeps its hint inside (its tensors do track versions)
    new_xyz = ops.gather_rows(outside, ops.furthest_point_sample(outside, levels[0]))
    counted.clear()
    with torch.inference_mode():
        got = ops.furthest_point_sample(new_xyz, levels[1])
    assert counted == {"prcnn_fps_nested": 1}
    assert np.array_equal(got.cpu().numpy(), oracle_levels("mixed")[1])


def test_call_routing(dev, counted):
    """only the very tensor gather_rows returned carries the hint: a clone, a view, a slice copy and the composed drop-in route do not"""
    from pointrcnn_amd import ops
    cloud, _ = case("mixed")
    x = T(cloud[:1], dev)
    idx = ops.furthest_point_sample(x, 128)
    new_xyz = ops.gather_rows(x, idx)
    assert new_xyz.contiguous() is new_xyz

    def calls_of(fn):
        before = dict(counted)
        fn()
        return {k: v - before.get(k, 0) for k, v in counted.items() if v != before.get(k, 0)}

    assert calls_of(lambda: ops.furthest_point_sample(new_xyz, 32)) == {"prcnn_fps_nested": 1}
    assert calls_of(lambda: ops.furthest_point_sample(new_xyz.contiguous(), 128)) == {"prcnn_fps_nested": 1}       # npoint == the parent's
    assert calls_of(lambda: ops.furthest_point_sample(new_xyz.clone(), 32)) == {"prcnn_fps": 1}
    assert calls_of(lambda: ops.furthest_point_sample(new_xyz.view(1, 128, 3), 32)) == {"prcnn_fps": 1}
    assert calls_of(lambda: ops.furthest_point_sample(new_xyz[:, :64].contiguous(), 32)) == {"prcnn_fps": 1}
    # indices that are not the FPS result of THAT tensor, or were edited since, make no hint
    other = ops.gather_rows(x.clone(), idx)
    assert getattr(other, "_prcnn_fps_parent", None) is None
    idx2 = ops.furthest_point_sample(x, 128)
    idx2[:, 3] = 7
    assert getattr(ops.gather_rows(x, idx2), "_prcnn_fps_parent", None) is None
    # the parent's indices edited AFTER the gather: void as well
    idx[:, 5] = 0
    assert calls_of(lambda: ops.furthest_point_sample(new_xyz, 32)) == {"prcnn_fps": 1}
    # the composed drop-in route carries no hint
    from pointnet2_lib.pointnet2 import pointnet2_utils
    flipped = x.transpose(1, 2).contiguous()
    composed = pointnet2_utils.gather_operation(flipped, pointnet2_utils.furthest_point_sample(x, 128)).transpose(1, 2).contiguous()
    assert calls_of(lambda: ops.furthest_point_sample(composed, 32)) == {"prcnn_fps": 1}


def test_rpn_forward_is_unchanged(dev, counted, monkeypatch):
    from pointrcnn_amd import ops, rpn
    torch.manual_seed(4)
    model = rpn.randomize_bn_stats(rpn.RPN()).to(dev).eval()
    pts = rpn.synthetic_clouds(1, 16384, device=dev)
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "FPS_NESTED", flag)
        counted.clear()
        with torch.no_grad():
            out = model({"pts_input": pts})
        outs.append({k: out[k].clone() for k in ("rpn_cls", "rpn_reg", "backbone_features")})
        assert counted.get("prcnn_fps_nested", 0) == (3 if flag else 0)
        assert counted["prcnn_fps"] == (1 if flag else 4)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_rpn_training_forward_takes_the_nested_route(dev, counted):
    """the training step draws the samples of all four levels in one chain (Pointnet2MSG._sample_ahead, or the SA modules' own
    furthest_point_sample + gather_rows): one plain level, three nested ones"""
    from pointrcnn_amd import rpn
    torch.manual_seed(5)
    model = rpn.RPN().to(dev).train()
    pts = rpn.synthetic_clouds(2, 16384, device=dev)
    counted.clear()
    with torch.enable_grad():
        out = model({"pts_input": pts})
    assert out["rpn_cls"].requires_grad
    assert counted.get("prcnn_fps_nested", 0) == 3 and counted["prcnn_fps"] == 1
