"""CPU: the training heads' device tail (csrc/head_tail.hip) -- everything about it that needs no GPU.

Mask: csrc/head_tail_math.h compiled for the host (tests/head_tail_host.cpp, -Wall -Wextra -Werror) equals the Python twin
train_mlp.head_keep_mask bit for bit; the keep share of a case lies within 4 sigma of 1 - p, sigma = sqrt(p (1 - p) / (R K)); masks of
different streams or calls agree on about half of their entries ([0.49, 0.51]: two independent p = 0.5 masks agree with probability 0.5,
sigma 6.9e-4 at 4096 x 128).  Measured on the generator: shares 0.49954, 0.49919, 0.50144, 0.69802 (0.7, 1.2, 2.1 and 1.1 sigma).
Plans: pytorch_utils._head_plan on the RPN and RCNN heads, switch on and off.  Dropout state: keys, call counters, checkpoints.
ABI: the four exports in the header, in _cabi.SIGNATURES and in the built library; the version stays 12."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import pointrcnn_amd
from pointrcnn_amd import _cabi, train_mlp

pointrcnn_amd.install()
import pointnet2_lib.pointnet2.pytorch_utils as pt_utils  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(0, 70, 0, 4096, 128, 0.5), (0, 71, 0, 4096, 128, 0.5), (0, 70, 1, 4096, 128, 0.5), (7, 70, 3, 257, 256, 0.3)]
EXPORTS = ("prcnn_head_tail_fwd", "prcnn_head_tail_work_bytes", "prcnn_head_tail_bwd", "prcnn_dropout_rows")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    work = tmp_path_factory.mktemp("head_tail_host")
    exe = os.path.join(str(work), "head_tail_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", os.path.join(ROOT, "pointrcnn_amd", "csrc"),
                    os.path.join(ROOT, "tests", "head_tail_host.cpp"), "-o", exe], check=True)

    def run(seed, stream, call, R, K, p):
        out = os.path.join(str(work), "mask.bin")
        subprocess.run([exe, str(seed), str(stream), str(call), str(R), str(K), repr(float(p)), out], check=True)
        blob = np.fromfile(out, np.uint8)
        return blob[:R * K].reshape(R, K).astype(bool), float(blob[R * K:].view(np.float32)[0])
    return run


@pytest.fixture(scope="module")
def twins():
    return [train_mlp.head_keep_mask(*c) for c in CASES]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_host_build_of_the_header_equals_the_python_twin(host, twins, ci):
    seed, stream, call, R, K, p = CASES[ci]
    got, scale = host(*CASES[ci])
    assert got.shape == twins[ci].shape == (R, K) and twins[ci].dtype == np.bool_
    assert np.array_equal(got, twins[ci])
    assert scale == float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def test_p_zero_keeps_everything(host):
    got, scale = host(3, 72, 5, 64, 32, 0.0)
    assert got.all() and scale == 1.0
    assert train_mlp.head_keep_mask(3, 72, 5, 64, 32, 0.0).all()


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_keep_share(twins, ci):
    _, _, _, R, K, p = CASES[ci]
    share = float(twins[ci].mean())
    sigma = math.sqrt(p * (1 - p) / (R * K))
    print("case %s: keep share %.5f, 1 - p %.2f, sigma %.2e, %.2f sigma" % (CASES[ci], share, 1 - p, sigma, abs(share - (1 - p)) / sigma))
    assert abs(share - (1 - p)) <= 4 * sigma


def test_streams_and_calls_draw_different_masks(twins):
    for a, b in ((0, 1), (0, 2), (1, 2)):
        agree = float((twins[a] == twins[b]).mean())
        print("cases %d, %d agree on %.5f of their entries" % (a, b, agree))
        assert 0.49 <= agree <= 0.51


def test_the_counter_wraps_at_two_to_the_32():
    """R * K = 2^32 is inside the domain: the last row's counters are 2^32 - K .. 2^32 - 1, and the twin takes r * K + k mod 2^32"""
    from pointrcnn_amd.kitti_input import counter_rand
    K = 128
    i = np.arange(2 ** 32 - K, 2 ** 32, dtype=np.uint64)
    u = (counter_rand(0, 70, 0, i) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert ((u >= 0) & (u < 1)).all() and 0.3 < float((u >= np.float32(0.5)).mean()) < 0.7


# ---- plans ---------------------------------------------------------------------------------------------------------------------
def _heads():
    from pointrcnn_amd import rcnn, rpn
    r = rpn.RPN()
    c = rcnn.RCNNNet()
    return (r.rpn_cls_layer, r.rpn_reg_layer), (c.cls_layer, c.reg_layer)


@pytest.fixture()
def device_blind_stack_ok(monkeypatch):
    """train_mlp.stack_ok asks for CUDA weights; the plan's SHAPE is what is under test here (tests/test_gpu_head_tail.py checks the
    plans again on the device with the real predicate), so this stand-in keeps the layer-form tests and drops the device test"""
    def form_ok(m):
        if not isinstance(m, pt_utils._ConvBase) or not m._prcnn_fusable:
            return False
        conv, bn, act = m._parts()
        if not isinstance(act, nn.ReLU) or (bn is not None and (conv.bias is not None or not bn.training)):
            return False
        return conv.kernel_size == (1,) and conv.out_channels % 4 == 0
    monkeypatch.setattr(train_mlp, "stack_ok", lambda mods: len(mods) > 0 and all(form_ok(m) for m in mods))


def _kinds(plan):
    return [s[0] for s in plan]


def test_plan_of_the_rpn_heads(device_blind_stack_ok):
    rpn_heads, _ = _heads()
    for seq, n in zip(rpn_heads, (1, 76)):
        seq.train()
        plan = pt_utils._head_plan(seq, True)
        assert _kinds(plan) == ["stack", "tail"]
        assert len(plan[0][1]) == 1 and isinstance(plan[1][1], nn.Dropout) and plan[1][1].p == 0.5
        assert plan[1][2]._parts()[0].out_channels == n and plan[1][2]._parts()[0].in_channels == 128
        off = pt_utils._head_plan(seq, False)
        assert _kinds(off) == ["stack", "dropout", "linear"] and off[1][1] is seq[1] and off[2][1] is seq[2]
        seq[1].eval()                                   # a Dropout in eval mode is the identity: a tail with no Dropout
        plan = pt_utils._head_plan(seq, True)
        assert _kinds(plan) == ["stack", "tail"] and plan[1][1] is None


def test_plan_of_the_rcnn_heads(device_blind_stack_ok):
    _, rcnn_heads = _heads()
    for seq, n in zip(rcnn_heads, (1, 46)):
        seq.train()
        plan = pt_utils._head_plan(seq, True)
        assert _kinds(plan) == ["stack", "tail"]
        assert len(plan[0][1]) == 2 and plan[1][1] is None            # Dropout(0) left the plan: one two-layer stack, tail with p = 0
        assert plan[1][2]._parts()[0].out_channels == n and plan[1][2]._parts()[0].in_channels == 256
        off = pt_utils._head_plan(seq, False)
        assert _kinds(off) == ["stack", "dropout", "stack", "linear"]


def test_plan_of_a_lone_dropout_and_of_an_uncovered_member(device_blind_stack_ok):
    seq = nn.Sequential(pt_utils.Conv1d(32, 32, bn=True), nn.Dropout(0.25), pt_utils.Conv1d(32, 32, bn=True)).train()
    assert _kinds(pt_utils._head_plan(seq, True)) == ["stack", "dropout_dev", "stack"]
    assert _kinds(pt_utils._head_plan(seq, False)) == ["stack", "dropout", "stack"]
    seq = nn.Sequential(pt_utils.Conv1d(32, 32, bn=True), nn.Sigmoid())
    assert pt_utils._head_plan(seq, True) is None and pt_utils._head_plan(seq, False) is None


def test_the_switch_is_off_by_default_and_rejects_other_values():
    env = {k: v for k, v in os.environ.items() if not k.startswith("PRCNN_HEAD_TAIL")}
    code = ("import pointrcnn_amd; pointrcnn_amd.install(); import pointnet2_lib.pointnet2.pytorch_utils as p; "
            "print(p.HEAD_TAIL, p.HEAD_TAIL_SEED)")
    run = lambda e: subprocess.run([os.sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True)  # noqa: E731
    assert run(env).stdout.split() == ["False", "0"]
    assert run(dict(env, PRCNN_HEAD_TAIL="0")).stdout.split() == ["False", "0"]
    assert run(dict(env, PRCNN_HEAD_TAIL="1", PRCNN_HEAD_TAIL_SEED="9")).stdout.split() == ["True", "9"]
    bad = run(dict(env, PRCNN_HEAD_TAIL="yes"))
    assert bad.returncode != 0 and "PRCNN_HEAD_TAIL" in bad.stderr


# ---- dropout state -------------------------------------------------------------------------------------------------------------
def test_key_dropouts_is_a_function_of_the_model_alone():
    from pointrcnn_amd import rpn
    a, b = rpn.RPN(), rpn.RPN()
    sa, sb = pt_utils.key_dropouts(a, 5), pt_utils.key_dropouts(b, 5, rank=2)
    assert sa == sb == {"rpn_cls_layer.1": 70, "rpn_reg_layer.1": 71}
    assert a.rpn_cls_layer[1]._prcnn_seed == 5 and b.rpn_cls_layer[1]._prcnn_seed == 7
    assert pt_utils.key_dropouts(a, 2 ** 32 - 1, rank=1) == sa and a.rpn_reg_layer[1]._prcnn_seed == 0        # mod 2^32
    m = a.rpn_reg_layer[1]
    assert pt_utils._take_key(m) == (0, 71, 0, 0.5) and pt_utils._take_key(m) == (0, 71, 1, 0.5)
    lone = nn.Dropout(0.1)                             # met un-keyed: the next ordinal, the environment's seed
    key = pt_utils._take_key(lone)
    assert key[0] == pt_utils.HEAD_TAIL_SEED and key[1] >= 72 and key[2] == 0
    assert pt_utils._take_key(nn.Dropout(0.1))[1] == key[1] + 1


def test_dropout_state_round_trip():
    from pointrcnn_amd import rpn
    a = rpn.RPN()
    pt_utils.key_dropouts(a, 0)
    for _ in range(3):
        pt_utils._take_key(a.rpn_cls_layer[1])
    pt_utils._take_key(a.rpn_reg_layer[1])
    state = pt_utils.dropout_state(a)
    assert state == {"rpn_cls_layer.1": 3, "rpn_reg_layer.1": 1}
    b = rpn.RPN()
    pt_utils.key_dropouts(b, 0)
    pt_utils.load_dropout_state(b, state)
    assert pt_utils.dropout_state(b) == state and pt_utils._take_key(b.rpn_cls_layer[1]) == (0, 70, 3, 0.5)
    with pytest.raises(ValueError, match="no Dropout named"):
        pt_utils.load_dropout_state(b, {"nowhere.1": 2})


def test_checkpoints_carry_the_state_only_with_the_switch_on(monkeypatch, tmp_path):
    from pointrcnn_amd import rpn, train_loop
    a = rpn.RPN()
    monkeypatch.setattr(pt_utils, "HEAD_TAIL", False)
    off = train_loop.checkpoint_state(a, None, epoch=1, it=2)
    assert sorted(off) == ["epoch", "it", "model_state", "optimizer_state"]
    monkeypatch.setattr(pt_utils, "HEAD_TAIL", True)
    pt_utils.key_dropouts(a, 0)
    pt_utils._take_key(a.rpn_cls_layer[1])
    on = train_loop.checkpoint_state(a, None, epoch=1, it=2)
    assert on["dropout_calls"] == {"rpn_cls_layer.1": 1, "rpn_reg_layer.1": 0}
    assert sorted(k for k in on if k != "dropout_calls") == sorted(off)
    train_loop.save_checkpoint(on, str(tmp_path / "ck"))
    b = rpn.RPN()
    pt_utils.key_dropouts(b, 0)
    train_loop.load_checkpoint(b, None, str(tmp_path / "ck.pth"))
    assert pt_utils.dropout_state(b) == on["dropout_calls"]
    monkeypatch.setattr(pt_utils, "HEAD_TAIL", False)               # switch off: the entry is ignored, as an older build would
    c = rpn.RPN()
    train_loop.load_checkpoint(c, None, str(tmp_path / "ck.pth"))
    assert pt_utils.dropout_state(c) == {"rpn_cls_layer.1": 0, "rpn_reg_layer.1": 0}


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_four_exports_are_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "prcnn_pointops.h")) as f:
        header = f.read()
    for name in EXPORTS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert name in _cabi.SIGNATURES
    syms = subprocess.run(["nm", "-D", "--defined-only", _cabi.library_path()], capture_output=True, text=True, check=True).stdout
    for name in EXPORTS:
        assert re.search(r" T %s$" % name, syms, re.M), name
    lib = _cabi.lib()
    assert lib.prcnn_abi_version() == 12
    from pointrcnn_amd import ops
    rows = ops.HEAD_TAIL_PART_ROWS
    assert lib.prcnn_head_tail_work_bytes(rows, 128, 76) == (76 * 128 + 76) * 4              # pure host queries
    assert lib.prcnn_head_tail_work_bytes(rows + 1, 128, 76) == 2 * (76 * 128 + 76) * 4
    for R, K, N in ((64, 48, 8), (64, 128, 97), (64, 288, 8), (0, 128, 8), (2 ** 32 // 128 + 1, 128, 8)):
        assert lib.prcnn_head_tail_work_bytes(R, K, N) == 0
        assert not ops.head_tail_supported(R, K, N, 0.5)
    assert ops.head_tail_supported(2 ** 32 // 128, 128, 8, 0.0) and not ops.head_tail_supported(64, 128, 8, 1.0)
