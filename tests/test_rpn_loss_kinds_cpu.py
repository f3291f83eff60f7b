"""CPU: the DiceLoss / BinaryCrossEntropy arithmetic of the fused RPN loss (pointrcnn_amd/csrc/rpn_loss_math.h: rl_bce_row,
rl_dice_row, rl_dice_grad), compiled for the host by tests/rpn_loss_kinds_host.cpp -- once plain, once with
-fsanitize=address,undefined -- and the pure-Python routing decision of train_functions (_fused_rpn_loss_kind, _fused_level).

Against float64 closed forms on a seeded grid of logits in [-12, 12], both targets and the ignore label.  The measure and the bar are
those of tests/test_rpn_loss_math_cpu.py (_check): |err| / S per point, at most 8 x what the COMPOSED float32 code (torch.sigmoid,
F.binary_cross_entropy, torch.min / max with autograd, torch CPU) has at that point and never below 8 x 2^-24.  S is the sum of the
absolute values of the addends that form the value, and for the values that are functions of the ROUNDED float32 p it carries the
condition of that function: p = 1 / (1 + exp(-x)) is three rounded operations, a relative error e of p moves log(p) by e and
log(1 - p) by e p / (1 - p), and (1 - p) p = p - p p has the addends p and p^2:
    BCE term        w (|log p| + 3) against t = 1,  w (|log(1 - p)| + 3 p / (1 - p)) against t = 0
    BCE d/dx        w (p + t)
    Dice lo, hi     p + t;   d lo, d hi: p + p^2 where the closed form is not 0
    Dice d/dx       |coefficient| (p + p^2)
Entries whose closed form is 0 (an ignored row, the inactive one of d lo / d hi, d/dx of a background row while B < 1) must be 0.
Worst figures over the grid (composed float32, header): BCE term 6.8e-8 / 6.8e-8, BCE derivative 1.94e-7 / 1.93e-7, Dice lo / hi
9.8e-8 / 9.8e-8, d lo / d hi 1.31e-7 / 1.31e-7, Dice d/dx 1.9e-7 / 1.33e-7.

At logits +-20, +-90, +-200, where float32 sigmoid has saturated on one or both sides, value and derivative EQUAL what the composed
float32 expressions give through torch on the CPU.
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pointrcnn_amd import train_functions as tf
from test_rpn_loss_math_cpu import F32, _check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
FG_WEIGHTS = (1.0, 15.0)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rpn_loss_kinds") / "rpn_loss_kinds_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "rpn_loss_kinds_host.cpp"),
                    "-o", exe], check=True)
    work = os.path.dirname(exe)

    def run(mode, records):
        records = np.ascontiguousarray(records, dtype=F32)
        records.tofile(os.path.join(work, "in.bin"))
        r = subprocess.run([exe, mode, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(os.path.join(work, "out.bin"), F32).reshape(len(records), -1)
    return run


def grid():
    """logits in [-12, 12]: a regular grid with both ends and 0, and seeded draws"""
    rng = np.random.default_rng(20240911)
    return np.concatenate([np.linspace(-12, 12, 97), rng.uniform(-12, 12, 400)]).astype(F32)


def records(xs, *cols):
    """every logit with every label of (-1, 0, 1) and every combination of the extra columns"""
    rec = [[x, lab]  for x in xs for lab in (-1.0, 0.0, 1.0)]
    for col in cols:
        rec = [r + [v] for r in rec for v in col]
    return np.array(rec, F32)


def sig64(x):
    """sigmoid(x), 1 - sigmoid(x) in float64 without cancellation"""
    return 1 / (1 + np.exp(-x)), 1 / (1 + np.exp(x))


def composed_bce(rec):
    """the composed float32 BCE row terms and their derivatives (get_rpn_loss's BinaryCrossEntropy branch, per point)"""
    x = torch.from_numpy(rec[:, 0].copy()).requires_grad_(True)
    lab = torch.from_numpy(rec[:, 1].copy())
    fg = lab > 0
    weight = torch.ones_like(x)
    weight[fg] = torch.from_numpy(rec[:, 2].copy())[fg]
    per = F.binary_cross_entropy(torch.sigmoid(x), fg.float(), weight=weight, reduction="none") * (lab >= 0).float()
    per.sum().backward()
    return per.detach().numpy(), x.grad.numpy()


def composed_dice(rec):
    """the composed float32 Dice addends min(p, t), max(p, t) per point (DiceLoss.sums before the sum) and their derivatives"""
    out = []
    for fn in (torch.min, torch.max):
        x = torch.from_numpy(rec[:, 0].copy()).requires_grad_(True)
        t = torch.from_numpy(rec[:, 1].copy())
        v = fn(torch.sigmoid(x), t) * (t != -1).float()
        v.sum().backward()
        out += [v.detach().numpy(), x.grad.numpy()]
    return out[0], out[2], out[1], out[3]


def composed_dice_grad(rec):
    """d/dx of the composed data-parallel form k (-lo / Bc + [B >= 1] A / Bc^2 hi) in float32 with A, B, k given"""
    x = torch.from_numpy(rec[:, 0].copy()).requires_grad_(True)
    t = torch.from_numpy(rec[:, 1].copy())
    A, B, k = (torch.from_numpy(rec[:, j].copy()) for j in (2, 3, 4))
    p = torch.sigmoid(x)
    live = (t != -1).float()
    free = (B >= 1.0).float()
    Bc = torch.clamp(B, min=1.0)
    (k * (-(torch.min(p, t) * live) / Bc + free * A / (Bc * Bc) * (torch.max(p, t) * live))).sum().backward()
    return x.grad.numpy()


def test_bce_rows_against_float64(host):
    rec = records(grid(), FG_WEIGHTS)
    got = host("bce", rec)
    x, lab, fgw = (rec[:, k].astype(np.float64) for k in range(3))
    t, valid = (lab > 0).astype(np.float64), lab >= 0
    w = np.where(lab > 0, fgw, 1.0)
    p, omp = sig64(x)
    ref_v = np.where(valid, -w * (t * np.log(p) + (1 - t) * np.log(omp)), 0.0)
    ref_d = np.where(valid, w * (p - t), 0.0)
    ref_d = np.where(valid & (t > 0), -w * omp, ref_d)                  # p - 1 without cancellation
    S_v = w * np.where(t > 0, np.abs(np.log(p)) + 3, np.abs(np.log(omp)) + 3 * p / omp)
    S_d = w * (p + t)
    cmp_v, cmp_d = composed_bce(rec)
    assert not got[~valid].any() and not cmp_v[~valid].any()
    _check("BCE term", got[valid, 0], ref_v[valid], cmp_v[valid], S_v[valid])
    _check("BCE derivative", got[valid, 1], ref_d[valid], cmp_d[valid], S_d[valid])


def test_dice_rows_against_float64(host):
    rec = records(grid())
    got = host("dice", rec)
    x, lab = rec[:, 0].astype(np.float64), rec[:, 1].astype(np.float64)
    valid, fg = lab >= 0, lab > 0
    p, omp = sig64(x)
    dp = p * omp
    ref = np.stack([np.where(fg, p, 0.0), np.where(fg, 1.0, p), np.where(fg, dp, 0.0), np.where(fg, 0.0, dp)], 1) * valid[:, None]
    cmp_ = np.stack(composed_dice(rec), 1)
    assert np.array_equal(got[ref == 0], np.zeros((ref == 0).sum(), F32))        # ignored rows, min(p, 0), the inactive derivative
    S = np.stack([p + lab, p + lab, p + p * p, p + p * p], 1)
    live = ref != 0
    _check("Dice lo / hi", got[:, :2][live[:, :2]], ref[:, :2][live[:, :2]], cmp_[:, :2][live[:, :2]], S[:, :2][live[:, :2]])
    _check("Dice d lo / d hi", got[:, 2:][live[:, 2:]], ref[:, 2:][live[:, 2:]], cmp_[:, 2:][live[:, 2:]], S[:, 2:][live[:, 2:]])


def test_dice_gradient_against_float64(host):
    # (A, B): the usual case, the clamp active (B < 1: the denominator is 1 and the [B >= 1] term is off), B exactly 1, no foreground
    sums = ((37.25, 412.5), (0.125, 0.75), (0.5, 1.0), (0.0, 55.0))
    xs = grid()[::5]
    rec = np.array([[x, lab, A, B, k] for x in xs for lab in (-1.0, 0.0, 1.0) for A, B in sums for k in (1.0, -0.37, 2.0)], F32)
    got = host("dicegrad", rec)[:, 0]
    x, lab, A, B, k = (rec[:, j].astype(np.float64) for j in range(5))
    p, omp = sig64(x)
    Bc = np.maximum(B, 1.0)
    coef = np.where(lab > 0, -k / Bc, np.where(B >= 1, k * A / (Bc * Bc), 0.0)) * (lab >= 0)
    ref = coef * p * omp
    assert np.array_equal(got[ref == 0], np.zeros((ref == 0).sum(), F32)) and (ref == 0).sum() > len(rec) // 3
    live = ref != 0
    _check("Dice d/dx", got[live], ref[live], composed_dice_grad(rec)[live], (np.abs(coef) * (p + p * p))[live])


def test_saturated_logits_equal_the_composed_float32_code(host):
    xs = np.array([20, -20, 90, -90, 200, -200], F32)
    rec = records(xs, FG_WEIGHTS)
    got = host("bce", rec)
    cmp_v, cmp_d = composed_bce(rec)
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, 0], cmp_v), np.stack([rec[:, 0], rec[:, 1], got[:, 0], cmp_v], 1)
    assert np.array_equal(got[:, 1], cmp_d), np.stack([rec[:, 0], rec[:, 1], got[:, 1], cmp_d], 1)
    big = np.abs(rec[:, 0]) >= 90                                       # p is exactly 0 or 1: the clamp at 100, a zero derivative
    wrong = big & (rec[:, 1] >= 0) & ((rec[:, 0] > 0) != (rec[:, 1] > 0))
    w = np.where(rec[:, 1] > 0, rec[:, 2], 1.0)
    assert wrong.sum() == 8 and np.array_equal(got[wrong, 0], (100 * w[wrong]).astype(F32)) and not got[big, 1].any()
    rec = records(xs)
    got = host("dice", rec)
    for k, c in enumerate(composed_dice(rec)):
        assert np.array_equal(got[:, k], c), (k, np.stack([rec[:, 0], rec[:, 1], got[:, k], c], 1))
    assert not got[np.abs(rec[:, 0]) >= 90][:, 2:].any()
    rec = np.array([[x, lab, 37.25, 412.5, -0.37] for x in xs for lab in (-1.0, 0.0, 1.0)], F32)
    assert np.array_equal(host("dicegrad", rec)[:, 0], composed_dice_grad(rec))


class _Focal(tf.RPNLossConfig):
    pass


class _Dice(tf.RPNLossConfig):
    LOSS_CLS = "DiceLoss"


class _Bce(tf.RPNLossConfig):
    LOSS_CLS = "BinaryCrossEntropy"


def test_routing_decision_for_levels_and_kinds():
    kind = tf._fused_rpn_loss_kind
    focal = tf.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0)
    for level in (1, 2):
        assert kind(_Focal, None, level) == 0 and kind(_Focal, focal, level) == 0
        assert kind(_Focal, tf.SigmoidFocalClassificationLoss(alpha=0.5, gamma=2.0), level) is None
        assert kind(_Focal, tf.DiceLoss(), level) is None
    # level 1 keeps its domain: the other two kinds run the composed code
    assert kind(_Dice, None, 1) is None and kind(_Dice, tf.DiceLoss(ignore_target=-1), 1) is None and kind(_Bce, None, 1) is None
    assert kind(_Dice, None) is None and kind(_Bce, None) is None       # the default level is 1
    # level 2: the stock DiceLoss only
    assert kind(_Dice, None, 2) == 1 and kind(_Dice, tf.DiceLoss(ignore_target=-1), 2) == 1

    class MyDice(tf.DiceLoss):
        pass
    assert kind(_Dice, MyDice(ignore_target=-1), 2) is None
    assert kind(_Dice, tf.DiceLoss(ignore_target=0), 2) is None
    assert kind(_Dice, focal, 2) is None
    # level 2: BinaryCrossEntropy never looks at cls_loss_func, as the composed branch; FG_WEIGHT must be finite
    assert kind(_Bce, None, 2) == 2 and kind(_Bce, focal, 2) == 2 and kind(_Bce, MyDice(), 2) == 2

    class BadWeight(_Bce):
        FG_WEIGHT = float("inf")

    class NanWeight(_Bce):
        FG_WEIGHT = float("nan")

    class Other(tf.RPNLossConfig):
        LOSS_CLS = "SomethingElse"
    assert kind(BadWeight, None, 2) is None and kind(NanWeight, None, 2) is None and kind(Other, None, 2) is None


def test_switch_levels_and_cpu_tensors_stay_composed(monkeypatch):
    lvl = tf._fused_level
    assert [lvl(v) for v in (False, True, 0, 1, 2, 3, "0", "1", "2", "yes")] == [0, 1, 0, 1, 2, 2, 0, 1, 2, 1]
    assert bool(tf.FUSED_RPN_LOSS) == (os.environ.get("PRCNN_FUSED_RPN_LOSS", "0") != "0")       # the truthiness it always had
    # CPU tensors are outside the domain at every level: _fused_rpn_loss_ok says no, and get_rpn_loss(fused=2) is the composed code
    g = torch.Generator().manual_seed(3)
    cls, reg = torch.randn(1, 50, 1, generator=g), torch.randn(1, 50, 76, generator=g)
    lab = torch.randint(-1, 2, (1, 50), generator=g)
    reg_lab = torch.rand(1, 50, 7, generator=g)
    for cfg in (_Focal, _Dice, _Bce):
        for level in (1, 2):
            assert not tf._fused_rpn_loss_ok(cls, reg, lab, reg_lab, cfg, None, level)
        assert torch.equal(tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=2), tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=False))

    # with the device test stubbed out, the decision is the kind's: the tensors' dtypes and the channel count hold here
    class OnDevice(torch.Tensor):
        is_cuda = True
    dev = [t.as_subclass(OnDevice) for t in (cls, reg, lab, reg_lab)]
    ok = lambda cfg, f, level: tf._fused_rpn_loss_ok(*dev, cfg, f, level)      # noqa: E731
    assert ok(_Focal, None, 1) and ok(_Focal, None, 2)
    assert not ok(_Dice, None, 1) and ok(_Dice, None, 2) and not ok(_Dice, tf.DiceLoss(ignore_target=0), 2)
    assert not ok(_Bce, None, 1) and ok(_Bce, None, 2)
    assert not tf._fused_rpn_loss_ok(dev[0], dev[1], dev[2].float().as_subclass(OnDevice), dev[3], _Dice, None, 2)
