"""GPU: the fused RCNN loss (csrc/rcnn_loss.hip through train_functions.get_rcnn_loss(fused=True)) against get_rcnn_loss as it stands,
run on the CPU with float64 inputs (the function is dtype-agnostic and pinned to the reference's loss by train_rcnn_ref.npz).

Inputs are seeded on the CPU, logits randn * 2.  Every label is redrawn (float64) until it is >= 1e-5 away from an x/y/z bin edge,
an angle bin edge, the pi/2 and 3pi/2 flip boundaries and both clamp ends of the offsets and of the angle shift, so no row is left
out of a comparison (the edges themselves: tests/test_rcnn_loss_math_cpu.py).  reg_valid_mask is drawn independently of cls_label.

Error measures: the loss and each named term relative to the term; a gradient entry as |err| / S, S the sum of the absolute values
of the addends that form the entry with every product expanded (the normalisation of tests/test_gpu_train_stack_f64.py):
  d/d logit:    BCE k w (p + t); focal as tests/test_gpu_rpn_loss.py
  bin logits:   k_r (softmax_j + onehot_j);   picked residual / y / size column: k_r (|pred| + the addends of the target) inside the
  quadratic zone, k_r outside it;  every other entry has S = 0 and must be exactly 0.
The bar is not fixed in advance: the composed float32 path on the CPU is measured against the float64 reference on the shape cases
below (the four configurations), and the bar is 8 x its worst figure.  Measured (worst over those cases; composed float32 on the
CPU / the device):
  loss and terms  2.35e-6 / 2.35e-6   (bar 1.9e-5)
  gradients       9.0e-7 / 6.3e-7     (bar 7.2e-6)
The term figure is the y-bin configuration at R = 1 (a single regressed row: one small smooth-L1 term, relative to itself, formed
from float32 label constants both routes share); the composed gradient figure is the focal configuration at R = 1000.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from pointrcnn_amd import train_functions as tf
from pointrcnn_amd.rcnn import RCNNConfig
from rcnn_loss_cases import (CFGS, CHANNELS, COUNT_KEYS, F64, MEAN, SHAPES, Bce46, Case, Focal46, Stub, case, composed, fused, reference,
                             ret_dict, scales)

pytestmark = pytest.mark.gpu


def errors(c, name, got, ref, go=1.0, peer=None):
    """(worst relative error of the loss and its named terms, worst |err| / S of a gradient entry); entries with S = 0 or a zero term
    must be exact, the key sets and the counts equal"""
    tb, dcls, dreg = got[0], np.asarray(got[1], np.float64), np.asarray(got[2], np.float64)
    assert set(tb) == set(ref[0]), set(tb) ^ set(ref[0])
    e_t = 0.0
    for key, want in ref[0].items():
        if key in COUNT_KEYS:
            assert tb[key] == want and isinstance(tb[key], (int, float)), (key, tb[key], want)
        elif want == 0:
            assert tb[key] == 0, (key, tb[key])
        else:
            e_t = max(e_t, abs(float(tb[key]) - want) / abs(want))
    e_g = 0.0
    for g, r, S in zip((dcls, dreg), ref[1:], scales(c, name, go, peer)):
        assert np.isfinite(g).all()
        assert np.array_equal(g[S == 0], np.zeros((S == 0).sum())) and not r[S == 0].any()
        if (S > 0).any():
            e_g = max(e_g, float((np.abs(g - r)[S > 0] / S[S > 0]).max()))
    return e_t, e_g


@functools.lru_cache(maxsize=None)
def bars():
    """8 x the composed float32 CPU path's worst figures on the shape cases"""
    e_t = e_g = 0.0
    for name in CFGS:
        for n in SHAPES:
            c = case(n, CHANNELS[name])
            t, g = errors(c, name, composed(c, name, torch.float32), reference(c, name))
            e_t, e_g = max(e_t, t), max(e_g, g)
    print("composed float32 on the CPU against float64: terms %.3g, gradients %.3g" % (e_t, e_g))
    return 8 * e_t, 8 * e_g


def check(c, name, got, what, go=1.0, peer=None):
    e_t, e_g = errors(c, name, got, reference(c, name, peer, go), go, peer)
    bt, bg = bars()
    print("%s %s: device terms %.3g (bar %.3g), gradients %.3g (bar %.3g)" % (name, what, e_t, bt, e_g, bg))
    assert e_t <= bt and e_g <= bg, (what, e_t, bt, e_g, bg)


NAMES = sorted(CFGS)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("R", SHAPES)
def test_loss_terms_and_gradients_against_float64(dev, name, R):
    c = case(R, CHANNELS[name])
    check(c, name, fused(c, name, dev), "R %d" % R)


def golden_cases():
    from util import GOLDEN
    sys.path.insert(0, GOLDEN)
    import ref_net
    from make_golden import crc
    from make_rcnn_train_golden import CASES
    g = np.load(os.path.join(GOLDEN, "train_rcnn_ref.npz"))
    for name in sorted(CASES):
        seed, loss_cls, nfg = CASES[name]
        arrays = ref_net.rcnn_loss_case(seed, nfg=nfg, nign=16 if nfg else 0)
        assert crc(*arrays) == g[name + "_crc"], "seeded inputs changed"
        yield name, loss_cls, arrays, g


def test_reference_fixture_loss_gradients_and_tensorboard_values(dev):
    """the seeded cases of tests/golden/train_rcnn_ref.npz (bce, focal, nofg; R = 128): the fused route against the REFERENCE'S OWN
    loss, gradients (to the bar above) and tensorboard values (1e-5 max(1, |v|), as tests/test_train_rcnn_functions.py)"""
    seen = []
    for name, loss_cls, a, g in golden_cases():
        cfg = "focal" if loss_cls == "SigmoidFocalLoss" else "bce"
        c = Case.__new__(Case)
        c.R, c.C = a[1].shape
        c.cls, c.reg, c.lab, c.mask, c.roi, c.gt = (torch.from_numpy(x) for x in a)
        tb, dcls, dreg, loss = fused(c, cfg, dev)
        want = float(g[name + "_loss"])
        bt, bg = bars()
        assert abs(float(loss) - want) <= bt * abs(want), (name, float(loss), want)
        S_cls, S_reg = scales(c, cfg)
        for got, ref, S in ((dcls.numpy(), g[name + "_gcls"], S_cls), (dreg.numpy(), g[name + "_greg"], S_reg)):
            ref = ref.reshape(got.shape).astype(np.float64)
            assert not got[S == 0].any() and not ref[S == 0].any(), name
            e = float((np.abs(got - ref)[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0
            print("%s: gradient |err| / S against the reference's %.3g (bar %.3g)" % (name, e, bg))
            assert e <= bg, (name, e, bg)
        ref_tb = dict(zip(g[name + "_tb_keys"].tolist(), g[name + "_tb_vals"].tolist()))
        assert set(ref_tb) == set(tb), (name, set(ref_tb) ^ set(tb))
        for k, v in ref_tb.items():
            assert abs(float(tb[k]) - v) <= 1e-5 * max(1.0, abs(v)), (name, k, tb[k], v)
        seen.append(name)
    assert seen == ["bce", "focal", "nofg"]


@pytest.mark.parametrize("name", NAMES)
def test_label_patterns(dev, name):
    base = case(300, CHANNELS[name])
    lab, mask = base.lab, base.mask
    ign = base.copy(lab=-torch.ones_like(lab), mask=torch.zeros_like(mask))
    got = fused(ign, name, dev)
    check(ign, name, got, "all ignored, nothing regressed")
    assert got[3] == 0 and not got[1].any() and not got[2].any() and got[0]["rcnn_loss"] == 0
    none = base.copy(mask=torch.zeros_like(mask))
    got = fused(none, name, dev)
    check(none, name, got, "no valid regression row")
    assert all(got[0][k] == 0 for k in ("rcnn_loss_reg", "rcnn_loss_loc", "rcnn_loss_angle", "rcnn_loss_size")) and got[0]["rcnn_reg_fg"] == 0
    assert not got[2].any() and got[1].abs().max() > 0 and "loss_x_bin" not in got[0]
    full = base.copy(lab=torch.ones_like(lab), mask=torch.ones_like(mask))
    check(full, name, fused(full, name, dev), "all foreground")
    cross = base.copy(mask=(lab <= 0).long())                  # regressed exactly where the classifier ignores or rejects
    got = fused(cross, name, dev)
    check(cross, name, got, "mask on the rows with label -1 or 0")
    assert got[2][lab == -1].abs().max() > 0 and not got[1][lab == -1].any()
    last_lab, last_mask = torch.where(lab > 0, 0, lab), torch.zeros_like(mask)
    last_lab[-1] = last_mask[-1] = 1
    last = base.copy(lab=last_lab, mask=last_mask)
    check(last, name, fused(last, name, dev), "a single foreground row, the last")


@pytest.mark.parametrize("name", NAMES)
def test_non_finite_values_in_unselected_rows_cannot_leak(dev, name):
    C = CHANNELS[name]
    c = case(257, C)
    clean = fused(c, name, dev)
    reg, cls = c.reg.clone(), c.cls.clone()
    rows = torch.nonzero(c.mask <= 0).view(-1)
    ign = torch.nonzero(c.lab < 0).view(-1)
    assert len(rows) > 30 and len(ign) > 10
    bad = (float("nan"), float("inf"), float("-inf"))
    for i, r in enumerate(rows.tolist()):
        reg[r, (7 * i) % C] = bad[i % 3]
    for i, r in enumerate(ign.tolist()):
        cls[r, 0] = bad[i % 3]
    got = fused(c.copy(reg=reg, cls=cls), name, dev)
    assert math.isfinite(got[0]["rcnn_loss"]) and got[0] == clean[0] and torch.equal(got[3], clean[3])
    assert torch.equal(got[1], clean[1]) and torch.equal(got[2], clean[2])
    assert not got[2][rows].any() and not got[1][ign].any()


@pytest.mark.parametrize("name", NAMES)
def test_saturated_cls_logits(dev, name):
    c = case(257, CHANNELS[name])
    sign = torch.where(torch.arange(257) % 2 == 0, 1.0, -1.0).view(-1, 1)
    check(c.copy(cls=20.0 * sign), name, fused(c.copy(cls=20.0 * sign), name, dev), "cls logits at +-20")
    tb, dcls, dreg, loss = fused(c.copy(cls=90.0 * sign), name, dev)
    assert math.isfinite(float(loss)) and all(math.isfinite(v) for v in tb.values())
    assert torch.isfinite(dcls).all() and torch.isfinite(dreg).all()
    valid = (c.lab >= 0).double()
    n = float(((c.lab > 0) if CFGS[name].LOSS_CLS == "SigmoidFocalLoss" else (c.lab >= 0)).sum())
    weight = (valid / max(n, 1.0)).view(-1, 1)                 # a row's weight in the classification term
    assert (dcls.double().abs() <= weight * (1 + 1e-6)).all()


@pytest.mark.parametrize("name", NAMES)
def test_strided_views_and_int32_labels(dev, name):
    C = CHANNELS[name]
    c = case(257, C)
    want = fused(c, name, dev)
    wide_reg = torch.full((257, C + 5), float("nan"), device=dev)
    wide_cls = torch.full((257, 3), float("nan"), device=dev)
    wide_reg[:, 2:C + 2] = c.reg.to(dev)
    wide_cls[:, 1:2] = c.cls.to(dev)
    ret = ret_dict(c, torch.float32, dev, int32=True)
    ret["rcnn_reg"], ret["rcnn_cls"] = wide_reg[:, 2:C + 2].requires_grad_(True), wide_cls[:, 1:2].requires_grad_(True)
    assert ret["rcnn_reg"].stride(0) == C + 5 and ret["rcnn_cls"].stride(0) == 3 and ret["cls_label"].dtype == torch.int32
    assert tf._fused_rcnn_loss_ok(ret, CFGS[name], None)
    tb = {}
    loss = tf.get_rcnn_loss(ret, CFGS[name], tb_dict=tb, fused=True)
    dcls, dreg = torch.autograd.grad(loss, (ret["rcnn_cls"], ret["rcnn_reg"]))
    assert dcls.is_contiguous() and dreg.is_contiguous() and dreg.shape == (257, C)
    assert tb == want[0] and torch.equal(dcls.cpu(), want[1]) and torch.equal(dreg.cpu(), want[2])


@pytest.mark.parametrize("name", NAMES)
def test_result_does_not_depend_on_how_the_batch_factors_R(dev, name):
    """the labels and the mask as (R) or (B, R/B), gt_of_rois as (R,7) or (B, R/B, 7) -- what the composed code flattens: the flat row
    order alone counts.  roi_boxes3d stays (R,7): the composed code indexes its columns, and a 3-D one is outside the fused domain"""
    c = case(1000, CHANNELS[name])
    base = fused(c, name, dev)
    for B in (2, 4):
        ret = ret_dict(c, torch.float32, dev)
        ret.update(cls_label=ret["cls_label"].view(B, -1), reg_valid_mask=ret["reg_valid_mask"].view(B, -1),
                   gt_of_rois=ret["gt_of_rois"].view(B, -1, 7))
        assert tf._fused_rcnn_loss_ok(ret, CFGS[name], None)
        assert not tf._fused_rcnn_loss_ok(dict(ret, roi_boxes3d=ret["roi_boxes3d"].view(B, -1, 7)), CFGS[name], None)
        tb = {}
        loss = tf.get_rcnn_loss(ret, CFGS[name], tb_dict=tb, fused=True)
        loss.backward()
        assert tb == base[0] and torch.equal(loss.detach().cpu(), base[3])
        assert torch.equal(ret["rcnn_cls"].grad.cpu(), base[1]) and torch.equal(ret["rcnn_reg"].grad.cpu(), base[2])


@pytest.mark.parametrize("name", NAMES)
def test_upstream_gradient_without_a_host_sync(dev, name):
    c = case(257, CHANNELS[name])
    base = fused(c, name, dev)
    ret = ret_dict(c, torch.float32, dev)
    cls, reg = ret["rcnn_cls"], ret["rcnn_reg"]
    tf.get_rcnn_loss(ret, CFGS[name], fused=True)              # constants are uploaded once, outside the guarded region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = tf.get_rcnn_loss(ret, CFGS[name], tb_dict=None, fused=True)
        (loss * 0.37).backward()
        g1 = (cls.grad.clone(), reg.grad.clone())
        cls.grad = reg.grad = None
        loss = tf.get_rcnn_loss(ret, CFGS[name], tb_dict=None, fused=True)
        (loss.sum() + (cls * 0.01).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(c, name, (base[0], g1[0].cpu(), g1[1].cpu()), "grad_output 0.37", go=0.37)
    assert torch.equal(reg.grad.cpu(), base[2])
    assert (cls.grad.cpu() - (base[1] + 0.01)).abs().max() <= 1e-7


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_give_identical_bytes(dev, name):
    c = case(1000, CHANNELS[name])
    a, b = fused(c, name, dev), fused(c, name, dev)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("name", ["bce", "focal"])
@pytest.mark.parametrize("R", [257, 129])
def test_global_normalisation_through_a_dist_stub(dev, name, R):
    c = case(R, CHANNELS[name])
    check(c, name, fused(c, name, dev, dist=Stub(37)), "dist stub, the peer counts 37", peer=37)
    none = c.copy(mask=torch.zeros_like(c.mask))
    got = fused(none, name, dev, dist=Stub(37))
    check(none, name, got, "dist stub, no local regression row", peer=37)
    assert not got[2].any() and got[0]["rcnn_loss_reg"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_tb_dict_entries_from_one_read(dev, name, monkeypatch):
    c = case(257, CHANNELS[name])
    got = fused(c, name, dev)
    ref = reference(c, name)
    assert set(got[0]) == set(ref[0]) and len(got[0]) == {"bce": 19, "focal": 21, "ybin": 20, "roi": 19}[name]
    assert got[0]["rcnn_reg_fg"] == int(c.mask.sum()) and got[0]["rcnn_cls_fg"] == int((c.lab > 0).sum())
    assert all(isinstance(got[0][k], int) for k in COUNT_KEYS)
    check(c, name, got, "tb_dict")
    ret = ret_dict(c, torch.float32, dev)
    reads = []
    for fn in ("item", "tolist", "cpu"):
        orig = getattr(torch.Tensor, fn)
        monkeypatch.setattr(torch.Tensor, fn, lambda self, *a, _o=orig, _n=fn, **k: (reads.append(_n), _o(self, *a, **k))[1])
    tf.get_rcnn_loss(ret, CFGS[name], tb_dict={}, fused=True)
    assert reads == ["tolist"], reads


def test_outside_the_domain_the_composed_code_runs(dev, monkeypatch):
    from pointrcnn_amd import ops

    def boom(*a, **k):
        raise AssertionError("the fused RCNN loss ran outside its domain")
    for fn in ("rcnn_loss_forward", "rcnn_loss_finalize", "rcnn_loss_backward"):
        monkeypatch.setattr(ops, fn, boom)
    c = case(257, 46)

    class Mine(tf.SigmoidFocalClassificationLoss):
        def forward(self, prediction_tensor, target_tensor, weights):
            return 2 * super().forward(prediction_tensor, target_tensor, weights)

    class Wide(RCNNConfig):                                     # nb = 12: C = 70 channels, beyond the kernel's rows
        LOC_SCOPE = 3.0
    wide = Case(64, 70, 5)
    runs = [(ret_dict(c, F64, dev), Bce46, None), (ret_dict(c, torch.float32, dev), Focal46, Mine(alpha=0.25, gamma=2.0)),
            (ret_dict(wide, torch.float32, dev), Wide, None), (ret_dict(c, torch.float32), Bce46, None)]
    for ret, cfg, func in runs:
        assert not tf._fused_rcnn_loss_ok(ret, cfg, func)
        a = tf.get_rcnn_loss(ret, cfg, cls_loss_func=func, fused=True)
        b = tf.get_rcnn_loss(ret, cfg, cls_loss_func=func, fused=False)
        assert torch.equal(a, b) and a.dtype == ret["rcnn_reg"].dtype and a.device == ret["rcnn_reg"].device
    with pytest.raises(AssertionError, match="outside its domain"):
        tf.get_rcnn_loss(ret_dict(c, torch.float32, dev), Bce46, fused=True)


def test_kernel_refuses_what_it_has_no_code_for(dev):
    from pointrcnn_amd import _cabi, ops
    c = Case(64, 70, 5)

    class Wide(RCNNConfig):
        LOC_SCOPE = 3.0
    ret = ret_dict(c, torch.float32, dev)
    args = [ret[k].detach() for k in ("rcnn_cls", "rcnn_reg", "cls_label", "reg_valid_mask", "roi_boxes3d", "gt_of_rois")]
    with pytest.raises(_cabi.PointOpsError, match=r"code -3.*70 channels"):
        ops.rcnn_loss_forward(*args, ops.rcnn_loss_cfg(Wide, MEAN))
    c = case(64, 46)
    ret = ret_dict(c, torch.float32, dev)
    args = [ret[k].detach() for k in ("rcnn_cls", "rcnn_reg", "cls_label", "reg_valid_mask", "roi_boxes3d", "gt_of_rois")]

    class Dice(RCNNConfig):
        LOSS_CLS = "DiceLoss"
    with pytest.raises(_cabi.PointOpsError, match=r"code -3.*loss_cls"):
        ops.rcnn_loss_forward(*args, ops.rcnn_loss_cfg(Dice, MEAN))


def test_default_route_does_not_reach_the_new_ops(dev, monkeypatch):
    from pointrcnn_amd import ops

    def boom(*a, **k):
        raise AssertionError("the fused RCNN loss ran without being asked for")
    for fn in ("rcnn_loss_forward", "rcnn_loss_finalize", "rcnn_loss_backward"):
        assert callable(getattr(ops, fn))
        monkeypatch.setattr(ops, fn, boom)
    monkeypatch.setattr(tf, "FUSED_RCNN_LOSS", False)                   # the switch unset
    ret = ret_dict(case(257, 46), torch.float32, dev)
    tf.get_rcnn_loss(ret, Bce46, fused=None).backward()
    assert ret["rcnn_cls"].grad is not None
    with pytest.raises(AssertionError, match="without being asked"):
        tf.get_rcnn_loss(ret, Bce46, fused=True)


def test_whole_training_step_fused_against_composed(dev, monkeypatch):
    """one RCNNTrainer step's loss and parameter gradients with fused_loss=True against False from the same weights, RoI sample and
    augmentation draws (the batch of tests/test_gpu_train_rcnn.py, B = 2): the loss to the bar above, every rcnn_net parameter
    gradient in norm to the 5e-3 that test gives fused vs composed"""
    from test_gpu_train_rcnn import _pm, _rcnn_batch
    _pm()
    from pointrcnn_amd import ops, point_rcnn, rpn
    torch.manual_seed(11)
    model = point_rcnn.PointRCNN(mode="TRAIN").to(dev)
    rpn.randomize_bn_stats(model.rpn, seed=3)
    batch = _rcnn_batch(dev)
    out, calls = {}, []
    forward = ops.rcnn_loss_forward
    monkeypatch.setattr(ops, "rcnn_loss_forward", lambda *a, **k: (calls.append(a[1].shape), forward(*a, **k))[1])
    for fused_loss in (True, False):
        trainer = tf.RCNNTrainer(model, fused_loss=fused_loss)
        assert trainer.fused_loss is fused_loss
        trainer.model.train()
        model.zero_grad(set_to_none=True)
        model.rcnn_net.proposal_target_layer.seed = 21
        torch.manual_seed(77)
        loss = trainer.loss(batch)
        loss.backward()
        out[fused_loss] = (float(loss.item()), {n: p.grad.double().clone() for n, p in model.rcnn_net.named_parameters()})
    (lf, gf), (lc, gc) = out[True], out[False]
    assert calls == [(2 * 64, 46)], calls                      # the fused route ran, once, in the fused step only
    assert abs(lf - lc) <= bars()[0] * abs(lc), (lf, lc)
    assert sorted(gf) == sorted(gc) and len(gc) > 10
    rel = {n: float((gf[n] - gc[n]).norm() / gc[n].norm().clamp(min=1e-12)) for n in gc}
    assert max(rel.values()) <= 5e-3, max(rel.items(), key=lambda kv: kv[1])
