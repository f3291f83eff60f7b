"""GPU: the fused RPN loss for LOSS_CLS = DiceLoss and BinaryCrossEntropy (csrc/rpn_loss.hip through
train_functions.get_rpn_loss(fused=2), the second level of the switch) against get_rpn_loss as it stands, run on the CPU with float64
inputs.  Inputs, cases and the regression measure are those of tests/test_gpu_rpn_loss.py (Case, scales, SHAPES).

Error measures: each named term relative to the term, except that the Dice loss 1 - A / Bc is a difference and is taken relative to
1 + A / Bc (and the total loss under Dice relative to that plus the regression loss); a d cls entry relative to the magnitude of the
entry itself -- it is a single product -- and an entry whose closed form is 0 (an ignored row; under Dice a background row while
A = 0 or B < 1) must be exactly 0; a d reg entry as |err| / S with the S of tests/test_gpu_rpn_loss.py.
The bar is not fixed in advance: per kind, the composed float32 path on the CPU is measured against the float64 reference on the
shape cases below (both channel counts, upstream gradient 1), and the bar is 8 x its worst figure.  Measured (worst over those cases
and both upstream gradients; composed float32 on the CPU / the device):
  dice  loss and terms  1.35e-7 / 2.2e-7  (bar 1.08e-6)    gradients  2.88e-5 / 2.88e-5  (bar 2.31e-4)
  bce   loss and terms  1.93e-7 / 2.2e-7  (bar 1.55e-6)    gradients  1.99e-5 / 1.99e-5  (bar 1.59e-4)
Both gradient figures are the float32 conditioning of 1 - p for a confident row -- p - 1 under BCE, (1 - p) p under Dice: the
error of p relative to 1 - p, about e^x 2^-24 at logit x -- which the device route shares with the composed one, down to the same
worst row.
Where float32 sigmoid saturates (logits of +-90) the float32 CPU route is the reference for the loss terms and for those rows' own
d cls entries: the composed float64 code does not clamp there.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from util import GOLDEN

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from pointrcnn_amd import train_functions as tf  # noqa: E402
from test_gpu_rpn_loss import SHAPES, Stub, case, relabel, scales  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
KINDS = {"dice": "DiceLoss", "bce": "BinaryCrossEntropy", "focal": "SigmoidFocalLoss"}
TERM_KEYS = ("rpn_loss", "rpn_loss_cls", "rpn_loss_reg", "rpn_loss_loc", "rpn_loss_angle", "rpn_loss_size")
NEW_OPS = ("rpn_loss_cls_sums", "rpn_loss_forward_kind", "rpn_loss_backward_kind")


@functools.lru_cache(maxsize=None)
def cfg_of(kind, C, fg_weight=15):
    return type("Cfg_%s_%d" % (kind, C), (tf.RPNLossConfig,), {"LOSS_CLS": KINDS[kind], "LOC_XZ_FINE": C == 76, "FG_WEIGHT": fg_weight})


def composed(c, cfg, dtype, dist=None, go=1.0):
    """get_rpn_loss as it stands, on the CPU in `dtype` -> terms dict, d cls, d reg (numpy float64)"""
    cls = c.cls.to(dtype).clone().requires_grad_(True)
    reg = c.reg.to(dtype).clone().requires_grad_(True)
    tb = {}
    loss = tf.get_rpn_loss(cls, reg, c.lab, c.reg_lab.to(dtype), cfg, tb_dict=tb, dist=dist, fused=False)
    (loss * go).backward()
    zero = lambda t, like: np.zeros(like.shape) if t is None else t.double().numpy()      # noqa: E731
    return tb, zero(cls.grad, cls), zero(reg.grad, reg)


@functools.lru_cache(maxsize=None)
def reference(c, cfg, peer=None, go=1.0):
    return composed(c, cfg, F64, None if peer is None else Stub(peer), go)


def fused(c, cfg, dev, dist=None, go=1.0, tb=True, int32=False, level=2):
    cls = c.cls.to(dev).requires_grad_(True)
    reg = c.reg.to(dev).requires_grad_(True)
    lab = c.lab.to(dev)
    tbd = {} if tb else None
    loss = tf.get_rpn_loss(cls, reg, lab.int() if int32 else lab, c.reg_lab.to(dev), cfg, tb_dict=tbd, dist=dist, fused=level)
    (loss * go).backward()
    assert cls.grad is not None and reg.grad is not None                        # rpn_reg stays in the graph, foreground or not
    assert cls.grad.is_contiguous() and reg.grad.is_contiguous() and cls.grad.shape == cls.shape and reg.grad.shape == reg.shape
    return tbd, cls.grad.cpu(), reg.grad.cpu(), loss.detach().cpu()


def errors(c, cfg, got, ref, go=1.0, peer=None, cls_rows=None):
    """(worst error of the loss and its named terms, worst error of a gradient entry), measures as in the module docstring;
    cls_rows: the rows whose d cls entries are compared (default: all)"""
    tb, dcls, dreg = got[0], np.asarray(got[1], np.float64), np.asarray(got[2], np.float64)
    rt = ref[0]
    assert set(tb) == set(TERM_KEYS) | {"rpn_fg_sum"} == set(rt), (sorted(tb), sorted(rt))      # the composed branch's keys for the kind
    assert tb["rpn_fg_sum"] == rt["rpn_fg_sum"] and isinstance(tb["rpn_fg_sum"], int)
    dice = cfg.LOSS_CLS == "DiceLoss"
    e_t = 0.0
    for key in TERM_KEYS:
        den = abs(rt[key])
        if dice and key == "rpn_loss_cls":
            den = 2.0 - rt[key]                                                 # 1 + A / Bc
        elif dice and key == "rpn_loss":
            den = cfg.LOSS_WEIGHT[0] * (2.0 - rt["rpn_loss_cls"]) + cfg.LOSS_WEIGHT[1] * abs(rt["rpn_loss_reg"])
        assert math.isfinite(tb[key]), (key, tb[key])
        if den == 0:
            assert tb[key] == 0, (key, tb[key])
        else:
            e_t = max(e_t, abs(tb[key] - rt[key]) / den)
    assert np.isfinite(dcls).all() and np.isfinite(dreg).all()
    g, r = dcls.reshape(-1), ref[1].reshape(-1)
    if cls_rows is not None:
        g, r = g[cls_rows], r[cls_rows]
    assert np.array_equal(g[r == 0], np.zeros((r == 0).sum())), "a d cls entry whose closed form is 0"
    e_g = float((np.abs(g - r)[r != 0] / np.abs(r[r != 0])).max()) if (r != 0).any() else 0.0
    S = scales(c, go, peer)[1]
    assert np.array_equal(dreg[S == 0], np.zeros((S == 0).sum())) and not ref[2][S == 0].any()
    if (S > 0).any():
        e_g = max(e_g, float((np.abs(dreg - ref[2])[S > 0] / S[S > 0]).max()))
    return e_t, e_g


@functools.lru_cache(maxsize=None)
def bars(kind):
    """8 x the composed float32 CPU path's worst figures on the shape cases, for this kind"""
    e_t = e_g = 0.0
    for C in (76, 52):
        for n in SHAPES:
            c, cfg = case(n, C), cfg_of(kind, C)
            t, g = errors(c, cfg, composed(c, cfg, torch.float32), reference(c, cfg))
            e_t, e_g = max(e_t, t), max(e_g, g)
    print("%s: composed float32 on the CPU against float64: terms %.3g, gradients %.3g" % (kind, e_t, e_g))
    return 8 * e_t, 8 * e_g


def check(c, cfg, kind, got, what, go=1.0, peer=None, ref=None, cls_rows=None):
    e_t, e_g = errors(c, cfg, got, reference(c, cfg, peer, go) if ref is None else ref, go, peer, cls_rows)
    bt, bg = bars(kind)
    print("%s %s: device terms %.3g (bar %.3g), gradients %.3g (bar %.3g)" % (kind, what, e_t, bt, e_g, bg))
    assert e_t <= bt and e_g <= bg, (kind, what, e_t, bt, e_g, bg)


# ------------------------------------------------------------------------------------------------ precision
@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("npts", SHAPES)
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_loss_terms_and_gradients_against_float64(dev, kind, C, npts):
    c, cfg = case(npts, C), cfg_of(kind, C)
    for go in (1.0, 0.37):
        check(c, cfg, kind, fused(c, cfg, dev, go=go), "npts %d C %d upstream %g" % (npts, C, go), go=go)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_label_patterns(dev, kind, C):
    base, cfg = case(300, C), cfg_of(kind, C)
    lab = base.lab.view(-1)
    ign = relabel(base, -torch.ones_like(lab))                                  # no valid row: Dice is 1 - 0 / 1, BCE 0
    got = fused(ign, cfg, dev)
    check(ign, cfg, kind, got, "no valid row")
    assert got[0]["rpn_loss_cls"] == (1.0 if kind == "dice" else 0.0) and got[0]["rpn_fg_sum"] == 0
    assert not got[1].any() and not got[2].any()
    none = relabel(base, torch.where(lab > 0, 0, lab))                          # no foreground row
    got = fused(none, cfg, dev)
    check(none, cfg, kind, got, "no foreground")
    assert all(got[0][k] == 0 for k in ("rpn_loss_reg", "rpn_loss_loc", "rpn_loss_angle", "rpn_loss_size")) and got[0]["rpn_fg_sum"] == 0
    assert not got[2].any()
    if kind == "bce":
        assert got[1].abs().max() > 0
    else:
        assert not got[1].any()                                                 # A = 0: min(p, 0) has no derivative, and A / Bc^2 is 0
    every = relabel(base, torch.ones_like(lab))
    check(every, cfg, kind, fused(every, cfg, dev), "all foreground")
    tail = torch.where(lab > 0, 0, lab)
    tail[256:] = torch.where(torch.arange(44) % 3 == 0, 1, tail[256:])          # rows 256..299: the last, partial tile of 128
    check(relabel(base, tail), cfg, kind, fused(relabel(base, tail), cfg, dev), "foreground only in the last partial tile")


@pytest.mark.parametrize("C", [76, 52])
def test_dice_below_the_clamp(dev, C):
    """B < 1: one valid background row with logit -6 (B = sigmoid(-6)); the denominator is the constant 1 and the [B >= 1] term is
    off, so with A = 0 the loss is 1 and every derivative 0.  With one foreground row added (A = p_fg, B = 1 + p_bg >= 1) both are on."""
    base, cfg = case(129, C), cfg_of("dice", C)
    lab = -torch.ones_like(base.lab.view(-1))
    lab[70] = 0
    c = relabel(base, lab)
    c.cls = base.cls.clone()
    c.cls.view(-1)[70] = -6.0
    got = fused(c, cfg, dev)
    check(c, cfg, "dice", got, "one valid background row")
    assert got[0]["rpn_loss_cls"] == 1.0 and not got[1].any()
    lab2 = lab.clone()
    lab2[128] = 1
    d = relabel(c, lab2)
    got = fused(d, cfg, dev)
    check(d, cfg, "dice", got, "one background and one foreground row")
    assert got[1].view(-1)[70] != 0 and got[1].view(-1)[128] != 0 and int((got[1] != 0).sum()) == 2


@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("fg_weight", [1, 15])
def test_bce_foreground_weight(dev, C, fg_weight):
    cfg = cfg_of("bce", C, fg_weight)
    for npts in (129, 257):
        c = case(npts, C)
        check(c, cfg, "bce", fused(c, cfg, dev), "FG_WEIGHT %g npts %d" % (fg_weight, npts))
    a, b = fused(case(257, C), cfg_of("bce", C, 1), dev), fused(case(257, C), cfg_of("bce", C, 15), dev)
    assert a[0]["rpn_loss_cls"] < b[0]["rpn_loss_cls"] and torch.equal(a[2], b[2])


@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_strided_views_and_int32_labels(dev, kind, C):
    c, cfg = case(257, C), cfg_of(kind, C)
    want = fused(c, cfg, dev)
    got = fused(c, cfg, dev, int32=True)
    assert got[0] == want[0] and all(torch.equal(x, y) for x, y in zip(got[1:], want[1:]))
    wide_reg = torch.full((1, 257, 80), float("nan"), device=dev)
    wide_cls = torch.full((1, 257, 4), float("nan"), device=dev)
    wide_reg[:, :, :C] = c.reg.to(dev)
    wide_cls[:, :, 1:2] = c.cls.to(dev)
    reg, cls = wide_reg[:, :, :C].requires_grad_(True), wide_cls[:, :, 1:2].requires_grad_(True)
    assert reg.stride(1) == 80 and cls.stride(1) == 4
    tb = {}
    loss = tf.get_rpn_loss(cls, reg, c.lab.to(dev).int(), c.reg_lab.to(dev), cfg, tb_dict=tb, fused=2)
    dcls, dreg = torch.autograd.grad(loss, (cls, reg))
    assert dcls.is_contiguous() and dreg.is_contiguous() and dreg.shape == (1, 257, C)
    assert tb == want[0] and torch.equal(dcls.cpu(), want[1]) and torch.equal(dreg.cpu(), want[2])


@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_saturated_cls_logits(dev, kind, C):
    base, cfg = case(257, C), cfg_of(kind, C)
    c = base.view(1)
    c.cls = base.cls.clone()
    lab = c.lab.view(-1)
    rows = [int(r) for v in (1, 0, -1) for r in torch.nonzero(lab == v).view(-1)[[0, 1, -1]]]      # the last row of its kind included
    for i, r in enumerate(rows):                                                # both signs against both targets and the ignore label
        c.cls.view(-1)[r] = 90.0 if i % 2 == 0 else -90.0
    got = fused(c, cfg, dev)
    f32, f64 = composed(c, cfg, torch.float32), reference(c, cfg)
    assert all(math.isfinite(v) for v in got[0].values()) and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    sat = np.zeros(257, bool)
    sat[rows] = True
    # the loss terms against the float32 CPU route, the other rows' gradients against float64, both within the bar
    check(c, cfg, kind, got, "logits of +-90 in %d rows" % len(rows), ref=(f32[0], f64[1], f64[2]), cls_rows=~sat)
    assert np.array_equal(got[1].numpy().reshape(-1)[sat], f32[1].reshape(-1)[sat].astype(np.float32))      # zeros: (1 - p) p == 0
    assert not got[1].numpy().reshape(-1)[sat].any()


# ------------------------------------------------------------------------------------------------ data-parallel arithmetic
@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_global_normalisation_through_a_dist_stub(dev, kind, C):
    c, cfg = case(257, C), cfg_of(kind, C)
    for go in (1.0, 0.37):
        check(c, cfg, kind, fused(c, cfg, dev, dist=Stub(37), go=go), "dist stub, the peer adds 37, upstream %g" % go, go=go, peer=37)
    lab = c.lab.view(-1)
    none = relabel(c, torch.where(lab > 0, 0, lab))
    got = fused(none, cfg, dev, dist=Stub(37))
    check(none, cfg, kind, got, "dist stub, no local foreground", peer=37)
    assert not got[2].any() and got[0]["rpn_loss_reg"] == 0 and got[1].abs().max() > 0


# ------------------------------------------------------------------------------------------------ the reference's own loss
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_reference_fixture_loss(dev, kind):
    """the dice / bce cases of tests/golden/train_ref.npz are the reference's own get_rpn_loss (float32 on the CPU)"""
    import ref_net
    from make_golden import crc
    g = np.load(os.path.join(GOLDEN, "train_ref.npz"))
    arrays = ref_net.train_loss_case({"dice": 2, "bce": 3}[kind])
    assert crc(*arrays) == g[kind + "_crc"], "seeded inputs changed"
    cfg = cfg_of(kind, 76)
    cls, reg, lab, reg_lab = (torch.from_numpy(a).to(dev) for a in arrays)
    loss = float(tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=2).item())
    want = float(g[kind + "_loss"])
    tb = dict(zip(g[kind + "_tb_keys"].tolist(), g[kind + "_tb_vals"].tolist()))
    den = (2.0 - tb["rpn_loss_cls"]) + abs(tb["rpn_loss_reg"]) if kind == "dice" else abs(want)
    print("%s fixture: device %.9g, reference %.9g, error %.3g (bar %.3g)" % (kind, loss, want, abs(loss - want) / den, bars(kind)[0]))
    assert abs(loss - want) / den <= bars(kind)[0]


# ------------------------------------------------------------------------------------------------ routing
def _inputs(c, dev):
    return c.cls.to(dev).requires_grad_(True), c.reg.to(dev).requires_grad_(True), c.lab.to(dev), c.reg_lab.to(dev)


def _count_calls(monkeypatch, names):
    from pointrcnn_amd import ops
    calls = dict.fromkeys(names, 0)
    for name in names:
        orig = getattr(ops, name)

        def counted(*a, _o=orig, _n=name, **k):
            calls[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    return calls


def _forbid(monkeypatch, names):
    from pointrcnn_amd import ops

    def boom(*a, **k):
        raise AssertionError("the second level of the fused RPN loss ran without being asked for")
    for name in names:
        assert callable(getattr(ops, name))
        monkeypatch.setattr(ops, name, boom)


@pytest.mark.parametrize("kind", ["focal", "dice", "bce"])
def test_level_two_reaches_the_kind_exports(dev, kind, monkeypatch):
    calls = _count_calls(monkeypatch, NEW_OPS + ("rpn_loss_counts", "rpn_loss_forward", "rpn_loss_backward"))
    cls, reg, lab, reg_lab = _inputs(case(255, 76), dev)
    tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg_of(kind, 76), fused=2).backward()
    assert calls == {"rpn_loss_counts": 1, "rpn_loss_cls_sums": int(kind == "dice"), "rpn_loss_forward_kind": 1, "rpn_loss_backward_kind": 1,
                     "rpn_loss_forward": 0, "rpn_loss_backward": 0}, calls
    assert cls.grad is not None and reg.grad is not None


@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_level_one_keeps_its_domain(dev, kind, monkeypatch):
    _forbid(monkeypatch, NEW_OPS)
    cfg = cfg_of(kind, 76)
    cls, reg, lab, reg_lab = _inputs(case(255, 76), dev)
    want = tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=False)
    for level in (True, 1):
        loss = tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=level)
        assert torch.equal(loss, want)
        loss.backward()
    assert cls.grad is not None and reg.grad is not None
    with pytest.raises(AssertionError, match="without being asked"):
        tf.get_rpn_loss(*_inputs(case(255, 76), dev), cfg, fused=2)


@pytest.mark.parametrize("C", [76, 52])
def test_focal_is_the_same_under_both_levels(dev, C):
    from test_gpu_rpn_loss import CFGS
    c = case(1000, C)
    a, b = fused(c, CFGS[C], dev, tb=False, level=True), fused(c, CFGS[C], dev, tb=False, level=2)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    a, b = fused(c, CFGS[C], dev, dist=Stub(37), tb=False, level=True, go=0.37), fused(c, CFGS[C], dev, dist=Stub(37), tb=False, level=2, go=0.37)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    tb1, tb2 = {}, {}
    cls, reg, lab, reg_lab = _inputs(c, dev)
    tf.get_rpn_loss(cls, reg, lab, reg_lab, CFGS[C], tb_dict=tb1, fused=True)
    tf.get_rpn_loss(cls, reg, lab, reg_lab, CFGS[C], tb_dict=tb2, fused=2)
    assert tb1 == tb2 and "rpn_loss_cls_pos" in tb2


@pytest.mark.parametrize("kind", ["focal", "dice", "bce"])
def test_module_switch(dev, kind, monkeypatch):
    cfg = cfg_of(kind, 76)
    calls = _count_calls(monkeypatch, NEW_OPS)
    monkeypatch.setattr(tf, "FUSED_RPN_LOSS", 2)                                # PRCNN_FUSED_RPN_LOSS=2
    cls, reg, lab, reg_lab = _inputs(case(255, 76), dev)
    tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=None).backward()
    assert calls["rpn_loss_forward_kind"] == calls["rpn_loss_backward_kind"] == 1
    _forbid(monkeypatch, NEW_OPS)
    for unset in (0, False, 1):                                                 # the switch unset, or at its first level
        monkeypatch.setattr(tf, "FUSED_RPN_LOSS", unset)
        cls, reg, lab, reg_lab = _inputs(case(255, 76), dev)
        tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, fused=None).backward()
        assert cls.grad is not None


@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_host_reads(dev, kind, monkeypatch):
    """with tb_dict the only host read is one tolist of the term vector; without it nothing waits for the device"""
    c, cfg = case(257, 76), cfg_of(kind, 76)
    base = fused(c, cfg, dev)
    cls, reg, lab, reg_lab = _inputs(c, dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, tb_dict=None, fused=2)
        (loss * 0.37).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(c, cfg, kind, (base[0], cls.grad.cpu(), reg.grad.cpu()), "no host sync, upstream 0.37", go=0.37)
    reads = []
    for name in ("item", "tolist", "cpu"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n), _o(self, *a, **k))[1])
    tf.get_rpn_loss(cls, reg, lab, reg_lab, cfg, tb_dict={}, fused=2)
    assert reads == ["tolist"], reads


@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_two_calls_give_identical_bytes(dev, kind, C):
    c, cfg = case(1000, C), cfg_of(kind, C)
    a, b = fused(c, cfg, dev), fused(c, cfg, dev)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    for B in (2, 4):                                                            # nothing but the rows in flat order
        got = fused(c.view(B), cfg, dev)
        assert got[0] == a[0] and torch.equal(got[3], a[3])
        assert torch.equal(got[1].view(-1), a[1].view(-1)) and torch.equal(got[2].view(-1), a[2].view(-1))


# ------------------------------------------------------------------------------------------------ one whole step
@pytest.mark.parametrize("kind", ["dice", "bce"])
def test_whole_training_step_fused_against_composed(dev, kind):
    """one RPNTrainer step's loss and parameter gradients with fused_loss=2 against False from the same state, under DiceLoss and
    under BinaryCrossEntropy: the bars of tests/test_gpu_rpn_loss.py::test_whole_training_step_fused_against_composed, unchanged"""
    from test_gpu_rpn_loss import bars as focal_bars
    from test_gpu_round2 import T, _Wrap, _fill
    from make_golden import TRAIN_CASE, train_batch
    from pointrcnn_amd import rpn
    pts, gt, cls, reg = train_batch(TRAIN_CASE)
    model = rpn.RPN()
    _fill(_Wrap(model), TRAIN_CASE["wseed"])
    model = model.to(dev)
    batch = {"pts_input": T(pts, dev), "rpn_cls_label": T(cls, dev), "rpn_reg_label": T(reg, dev)}
    cfg = cfg_of(kind, 76)
    out = {}
    for fused_loss in (2, False):
        trainer = tf.RPNTrainer(model, cfg=cfg, ddp=False, fused_loss=fused_loss)
        assert trainer.fused_loss is fused_loss
        trainer.model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
        model.zero_grad(set_to_none=True)
        loss = trainer.loss(batch)
        loss.backward()
        out[fused_loss] = (float(loss.item()), {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None})
    (lf, gf), (lc, gc) = out[2], out[False]
    assert abs(lf - lc) <= focal_bars()[0] * abs(lc), (lf, lc)
    assert sorted(gf) == sorted(gc)
    rel = {n: float((gf[n] - gc[n]).norm() / gc[n].norm().clamp(min=1e-30)) for n in gc}
    heads = [n for n in rel if "rpn_cls_layer" in n or "rpn_reg_layer" in n]
    assert len(heads) == 10 and max(rel[n] for n in heads) <= 1e-4, [(n, rel[n]) for n in heads]
    assert max(rel.values()) <= 3e-2 and float(np.median(list(rel.values()))) <= 1e-3, max(rel.items(), key=lambda kv: kv[1])
