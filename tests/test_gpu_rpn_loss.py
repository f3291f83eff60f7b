"""GPU: the fused RPN loss (csrc/rpn_loss.hip through train_functions.get_rpn_loss(fused=True)) against get_rpn_loss as it stands,
run on the CPU with float64 inputs (the function is dtype-agnostic and pinned to the reference's loss by train_ref.npz).

Inputs are seeded on the CPU; every angle label is redrawn until |shift/apc - round(shift/apc)| > 1e-5 and every x/z offset until
it is >= 1e-5 from a multiple of 0.5 (float64), so no row is left out of a comparison (bin edges: tests/test_rpn_loss_math_cpu.py).

Error measures: the loss and each named term relative to the term; a gradient entry as |err| / S, S the sum of the absolute values
of the addends that form the entry with every product expanded (the normalisation of tests/test_gpu_train_stack_f64.py):
  d/d logit:    k a w (gamma (1 + p_t)^(gamma-1) p (1-p) (max(x,0) + |x t| + log1p(e^-|x|)) + (1 + p_t)^gamma (p + t))
  bin logits:   k_r (softmax_j + onehot_j);   picked residual / y / size column: k_r (|pred| + the addends of the target, e.g.
  (|offset| + scope + bin * bin_size + bin_size / 2) / bin_size) inside the quadratic zone, k_r outside it;
  every other entry has S = 0 and must be exactly 0.
The bar is not fixed in advance: the composed float32 path on the CPU is measured against the float64 reference on the shape
cases below (both channel counts), and the bar is 8 x its worst figure -- the margin test_gpu_train_stack_f64.py gives a different but
equally valid float32 summation order.  Measured (worst over those cases; composed float32 on the CPU / the device):
  loss and terms  3.1e-7 / 3.1e-7    (bar 2.5e-6)
  gradients       7.25e-7 / 6.9e-7   (bar 5.8e-6)
Both are dominated by the float32 label constants (2 pi, pi / 6 rounded once), which the device route shares with the composed one.
"""
import functools
import math

import numpy as np
import pytest
import torch

from pointrcnn_amd import train_functions as tf

pytestmark = pytest.mark.gpu

F64 = torch.float64
SHAPES = (1, 63, 64, 65, 127, 128, 129, 255, 257, 1000)
TB_KEYS = ("rpn_loss", "rpn_loss_cls", "rpn_loss_reg", "rpn_loss_loc", "rpn_loss_angle", "rpn_loss_size", "rpn_loss_cls_pos",
           "rpn_loss_cls_neg")


class Cfg76(tf.RPNLossConfig):
    pass


class Cfg52(tf.RPNLossConfig):
    LOC_XZ_FINE = False


CFGS = {76: Cfg76, 52: Cfg52}


class Case:
    """seeded CPU inputs: cls (B,N,1), reg (B,N,C) float32, lab (B,N) int64, reg_lab (B,N,7) float32"""

    def __init__(self, npts, C, seed, fg=0.2, ign=0.1, B=1):
        g = torch.Generator().manual_seed(seed)
        self.C, self.npts = C, npts
        self.cls = (torch.randn(npts, generator=g) * 2).view(B, -1, 1)
        self.reg = torch.randn(npts, C, generator=g).view(B, -1, C)
        u = torch.rand(npts, generator=g)
        self.lab = torch.where(u < fg, 1, torch.where(u < fg + ign, -1, 0)).long().view(B, -1)
        lab = torch.empty(npts, 7)
        apc = 2 * math.pi / 12

        def draw(n, lo, hi, ok):
            v = torch.empty(n)
            todo = torch.ones(n, dtype=torch.bool)
            while todo.any():
                v[todo] = torch.rand(int(todo.sum()), generator=g) * (hi - lo) + lo
                todo = ~ok(v.double())
            return v
        off_ok = lambda v: ((v / 0.5) - torch.round(v / 0.5)).abs() * 0.5 >= 1e-5
        lab[:, 0] = draw(npts, -3.5, 3.5, off_ok)
        lab[:, 2] = draw(npts, -3.5, 3.5, off_ok)
        lab[:, 1] = torch.rand(npts, generator=g) * 3 - 1.5
        lab[:, 3:6] = torch.rand(npts, 3, generator=g) * 3 + 1

        def ry_ok(v):
            s = ((v % (2 * math.pi)) + apc / 2) % (2 * math.pi) / apc
            return (s - torch.round(s)).abs() > 1e-5
        lab[:, 6] = draw(npts, -7.0, 7.0, ry_ok)
        self.reg_lab = lab.view(B, -1, 7)

    def view(self, B):
        c = Case.__new__(Case)
        c.C, c.npts = self.C, self.npts
        c.cls, c.reg, c.lab, c.reg_lab = self.cls.view(B, -1, 1), self.reg.view(B, -1, self.C), self.lab.view(B, -1), self.reg_lab.view(B, -1, 7)
        return c


class Stub:
    """one process standing in for two: all_reduce adds the peer's (fixed) counts"""

    def __init__(self, peer):
        self.peer = float(peer)

    def get_world_size(self):
        return 2

    def all_reduce(self, t):
        t.add_(self.peer)


@functools.lru_cache(maxsize=None)
def case(npts, C, seed=0, fg=0.2, ign=0.1):
    return Case(npts, C, 1000 * npts + C + seed, fg, ign)


def composed(c, dtype, dist=None, go=1.0):
    """get_rpn_loss as it stands, on the CPU in `dtype` -> terms dict, d cls, d reg (numpy float64)"""
    cls = c.cls.to(dtype).clone().requires_grad_(True)
    reg = c.reg.to(dtype).clone().requires_grad_(True)
    tb = {}
    loss = tf.get_rpn_loss(cls, reg, c.lab, c.reg_lab.to(dtype), CFGS[c.C], tb_dict=tb, dist=dist, fused=False)
    (loss * go).backward()
    zero = lambda t, like: np.zeros(like.shape) if t is None else t.double().numpy()
    return tb, zero(cls.grad, cls), zero(reg.grad, reg)


@functools.lru_cache(maxsize=None)
def reference(c, peer=None, go=1.0):
    return composed(c, F64, None if peer is None else Stub(peer), go)


def fused(c, dev, dist=None, go=1.0, tb=True, int32=False):
    cls = c.cls.to(dev).requires_grad_(True)
    reg = c.reg.to(dev).requires_grad_(True)
    lab = c.lab.to(dev)
    tbd = {} if tb else None
    loss = tf.get_rpn_loss(cls, reg, lab.int() if int32 else lab, c.reg_lab.to(dev), CFGS[c.C], tb_dict=tbd, dist=dist, fused=True)
    (loss * go).backward()
    assert cls.grad.is_contiguous() and reg.grad.is_contiguous() and cls.grad.shape == cls.shape and reg.grad.shape == reg.shape
    return tbd, cls.grad.cpu(), reg.grad.cpu(), loss.detach().cpu()


def scales(c, go=1.0, peer=None):
    """S of every gradient entry (module docstring), float64"""
    cfg = CFGS[c.C]
    world = 1 if peer is None else 2
    x, lab = c.cls.double().view(-1), c.lab.view(-1)
    t, valid = (lab > 0).double(), (lab >= 0).double()
    w = valid * world / max(float(t.sum()) + (peer or 0), 1.0)
    p, omp = torch.sigmoid(x), torch.sigmoid(-x)
    p_t = t * p + (1 - t) * omp
    ce = torch.clamp(x, min=0) + (x * t).abs() + torch.log1p(torch.exp(-x.abs()))
    a = t * cfg.FOCAL_ALPHA[0] + (1 - t) * (1 - cfg.FOCAL_ALPHA[0])
    gm = cfg.FOCAL_GAMMA
    S_cls = abs(go) * cfg.LOSS_WEIGHT[0] * a * w * (gm * (1 + p_t) ** (gm - 1) * p * omp * ce + (1 + p_t) ** gm * (p + t))
    n_fg = float(t.sum())
    k = abs(go) * cfg.LOSS_WEIGHT[1] * (world * n_fg / max(n_fg + (peer or 0), 1.0) if peer is not None else 1.0) / max(n_fg, 1.0)
    pred, rl = c.reg.double().view(-1, c.C), c.reg_lab.double().view(-1, 7)
    S = torch.zeros_like(pred)
    fg = lab > 0
    nb, nh = 12, cfg.NUM_HEAD_BIN
    xb, xr = tf._bin_and_residual(rl[:, 0], cfg.LOC_SCOPE, cfg.LOC_BIN_SIZE)
    zb, zr = tf._bin_and_residual(rl[:, 2], cfg.LOC_SCOPE, cfg.LOC_BIN_SIZE)
    apc = 2 * math.pi / nh
    shift = ((rl[:, 6] % (2 * math.pi)) + apc / 2) % (2 * math.pi)
    rb = torch.clamp((shift / apc).floor().long(), 0, nh - 1)
    rr = (shift - (rb.double() * apc + apc / 2)) / (apc / 2)
    rows = torch.arange(len(pred))

    def bins(off, n, b):
        S[:, off:off + n] = torch.softmax(pred[:, off:off + n], 1)
        S[rows, off + b] += 1

    def col(cols, target, mag):
        d = pred[rows, cols] - target
        S[rows, cols] = torch.where(d.abs() < 1, pred[rows, cols].abs() + mag, torch.ones_like(d))

    def res_mag(off_label, b):                              # the addends of _bin_and_residual's residual
        return (off_label.abs() + cfg.LOC_SCOPE + b.double() * cfg.LOC_BIN_SIZE + cfg.LOC_BIN_SIZE / 2) / cfg.LOC_BIN_SIZE
    bins(0, nb, xb)
    bins(nb, nb, zb)
    off = 2 * nb
    if cfg.LOC_XZ_FINE:
        col(off + xb, xr, res_mag(rl[:, 0], xb))
        col(off + nb + zb, zr, res_mag(rl[:, 2], zb))
        off += 2 * nb
    col(torch.full_like(xb, off), rl[:, 1], rl[:, 1].abs())
    off += 1
    bins(off, nh, rb)
    col(off + nh + rb, rr, ((rl[:, 6] % (2 * math.pi)) + apc / 2 + rb.double() * apc + apc / 2) / (apc / 2))
    off += 2 * nh
    anchor = torch.tensor(cfg.MEAN_SIZE, dtype=F64)
    for j in range(3):
        col(torch.full_like(xb, off + j), (rl[:, 3 + j] - anchor[j]) / anchor[j], (rl[:, 3 + j].abs() + anchor[j]) / anchor[j])
    S = S * k * fg.double().unsqueeze(1)
    return S_cls.numpy().reshape(c.cls.shape), S.numpy().reshape(c.reg.shape)


def errors(c, got, ref, go=1.0, peer=None):
    """(worst relative error of the loss and its named terms, worst |err| / S of a gradient entry); entries with S = 0 or a zero term
    must be exact"""
    tb, dcls, dreg = got[0], np.asarray(got[1], np.float64), np.asarray(got[2], np.float64)
    e_t = 0.0
    for key in TB_KEYS:
        if ref[0][key] == 0:
            assert tb[key] == 0, (key, tb[key])
        else:
            e_t = max(e_t, abs(tb[key] - ref[0][key]) / abs(ref[0][key]))
    assert tb["rpn_fg_sum"] == ref[0]["rpn_fg_sum"]
    e_g = 0.0
    for g, r, S in zip((dcls, dreg), ref[1:], scales(c, go, peer)):
        assert np.isfinite(g).all()
        assert np.array_equal(g[S == 0], np.zeros((S == 0).sum())) and not r[S == 0].any()
        if (S > 0).any():
            e_g = max(e_g, float((np.abs(g - r)[S > 0] / S[S > 0]).max()))
    return e_t, e_g


@functools.lru_cache(maxsize=None)
def bars():
    """8 x the composed float32 CPU path's worst figures on the shape cases"""
    e_t = e_g = 0.0
    for C in CFGS:
        for n in SHAPES:
            c = case(n, C)
            t, g = errors(c, composed(c, torch.float32), reference(c))
            e_t, e_g = max(e_t, t), max(e_g, g)
    print("composed float32 on the CPU against float64: terms %.3g, gradients %.3g" % (e_t, e_g))
    return 8 * e_t, 8 * e_g


def check(c, got, what, go=1.0, peer=None):
    e_t, e_g = errors(c, got, reference(c, peer, go), go, peer)
    bt, bg = bars()
    print("%s: device terms %.3g (bar %.3g), gradients %.3g (bar %.3g)" % (what, e_t, bt, e_g, bg))
    assert e_t <= bt and e_g <= bg, (what, e_t, bt, e_g, bg)


def relabel(c, lab):
    d = c.view(1)
    d.lab = lab.view(1, -1)
    return d


@pytest.mark.parametrize("C", [76, 52])
@pytest.mark.parametrize("npts", SHAPES)
def test_loss_terms_and_gradients_against_float64(dev, C, npts):
    c = case(npts, C)
    check(c, fused(c, dev), "npts %d C %d" % (npts, C))


@pytest.mark.parametrize("C", [76, 52])
def test_result_does_not_depend_on_how_B_and_N_factor_npts(dev, C):
    c = case(1000, C)
    base = fused(c, dev)
    for B in (2, 4):
        got = fused(c.view(B), dev)
        assert got[0] == base[0] and torch.equal(got[3], base[3])
        assert torch.equal(got[1].view(-1), base[1].view(-1)) and torch.equal(got[2].view(-1), base[2].view(-1))


@pytest.mark.parametrize("C", [76, 52])
def test_label_patterns(dev, C):
    base = case(300, C)
    lab = base.lab.view(-1)
    none = relabel(base, torch.where(lab > 0, 0, lab))
    got = fused(none, dev)
    check(none, got, "no foreground")
    assert all(got[0][k] == 0 for k in ("rpn_loss_reg", "rpn_loss_loc", "rpn_loss_angle", "rpn_loss_size")) and got[0]["rpn_fg_sum"] == 0
    assert not got[2].any() and got[1].abs().max() > 0
    check(relabel(base, torch.ones_like(lab)), fused(relabel(base, torch.ones_like(lab)), dev), "all foreground")
    ign = relabel(base, -torch.ones_like(lab))
    got = fused(ign, dev)
    assert all(got[0][k] == 0 for k in TB_KEYS) and got[0]["rpn_fg_sum"] == 0 and got[3] == 0
    assert not got[1].any() and not got[2].any()
    last = torch.where(lab > 0, 0, lab)
    last[-1] = 1
    check(relabel(base, last), fused(relabel(base, last), dev), "a single foreground row, the last")
    tail = torch.where(lab > 0, 0, lab)
    tail[256:] = torch.where(torch.arange(44) % 3 == 0, 1, tail[256:])                  # rows 256..299: the last, partial tile of 128
    check(relabel(base, tail), fused(relabel(base, tail), dev), "foreground only in the last partial tile", )


@pytest.mark.parametrize("C", [76, 52])
def test_non_finite_predictions_in_unselected_rows_cannot_leak(dev, C):
    c = case(257, C)
    clean = fused(c, dev)
    d = c.view(1)
    d.reg = c.reg.clone()
    rows = torch.nonzero(c.lab.view(-1) <= 0).view(-1)
    assert len(rows) > 30
    for i, r in enumerate(rows.tolist()):
        d.reg.view(-1, C)[r, (7 * i) % C] = (float("nan"), float("inf"), float("-inf"))[i % 3]
    got = fused(d, dev)
    assert math.isfinite(got[0]["rpn_loss"]) and got[0] == clean[0] and torch.equal(got[3], clean[3])
    assert torch.equal(got[1], clean[1]) and torch.equal(got[2], clean[2])
    assert not got[2].view(-1, C)[rows].any()


@pytest.mark.parametrize("C", [76, 52])
def test_saturated_cls_logits(dev, C):
    c = case(255, C).view(1)
    c.cls = torch.where(torch.arange(255) % 2 == 0, 100.0, -100.0).view(1, -1, 1)
    check(c, fused(c, dev), "cls logits at +-100")


@pytest.mark.parametrize("C", [76, 52])
def test_strided_views_and_int32_labels(dev, C):
    c = case(257, C)
    want = fused(c, dev)
    wide_reg = torch.full((1, 257, 80), float("nan"), device=dev)
    wide_cls = torch.full((1, 257, 4), float("nan"), device=dev)
    wide_reg[:, :, :C] = c.reg.to(dev)
    wide_cls[:, :, 1:2] = c.cls.to(dev)
    reg, cls = wide_reg[:, :, :C].requires_grad_(True), wide_cls[:, :, 1:2].requires_grad_(True)
    assert reg.stride(1) == 80 and cls.stride(1) == 4
    tb = {}
    loss = tf.get_rpn_loss(cls, reg, c.lab.to(dev).int(), c.reg_lab.to(dev), CFGS[C], tb_dict=tb, fused=True)
    dcls, dreg = torch.autograd.grad(loss, (cls, reg))
    assert dcls.is_contiguous() and dreg.is_contiguous() and dreg.shape == (1, 257, C)
    assert tb == want[0] and torch.equal(dcls.cpu(), want[1]) and torch.equal(dreg.cpu(), want[2])


@pytest.mark.parametrize("C", [76, 52])
def test_upstream_gradient_without_a_host_sync(dev, C):
    c = case(257, C)
    base = fused(c, dev)
    cls, reg = c.cls.to(dev).requires_grad_(True), c.reg.to(dev).requires_grad_(True)
    lab, reg_lab = c.lab.to(dev), c.reg_lab.to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = tf.get_rpn_loss(cls, reg, lab, reg_lab, CFGS[C], tb_dict=None, fused=True)
        (loss * 0.37).backward()
        g1 = (cls.grad.clone(), reg.grad.clone())
        cls.grad = reg.grad = None
        loss = tf.get_rpn_loss(cls, reg, lab, reg_lab, CFGS[C], tb_dict=None, fused=True)
        (loss.sum() + (cls * 0.01).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(c, (base[0], g1[0].cpu(), g1[1].cpu()), "grad_output 0.37", go=0.37)
    assert torch.equal(reg.grad.cpu(), base[2])
    assert (cls.grad.cpu() - (base[1] + 0.01)).abs().max() <= 1e-7


@pytest.mark.parametrize("C", [76, 52])
def test_two_calls_give_identical_bytes(dev, C):
    c = case(1000, C)
    a, b = fused(c, dev), fused(c, dev)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("C", [76, 52])
def test_global_normalisation_through_a_dist_stub(dev, C):
    c = case(257, C)
    check(c, fused(c, dev, dist=Stub(37)), "dist stub, peer with 37 foreground points", peer=37)
    lab = c.lab.view(-1)
    none = relabel(c, torch.where(lab > 0, 0, lab))
    got = fused(none, dev, dist=Stub(37))
    check(none, got, "dist stub, no local foreground", peer=37)
    assert not got[2].any() and got[0]["rpn_loss_reg"] == 0


@pytest.mark.parametrize("C", [76, 52])
def test_tb_dict_entries_from_one_read(dev, C, monkeypatch):
    c = case(255, C)
    got = fused(c, dev)
    ref = reference(c)
    assert set(got[0]) == set(TB_KEYS) | {"rpn_fg_sum"}
    assert got[0]["rpn_fg_sum"] == ref[0]["rpn_fg_sum"] == int((c.lab > 0).sum()) and isinstance(got[0]["rpn_fg_sum"], int)
    check(c, got, "tb_dict")
    reads = []
    for name in ("item", "tolist", "cpu"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n), _o(self, *a, **k))[1])
    tf.get_rpn_loss(c.cls.to(dev), c.reg.to(dev), c.lab.to(dev), c.reg_lab.to(dev), CFGS[C], tb_dict={}, fused=True)
    assert reads == ["tolist"], reads


def test_outside_the_family_the_composed_code_runs(dev):
    c = case(255, 76)

    class Dice(tf.RPNLossConfig):
        LOSS_CLS = "DiceLoss"

    class Mine(tf.SigmoidFocalClassificationLoss):
        def forward(self, prediction_tensor, target_tensor, weights):
            return 2 * super().forward(prediction_tensor, target_tensor, weights)
    cls, reg, lab, reg_lab = c.cls.to(dev), c.reg.to(dev), c.lab.to(dev), c.reg_lab.to(dev)
    for kw in (dict(cfg=Dice), dict(cfg=Cfg76, cls_loss_func=Mine(alpha=0.25, gamma=2.0))):
        a = tf.get_rpn_loss(cls, reg, lab, reg_lab, fused=True, **kw)
        b = tf.get_rpn_loss(cls, reg, lab, reg_lab, fused=False, **kw)
        assert torch.equal(a, b)
    a = tf.get_rpn_loss(c.cls, c.reg, c.lab, c.reg_lab, Cfg76, fused=True)
    assert not a.is_cuda and torch.equal(a, tf.get_rpn_loss(c.cls, c.reg, c.lab, c.reg_lab, Cfg76, fused=False))


def test_default_route_does_not_reach_the_new_ops(dev, monkeypatch):
    from pointrcnn_amd import ops

    def boom(*a, **k):
        raise AssertionError("the fused RPN loss ran without being asked for")
    for name in ("rpn_loss_counts", "rpn_loss_forward", "rpn_loss_backward"):
        assert callable(getattr(ops, name))
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(tf, "FUSED_RPN_LOSS", False)                    # the switch unset
    c = case(255, 76)
    cls = c.cls.to(dev).requires_grad_(True)
    tf.get_rpn_loss(cls, c.reg.to(dev), c.lab.to(dev), c.reg_lab.to(dev), Cfg76, fused=None).backward()
    assert cls.grad is not None
    with pytest.raises(AssertionError, match="without being asked"):
        tf.get_rpn_loss(cls, c.reg.to(dev), c.lab.to(dev), c.reg_lab.to(dev), Cfg76, fused=True)


def test_whole_training_step_fused_against_composed(dev):
    """one RPNTrainer step's loss and parameter gradients with fused_loss=True against False from the same state: the loss to the
    bar above, the gradients in norm with the tolerances of test_gpu_round2.test_rpn_training_step_matches_reference_golden (heads
    1e-4; behind the max-pools 3e-2 with a median below 1e-3)"""
    from test_gpu_round2 import T, _Wrap, _fill
    from make_golden import TRAIN_CASE, train_batch
    from pointrcnn_amd import rpn
    pts, gt, cls, reg = train_batch(TRAIN_CASE)
    model = rpn.RPN()
    _fill(_Wrap(model), TRAIN_CASE["wseed"])
    model = model.to(dev)
    batch = {"pts_input": T(pts, dev), "rpn_cls_label": T(cls, dev), "rpn_reg_label": T(reg, dev)}
    out = {}
    for fused_loss in (True, False):
        trainer = tf.RPNTrainer(model, ddp=False, fused_loss=fused_loss)
        assert trainer.fused_loss is fused_loss
        trainer.model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
        model.zero_grad(set_to_none=True)
        loss = trainer.loss(batch)
        loss.backward()
        out[fused_loss] = (float(loss.item()), {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None})
    (lf, gf), (lc, gc) = out[True], out[False]
    assert abs(lf - lc) <= bars()[0] * abs(lc), (lf, lc)
    assert sorted(gf) == sorted(gc)
    rel = {n: float((gf[n] - gc[n]).norm() / gc[n].norm().clamp(min=1e-30)) for n in gc}
    heads = [n for n in rel if "rpn_cls_layer" in n or "rpn_reg_layer" in n]
    assert len(heads) == 10 and max(rel[n] for n in heads) <= 1e-4, [(n, rel[n]) for n in heads]
    assert max(rel.values()) <= 3e-2 and float(np.median(list(rel.values()))) <= 1e-3, max(rel.items(), key=lambda kv: kv[1])
