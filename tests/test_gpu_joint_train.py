"""The joint RPN + RCNN training step (`train_rcnn.py --train_mode rcnn --set RPN.FIXED False`): PointRCNN(rpn_fixed=False),
RCNNNet's opt-in RoI-pooling backward (pool_grad) and train_functions.JointTrainer.  Shapes and bars follow
tests/test_gpu_train_rcnn.py: its _rcnn_batch at B = 2, labels from synthetic_rpn_labels, loss 1e-5 relative, parameter gradients
5e-3 in norm."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_train_rcnn import _both, _pm, _rcnn_batch

pytestmark = pytest.mark.gpu

KEYS = {"rpn_cls", "rpn_reg", "backbone_xyz", "backbone_features", "rois", "roi_scores_raw", "seg_result", "rcnn_cls", "rcnn_reg",
        "pooled_empty_flag", "pts_input", "sampled_pts", "pts_feature", "cls_label", "reg_valid_mask", "gt_of_rois", "gt_iou", "roi_boxes3d"}
_CACHE = {}


def _batch(dev):
    if "batch" not in _CACHE:
        from pointrcnn_amd import ops, train_functions as tf
        batch = _rcnn_batch(dev)
        cls, reg = tf.synthetic_rpn_labels(batch["pts_input"], batch["gt_boxes3d"], ops.pts_in_boxes3d)
        batch["rpn_cls_label"], batch["rpn_reg_label"] = cls, reg
        _CACHE["batch"] = batch
    return _CACHE["batch"]


def _model(dev, **kw):
    from pointrcnn_amd import point_rcnn, rpn
    torch.manual_seed(11)
    model = point_rcnn.PointRCNN(mode="TRAIN", **kw).to(dev)
    rpn.randomize_bn_stats(model.rpn, seed=3)
    return model


def _forward(m, batch, retain=()):
    m.train()
    m.rcnn_net.proposal_target_layer.seed = 21
    torch.manual_seed(77)                                      # the elementwise RoI augmentation draws from torch's generator
    out = m(batch)
    for k in retain:
        out[k].retain_grad()
    return out


def _losses(m, out, batch):
    from pointrcnn_amd import train_functions as tf
    rpn_loss = tf.get_rpn_loss(out["rpn_cls"], out["rpn_reg"], batch["rpn_cls_label"], batch["rpn_reg_label"])
    return rpn_loss, tf.get_rcnn_loss(out, m.rcnn_cfg)


def _rel(a, b):
    return (a - b).double().norm().item() / max(1e-12, b.double().norm().item())


def _worst(ma, mb, part):
    pa, pb = dict(getattr(ma, part).named_parameters()), dict(getattr(mb, part).named_parameters())
    worst, bitwise = 0.0, True
    for n in pa:
        assert pa[n].grad is not None and pb[n].grad is not None, (part, n)
        worst = max(worst, _rel(pa[n].grad, pb[n].grad))
        bitwise = bitwise and torch.equal(pa[n].grad, pb[n].grad)
    return worst, bitwise


def test_default_is_untouched_and_eval_ignores_the_flag(dev):
    from pointrcnn_amd import train_functions as tf
    batch = _batch(dev)
    model = _model(dev)
    assert model.rpn_fixed is True and model.rcnn_net.pool_grad is False
    out = _forward(model, batch)
    assert set(out) == KEYS
    assert not out["rpn_cls"].requires_grad and not out["backbone_features"].requires_grad and not out["pts_input"].requires_grad
    assert not model.rpn.training                              # a fixed RPN stays in eval mode
    tf.get_rcnn_loss(out, model.rcnn_cfg).backward()
    assert all(p.grad is None for p in model.rpn.parameters())
    assert all(p.grad is not None for p in model.rcnn_net.parameters())
    # evaluation: the flag changes nothing
    joint = _model(dev, rpn_fixed=False, pool_grad=True)
    joint.load_state_dict(model.state_dict())
    model.eval(), joint.eval()
    with torch.no_grad():
        a, b = model({"pts_input": batch["pts_input"]}), joint({"pts_input": batch["pts_input"]})
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_joint_loss_is_the_sum_and_its_gradients_the_two_parts(dev):
    """pool_grad off: the joint backward gives rcnn_net the RCNN-only gradients and the RPN the RPN-only gradients (disjoint paths
    through one forward), with the hand-written stacks; and the joint step on the stacks against the composed torch path"""
    pm, pt = _pm()
    batch = _batch(dev)
    base = _model(dev, rpn_fixed=False)
    joint, only_rcnn, only_rpn, composed = base, copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)

    out = _forward(joint, batch)
    assert set(out) == KEYS and out["rpn_cls"].requires_grad and out["rpn_reg"].requires_grad and joint.rpn.training
    assert not out["rois"].requires_grad and not out["pts_input"].requires_grad
    l_rpn, l_rcnn = _losses(joint, out, batch)
    loss = l_rpn + l_rcnn
    loss.backward()
    o2 = _forward(only_rcnn, batch)
    _, b_rcnn = _losses(only_rcnn, o2, batch)
    b_rcnn.backward()
    o3 = _forward(only_rpn, batch)
    c_rpn, _ = _losses(only_rpn, o3, batch)
    c_rpn.backward()
    for k in ("rcnn_cls", "rcnn_reg", "rpn_cls", "rpn_reg", "roi_boxes3d", "cls_label"):
        assert torch.equal(out[k], o2[k]) and torch.equal(out[k], o3[k]), k
    want = b_rcnn.item() + c_rpn.item()
    assert abs(loss.item() - want) <= 1e-5 * max(1.0, abs(want)), (loss.item(), want)
    assert all(p.grad is None for p in only_rcnn.rpn.parameters())             # without pool_grad the RCNN loss stops at the pooling
    assert all(p.grad is None for p in only_rpn.rcnn_net.parameters())
    w_rcnn, bit_rcnn = _worst(joint, only_rcnn, "rcnn_net")
    w_rpn, bit_rpn = _worst(joint, only_rpn, "rpn")
    print("joint vs separate backward: rcnn_net worst %.3e (bitwise %s), rpn worst %.3e (bitwise %s)" % (w_rcnn, bit_rcnn, w_rpn, bit_rpn))
    assert w_rcnn <= 5e-3 and w_rpn <= 5e-3, (w_rcnn, w_rpn)

    # fused stacks against the composed torch path (TRAIN_FUSED off), as the RCNN test does.  The RPN heads' Dropout is switched off
    # for this pair, as in the RPN stack tests: the rows path and the Sequential draw their masks in different element orders.
    import time
    fused = copy.deepcopy(composed)
    for m in (fused, composed):
        m.zero_grad(set_to_none=True)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0

    def run(m):
        torch.cuda.synchronize()
        t0 = time.time()
        o = _forward(m, batch)
        a, b = _losses(m, o, batch)
        (a + b).backward()
        torch.cuda.synchronize()
        return o, a + b, time.time() - t0
    of, lf, tf_ = run(fused)
    pm.TRAIN_FUSED = False
    try:
        with torch.backends.cudnn.flags(enabled=False):        # torch's own convolution / batch-norm kernels: nothing to tune or build
            oc, lc, tc_ = run(composed)
    finally:
        pm.TRAIN_FUSED = True
    # the RPN is in train mode here, so its outputs -- and with them the proposals -- agree to rounding, not to the bit (in the RCNN
    # test the fixed RPN runs the same inference kernels on both sides); the sampler must still pick the same RoIs
    roi_err = (of["roi_boxes3d"] - oc["roi_boxes3d"]).abs().max().item()
    wc_rcnn, _ = _worst(fused, composed, "rcnn_net")
    pf, pc = dict(fused.rpn.named_parameters()), dict(composed.rpn.named_parameters())
    rel = {n: _rel(pf[n].grad, pc[n].grad) for n in pf}
    heads = [n for n in rel if "rpn_cls_layer" in n or "rpn_reg_layer" in n]
    top = sorted(rel.items(), key=lambda kv: -kv[1])[:3]
    print("fused vs composed joint step: sampled RoIs max abs diff %.3e, labels equal %s, seg flips %d, loss %.8f vs %.8f, rcnn_net worst "
          "%.3e, rpn heads worst %.3e, rpn worst %s, rpn median %.3e, seconds fused %.2f composed %.2f"
          % (roi_err, torch.equal(of["cls_label"], oc["cls_label"]), int((of["seg_result"] != oc["seg_result"]).sum()), lf.item(), lc.item(),
             wc_rcnn, max(rel[n] for n in heads), ["%s %.3e (|g| %.2e)" % (n, r, pc[n].grad.norm().item()) for n, r in top],
             float(np.median(list(rel.values()))), tf_, tc_))
    assert roi_err <= 1e-4 and torch.equal(of["cls_label"], oc["cls_label"]) and torch.equal(of["reg_valid_mask"], oc["reg_valid_mask"])
    assert abs(lf.item() - lc.item()) <= 1e-5 * max(1.0, abs(lc.item())), (lf.item(), lc.item())
    # measured: rcnn_net worst 1.8e-3, rpn worst 1.1e-3 (SA_modules.0.mlps.1.layer0.conv.weight), rpn heads 2.6e-5, rpn median 5.8e-4
    assert wc_rcnn <= 5e-3 and max(rel.values()) <= 5e-3, (wc_rcnn, top)
    assert len(heads) == 10 and max(rel[n] for n in heads) <= 1e-4, [(n, rel[n]) for n in heads]       # no pooling behind the heads


def test_pool_grad_on_against_off(dev):
    """the forward does not change; rcnn_net's gradients do not change; backbone_features receives, on top of the RPN loss's
    gradient, exactly ops.roipool3d_grad of pts_input's gradient; and that reaches the backbone's parameters"""
    from pointrcnn_amd import ops
    batch = _batch(dev)
    off = _model(dev, rpn_fixed=False)
    on = copy.deepcopy(off)
    on.rcnn_net.pool_grad = True
    res = {}
    for name, m in (("off", off), ("on", on)):
        out = _forward(m, batch, retain=("backbone_features",))
        if name == "on":
            out["pts_input"].retain_grad()
        else:
            assert not out["pts_input"].requires_grad
        a, b = _losses(m, out, batch)
        loss = a + b
        loss.backward()
        res[name] = (out, loss)
    (oa, la), (ob, lb) = res["off"], res["on"]
    assert ob["pts_input"].requires_grad and "pool_idx" in ob and set(ob) - {"pool_idx", "pool_distinct"} == set(oa) == KEYS
    assert torch.equal(la, lb)
    for k in KEYS:
        assert (oa[k] is None and ob[k] is None) or torch.equal(oa[k], ob[k]), k       # (pooled_empty_flag is None in training)
    w, bitwise = _worst(on, off, "rcnn_net")
    assert bitwise, w
    g_on, g_off = ob["backbone_features"].grad, oa["backbone_features"].grad                   # (B, C, N)
    B, C, N = g_on.shape
    c0 = ob["pts_input"].shape[2] - C
    assert c0 == on.rcnn_net.rcnn_input_channel == 5
    idx, distinct = ob["pool_idx"], ob["pool_distinct"]
    assert tuple(idx.shape) == (B, 64, 512) and tuple(distinct.shape) == (B, 64)
    pg = ops.roipool3d_grad(ob["pts_input"].grad, idx, distinct, N, C, col0=c0).permute(0, 2, 1)
    err = (g_on.double() - g_off.double() - pg.double()).abs()
    bound = 2.0 ** -23 * (g_on.double().abs() + g_off.double().abs())
    print("pool_grad on - off on backbone_features: max |diff - roipool3d_grad| %.3e, worst err/bound %.3f, |roipool3d_grad| max %.3e, "
          "exact in %.4f of the elements" % (err.max().item(), (err / bound.clamp(min=1e-300)).max().item(), pg.abs().max().item(),
                                            (err == 0).double().mean().item()))
    assert pg.abs().max().item() > 0
    assert (err <= bound).all()
    pa, pb = dict(on.rpn.backbone_net.named_parameters()), dict(off.rpn.backbone_net.named_parameters())
    assert any(not torch.equal(pa[n].grad, pb[n].grad) for n in pa)


def test_joint_trainer(dev, monkeypatch):
    from pointrcnn_amd import optim, train_functions as tf
    batch = _batch(dev)
    for pool_grad in (False, True):
        tr = tf.JointTrainer(_model(dev), pool_grad=pool_grad)
        assert tr.net.rpn_fixed is False and tr.net.rcnn_net.pool_grad is pool_grad
        ids = {id(p) for p in tr.params}
        assert ids == {id(p) for p in tr.net.rpn.parameters()} | {id(p) for p in tr.net.rcnn_net.parameters()}
        tb = {}
        l0 = tr.step(batch, tb_dict=tb)
        assert {"loss", "rpn_loss", "rcnn_loss", "rpn_loss_cls", "rcnn_loss_cls"} <= set(tb)
        assert abs(tb["loss"] - (tb["rpn_loss"] + tb["rcnn_loss"])) <= 1e-5 * max(1.0, abs(tb["loss"]))
        # tb_dict None: no device-to-host read inside the step (the read counter of the loss tests, on device tensors)
        reads = []
        with monkeypatch.context() as mp:
            for name in ("item", "tolist", "cpu", "numpy"):
                orig = getattr(torch.Tensor, name)
                mp.setattr(torch.Tensor, name, lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n) if self.is_cuda else None, _o(self, *a, **k))[1])
            for _ in range(5):
                l = tr.step(batch, next_batch=batch)
        assert reads == [], reads
        assert np.isfinite(float(l0.item())) and np.isfinite(float(l.item()))
        assert all(torch.isfinite(p).all() for p in tr.params)
    # an optimizer that clips in its step: no second clip
    calls = []
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    class ClippingSGD(torch.optim.SGD):                        # says it clips in its step(), and calls nothing that would be counted
        clips_in_step = True

    tr = tf.JointTrainer(_model(dev), optimizer=lambda params: ClippingSGD(params, lr=1e-4))
    assert type(tr.optimizer) is ClippingSGD and tr.optimizer_name == "ClippingSGD"
    tr.step(batch)
    assert len(calls) == 0
    tr2 = tf.JointTrainer(_model(dev))
    tr2.step(batch)
    assert len(calls) == 1                                     # the counter does see the trainer's own clip
    # the reference's recipe, resolved by name as the other trainers do
    tr3 = tf.JointTrainer(_model(dev), optimizer="adam_onecycle", total_steps=10)
    assert type(tr3.optimizer) is optim.OneCycleAdam and tr3.optimizer.clips_in_step
    assert np.isfinite(float(tr3.step(batch).item()))
