"""The opt-in split-bf16 weight gradient of the wide training layers (train_mlp.TRAIN_SPLIT_WGRAD = 6: train_wgrad_s_kernel of
csrc/mlp_train.h wherever the default path runs train_wgrad_lds_kernel) against float64, entry by entry, on the cases of
tests/train_wsplit_cases.py.

Every case runs tests/test_gpu_train_stack_f64.py's own comparison (test_case_equals_float64_closed_form is called as it is, with
the attribute on), once with the forward / dgrad GEMMs on fp32 (TRAIN_SPLIT = 0) and once on split-bf16 (TRAIN_SPLIT = 6):
decisions shared with the device, the decision-band share <= MAX_BAND_SHARE on the device's decisions, and that file's bars
unchanged -- dW per entry within ratio_bar = 8 x CPU_F32_RATIO, every gradient 1e-4 max(1, max |ref|).  The split must be
fp32-grade.  Which kernel each layer of each case gets is proven on the CPU (tests/test_train_wsplit_cpu.py).
  worst seen with the attribute on (one MI355X): dW ratio 2.3e-06 (w_rows_32, bar 3.3e-05); input gradient ratio 4.9e-07 (bar
  1.3e-05); whole RPN step: loss equal to nine digits, worst parameter-gradient distance 3.8e-06 in norm (bar 5e-3)

Further: on the mixed stack the narrow layers' dW is bit-identical with the attribute on and off while the wide layer's dW differs
in at least one bit, and with TRAIN_SPLIT = 0 everything but wgrad -- saved y, output, running statistics, dgamma, dbeta, the
input gradient -- is bit-identical; two runs are bit-identical (a plain wide stack crossing two range boundaries, the padding-free
stack); with the attribute off the new export is never reached (TRAIN_SPLIT 0 and 6), with it on it is; one whole RPN training
step with the attribute on stays within the bars of test_gpu_train_split.test_one_whole_rpn_step_on_against_off (loss 1e-5
max(1, |loss|), every parameter gradient 5e-3 in norm) and differs from the step with it off in at least one bit."""
import pytest
import torch

import test_gpu_train_stack_f64 as F
import train_stack_cases as T
import train_wsplit_cases as WC

pytestmark = [pytest.mark.gpu, pytest.mark.own_arithmetic]


@pytest.mark.parametrize("terms", [0, 6], ids=["fwd_fp32", "fwd_split"])
@pytest.mark.parametrize("case", WC.CASES, ids=[c.name for c in WC.CASES])
def test_wsplit_case_equals_float64_closed_form(dev, case, terms, monkeypatch):
    from pointrcnn_amd import train_mlp
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", terms)
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", 6)
    F.test_case_equals_float64_closed_form(dev, case)


def test_the_split_is_in_use_and_only_where_it_should_be(dev, monkeypatch):
    from pointrcnn_amd import train_mlp
    case = WC.BY_NAME[WC.MIXED]
    I = T.build_inputs(case)
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", 0)
    runs = {}
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", terms)
        runs[terms] = F._run(case, I, dev)
    off, on = runs[0], runs[6]
    for l in WC.MIXED_NARROW_LAYERS:
        assert torch.equal(off.grads[3 * l], on.grads[3 * l]), "dW of the narrow layer %d moved" % l
    for l in WC.MIXED_WIDE_LAYERS:
        assert not torch.equal(off.grads[3 * l], on.grads[3 * l]), "dW of the wide layer %d is the fp32 kernel's, bit for bit" % l
    # only wgrad changed
    assert torch.equal(off.out, on.out) and torch.equal(off.gx0, on.gx0)
    for l in range(len(case.chans) - 1):
        assert torch.equal(off.y[l], on.y[l]) and torch.equal(off.cst[l], on.cst[l]), "saved y / constants of layer %d" % l
        assert torch.equal(off.run_mean[l], on.run_mean[l]) and torch.equal(off.run_var[l], on.run_var[l])
        assert torch.equal(off.grads[3 * l + 1], on.grads[3 * l + 1]), "dgamma of layer %d" % l
        assert torch.equal(off.grads[3 * l + 2], on.grads[3 * l + 2]), "dbeta of layer %d" % l


@pytest.mark.parametrize("name", WC.REPEAT_CASES)
def test_two_wsplit_runs_are_bit_identical(dev, name, monkeypatch):
    from pointrcnn_amd import train_mlp
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", 6)
    case = WC.BY_NAME[name]
    I = T.build_inputs(case)
    a, b = F._run(case, I, dev, read_saved=False), F._run(case, I, dev, read_saved=False)
    assert torch.equal(a.out, b.out)
    for l, (ga, gb) in enumerate(zip(a.grads, b.grads)):
        assert (ga is None and gb is None) or torch.equal(ga, gb), "parameter gradient %d of layer %d" % (l % 3, l // 3)
    assert (a.gx0 is None and b.gx0 is None) or torch.equal(a.gx0, b.gx0)


def test_default_route_does_not_reach_the_new_export(dev, monkeypatch):
    from pointrcnn_amd import _cabi, train_mlp

    def boom(*a, **k):
        raise AssertionError("the split-wgrad export ran without being asked for")
    L = _cabi.lib()
    assert callable(L.prcnn_train_stack_bwd_wsplit)
    monkeypatch.setattr(L, "prcnn_train_stack_bwd_wsplit", boom)
    assert train_mlp.TRAIN_SPLIT_WGRAD == 0                    # the variable unset: off
    case = WC.BY_NAME["w_rows_33"]
    I = T.build_inputs(case)
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", terms)
        r = F._run(case, I, dev, read_saved=False)
        assert r.gx0 is not None and bool(torch.isfinite(r.grads[0]).all())
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", terms)
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", 6)
        with pytest.raises(AssertionError, match="without being asked"):
            F._run(case, I, dev, read_saved=False)
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", 0)


def test_one_whole_rpn_step_on_against_off(dev, monkeypatch):
    """the B = 2 RPN training batch of the golden step (tests/golden/make_golden.py), same weights, no dropout: loss and parameter
    gradients with the attribute on against off (forward / dgrad on fp32 under both)"""
    from test_gpu_round2 import T as to_dev, _Wrap, _fill          # (puts tests/golden on the path)
    from make_golden import TRAIN_CASE, train_batch
    from pointrcnn_amd import rpn, train_functions as tf, train_mlp
    pts, gt, cls, reg = train_batch(TRAIN_CASE)
    model = rpn.RPN()
    _fill(_Wrap(model), TRAIN_CASE["wseed"])
    model = model.to(dev)
    batch = {"pts_input": to_dev(pts, dev), "rpn_cls_label": to_dev(cls, dev), "rpn_reg_label": to_dev(reg, dev)}
    state = {k: v.clone() for k, v in model.state_dict().items()}
    out = {}
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", terms)
        model.load_state_dict(state)                           # (the running statistics move with every forward)
        trainer = tf.RPNTrainer(model, ddp=False)
        trainer.model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
        model.zero_grad(set_to_none=True)
        loss = trainer.loss(batch)
        loss.backward()
        out[terms] = (float(loss.item()), {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None})
    (l0, g0), (l6, g6) = out[0], out[6]
    assert abs(l6 - l0) <= 1e-5 * max(1.0, abs(l0)), (l6, l0)
    assert sorted(g0) == sorted(g6) and len(g0) > 50
    rel = {n: float((g6[n] - g0[n]).norm() / g0[n].norm().clamp(min=1e-12)) for n in g0}
    print("\nwhole step: loss off %.9g on %.9g; worst gradient distance in norm %.3e (%s)" % ((l0, l6) + max((v, k) for k, v in rel.items())))
    assert any(not torch.equal(g0[n], g6[n]) for n in g0), "the split wgrad was not in use"
    assert max(rel.values()) <= 5e-3, max(rel.items(), key=lambda kv: kv[1])
