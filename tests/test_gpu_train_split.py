"""The opt-in split-bf16 training GEMMs (train_mlp.TRAIN_SPLIT = 6: train_fwd_s_kernel / train_dgrad_s_kernel of
csrc/mlp_train.h on the eligible layers) against float64, entry by entry, on the cases of tests/train_split_cases.py.

Every case runs tests/test_gpu_train_stack_f64.py's own comparison (test_case_equals_float64_closed_form is called as it is, with
the attribute on): decisions shared with the device, and that file's bars, unchanged -- the split must be fp32-grade:
  saved y of every layer        per entry 1e-5 sum |a| |w|
  constant rows, output rows, running statistics    1e-5 max(1, max |ref|)
  every gradient                1e-4 max(1, max |ref|);  dW / input gradients per entry: entry_ratio <= ratio_bar (8 x CPU_F32_RATIO)
  untouched memory              gout is a slice of a NaN-framed buffer there; nothing the caller reads may be NaN
  worst seen with the attribute on (one MI355X):
      saved y 6.6e-07 sum |a| |w| (s_flat);  dW ratio 2.7e-06 (s_group_wide, bar 3.3e-05);  input gradient ratio 4.3e-07 (s_narrow_6016,
      bar 1.3e-05);  whole RPN step: loss equal to nine digits, worst parameter-gradient distance 8.1e-04 in norm (bar 5e-3)
Which kernel each layer of each case gets is proven on the CPU (tests/test_train_split_cpu.py).

Further: the fp32 layer of the mixed stack and its statistics are bit-identical with the attribute on and off, while the saved y
of an eligible layer differs in at least one bit (the split is really in use) and both settings meet the bars; two runs are
bit-identical (wide plain stack, padding-free stack); a +inf operand makes its own row of y non-finite and leaves every other row
inside the bar (ordinary IEEE data: the rule of the kernels' header comment); one whole RPN training step with the attribute on
stays within the fused-against-composed bars of tests/test_gpu_train_rcnn.py (loss 1e-5 max(1, |loss|), every parameter gradient
5e-3 in norm); with the attribute off the new entry points are never reached."""
import pytest
import torch

import test_gpu_train_stack_f64 as F
import train_split_cases as S
import train_stack_cases as T
from train_stack_cases import F64

pytestmark = [pytest.mark.gpu, pytest.mark.own_arithmetic]


@pytest.fixture
def split_on(monkeypatch):
    from pointrcnn_amd import train_mlp
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", 6)


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_split_case_equals_float64_closed_form(dev, case, split_on):
    F.test_case_equals_float64_closed_form(dev, case)


def test_ineligible_layers_are_untouched_and_the_split_is_in_use(dev, monkeypatch):
    """s_mixed: layer 0 (K = 33) runs the fp32 kernel under both settings -- its saved y, constants and running statistics are the
    same bits; layer 1 (K = 32) runs train_fwd_s_kernel with the attribute on -- its saved y differs somewhere; the full float64
    comparison holds under both"""
    from pointrcnn_amd import train_mlp
    case = S.BY_NAME["s_mixed"]
    I = T.build_inputs(case)
    runs = {}
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", terms)
        runs[terms] = F._run(case, I, dev)
        F.test_case_equals_float64_closed_form(dev, case)
    off, on = runs[0], runs[6]
    assert torch.equal(off.y[0], on.y[0]) and torch.equal(off.cst[0], on.cst[0])
    assert torch.equal(off.run_mean[0], on.run_mean[0]) and torch.equal(off.run_var[0], on.run_var[0])
    assert not torch.equal(off.y[1], on.y[1]), "the saved y of the K = 32 layer is the fp32 kernel's, bit for bit"


@pytest.mark.parametrize("name", S.REPEAT_CASES)
def test_two_split_runs_are_bit_identical(dev, name, split_on):
    case = S.BY_NAME[name]
    I = T.build_inputs(case)
    a, b = F._run(case, I, dev), F._run(case, I, dev)
    assert torch.equal(a.out, b.out)
    nlive = T.Rows(case, I).live.numel()                       # (rows past the live ones are never written)
    for l, (ya, yb) in enumerate(zip(a.y, b.y)):
        assert torch.equal(ya[:nlive], yb[:nlive]), "saved y of layer %d" % l
    for l, (ga, gb) in enumerate(zip(a.grads, b.grads)):
        assert (ga is None and gb is None) or torch.equal(ga, gb), "parameter gradient %d of layer %d" % (l % 3, l // 3)
    assert (a.gx0 is None and b.gx0 is None) or torch.equal(a.gx0, b.gx0)
    for ma, mb in zip(a.run_mean + a.run_var, b.run_mean + b.run_var):
        assert torch.equal(ma, mb)


def test_a_non_finite_operand_stays_in_its_row(dev, split_on):
    """plain [32, 32], 130 rows, no BatchNorm, one +inf in row 70: row 70 of y is non-finite, every other row meets the bar"""
    case = T.Case("s_inf_row", "plain", [32, 32], bn=False, R=130)
    I = T.build_inputs(case)
    I.x0[70, 5] = float("inf")
    r = F._run(case, I, dev)
    y = r.y[0]
    assert bool((~torch.isfinite(y[70])).all()), y[70]
    keep = torch.arange(130) != 70
    a, w = I.x0[keep].to(F64), I.W[0].to(F64)
    want, bar = a @ w.t(), 1e-5 * (a.abs() @ w.abs().t())
    assert bool(torch.isfinite(y[keep]).all())
    over = (y[keep].to(F64) - want).abs() - bar
    assert float(over.max()) <= 0.0, float(over.max())


def test_one_whole_rpn_step_on_against_off(dev, monkeypatch):
    """the B = 2 RPN training batch of the golden step (tests/golden/make_golden.py), same weights, no dropout: loss and parameter
    gradients with the attribute on against off"""
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
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", terms)
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
    assert any(not torch.equal(g0[n], g6[n]) for n in g0), "the split arithmetic was not in use"
    assert max(rel.values()) <= 5e-3, max(rel.items(), key=lambda kv: kv[1])


def test_default_route_does_not_reach_the_new_entry_points(dev, monkeypatch):
    from pointrcnn_amd import _cabi, train_mlp

    def boom(*a, **k):
        raise AssertionError("a split entry point ran without being asked for")
    L = _cabi.lib()
    for name in ("prcnn_train_stack_fwd_split", "prcnn_train_stack_bwd_split"):
        assert callable(getattr(L, name))
        monkeypatch.setattr(L, name, boom)
    assert train_mlp.TRAIN_SPLIT == 0                          # the variable unset: off
    case = S.BY_NAME["s_rows_129"]
    I = T.build_inputs(case)
    r = F._run(case, I, dev)
    assert r.gx0 is not None and bool(torch.isfinite(r.out).all())
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", 6)
    with pytest.raises(AssertionError, match="without being asked"):
        F._run(case, I, dev)
