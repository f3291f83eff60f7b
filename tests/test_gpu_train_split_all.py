"""The third split-bf16 opt-in of the training SharedMLP (train_mlp.TRAIN_SPLIT_ALL = 6: train_fwd_sa_kernel on the gathered first
layers and the ragged plain widths, train_dgrad_sa_kernel on the ragged dgrads, the layers TRAIN_SPLIT already takes on its
kernels, one train_pack_split_all_kernel launch per call; csrc/mlp_train.h) against float64, entry by entry, on the cases of
tests/train_split_all_cases.py.

Every case runs tests/test_gpu_train_stack_f64.py's own comparison (test_case_equals_float64_closed_form is called as it is, with
the attribute on): decisions shared with the device, and that file's bars, unchanged -- the split must be fp32-grade:
  saved y of every layer        per entry 1e-5 sum |a| |w|
  constant rows, output rows, running statistics    1e-5 max(1, max |ref|)
  every gradient                1e-4 max(1, max |ref|);  dW / input gradients per entry: entry_ratio <= ratio_bar (8 x CPU_F32_RATIO)
  untouched memory              gout is a slice of a NaN-framed buffer there; nothing the caller reads may be NaN
  worst seen with the attribute on (one MI355X):
      saved y 5.4e-07 sum |a| |w|;  dW ratio 6.0e-06 (bar 3.3e-05);  input gradient ratio 6.2e-07 (bar 1.3e-05);  whole RPN step: loss
      equal to nine digits, worst parameter-gradient distance 1.2e-03 in norm (bar 5e-3);  whole RCNN step: nine digits, 9.8e-07
Which kernel each layer of each case gets is proven on the CPU (tests/test_train_split_all_cpu.py).

Further:
  * the split is in use and changes only arithmetic: a grouped and an interpolated case, attribute off against on -- the dumped
    first-layer rows (a_dump, read by wgrad and by the row-gradient scatter) are the same bytes, the saved y of layer 0 differs
    in at least one bit; a layer that stays fp32 (the K = 19 grouped layer 0, the K = 28 plain layer 0) and its statistics are
    bit-identical;
  * the split images the device built are the bytes of the numpy twin (tests/test_train_split_all_cpu.py: rotation, zero
    padding, the xyz columns left out of the transposed image);
  * two runs with the attribute on are bit-identical (the wide grouped stack and its padding-free twin): output, every saved y,
    every parameter gradient, the statistics, and the padding-free stack's feature gradient; the padded grouped source's feature
    gradient comes from an atomicAdd scatter outside the stack (under every arithmetic) and is held to 1e-5 of its largest entry:
    a point is gathered by 8 rows on average here (3 200 rows per frame over 400 points), by a few dozen at most, and n fp32
    additions in another order differ by at most n x 2^-24 of the sum of their magnitudes -- 64 x 2^-24 = 3.8e-6;
  * a +inf in one gathered feature (group, K = 35, no BatchNorm) makes exactly the rows that gather that point non-finite in y and
    leaves every other row inside the bar -- ordinary IEEE data, the rule of the kernels' header comment;
  * padding stays zero: plain [36, 32] at 129 rows whose input rows are a slice of a NaN-framed buffer (NaN behind every row's
    36 floats, before the first row and after the last): everything the caller reads is finite and inside the bars;
  * one whole RPN training step and one RCNN training step, attribute on against off, within the bars of
    tests/test_gpu_train_rcnn.py: loss 1e-5 max(1, |loss|), every parameter gradient 5e-3 in norm;
  * with the attribute off the new entry points are never reached."""
import pytest
import torch

import test_gpu_train_stack_f64 as F
import test_train_split_all_cpu as C
import train_split_all_cases as A
import train_stack_cases as T
from train_stack_cases import F64

pytestmark = [pytest.mark.gpu, pytest.mark.own_arithmetic]


@pytest.fixture
def all_on(monkeypatch):
    from pointrcnn_amd import train_mlp
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_ALL", 6)


@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_split_all_case_equals_float64_closed_form(dev, case, all_on):
    F.test_case_equals_float64_closed_form(dev, case)


@pytest.mark.parametrize("name", ["a_interp_72", "a_wide_6017"])
def test_with_the_wgrad_split_as_well(dev, name, all_on, monkeypatch):
    """TRAIN_SPLIT_WGRAD composes: the cases with a wide (K > 64, N > 64) layer, wgrad_split = 1 through the one backward entry"""
    from pointrcnn_amd import train_mlp
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", 6)
    F.test_case_equals_float64_closed_form(dev, A.BY_NAME[name])


class _Spy:
    """what a SharedMLPTrain invocation keeps for itself: the dumped first-layer rows and the split images, copied around backward"""

    def __init__(self, monkeypatch):
        from pointrcnn_amd import train_mlp
        self.a_dump, self.images = None, None
        inner = train_mlp.SharedMLPTrain.backward
        spy = self

        def backward(ctx, gout):
            st = ctx.st
            spy.a_dump = None if ctx.a_dump is None else ctx.a_dump.clone()
            res = inner(ctx, gout)
            torch.cuda.synchronize()
            if st.wsplit is not None:
                base = st.sbuf.data_ptr()
                buf = st.sbuf.cpu().numpy()
                off = lambda p: None if not p else int(p) - base                 # noqa: E731
                spy.images = (buf, [off(st.wsplit[l]) for l in range(st.nl)], [off(st.wsplit_t[l]) for l in range(st.nl)])
            return res
        monkeypatch.setattr(train_mlp.SharedMLPTrain, "backward", staticmethod(backward))


@pytest.mark.parametrize("name,fp32_name", [("a_group_35", "a_group_19"), ("a_interp_37", "a_rows_129")])
def test_the_split_is_in_use_and_changes_only_arithmetic(dev, name, fp32_name, monkeypatch):
    from pointrcnn_amd import train_mlp
    spy = _Spy(monkeypatch)
    case, keep = A.BY_NAME[name], A.BY_NAME[fp32_name]
    assert A.EXPECT[name][0][0].startswith("train_fwd_sa_kernel") and A.EXPECT[fp32_name][0][0].startswith("train_fwd_kernel")
    runs, dumps, kept = {}, {}, {}
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_ALL", terms)
        runs[terms] = F._run(case, T.build_inputs(case), dev)
        dumps[terms] = spy.a_dump.cpu()
        kept[terms] = F._run(keep, T.build_inputs(keep), dev)
    assert dumps[0].shape[0] == case.rows and dumps[0].shape[1] >= case.chans[0]
    assert torch.equal(dumps[0].view(torch.int32), dumps[6].view(torch.int32)), "a_dump is not the fp32 kernel's bytes"
    assert not torch.equal(runs[0].y[0], runs[6].y[0]), "the saved y of the gathered layer 0 is the fp32 kernel's, bit for bit"
    off, on = kept[0], kept[6]
    assert torch.equal(off.y[0], on.y[0]) and torch.equal(off.cst[0], on.cst[0]), "a layer that stays fp32 changed"
    assert torch.equal(off.run_mean[0], on.run_mean[0]) and torch.equal(off.run_var[0], on.run_var[0])
    assert not torch.equal(off.y[1], on.y[1])                    # (its ragged second layer is split)


def test_the_device_images_are_the_numpy_twin(dev, all_on, monkeypatch):
    """a_group_61: layer 0 is grouped, K = 61 (rotation 3, padded to 64), N = 32; layer 1 K = 32, N = 36 (its transposed image is
    padded in N to 64)"""
    import numpy as np
    spy = _Spy(monkeypatch)
    case = A.BY_NAME["a_group_61"]
    I = T.build_inputs(case)
    F._run(case, I, dev)
    buf, fwd, bwd = spy.images
    assert all(o is not None for o in fwd + bwd)
    for l, W in enumerate(I.W):
        rot = 3 if l == 0 else 0
        for o, transposed in ((fwd[l], False), (bwd[l], True)):
            want = C.twin_bytes(C.twin_planes(W.numpy(), rot, transposed))
            assert np.array_equal(buf[o: o + want.size], want), "layer %d %s image" % (l, "transposed" if transposed else "forward")


@pytest.mark.parametrize("name", A.REPEAT_CASES)
def test_two_runs_are_bit_identical(dev, name, all_on):
    case = A.BY_NAME[name]
    I = T.build_inputs(case)
    a, b = F._run(case, I, dev), F._run(case, I, dev)
    assert torch.equal(a.out, b.out)
    nlive = T.Rows(case, I).live.numel()                       # (rows past the live ones are never written)
    for l, (ya, yb) in enumerate(zip(a.y, b.y)):
        assert torch.equal(ya[:nlive], yb[:nlive]), "saved y of layer %d" % l
    for l, (ga, gb) in enumerate(zip(a.grads, b.grads)):
        assert (ga is None and gb is None) or torch.equal(ga, gb), "parameter gradient %d of layer %d" % (l % 3, l // 3)
    # the feature gradient: the padded grouped source scatters the row gradients with atomicAdd (prcnn_group_rows_grad, in any
    # arithmetic: its order is not fixed, and it is no part of the stack), the padding-free one gathers them in row order when the
    # feature rows are 16-byte pieces (C = 32 here) -- there the row gradients of layer 0's dgrad are compared bit for bit through it
    if case.source == "flat":
        assert case.chans[0] % 4 == 3 and torch.equal(a.gx0, b.gx0)
    else:
        assert float((a.gx0 - b.gx0).abs().max()) <= 1e-5 * float(a.gx0.abs().max())
    for ma, mb in zip(a.run_mean + a.run_var, b.run_mean + b.run_var):
        assert torch.equal(ma, mb)


def test_a_non_finite_operand_stays_in_its_rows(dev, all_on):
    """group [35, 32], no BatchNorm, unpooled, one +inf in feature 5 of point 17 of frame 0: exactly the rows that gather that point
    are non-finite in y, every other row meets the bar"""
    case = T.Case("a_inf_rows", "group", [35, 32], bn=False, B=2, N=100, M=12, ns=8)
    assert case.chans[0] >= 32
    I = T.build_inputs(case)
    I.idx[0, 0, 0] = 17                                          # (the point is gathered at least once)
    I.x0[0, 17, 5] = float("inf")
    r = F._run(case, I, dev)
    y = r.y[0]
    hit = torch.zeros_like(I.idx, dtype=torch.bool)
    hit[0] = I.idx[0] == 17
    hit = hit.reshape(-1)
    assert 0 < int(hit.sum()) < hit.numel()
    assert bool((~torch.isfinite(y[hit])).all()), "a row that gathers the +inf is finite somewhere"
    a = T.first_rows(case, I, F64)[~hit]
    w = I.W[0].to(F64)
    want, bar = a @ w.t(), 1e-5 * (a.abs() @ w.abs().t())
    assert bool(torch.isfinite(y[~hit]).all()), "a row that does not gather the +inf is not finite"
    over = (y[~hit].to(F64) - want).abs() - bar
    assert float(over.max()) <= 0.0, float(over.max())


def test_padding_stays_zero_next_to_nan(dev, all_on, monkeypatch):
    """plain [36, 32] at 129 rows (the forward reduces over a ragged K = 36: two chunks, the second 4 wide), the input rows laid out
    in a NaN-framed buffer: row stride 40 with NaN in the four floats behind every row, a NaN row before the first and after the last.
    Everything the caller reads is finite and inside the bars of the float64 comparison"""
    from pointrcnn_amd import train_mlp
    case = T.Case("a_nan_frame", "plain", [36, 32], R=129)
    inner = train_mlp._rows2
    seen = []

    def framed(t):
        R, K = t.shape
        buf = torch.full((R + 2, K + 4), float("nan"), dtype=t.dtype, device=t.device)
        buf[1:R + 1, :K] = t.detach()
        v = buf[1:R + 1, :K]
        assert v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 0
        seen.append(v)
        return inner(v)                                           # (taken as it is: aligned, unit channel stride)
    monkeypatch.setattr(train_mlp, "_rows2", framed)
    F.test_case_equals_float64_closed_form(dev, case)
    assert seen and all(bool(torch.isnan(v._base if v._base is not None else v).any()) for v in seen)


def _step_distance(out):
    (l0, g0), (l6, g6) = out[0], out[6]
    assert abs(l6 - l0) <= 1e-5 * max(1.0, abs(l0)), (l6, l0)
    assert sorted(g0) == sorted(g6) and len(g0) > 10
    rel = {n: float((g6[n] - g0[n]).norm() / g0[n].norm().clamp(min=1e-12)) for n in g0}
    print("\nwhole step: loss off %.9g on %.9g; worst gradient distance in norm %.3e (%s)" % ((l0, l6) + max((v, k) for k, v in rel.items())))
    assert any(not torch.equal(g0[n], g6[n]) for n in g0), "the split arithmetic was not in use"
    assert max(rel.values()) <= 5e-3, max(rel.items(), key=lambda kv: kv[1])


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
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_ALL", terms)
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
    _step_distance(out)


def test_one_whole_rcnn_step_on_against_off(dev, monkeypatch):
    """the RCNN training step of tests/test_gpu_train_rcnn.py (fixed RPN -> proposals -> device ProposalTargetLayer -> RCNNNet ->
    loss -> backward), same weights, same sampled RoIs: loss and rcnn_net parameter gradients with the attribute on against off"""
    from test_gpu_train_rcnn import _pm, _rcnn_batch
    _pm()
    from pointrcnn_amd import point_rcnn, rpn, train_functions as tf, train_mlp
    torch.manual_seed(11)
    model = point_rcnn.PointRCNN(mode="TRAIN").to(dev)
    rpn.randomize_bn_stats(model.rpn, seed=3)
    batch = _rcnn_batch(dev)
    out, rois = {}, {}
    for terms in (0, 6):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_ALL", terms)
        model.train()
        model.zero_grad(set_to_none=True)
        model.rcnn_net.proposal_target_layer.seed = 21
        torch.manual_seed(77)                                  # the elementwise RoI augmentation draws from torch's generator
        res = model(batch)
        loss = tf.get_rcnn_loss(res, model.rcnn_cfg)
        loss.backward()
        rois[terms] = res["roi_boxes3d"].clone()
        out[terms] = (float(loss.item()), {n: p.grad.double().clone() for n, p in model.rcnn_net.named_parameters() if p.grad is not None})
    assert torch.equal(rois[0], rois[6])                       # (the RPN runs in evaluation mode: the same proposals)
    _step_distance(out)


def test_default_route_does_not_reach_the_new_entry_points(dev, monkeypatch):
    from pointrcnn_amd import _cabi, train_mlp

    def boom(*a, **k):
        raise AssertionError("a split-all entry point ran without being asked for")
    L = _cabi.lib()
    for name in ("prcnn_train_stack_fwd_split_all", "prcnn_train_stack_bwd_split_all"):
        assert callable(getattr(L, name))
        monkeypatch.setattr(L, name, boom)
    assert train_mlp.TRAIN_SPLIT_ALL == 0                      # the variable unset: off
    case = A.BY_NAME["a_rows_129"]
    I = T.build_inputs(case)
    for split, wgrad in ((0, 0), (6, 0), (6, 6), (0, 6)):
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT", split)
        monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_WGRAD", wgrad)
        r = F._run(case, I, dev)
        assert r.gx0 is not None and bool(torch.isfinite(r.out).all())
    monkeypatch.setattr(train_mlp, "TRAIN_SPLIT_ALL", 6)
    with pytest.raises(AssertionError, match="without being asked"):
        F._run(case, I, dev)
