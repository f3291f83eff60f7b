"""GPU: the training heads' device tail (csrc/head_tail.hip: Dropout keyed by a counter + the output layer) against a float64 closed
form that takes its mask from the PYTHON twin (train_mlp.head_keep_mask), so that one wrong mask bit is an O(1) error.

Cases (R, K, N, p, bias): the smallest shape, partial row tiles, p = 0 without bias, the widest N with the RCNN K, and two with
R = 3 * ops.HEAD_TAIL_PART_ROWS + 5 rows (three full partial tiles of the backward and a ragged fourth, so that the fixed-order
reduce and the last tile are both reached).  Every case also runs with g as a column slice of a wider buffer whose other columns are
NaN, and with gx, gw, gb null in turn.

Bars (those of tests/test_gpu_train_stack_f64.py):
  out             per entry 1e-5 (sum_k |drop(x)| |w| + |b|)
  every gradient  1e-4 max(1, max |ref|)
  gw, gx          additionally per entry |got - ref| / S, S = the float64 sum of the absolute values of the entry's terms: at most 8 x
                  the worst ratio of a plain float32 CPU evaluation of the same closed form over these cases, never less than 2^-20
                  (8 x: one fp32 accumulator takes up to 512 rows where a CPU BLAS sums in short blocks).
                    float32 on the CPU:  gw 2.09e-07 (65x256x46)    gx 2.91e-07 (1541x128x76)      bars: gw 1.67e-06   gx 2.33e-06
                    device, worst seen:  gw 2.25e-07 (257x256x96)   gx 2.91e-07 (1541x128x76)      out: 2.38e-07 of its bar's unit
                    (sum |drop(x)| |w| + |b|; 1541x128x76).  gx sums at most 96 terms, so device and CPU agree to the digit shown.
Exactness: gx is exactly zero at every dropped entry; all outputs are byte-identical across two calls; a row of out has the same bytes
in a batch of R and of 2 R rows; nothing the caller reads is NaN; an Inf planted in a dropped entry of x changes nothing; arguments
outside the domain return an error status and launch nothing.
Wiring: the RPN heads through pytorch_utils.fused_sequential with the switch on against the composed path with F.dropout replaced by
the twin's mask; the call counter; the default route; one RPN training step replayed after load_dropout_state (the resume property)."""
import copy

import numpy as np
import pytest
import torch

from pointrcnn_amd import _cabi, ops, train_mlp

pytestmark = [pytest.mark.gpu, pytest.mark.own_arithmetic]

F64 = torch.float64
RP = 3 * ops.HEAD_TAIL_PART_ROWS + 5
assert RP <= 8192
CASES = [(1, 32, 1, 0.5, True), (31, 128, 76, 0.5, True), (33, 128, 1, 0.5, True), (65, 256, 46, 0.0, False),
         (257, 256, 96, 0.3, True), (RP, 128, 76, 0.5, True), (RP, 128, 4, 0.5, True)]
IDS = ["%dx%dx%d" % c[:3] for c in CASES]
FLOOR = 2.0 ** -20


def key_of(ci):
    return (ci, 70 + ci % 3, ci, CASES[ci][3])


class Ref:
    """seeded CPU inputs of a case, the twin's mask and the float64 closed form"""

    def __init__(self, ci):
        R, K, N, p, bias = CASES[ci]
        g = torch.Generator().manual_seed(100 + ci)
        self.x = torch.randn((R, K), generator=g)
        self.w = torch.randn((N, K), generator=g) * 0.2
        self.b = torch.randn((N,), generator=g) if bias else None
        self.g = torch.randn((R, N), generator=g)
        seed, stream, call, _ = key_of(ci)
        self.mask = torch.from_numpy(train_mlp.head_keep_mask(seed, stream, call, R, K, p))
        self.scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        x, w, gg = self.x.to(F64), self.w.to(F64), self.g.to(F64)
        self.dx = torch.where(self.mask, x * self.scale, torch.zeros((), dtype=F64))
        self.out = self.dx @ w.t() + (0 if self.b is None else self.b.to(F64))
        self.out_unit = self.dx.abs() @ w.abs().t() + (0 if self.b is None else self.b.to(F64).abs())
        self.gx = torch.where(self.mask, (gg @ w) * self.scale, torch.zeros((), dtype=F64))
        self.gx_S = torch.where(self.mask, (gg.abs() @ w.abs()) * self.scale, torch.zeros((), dtype=F64))
        self.gw = gg.t() @ self.dx
        self.gw_S = gg.abs().t() @ self.dx.abs()
        self.gb = gg.sum(0)
        # the same closed form in plain float32 on the CPU: the yardstick of the per-entry bars
        dx32 = torch.where(self.mask, self.x * torch.tensor(self.scale, dtype=torch.float32), torch.zeros(()))
        self.f32_gx = ratio(torch.where(self.mask, (self.g @ self.w) * torch.tensor(self.scale, dtype=torch.float32), torch.zeros(())), self.gx, self.gx_S)
        self.f32_gw = ratio(self.g.t() @ dx32, self.gw, self.gw_S)


def ratio(got, ref, S):
    """worst |got - ref| / S over the entries with S > 0; an entry with S == 0 has no terms and must be exactly zero"""
    got = got.detach().cpu().to(F64)
    assert bool((got[S == 0] == 0).all()), "an entry without terms is not exactly zero"
    live = S > 0
    return float(((got - ref).abs()[live] / S[live]).max()) if bool(live.any()) else 0.0


@pytest.fixture(scope="module")
def refs():
    return [Ref(ci) for ci in range(len(CASES))]


@pytest.fixture(scope="module")
def bars(refs):
    f32_gw, f32_gx = max(r.f32_gw for r in refs), max(r.f32_gx for r in refs)
    print("float32 on the CPU, worst ratio over the cases: gw %.2e  gx %.2e" % (f32_gw, f32_gx))
    return max(8 * f32_gw, FLOOR), max(8 * f32_gx, FLOOR)


def on(dev, t):
    return None if t is None else t.to(dev)


@pytest.fixture(scope="module")
def runs(dev, refs):
    """forward and backward of every case once: (x, w, b, g, out, gx, gw, gb) on the device"""
    res = []
    for ci, r in enumerate(refs):
        x, w, b, g = on(dev, r.x), on(dev, r.w), on(dev, r.b), on(dev, r.g)
        out = ops.head_tail_forward(x, w, b, key_of(ci))
        res.append((x, w, b, g, out) + ops.head_tail_backward(x, w, g, key_of(ci)))
    torch.cuda.synchronize()
    return res


def close(got, want, what):
    got = got.detach().cpu().to(F64)
    assert got.shape == want.shape and not bool(torch.isnan(got).any()), what
    err, bar = float((got - want).abs().max()), 1e-4 * max(1.0, float(want.abs().max()))
    assert err <= bar, (what, err, bar)


def same(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def test_part_rows_constant_is_the_kernels(dev):
    lib = _cabi.lib()
    tile = (76 * 128 + 76) * 4
    assert lib.prcnn_head_tail_work_bytes(ops.HEAD_TAIL_PART_ROWS, 128, 76) == tile
    assert lib.prcnn_head_tail_work_bytes(RP, 128, 76) == 4 * tile                 # three full partial tiles and a ragged fourth


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_case_equals_float64_closed_form(refs, bars, runs, ci):
    r = refs[ci]
    x, w, b, g, out, gx, gw, gb = runs[ci]
    o = out.cpu().to(F64)
    assert not bool(torch.isnan(o).any())
    unit = float(((o - r.out).abs() / r.out_unit.clamp(min=1e-300)).max())
    assert bool(((o - r.out).abs() <= 1e-5 * r.out_unit).all()), unit
    close(gx, r.gx, "gx"); close(gw, r.gw, "gw"); close(gb, r.gb, "gb")
    assert bool((gx.cpu()[~r.mask] == 0).all()), "gx is not exactly zero at a dropped entry"
    rw, rx = ratio(gw, r.gw, r.gw_S), ratio(gx, r.gx, r.gx_S)
    print("%s: out %.2e of sum |drop(x)| |w| + |b|; |err| / S: gw %.2e (float32 CPU %.2e, bar %.2e)  gx %.2e (float32 CPU %.2e, bar %.2e)"
          % (IDS[ci], unit, rw, r.f32_gw, bars[0], rx, r.f32_gx, bars[1]))
    assert rw <= bars[0] and rx <= bars[1]


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_strided_g_and_null_outputs(dev, refs, runs, ci):
    R, K, N, p, bias = CASES[ci]
    x, w, b, g, out, gx, gw, gb = runs[ci]
    wide = torch.full((R, N + 5), float("nan"), device=dev)
    wide[:, 3:3 + N] = g
    sx, sw, sb = ops.head_tail_backward(x, w, wide[:, 3:3 + N], key_of(ci))
    assert same(sx, gx) and same(sw, gw) and same(sb, gb)
    for skip in range(3):
        want = [k != skip for k in range(3)]
        got = ops.head_tail_backward(x, w, g, key_of(ci), *want)
        for k, (a, full) in enumerate(zip(got, (gx, gw, gb))):
            assert (a is None) if k == skip else same(a, full), (skip, k)
    assert ops.head_tail_backward(x, w, g, key_of(ci), False, False, False) == (None, None, None)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_two_calls_give_identical_bytes(runs, ci):
    x, w, b, g, out, gx, gw, gb = runs[ci]
    assert same(ops.head_tail_forward(x, w, b, key_of(ci)), out)
    ax, aw, ab = ops.head_tail_backward(x, w, g, key_of(ci))
    assert same(ax, gx) and same(aw, gw) and same(ab, gb)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_a_row_does_not_depend_on_the_batch_it_is_in(dev, runs, ci):
    R = CASES[ci][0]
    x, w, b, g, out = runs[ci][:5]
    more = torch.randn((R, x.shape[1]), generator=torch.Generator().manual_seed(7)).to(dev)
    both = ops.head_tail_forward(torch.cat([x, more]), w, b, key_of(ci))
    assert same(both[:R].contiguous(), out)


@pytest.mark.parametrize("ci", [1, 2, 4, 5], ids=[IDS[i] for i in (1, 2, 4, 5)])
def test_inf_in_a_dropped_entry_contributes_nothing(refs, runs, ci):
    x, w, b, g, out, gx, gw, gb = runs[ci]
    dropped = (~refs[ci].mask).nonzero()
    assert len(dropped) > 0
    xi = x.clone()
    for r, k in dropped[:: max(1, len(dropped) // 50)].tolist():
        xi[r, k] = float("inf") if (r + k) % 3 else float("nan")
    assert not bool(torch.isfinite(xi).all())
    oi = ops.head_tail_forward(xi, w, b, key_of(ci))
    assert bool(torch.isfinite(oi).all()) and same(oi, out)
    ix, iw, ib = ops.head_tail_backward(xi, w, g, key_of(ci))
    assert same(ix, gx) and same(iw, gw) and same(ib, gb)
    di = ops.dropout_rows(xi, key_of(ci))
    assert bool(torch.isfinite(di).all())


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_dropout_rows_is_the_twins_mask(refs, runs, ci):
    r = refs[ci]
    x = runs[ci][0]
    want = torch.where(r.mask, r.x * torch.tensor(r.scale, dtype=torch.float32), torch.zeros(()))
    got = ops.dropout_rows(x, key_of(ci))
    assert same(got.cpu(), want)                    # one float32 product per kept entry: exact
    assert same(ops.dropout_rows(x, key_of(ci)), got)


def test_outside_the_domain_is_an_error_and_nothing_is_launched(dev):
    lib = _cabi.lib()
    p = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    for R, K, N, prob in ((64, 48, 8, 0.5), (64, 128, 97, 0.5), (64, 128, 8, 1.0)):
        x, w, g = torch.ones((R, K), device=dev), torch.ones((N, K), device=dev), torch.ones((R, N), device=dev)
        out, gx = torch.full((R, N), -7.0, device=dev), torch.full((R, K), -7.0, device=dev)
        gw, gb = torch.full((N, K), -7.0, device=dev), torch.full((N,), -7.0, device=dev)
        work = torch.full((4 * (N * K + N),), -7.0, device=dev)
        assert lib.prcnn_head_tail_fwd(p(x), p(w), None, p(out), R, K, N, 0, 70, 0, prob, s) == -1
        assert lib.prcnn_head_tail_bwd(p(x), p(w), p(g), N, p(gx), p(gw), p(gb), p(work), work.numel() * 4, R, K, N, 0, 70, 0, prob, s) == -1
        torch.cuda.synchronize()
        for t in (out, gx, gw, gb, work):
            assert bool((t == -7.0).all())
        assert not ops.head_tail_supported(R, K, N, prob)
        with pytest.raises(_cabi.PointOpsError):
            ops.head_tail_forward(x, w, None, (0, 70, 0, prob))
    x = torch.ones((8, 6), device=dev)
    o = torch.full((8, 6), -7.0, device=dev)
    assert lib.prcnn_dropout_rows(p(x), p(o), 8, 6, 0, 70, 0, 0.5, s) == -1 and lib.prcnn_dropout_rows(p(x), p(o), 8, 8, 0, 70, 0, 1.0, s) == -1
    torch.cuda.synchronize()
    assert bool((o == -7.0).all())


# ---- wiring --------------------------------------------------------------------------------------------------------------------
def _pt():
    import pointnet2_lib.pointnet2.pytorch_utils as pt_utils
    return pt_utils


def _rpn_heads(dev):
    from pointrcnn_amd import rpn
    torch.manual_seed(3)
    model = rpn.RPN()
    return model, model.rpn_cls_layer.to(dev).train(), model.rpn_reg_layer.to(dev).train()


def _head_run(seq, x, gout):
    pt = _pt()
    x = x.clone().requires_grad_(True)
    y = pt.fused_sequential(seq, x)
    (y * gout).sum().backward()
    return y.detach(), x.grad, {n: q.grad.clone() for n, q in seq.named_parameters()}


def test_plans_on_the_device(dev):
    from pointrcnn_amd import rcnn
    pt = _pt()
    _, cls, reg = _rpn_heads(dev)
    for seq in (cls, reg):
        plan = pt._head_plan(seq, True)
        assert [s[0] for s in plan] == ["stack", "tail"] and plan[1][1].p == 0.5 and len(plan[0][1]) == 1
        assert [s[0] for s in pt._head_plan(seq, False)] == ["stack", "dropout", "linear"]
    net = rcnn.RCNNNet().to(dev).train()
    for seq in (net.cls_layer, net.reg_layer):
        plan = pt._head_plan(seq, True)
        assert [s[0] for s in plan] == ["stack", "tail"] and plan[1][1] is None and len(plan[0][1]) == 2
        assert [s[0] for s in pt._head_plan(seq, False)] == ["stack", "dropout", "stack", "linear"]


def test_rpn_heads_with_the_switch_on_against_the_composed_path(dev, monkeypatch):
    pt = _pt()
    B, L = 2, 1024
    model, cls, reg = _rpn_heads(dev)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((B, 128, L), generator=gen).to(dev)
    for seq, stream in ((cls, 70), (reg, 71)):
        N = seq[2]._parts()[0].out_channels
        gout = torch.randn((B, N, L), generator=gen).to(dev)
        monkeypatch.setattr(pt, "HEAD_TAIL", True)
        assert pt.key_dropouts(model, 5) == {"rpn_cls_layer.1": 70, "rpn_reg_layer.1": 71}
        a, b = copy.deepcopy(seq), copy.deepcopy(seq)
        assert (a[1]._prcnn_stream, a[1]._prcnn_seed, a[1]._prcnn_calls) == (stream, 5, 0)
        keys = []
        real = ops.head_tail_forward
        monkeypatch.setattr(ops, "head_tail_forward", lambda x_, w_, b_, key: (keys.append(key), real(x_, w_, b_, key))[1])
        y_on, gx_on, gp_on = _head_run(a, x, gout)
        y_again = pt.fused_sequential(a, x).detach()
        monkeypatch.setattr(ops, "head_tail_forward", real)
        assert keys == [(5, stream, 0, 0.5), (5, stream, 1, 0.5)] and a[1]._prcnn_calls == 2
        assert float((y_again - y_on).abs().max()) > 1e-3            # the second forward drew another mask

        def twin_dropout(rows, p, training, inplace, stream=stream):
            assert training and p == 0.5
            m = torch.from_numpy(train_mlp.head_keep_mask(5, stream, 0, rows.shape[0], rows.shape[1], p)).to(rows.device)
            return torch.where(m, rows * 2.0, torch.zeros((), device=rows.device))
        monkeypatch.setattr(pt, "HEAD_TAIL", False)
        monkeypatch.setattr(pt.F, "dropout", twin_dropout)
        y_ref, gx_ref, gp_ref = _head_run(b, x, gout)
        monkeypatch.undo()
        assert y_on.shape == y_ref.shape == (B, N, L)
        assert float((y_on - y_ref).abs().max()) <= 1e-5 * max(1.0, float(y_ref.abs().max()))
        assert float((gx_on - gx_ref).abs().max()) <= 1e-4 * max(1.0, float(gx_ref.abs().max()))
        assert sorted(gp_on) == sorted(gp_ref) and len(gp_on) == 5
        for n in gp_ref:
            err, bar = float((gp_on[n] - gp_ref[n]).abs().max()), 1e-4 * max(1.0, float(gp_ref[n].abs().max()))
            assert err <= bar, (n, err, bar)


def test_default_route_does_not_reach_the_new_ops(dev, monkeypatch):
    pt = _pt()

    def boom(*a, **k):
        raise AssertionError("the device tail ran without being asked for")
    for name in ("head_tail_forward", "head_tail_backward", "dropout_rows"):
        assert callable(getattr(ops, name))
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(pt, "HEAD_TAIL", False)                         # the switch unset
    _, cls, reg = _rpn_heads(dev)
    x = torch.randn((2, 128, 256), generator=torch.Generator().manual_seed(1)).to(dev)
    for seq in (cls, reg):
        y, gx, gp = _head_run(seq, x, torch.ones((2, seq[2]._parts()[0].out_channels, 256), device=dev))
        assert gx is not None and len(gp) == 5
    monkeypatch.setattr(pt, "HEAD_TAIL", True)
    with pytest.raises(AssertionError, match="without being asked"):
        pt.fused_sequential(cls, x.clone().requires_grad_(True))


def test_a_training_step_is_replayed_after_load_dropout_state(dev, monkeypatch):
    """the resume property: the step's loss has the same bytes once the Dropout call counters are put back"""
    from test_gpu_round2 import T, _Wrap, _fill
    from make_golden import TRAIN_CASE, train_batch
    from pointrcnn_amd import rpn
    from pointrcnn_amd import train_functions as tf
    pt = _pt()
    monkeypatch.setattr(pt, "HEAD_TAIL", True)
    pts, gt, cls, reg = train_batch(TRAIN_CASE)
    model = rpn.RPN()
    _fill(_Wrap(model), TRAIN_CASE["wseed"])
    model = model.to(dev)
    batch = {"pts_input": T(pts, dev), "rpn_cls_label": T(cls, dev), "rpn_reg_label": T(reg, dev)}
    trainer = tf.RPNTrainer(model, ddp=False)
    trainer.model.train()
    saved = pt.dropout_state(model)
    assert saved == {"rpn_cls_layer.1": 0, "rpn_reg_layer.1": 0} and model.rpn_cls_layer[1]._prcnn_stream == 70

    def step():
        model.zero_grad(set_to_none=True)
        loss = trainer.loss(batch)
        loss.backward()
        return loss.detach().clone(), model.rpn_reg_layer[2]._parts()[0].weight.grad.clone()
    l1, g1 = step()
    assert pt.dropout_state(model) == {"rpn_cls_layer.1": 1, "rpn_reg_layer.1": 1}
    l2, g2 = step()                                      # the run goes on: other masks
    pt.load_dropout_state(model, saved)
    l3, g3 = step()
    assert bool(torch.isfinite(l1)) and not same(l2.view(1), l1.view(1))
    assert same(l3.view(1), l1.view(1)) and same(g3, g1)
