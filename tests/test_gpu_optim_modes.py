"""GPU: the device route of TRAIN.OPTIMIZER adam and sgd (csrc/optim.hip through ops.optim_step_adam / ops.optim_step_sgd and
optim.ClipAdam / optim.ClipSGD), and the train loop (pointrcnn_amd/train_loop.py) on the device.

  element update   p, m, v equal the host build of csrc/optim_math.h (tests/optim_modes_host.cpp) BIT FOR BIT: both modes, the
                   16-byte and the 4-byte path, two steps, tensors without gradient, wd 0 and 0.001, momentum 0 and 0.9
  norm and coef    the bits of the adam_onecycle path on the same gradients
  whole step       ClipAdam / ClipSGD(fused=True) on rpn.RPN()'s parameter list against stock torch on float64 CPU copies, within
                   8 x torch's own float32-against-float64 figures (the bar of tests/test_optim_modes_cpu.py)
  schedules        a scheduler's change of lr is used by the next step; BatchNorm momentum reaches the hand-written stacks
  train loop       two epochs with RPNTrainer and each optimizer; checkpoints; no host read inside an iteration
  routes           defaults, "sgd" and "adam_onecycle" do not reach the new entry points

Every test runs under both mlp_modes of the suite; the arithmetic mode does not reach the optimizer kernels."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_modes_cases as mc
from pointrcnn_amd import ops, optim
from pointrcnn_amd import train_functions as tf
from test_gpu_optim import carve, tables

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = ("adam", "sgd")
SIZES = oc.SIZES


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    work = tmp_path_factory.mktemp("optim_modes_host_gpu")
    return mc.build_host(work, False), work


def dev_step(mode):
    return ops.optim_step_adam if mode == "adam" else ops.optim_step_sgd


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("mode", MODES)
def test_element_update_equals_the_host_build_bit_for_bit(dev, host, mode, shift):
    exe, work = host
    params, grads = oc.case("clip", sizes=SIZES, steps=2)
    coefs = [F32(1.0), F32(0.37)]
    has_grad = [k % 4 != 2 for k in range(len(SIZES))]                          # 1, 1, 0, 1, ...
    zeros = [np.zeros(n, F32) for n in SIZES]
    for wd in (0.0, mc.WD):
        for momentum in ((0.0, mc.MOMENTUM) if mode == "sgd" else (None,)):
            sc = [mc.scalars(mode, t, wd=wd, **({} if momentum is None else {"momentum": momentum})) for t in (1, 2)]
            hp, hm, hv, _, _ = mc.run_host(exe, work, mode, params, grads, sc, coefs=coefs, has_grad=has_grad)
            pbuf, p = carve(params, 0, shift, dev)
            mbuf, m = carve(zeros, 2, shift, dev)
            vbuf, v = carve(zeros, 3, shift, dev)
            kinds = set()
            for t in range(2):                                                  # the second step starts from non-zero moments
                gbuf, g = carve(grads[t], 1, shift, dev)
                gl = [x if has_grad[k] else None for k, x in enumerate(g)]
                for k in range(len(SIZES)):
                    if has_grad[k]:
                        kinds.add((SIZES[k] > 4, all(x[k].data_ptr() % 16 == 0 for x in (p, g, m, v))))
                table, chunks = tables(p, gl, m, v, dev)
                before = gbuf.clone()
                dev_step(mode)(table, chunks, sc[t], coef=torch.tensor([coefs[t]], dtype=torch.float32, device=dev))
                assert torch.equal(gbuf, before)                                # the gradient is read, never written
            assert kinds >= {(True, True), (True, False)}                       # both access paths ran on real sizes
            for k, n in enumerate(SIZES):
                for name, got, want in (("p", p[k], hp[k]), ("m", m[k], hm[k]), ("v", v[k], hv[k])):
                    got = got.cpu().numpy()
                    assert got.tobytes() == want.tobytes(), (mode, wd, momentum, name, k, n, int((got != want).sum()))
                if not has_grad[k]:                                             # not touched at all
                    assert p[k].cpu().numpy().tobytes() == params[k].tobytes() and not m[k].any() and not v[k].any()
            assert any(x.any() for x in m) == (momentum != 0.0) and any(x.any() for x in v) == (mode == "adam")
            for buf, views in ((pbuf, p), (mbuf, m), (vbuf, v)):                # nothing outside the tensors was written
                mask = torch.ones_like(buf, dtype=torch.bool)
                for x in views:
                    o = (x.data_ptr() - buf.data_ptr()) // 4
                    mask[o:o + x.numel()] = False
                assert not buf[mask].any()


@pytest.mark.parametrize("name", ["clip", "noclip"])
def test_norm_and_coefficient_have_the_bits_of_the_existing_path(dev, name):
    params, grads = oc.case(name, sizes=SIZES, steps=1)
    zeros = [np.zeros(n, F32) for n in SIZES]
    states = []
    for step, still in ((ops.optim_step, (1.0, 0.1, 0.99, 0.01, 0.1, 1e-8, 0.0)),
                        (ops.optim_step_adam, (0.001, 0.1, 0.99, 0.01, 0.1, 1e-8, 0.0)), (ops.optim_step_sgd, (0.001, 0.9, 0.0))):
        _, p = carve(params, 0, 0, dev)
        _, g = carve(grads[0], 1, 0, dev)
        _, m = carve(zeros, 2, 0, dev)
        _, v = carve(zeros, 3, 0, dev)
        gl = [x if k != 4 else None for k, x in enumerate(g)]
        table, chunks = tables(p, gl, m, v, dev)
        part = ops.optim_grad_norm(table, chunks)
        states.append(step(table, chunks, still, partial=part, max_norm=oc.MAX_NORM).cpu().numpy())
        assert all(torch.equal(a, torch.from_numpy(b).to(dev)) for a, b in zip(p, params))     # a zero rate moves nothing
    assert states[0][0] > 0 and (states[0][1] < 0.25 if name == "clip" else states[0][1] == 1)
    assert states[1].tobytes() == states[0].tobytes() and states[2].tobytes() == states[0].tobytes()


@pytest.fixture(scope="module")
def rpn_case():
    """rpn.RPN()'s trainable parameters and three sets of gradients on the CPU, with stock torch's float64 and float32 runs"""
    from pointrcnn_amd import rpn
    torch.manual_seed(5)
    init = [p.detach().clone() for p in rpn.RPN().parameters() if p.requires_grad]
    gen = torch.Generator().manual_seed(9)
    grads = [[torch.randn(p.shape, generator=gen) * 0.01 for p in init] for _ in range(3)]
    runs = {}
    for mode in MODES:
        for dtype in (torch.float64, torch.float32):
            ps = [torch.nn.Parameter(p.clone().to(dtype)) for p in init]
            opt = mc.make_optimizer(mode, ps, True)
            for gs in grads:
                for p, g in zip(ps, gs):
                    p.grad = g.to(dtype, copy=True)                            # clip_grad_norm_ rescales it in memory
                norm = float(torch.nn.utils.clip_grad_norm_(ps, oc.MAX_NORM))
                opt.step()
            runs[mode, dtype] = ([p.detach().reshape(-1).numpy() for p in ps],) + tuple(
                [a.reshape(-1) for a in x] for x in mc.state_arrays(mode, opt, ps)) + (norm,)
    return init, grads, runs


@pytest.mark.parametrize("mode", MODES)
def test_whole_step_on_the_rpn_parameter_list(dev, rpn_case, mode):
    init, grads, runs = rpn_case
    sizes = [p.numel() for p in init]
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
    opt = mc.make_optimizer(mode, ps, False, fused=True)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dev)
        kept = [p.grad.clone() for p in ps]
        opt.step()
        assert all(torch.equal(p.grad, k) for p, k in zip(ps, kept))           # .grad keeps its unclipped values
    r64, r32 = runs[mode, torch.float64], runs[mode, torch.float32]
    n32 = float(opt.last_grad_norm)
    assert r64[3] > 2 * oc.MAX_NORM and abs(n32 - r64[3]) <= 2e-7 * r64[3], (n32, r64[3])
    assert 1 <= opt.table_uploads <= 3
    m, v = mc.state_arrays(mode, opt, ps)
    got = ([p.detach().reshape(-1).cpu().numpy() for p in ps], m, v)
    e = oc.errors(got[0], got[1], got[2], r64[0], r64[1], r64[2], 3 * mc.LR, sizes=sizes)
    yard = oc.errors(r32[0], r32[1], r32[2], r64[0], r64[1], r64[2], 3 * mc.LR, sizes=sizes)
    k = 3 if mode == "adam" else 2
    print("whole step %s, %d tensors, %d elements: figures %s; torch float32 %s, bar 8 x" % (mode, len(ps), sum(sizes), e[:k], yard[:k]))
    assert all(yard[i] > 0 and e[i] <= oc.MARGIN * yard[i] for i in range(k)), (e, yard)
    if mode == "adam":
        assert all(int(opt.state[p]["step"]) == 3 for p in ps)
    # the same gradient tensors again: the pointers did not change, so the table is not uploaded again
    n = opt.table_uploads
    opt.step()
    assert opt.table_uploads == n


@pytest.mark.parametrize("mode", MODES)
def test_a_schedulers_change_of_lr_is_used_by_the_next_step(dev, host, mode):
    exe, work = host
    params, grads = oc.case("noclip", sizes=SIZES, steps=2)
    rates = [mc.LR, mc.LR * 0.25]
    want = mc.run_host(exe, work, mode, params, grads, [mc.scalars(mode, t + 1, lr=rates[t]) for t in range(2)], max_norm=None)
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in params]
    opt = mc.make_optimizer(mode, ps, False, max_norm=None, fused=True)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.25 ** epoch)
    for t in range(2):
        assert opt.param_groups[0]["lr"] == rates[t]
        for p, g in zip(ps, grads[t]):
            p.grad = torch.from_numpy(g.copy()).to(dev)
        opt.step()
        sched.step()
    assert opt.last_grad_norm is None
    m, v = mc.state_arrays(mode, opt, ps)
    for got, ref in (([p.detach().cpu().numpy() for p in ps], want[0]), (m, want[1]), (v, want[2])):
        assert oc.flat(got).tobytes() == oc.flat(ref).tobytes()
    stale = mc.run_host(exe, work, mode, params, grads, [mc.scalars(mode, t + 1) for t in range(2)], max_norm=None)
    assert oc.flat(stale[0]).tobytes() != oc.flat(want[0]).tobytes()


def test_steps_that_differ_take_the_composed_route(dev):
    ps = [torch.nn.Parameter(torch.ones(5, device=dev)) for _ in range(2)]
    ps[0].grad = torch.ones(5, device=dev)
    opt = optim.ClipAdam(ps, lr=0.01, grad_norm_clip=1.0)
    opt.step()                                                                  # only the first tensor has a step now
    assert opt.table_uploads == 1
    ps[1].grad = torch.ones(5, device=dev)
    opt.step()                                                                  # steps 1 and 0: composed
    assert opt.table_uploads == 1 and int(opt.state[ps[0]]["step"]) == 2 and int(opt.state[ps[1]]["step"]) == 1
    opt.fused = True
    with pytest.raises(RuntimeError, match="share one"):
        opt.step()


# ---------------------------------------------------------------------------------------------- schedules, loop, routes
def _rpn_and_batch(dev):
    """-> (a function building the RPN of make_golden's TRAIN_CASE on the device, that case's batch)"""
    from test_gpu_round2 import T, _Wrap, _fill
    from make_golden import TRAIN_CASE, train_batch
    from pointrcnn_amd import rpn
    pts, gt, cls, reg = train_batch(TRAIN_CASE)

    def model(fill=True):
        m = rpn.RPN()
        if fill:
            _fill(_Wrap(m), TRAIN_CASE["wseed"])
        return m.to(dev)
    return model, {"pts_input": T(pts, dev), "rpn_cls_label": T(cls, dev), "rpn_reg_label": T(reg, dev)}


def test_bn_momentum_reaches_the_hand_written_stacks(dev):
    """running_mean' = (1 - momentum) * running_mean + momentum * batch_mean, so one step at half the momentum moves every
    running_mean half as far.  Tolerance: each run rounds its update once or twice in float32 relative to the larger of
    |running_mean| and |momentum * batch_mean|, and the batch means of two runs may differ in their last bits; 16 ulps of the
    largest magnitude involved (|running_mean|, |batch_mean|) covers both with room, and is far below a wrong factor's effect."""
    from pointrcnn_amd import train_loop as tl
    make, batch = _rpn_and_batch(dev)
    moved = {}
    for momentum in (0.1, 0.05):
        model = make()
        sched = tl.BNMomentumScheduler(model, lambda it: 0.1 if it < 3 else 0.05)
        bns = [m for m in model.modules() if isinstance(m, tl.BN_TYPES)]
        assert bns and all(m.momentum == 0.1 for m in bns)
        if momentum != 0.1:
            sched.step(3)
        assert all(m.momentum == momentum for m in bns)
        before = [m.running_mean.clone() for m in bns]
        tf.RPNTrainer(model).step(batch)
        moved[momentum] = [(b.double().cpu(), (m.running_mean.double() - b.double()).cpu()) for b, m in zip(before, bns)]
    worst = 0.0
    for (rm, full), (_, half) in zip(moved[0.1], moved[0.05]):
        scale = float(torch.maximum(rm.abs(), (rm + full / 0.1).abs()).max())
        assert float(full.abs().max()) > 0
        err = float((half - 0.5 * full).abs().max())
        worst = max(worst, err / (scale * 2.0 ** -24))
        assert err <= 16 * 2.0 ** -24 * scale, (err, scale)
    print("BatchNorm momentum 0.05 against 0.1 over %d layers: worst deviation %.2f ulps of the layer's scale (bar 16)" % (len(moved[0.1]), worst))


@pytest.mark.parametrize("name", ["adam", "sgd", "adam_onecycle"])
def test_train_loop_on_the_device(dev, tmp_path, name):
    from pointrcnn_amd import train_loop as tl

    class cfg(tl.TrainConfig):
        OPTIMIZER = name
    make, batch = _rpn_and_batch(dev)
    model = make()
    opt = tl.create_optimizer(cfg, [p for p in model.parameters() if p.requires_grad], total_steps=4)
    sched, bnm = tl.create_scheduler(cfg, opt, model)
    trainer = tf.RPNTrainer(model, optimizer=opt)
    assert trainer.optimizer is opt
    tb_rows = []

    class Tb:
        def add_scalar(self, tag, value, step):
            tb_rows.append((tag, float(value), step))
    loop = tl.TrainLoop(trainer, opt, sched, bnm, str(tmp_path), tb_log=Tb(), log_interval=100)
    before = [p.detach().clone() for p in model.parameters()]
    assert loop.train(0, 0, 2, [batch, batch], ckpt_save_interval=1) == 4
    # nothing was read from the device inside an iteration: log_interval exceeds the run, so the ring left twice, at the epochs' ends
    assert loop.host_reads == 2
    losses = [v for t, v, _ in tb_rows if t == "train_loss"]
    norms = [v for t, v, _ in tb_rows if t == "grad_norm"]
    assert len(losses) == 4 and np.isfinite(losses).all() and loop.last_loss == losses[-1]
    assert len(norms) == 4 and np.isfinite(norms).all() and min(norms) > 0
    assert opt.table_uploads >= 1                                               # the device route ran
    assert all(not torch.equal(a, b) for a, b in zip(before, model.parameters()) if b.requires_grad)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert sorted(p.name for p in tmp_path.iterdir()) == ["checkpoint_epoch_1.pth", "checkpoint_epoch_2.pth"]
    fresh = make(fill=False)
    opt2 = tl.create_optimizer(cfg, [p for p in fresh.parameters() if p.requires_grad], total_steps=4)
    assert tl.load_checkpoint(fresh, opt2, str(tmp_path / "checkpoint_epoch_2.pth")) == (4, 2)
    want, got = model.state_dict(), fresh.state_dict()
    assert list(want) == list(got) and all(torch.equal(want[k], got[k]) for k in want)
    a, b = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert sorted(a) == sorted(b) and all(torch.equal(torch.as_tensor(a[k][key]).cpu(), torch.as_tensor(b[k][key]).cpu())
                                          for k in a for key in a[k])


def test_default_routes_do_not_reach_the_new_entry_points(dev, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the adam / sgd kernels ran without being asked for")
    for name in ("optim_step_adam", "optim_step_sgd"):
        assert callable(getattr(ops, name))
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(tf, "TRAIN_OPTIMIZER", "")
    model = torch.nn.Linear(7, 3).to(dev)
    for kw, cls in (({}, torch.optim.AdamW), ({"optimizer": "sgd"}, torch.optim.SGD),
                    ({"optimizer": "adam_onecycle", "total_steps": 10}, optim.OneCycleAdam)):
        opt = tf.RPNTrainer(model, **kw).optimizer
        assert type(opt) is cls
        before = model.weight.detach().clone()
        model.zero_grad()
        model(torch.ones(2, 7, device=dev)).sum().backward()
        opt.step()
        assert not torch.equal(before, model.weight)
    with pytest.raises(AssertionError, match="without being asked"):            # ... and the new classes do
        opt = optim.ClipSGD(model.parameters(), lr=0.1, grad_norm_clip=1.0)
        opt.step()
