"""GPU: the device route of adam_onecycle (csrc/optim.hip through ops.optim_grad_norm / ops.optim_step and optim.OneCycleAdam).

  element update   the device's p, m, v equal the host build of csrc/optim_math.h (tests/optim_host.cpp) BIT FOR BIT, with the clip
                   coefficient supplied by the caller, tensors at mixed 4- / 8- / 16-byte alignments, one tensor without gradient
  norm pass        sum of g^2 against numpy float64 within n * 2^-53 relative (the bound of any float64 summation order of n
                   non-negative terms); two calls give the same bytes; coef is exactly the float32 expression of the device's own norm
  whole step       OneCycleAdam(fused=True) on rpn.RPN()'s parameter list against the float64 evaluation, within 8 x the reference's
                   own float32-against-float64 figures (tests/golden/optim_ref.npz; the bar of tests/test_optim_cpu.py)
  routes           the default trainer does not reach the new ops; one real RPNTrainer step with optimizer="adam_onecycle"
"""
import numpy as np
import pytest
import torch

import optim_cases as oc
from pointrcnn_amd import ops, optim
from pointrcnn_amd import train_functions as tf

pytestmark = pytest.mark.gpu

F32 = np.float32
CHUNK = ops.OPTIM_CHUNK
SIZES = oc.SIZES + (2 * CHUNK + 7,)
# float offsets (mod 4) of param, grad, exp_avg, exp_avg_sq inside their flat buffers: 0 = 16-byte, 2 = 8-byte, 1 / 3 = 4-byte aligned
ALIGN = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 2), (2, 2, 2, 2), (1, 2, 3, 0), (0, 0, 0, 0), (3, 3, 3, 3),
         (0, 1, 0, 0), (0, 0, 0, 0), (2, 0, 1, 0), (0, 0, 0, 0))
NO_GRAD = 4                                     # the tensor without gradient (63 elements)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    work = tmp_path_factory.mktemp("optim_host_gpu")
    return oc.build_host(work, False), work


def carve(arrays, which, shift, dev):
    """views of ONE flat device buffer holding `arrays`, tensor k at a float offset = ALIGN[(k + shift) % len][which] modulo 4"""
    offs, at = [], 0
    for k, a in enumerate(arrays):
        want = ALIGN[(k + shift) % len(ALIGN)][which]
        at += (want - at) % 4
        offs.append(at)
        at += len(a) + 1
    buf = torch.zeros(at + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    views = [buf[o:o + len(a)] for o, a in zip(offs, arrays)]
    for v, a in zip(views, arrays):
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, views


def tables(p, g, m, v, dev):
    rows = [(a.data_ptr(), 0 if b is None else b.data_ptr(), c.data_ptr(), d.data_ptr(), a.numel()) for a, b, c, d in zip(p, g, m, v)]
    chunks = ops.optim_chunk_rows([a.numel() for a in p])
    assert all(0 <= first < p[t].numel() and first % CHUNK == 0 for t, first in chunks)
    assert sum(min(CHUNK, p[t].numel() - first) for t, first in chunks) == sum(a.numel() for a in p)
    return (torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).to(dev), torch.tensor(chunks, dtype=torch.int64).reshape(-1, 2).to(dev))


@pytest.mark.parametrize("shift", [0, 5])
def test_element_update_equals_the_host_build_bit_for_bit(dev, host, shift):
    exe, work = host
    params, grads = oc.case("clip", sizes=SIZES, steps=5)
    coefs = [F32(1.0), F32(0.37), F32(0.5), F32(1.0), F32(0.123)]
    scalars = [oc.step_scalars(t, oc.TOTAL_STEPS) for t in range(1, 6)]         # iterations 1 .. 5: across the phase boundary at 4
    has_grad = [k != NO_GRAD for k in range(len(SIZES))]
    hp, hm, hv, _, _ = oc.run_host(exe, work, params, grads, scalars, coefs=coefs, has_grad=has_grad)
    zeros = [np.zeros(n, F32) for n in SIZES]
    pbuf, p = carve(params, 0, shift, dev)
    mbuf, m = carve(zeros, 2, shift, dev)
    vbuf, v = carve(zeros, 3, shift, dev)
    kinds = set()
    for t in range(5):
        gbuf, g = carve(grads[t], 1, shift, dev)
        gl = [x if has_grad[k] else None for k, x in enumerate(g)]
        for k in range(len(SIZES)):
            ptrs = [p[k].data_ptr(), m[k].data_ptr(), v[k].data_ptr()] + ([g[k].data_ptr()] if has_grad[k] else [])
            kinds.add((SIZES[k] > 4, all(x % 16 == 0 for x in ptrs)))
        table, chunks = tables(p, gl, m, v, dev)
        before = gbuf.clone()
        ops.optim_step(table, chunks, scalars[t], coef=torch.tensor([coefs[t]], dtype=torch.float32, device=dev))
        assert torch.equal(gbuf, before)                                        # the gradient is read, never written
    assert kinds >= {(True, True), (True, False)}                               # both the 16-byte and the 4-byte path ran on real sizes
    for k, n in enumerate(SIZES):
        for name, got, want in (("p", p[k], hp[k]), ("m", m[k], hm[k]), ("v", v[k], hv[k])):
            got = got.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (name, k, n, int((got != want).sum()), float(np.abs(got - want).max()))
    assert not m[NO_GRAD].any() and not v[NO_GRAD].any()
    # nothing outside the tensors was written: the gaps of the flat buffers are still zero
    for buf, views, arrays in ((pbuf, p, params), (mbuf, m, zeros), (vbuf, v, zeros)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        base = buf.data_ptr()
        for x in views:
            o = (x.data_ptr() - base) // 4
            mask[o:o + x.numel()] = False
        assert not buf[mask].any()


@pytest.mark.parametrize("name", ["clip", "noclip", "zero"])
def test_norm_pass(dev, name):
    params, grads = oc.case("clip" if name == "zero" else name, sizes=SIZES, steps=1)
    gs = [np.zeros_like(g) for g in grads[0]] if name == "zero" else grads[0]
    _, p = carve(params, 0, 0, dev)
    _, g = carve(gs, 1, 0, dev)
    _, m = carve([np.zeros(n, F32) for n in SIZES], 2, 0, dev)
    _, v = carve([np.zeros(n, F32) for n in SIZES], 3, 0, dev)
    gl = [x if k != NO_GRAD else None for k, x in enumerate(g)]
    table, chunks = tables(p, gl, m, v, dev)
    part = ops.optim_grad_norm(table, chunks)
    again = ops.optim_grad_norm(table, chunks, partial=torch.full_like(part, -1.0))
    assert part.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    want = sum(float((a.astype(np.float64) ** 2).sum()) for k, a in enumerate(gs) if k != NO_GRAD)
    n = sum(len(a) for k, a in enumerate(gs) if k != NO_GRAD)
    got = float(part.cpu().numpy().sum())
    print("norm pass %s: device %.17g numpy %.17g relative %.3e (bound %.3e)" % (name, got, want, abs(got - want) / max(want, 1e-300),
                                                                                n * 2.0 ** -53))
    assert abs(got - want) <= n * 2.0 ** -53 * want
    rows = ops.optim_chunk_rows(SIZES)
    assert all(float(part[i]) == 0 for i, (t, first) in enumerate(rows) if t == NO_GRAD)
    # norm and coef as the update pass forms them (lr 0, wd 0: the parameters themselves do not move)
    before = [x.clone() for x in p]
    state = ops.optim_step(table, chunks, (1.0, 0.1, 0.99, 0.01, 0.1, 1e-8, 0.0), partial=part, max_norm=oc.MAX_NORM)
    norm, coef = (F32(x) for x in state.cpu().numpy())
    assert abs(float(norm) - np.sqrt(want)) <= 2e-7 * np.sqrt(want)
    one = F32(oc.MAX_NORM) / (norm + F32(1e-6))
    assert one.dtype == np.float32 and coef == min(one, F32(1.0))
    assert {"clip": coef < 0.25, "noclip": coef == 1 and norm > 0.1, "zero": coef == 1 and norm == 0}[name]
    assert all(torch.equal(a, b) for a, b in zip(p, before))
    if name == "clip":                                   # the clipped gradient is what entered the moments
        k = len(SIZES) - 1
        assert np.array_equal(m[k].cpu().numpy(), F32(0.1) * (gs[k] * coef))


def test_whole_step_on_the_rpn_parameter_list(dev):
    from pointrcnn_amd import rpn
    fx = oc.fixture()
    torch.manual_seed(5)
    model = rpn.RPN().to(dev)
    ps = [p for p in model.parameters() if p.requires_grad]
    sizes = [p.numel() for p in ps]
    gen = torch.Generator().manual_seed(9)
    grads = [[torch.randn(p.shape, generator=gen) * 0.01 for p in ps] for _ in range(3)]
    # float64 evaluation: the composed route on float64 copies, on the CPU
    ref = [torch.nn.Parameter(p.detach().cpu().double()) for p in ps]
    opt64 = optim.OneCycleAdam(ref, oc.TOTAL_STEPS, fused=False, **oc.HYPER)
    opt = optim.OneCycleAdam(ps, oc.TOTAL_STEPS, fused=True, **oc.HYPER)
    for gs in grads:
        for p, r, g in zip(ps, ref, gs):
            p.grad, r.grad = g.to(dev), g.double()
        kept = [p.grad.clone() for p in ps]
        opt.step()
        opt64.step()
        assert all(torch.equal(p.grad, k) for p, k in zip(ps, kept))           # .grad keeps its unclipped values
        n64, n32 = float(opt64.last_grad_norm), float(opt.last_grad_norm)
        assert n64 > 2 * oc.MAX_NORM and abs(n32 - n64) <= 2e-7 * n64, (n32, n64)
    assert 1 <= opt.table_uploads <= 3 and opt.iteration == opt64.iteration == 3    # fresh gradient tensors: new addresses, as a rule

    def cat(xs):
        return torch.cat([x.detach().reshape(-1).cpu().double() for x in xs]).numpy()
    e = oc.errors(cat(ps), cat([opt.state[p]["exp_avg"] for p in ps]), cat([opt.state[p]["exp_avg_sq"] for p in ps]),
                  cat(ref), cat([opt64.state[r]["exp_avg"] for r in ref]), cat([opt64.state[r]["exp_avg_sq"] for r in ref]),
                  oc.lr_sum(oc.TOTAL_STEPS, 3), sizes=sizes)
    yard = fx["clip_yard"]
    print("whole step, %d tensors, %d elements: E_p %.3e E_m %.3e E_v %.3e; reference float32 %s, bar 8 x"
          % (len(ps), sum(sizes), e[0], e[1], e[2], yard.tolist()))
    assert all(e[k] <= oc.MARGIN * yard[k] for k in range(3)), (e, yard)


def test_default_route_does_not_reach_the_new_ops(dev, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the adam_onecycle kernels ran without being asked for")
    for name in ("optim_grad_norm", "optim_step"):
        assert callable(getattr(ops, name))
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(tf, "TRAIN_OPTIMIZER", "")                              # the variable unset
    model = torch.nn.Linear(7, 3).to(dev)
    for trainer_opt in (tf.RPNTrainer(model).optimizer,):
        assert type(trainer_opt) is torch.optim.AdamW
        model(torch.ones(2, 7, device=dev)).sum().backward()
        trainer_opt.step()
    monkeypatch.setattr(tf, "TRAIN_OPTIMIZER", "adam_onecycle")                 # ... and set: the default argument now selects the recipe
    opt = tf.RPNTrainer(model).optimizer
    assert isinstance(opt, optim.OneCycleAdam) and opt.param_groups[0]["total_steps"] == tf.TRAIN_TOTAL_STEPS
    with pytest.raises(AssertionError, match="without being asked"):
        opt.step()


def test_one_real_trainer_step_with_the_new_optimizer(dev):
    from test_gpu_round2 import T, _Wrap, _fill
    from make_golden import TRAIN_CASE, train_batch
    from pointrcnn_amd import rpn
    pts, gt, cls, reg = train_batch(TRAIN_CASE)
    model = rpn.RPN()
    _fill(_Wrap(model), TRAIN_CASE["wseed"])
    model = model.to(dev)
    batch = {"pts_input": T(pts, dev), "rpn_cls_label": T(cls, dev), "rpn_reg_label": T(reg, dev)}
    trainer = tf.RPNTrainer(model, optimizer="adam_onecycle", total_steps=10)
    opt = trainer.optimizer
    assert isinstance(opt, optim.OneCycleAdam)
    before = [p.detach().clone() for p in model.parameters()]
    loss = trainer.step(batch)
    assert np.isfinite(float(loss.item())) and np.isfinite(float(opt.last_grad_norm)) and float(opt.last_grad_norm) > 0
    moved = [not torch.equal(a, b) for a, b in zip(before, model.parameters())]
    assert all(moved) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert opt.table_uploads == 1 and opt.iteration == 1
    # the same gradient tensors again (no zero_grad in between): the pointers did not change, so the table is not uploaded again
    for _ in range(2):
        opt.step()
    assert opt.table_uploads == 1 and opt.iteration == 3
