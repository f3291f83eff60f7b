"""CPU: adam_onecycle (pointrcnn_amd/optim.py, arithmetic pointrcnn_amd/csrc/optim_math.h) against the reference's own
OptimWrapper + OneCycle + clip_grad_norm_ run recorded in tests/golden/optim_ref.npz (generator: tests/golden/ref_optim.py).

The bar (tests/optim_cases.py errors): E_p = max |p - p64| / (|p64| + sum_t lr_t) over all entries, E_m / E_v = max |x - x64| / max |x64|
per tensor, each against the reference's float64 run.  The yardstick is the reference's own float32 run against its float64 run
(stored in the fixture); the composed route and the host build of the header may be at most 8 x that -- the margin the fused losses
use: room for a different, equally valid rounding sequence, none for a wrong term."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import optim_cases as oc
from pointrcnn_amd import optim

F32 = np.float32


@pytest.fixture(scope="module")
def fx():
    return oc.fixture()


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    work = tmp_path_factory.mktemp("optim_host")
    return oc.build_host(work, request.param), work


def test_one_cycle_equals_the_reference_schedule_exactly(fx):
    for n in (10, 7):
        got = np.array([optim.one_cycle(s, n, oc.HYPER["lr_max"], oc.HYPER["moms"], oc.HYPER["div_factor"], oc.HYPER["pct_start"])
                        for s in range(n)], np.float64)
        assert np.array_equal(got, fx["sched_%d" % n]), n
    got = np.array([optim.one_cycle(int(s), 10000) for s in fx["sched_default_steps"]], np.float64)
    assert np.array_equal(got, fx["sched_default"])
    # the odd split: int(0.4 * 7) = 2, so iteration 2 is the peak
    assert fx["sched_7"][2, 0] == oc.HYPER["lr_max"] and fx["sched_7"][2, 1] == oc.HYPER["moms"][1]
    # past the end nothing is clamped: the second phase's cosine turns back up
    assert optim.one_cycle(11, 10)[0] > optim.one_cycle(10, 10)[0]


@pytest.mark.parametrize("name", ["clip", "noclip"])
def test_composed_route_follows_the_reference(fx, name):
    params, grads = oc.case(name)
    p, m, v, norms = oc.run_composed(params, grads, oc.TOTAL_STEPS, torch.float32)
    e = oc.errors(p, m, v, fx[name + "_p64"], fx[name + "_m64"], fx[name + "_v64"], oc.lr_sum(oc.TOTAL_STEPS, oc.STEPS))
    yard = fx[name + "_yard"]
    same = all(np.array_equal(oc.flat(a), fx["%s_%s" % (name, k)]) for k, a in (("p", p), ("m", m), ("v", v)))
    print("composed %s: E_p %.3e E_m %.3e E_v %.3e, reference %s, bit-identical to the reference's float32 run: %s"
          % ((name,) + e + (yard.tolist(), same)))
    assert all(e[k] <= oc.MARGIN * yard[k] for k in range(3)), (e, yard)
    assert np.allclose(norms, fx[name + "_norms"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["clip", "noclip"])
def test_host_build_of_the_header_follows_the_float64_run(fx, host, name):
    exe, work = host
    params, grads = oc.case(name)
    scalars = [oc.step_scalars(t, oc.TOTAL_STEPS) for t in range(1, oc.STEPS + 1)]
    p, m, v, norms, coefs = oc.run_host(exe, work, params, grads, scalars)
    e = oc.errors(p, m, v, fx[name + "_p64"], fx[name + "_m64"], fx[name + "_v64"], oc.lr_sum(oc.TOTAL_STEPS, oc.STEPS))
    yard = fx[name + "_yard"]
    differ = [int((oc.flat(a) != fx["%s_%s" % (name, k)]).sum()) for k, a in (("p", p), ("m", m), ("v", v))]
    print("host %s: E_p %.3e E_m %.3e E_v %.3e, reference %s; entries that differ from torch's float32 result (p, m, v): %s of %d"
          % ((name,) + e + (yard.tolist(), differ, oc.flat(p).size)))
    assert all(e[k] <= oc.MARGIN * yard[k] for k in range(3)), (e, yard)
    assert np.allclose(norms, fx[name + "_norms"], rtol=1e-6, atol=0)
    assert (coefs < 0.25).all() if name == "clip" else (coefs == 1.0).all()


def test_edge_rows(host):
    exe, work = host
    sizes = (5, 0, 64, 7)
    params, grads = oc.case("clip", sizes=sizes, steps=1)
    zero = [[np.zeros(n, F32) for n in sizes]]
    sc = [oc.step_scalars(1, oc.TOTAL_STEPS)]
    decay = sc[0][0]
    # an all-zero gradient: norm 0, coef 1, update 0 -> the decay alone; the moments stay 0
    for route in ("host", "composed"):
        if route == "host":
            p, m, v, norms, coefs = oc.run_host(exe, work, params, zero, sc)
            assert norms[0] == 0 and coefs[0] == 1
        else:
            p, m, v, norms = oc.run_composed(params, zero, oc.TOTAL_STEPS, torch.float32)
            assert norms[0] == 0
        for k, n in enumerate(sizes):
            assert p[k].shape == (n,) and np.array_equal(p[k], params[k] * decay), (route, k)
            assert not m[k].any() and not v[k].any()
    # a tensor without gradient: decayed, moments untouched, nothing added to the norm; a tensor without elements changes nothing
    hp, hm, hv, hn, hc = oc.run_host(exe, work, params, grads, sc, has_grad=[1, 1, 0, 1])
    cp, cm, cv, cn = oc.run_composed(params, grads, oc.TOTAL_STEPS, torch.float32, none_grad=(2,))
    want = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for k, g in enumerate(grads[0]) if k != 2))
    assert abs(hn[0] - want) <= 1e-6 * want and abs(cn[0] - want) <= 1e-6 * want
    for p, m, v in ((hp, hm, hv), (cp, cm, cv)):
        assert np.array_equal(p[2], params[2] * decay) and not m[2].any() and not v[2].any()
        assert m[0].any() and v[3].any() and not np.array_equal(p[0], params[0] * decay)
    for k in range(4):
        assert np.abs(hp[k] - cp[k]).max(initial=0) <= 1e-6
    # grad_norm_clip=None: coef 1 whatever the norm (gradients ten times larger: their norm is about 4)
    grads = [[g * F32(10) for g in grads[0]]]
    hp, hm, hv, hn, hc = oc.run_host(exe, work, params, grads, sc, max_norm=None)
    cp, cm, cv, cn = oc.run_composed(params, grads, oc.TOTAL_STEPS, torch.float32, max_norm=None)
    assert hc[0] == 1 and hn[0] > 2 and cn[0] is None
    for k in (0, 2, 3):
        g = grads[0][k]
        assert np.allclose(hm[k], sc[0][1] * g, rtol=1e-6) and np.allclose(cm[k], hm[k], rtol=1e-6)   # the unclipped gradient entered
        assert np.abs(hp[k] - cp[k]).max() <= 1e-6


def test_state_dict_round_trip_continues_identically():
    params, grads = oc.case("clip", sizes=(5, 64, 257))

    def make():
        ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
        return ps, optim.OneCycleAdam(ps, oc.TOTAL_STEPS, **oc.HYPER)

    def run(ps, opt, steps):
        for gs in steps:
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(g.copy())
            opt.step()
    ps, opt = make()
    run(ps, opt, grads[:6])                                 # past the phase boundary (iteration 4)
    sd = copy.deepcopy(opt.state_dict())                    # as a save / load would: state_dict() hands out the live tensors
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and sd["state"][0]["step"] == 6
    ps2, opt2 = make()
    with torch.no_grad():
        for a, b in zip(ps2, ps):
            a.copy_(b)
    opt2.load_state_dict(sd)
    assert opt2.iteration == 6 and opt2.schedule() == opt.schedule() == optim.one_cycle(6, oc.TOTAL_STEPS, oc.HYPER["lr_max"])
    run(ps, opt, grads[6:])
    run(ps2, opt2, grads[6:])
    for a, b in zip(ps, ps2):
        assert torch.equal(a, b)
    for a, b in zip(ps, ps2):
        assert torch.equal(opt.state[a]["exp_avg_sq"], opt2.state[b]["exp_avg_sq"])


def test_constructor_refuses_what_has_no_schedule():
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="phases"):
        optim.OneCycleAdam(p, 2)                            # int(0.4 * 2) == 0: the first phase is empty
    with pytest.raises(ValueError, match="grad_norm_clip"):
        optim.OneCycleAdam(p, 10, grad_norm_clip=0.0)
    with pytest.raises(RuntimeError, match="device route"):
        opt = optim.OneCycleAdam(p, 10, fused=True)
        p[0].grad = torch.ones(3)
        opt.step()


def test_trainer_builds_the_scheduled_optimizer_not_constant_rate_adamw():
    """on the parent every string but "sgd" built constant-rate AdamW"""
    import test_train_ddp_gloo as g
    from pointrcnn_amd import train_functions as tf
    model = g._model(True)
    trainer = tf.RPNTrainer(model, optimizer="adam_onecycle", total_steps=10)
    opt = trainer.optimizer
    assert isinstance(opt, optim.OneCycleAdam) and not isinstance(opt, torch.optim.AdamW)
    gen = torch.Generator().manual_seed(0)
    rates = []
    before = [p.detach().clone() for p in model.parameters()]
    for _ in range(3):
        rates.append(opt.lr)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=gen) * 0.01
        opt.step()
    assert rates == [optim.one_cycle(s, 10, tf.RPNLossConfig.LR)[0] for s in range(3)] and rates[0] < rates[1] < rates[2]
    assert all(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    # the default is what it was
    assert type(tf.RPNTrainer(g._model(True)).optimizer) is torch.optim.AdamW
    assert type(tf.RPNTrainer(g._model(True), optimizer="sgd").optimizer) is torch.optim.SGD


def _onecycle_worker(rank, world, port, q, bn_eval, empty_frame):
    import torch.distributed as dist
    tests = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(tests))
    sys.path.insert(0, tests)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import cpu_ops
    import test_train_ddp_gloo as g
    from pointrcnn_amd import train_functions as tf
    pts, cls, reg = g._batch(world, seed=0)
    shard = {"pts_input": pts[rank:rank + 1], "rpn_cls_label": cls[rank:rank + 1], "rpn_reg_label": reg[rank:rank + 1]}
    model = g._model(bn_eval)
    if rank == 1:
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)
    trainer = tf.RPNTrainer(model, ddp=True, optimizer="adam_onecycle", total_steps=10)
    g._freeze_norm_and_dropout(trainer, bn_eval)
    start = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    with cpu_ops.oracle_ops():
        for _ in range(3):
            loss = trainer.step(shard)
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    q.put((rank, float(loss.item()), start, params.numpy(), (trainer.optimizer.iteration, float(trainer.optimizer.last_grad_norm))))
    dist.barrier()
    dist.destroy_process_group()


def test_composed_route_under_gloo_ddp_keeps_ranks_identical():
    import oracle
    import test_train_ddp_gloo as g
    oracle.cpu()                                    # built here, once: two ranks that both find it missing would build it at the same time
    res = g._run(True, None, target=_onecycle_worker)
    assert np.array_equal(res[0][3], res[1][3])                      # identical parameters after three steps
    assert np.array_equal(res[0][2], res[1][2]) and not np.array_equal(res[0][2], res[0][3])
    assert res[0][4] == res[1][4] and res[0][4][0] == 3 and res[0][4][1] > 0
    assert np.isfinite(res[0][1]) and np.isfinite(res[0][3]).all()
