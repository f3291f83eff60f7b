"""CPU: TRAIN.OPTIMIZER adam and sgd (pointrcnn_amd/optim.py ClipAdam / ClipSGD; arithmetic pointrcnn_amd/csrc/optim_math.h
om_adam_l2 / om_sgd) against stock torch.

The reference is clip_grad_norm_ + torch.optim.Adam / SGD on float64 copies, the yardstick is torch's own float32 run against
that float64 run in the figures of tests/optim_cases.py errors (E_p, E_m, E_v; sgd: E_p, E_buf), and the host build of the header
(tests/optim_modes_host.cpp, plain and under AddressSanitizer + UBSan) may be at most optim_cases.MARGIN (8) times that: the margin
the adam_onecycle update has over the reference's own rounding.  The composed route IS stock torch, so it is held bit for bit."""
import copy

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_modes_cases as mc
from pointrcnn_amd import optim

F32 = np.float32
MODES = ("adam", "sgd")


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    work = tmp_path_factory.mktemp("optim_modes_host")
    return mc.build_host(work, request.param), work


@pytest.fixture(scope="module")
def torch_runs():
    """stock torch in float64 and float32 on every case, computed once: {(mode, name): (run64, run32)}"""
    out = {}
    for mode in MODES:
        for name in ("clip", "noclip"):
            params, grads = oc.case(name)
            out[mode, name] = (mc.run_torch(mode, params, grads, torch.float64), mc.run_torch(mode, params, grads, torch.float32))
    return out


def figures(mode, run, run64, steps=oc.STEPS):
    e = oc.errors(run[0], run[1], run[2], run64[0], run64[1], run64[2], steps * mc.LR)
    return e if mode == "adam" else e[:2]


@pytest.mark.parametrize("name", ["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_host_build_follows_torch_float64(host, torch_runs, mode, name):
    exe, work = host
    params, grads = oc.case(name)
    run64, run32 = torch_runs[mode, name]
    sc = [mc.scalars(mode, t) for t in range(1, oc.STEPS + 1)]
    p, m, v, norms, coefs = mc.run_host(exe, work, mode, params, grads, sc)
    e, yard = figures(mode, (p, m, v), run64), figures(mode, run32, run64)
    differ = [int((oc.flat(a) != oc.flat(b)).sum()) for a, b in zip((p, m, v), run32[:3])]
    print("host %s %s: figures %s, torch float32 %s; entries that differ from torch's float32 bits (p, m, v): %s of %d"
          % (mode, name, ["%.3e" % x for x in e], ["%.3e" % x for x in yard], differ, oc.flat(p).size))
    assert all(y > 0 for y in yard)
    assert all(a <= oc.MARGIN * y for a, y in zip(e, yard)), (e, yard)
    assert np.allclose(norms, run64[3], rtol=1e-6, atol=0)
    assert (coefs < 0.25).all() if name == "clip" else (coefs == 1.0).all()


@pytest.mark.parametrize("name", ["clip", "noclip"])
@pytest.mark.parametrize("mode", MODES)
def test_composed_route_is_stock_torch_bit_for_bit(torch_runs, mode, name):
    params, grads = oc.case(name)
    got = mc.run_torch(mode, params, grads, torch.float32, stock=False)
    want = torch_runs[mode, name][1]
    for a, b in zip(got[:3], want[:3]):
        assert oc.flat(a).tobytes() == oc.flat(b).tobytes()
    assert got[3] == want[3]


def test_adam_without_decay_has_the_bits_of_the_adam_onecycle_update_at_decay_one(host, tmp_path):
    exe, work = host
    params, grads = oc.case("clip", steps=3)
    sc = [mc.scalars("adam", t, wd=0.0) for t in range(1, 4)]
    p, m, v, _, _ = mc.run_host(exe, work, "adam", params, grads, sc)
    old = oc.build_host(tmp_path, False)
    q, n, w, _, _ = oc.run_host(old, tmp_path, params, grads, [[F32(1.0)] + s[1:] for s in sc])
    for a, b in zip((p, m, v), (q, n, w)):
        assert oc.flat(a).tobytes() == oc.flat(b).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_edge_rows(host, mode):
    exe, work = host
    sizes = (5, 0, 64, 7)
    params, grads = oc.case("clip", sizes=sizes, steps=1)
    zero = [[np.zeros(n, F32) for n in sizes]]

    def both(grads, max_norm=oc.MAX_NORM, has_grad=(1, 1, 1, 1), **hyper):
        """-> the host build's and the composed route's (p, m, v, norm of the step)"""
        sc = [mc.scalars(mode, 1, **hyper)]
        hp, hm, hv, hn, hc = mc.run_host(exe, work, mode, params, grads, sc, max_norm=max_norm, has_grad=has_grad)
        cp, cm, cv, cn = mc.run_torch(mode, params, grads, torch.float32, stock=False, max_norm=max_norm,
                                      none_grad=[k for k, h in enumerate(has_grad) if not h], **hyper)
        for k in range(len(sizes)):
            assert hp[k].shape == cp[k].shape == (sizes[k],)
            assert np.abs(hp[k] - cp[k]).max(initial=0) <= 1e-6 and np.allclose(hm[k], cm[k], rtol=1e-5, atol=1e-12)
        return (hp, hm, hv, hn[0], hc[0]), (cp, cm, cv, cn[0])

    # an all-zero gradient with wd 0: nothing moves, the moments stay 0; norm 0 and coef 1
    h, c = both(zero, wd=0.0)
    assert h[3] == 0 and h[4] == 1 and c[3] == 0
    for run in (h, c):
        for k in range(4):
            assert np.array_equal(run[0][k], params[k]) and not run[1][k].any() and not run[2][k].any()
    # ... and with wd: the decay term alone is the gradient
    h, c = both(zero)
    assert not np.array_equal(h[0][0], params[0]) and h[1][2].any()
    # a tensor without a gradient: bits and moments unchanged, nothing added to the norm; a tensor of 0 elements changes nothing
    h, c = both(grads, has_grad=(1, 1, 0, 1))
    want = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for k, g in enumerate(grads[0]) if k != 2))
    for run in (h, c):
        assert abs(run[3] - want) <= 1e-6 * want
        assert run[0][2].tobytes() == params[2].tobytes() and not run[1][2].any() and not run[2][2].any()
        assert run[1][0].any() and not np.array_equal(run[0][3], params[3])
    # wd == 0 and momentum == 0
    both(grads, wd=0.0)
    if mode == "sgd":
        h, c = both(grads, momentum=0.0)
        assert not any(x.any() for x in h[1]) and not any(x.any() for x in c[1])          # no buffer is kept
        assert np.array_equal(h[0][0], params[0] + F32(-mc.LR) * (grads[0][0] * h[4] + F32(mc.WD) * params[0]))
    # grad_norm_clip=None with a norm above 1: coef 1, the unclipped gradient enters
    big = [[g * F32(10) for g in grads[0]]]
    h, c = both(big, max_norm=None, wd=0.0)
    assert h[4] == 1 and h[3] > 2 and c[3] is None
    for k in (0, 2, 3):
        first = big[0][k] * (F32(1 - mc.BETAS[0]) if mode == "adam" else F32(1))
        assert np.allclose(h[1][k], first, rtol=1e-6) and np.allclose(c[1][k], first, rtol=1e-6)


@pytest.mark.parametrize("mode", MODES)
def test_state_dict_loads_into_stock_torch_and_back(mode):
    params, grads = oc.case("clip", sizes=(5, 64, 257))
    stock_cls = torch.optim.Adam if mode == "adam" else torch.optim.SGD

    def make(stock):
        ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
        return ps, mc.make_optimizer(mode, ps, stock)

    def run(ps, opt, steps):
        for gs in steps:
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(g.copy())
            if type(opt) is stock_cls:
                torch.nn.utils.clip_grad_norm_(ps, oc.MAX_NORM)
            opt.step()

    def move(src_ps, src, stock):
        ps, opt = make(stock)
        with torch.no_grad():
            for a, b in zip(ps, src_ps):
                a.copy_(b)
        opt.load_state_dict(copy.deepcopy(src.state_dict()))
        return ps, opt
    ref_ps, ref = make(True)
    run(ref_ps, ref, grads)                                                     # ten steps of stock torch
    ps, opt = make(False)
    run(ps, opt, grads[:3])
    assert sorted(opt.state_dict()["state"][0]) == (["exp_avg", "exp_avg_sq", "step"] if mode == "adam" else ["momentum_buffer"])
    ps, opt = move(ps, opt, True)                                               # ours -> stock
    assert type(opt) is stock_cls
    run(ps, opt, grads[3:6])
    ps, opt = move(ps, opt, False)                                              # stock -> ours
    assert isinstance(opt, stock_cls) and type(opt) is not stock_cls and opt.clips_in_step
    run(ps, opt, grads[6:])
    for a, b in zip(ps, ref_ps):
        assert torch.equal(a, b)
    m, v = mc.state_arrays(mode, opt, ps)
    rm, rv = mc.state_arrays(mode, ref, ref_ps)
    assert all(np.array_equal(a, b) for a, b in zip(m + v, rm + rv))
    if mode == "adam":
        assert all(int(opt.state[p]["step"]) == oc.STEPS for p in ps)


def test_constructors_refuse_what_is_not_built():
    p = [torch.nn.Parameter(torch.zeros(3))]
    q = [torch.nn.Parameter(torch.zeros(2))]
    for kw in (dict(nesterov=True, momentum=0.9), dict(dampening=0.1, momentum=0.9), dict(maximize=True)):
        with pytest.raises(ValueError, match="not built"):
            optim.ClipSGD(p, lr=0.1, **kw)
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="not built"):
            optim.ClipAdam(p, **kw)
    for cls in (optim.ClipAdam, optim.ClipSGD):
        with pytest.raises(ValueError, match="one parameter group"):
            cls([{"params": p}, {"params": q}], lr=0.1)
        with pytest.raises(ValueError, match="grad_norm_clip"):
            cls(p, lr=0.1, grad_norm_clip=0.0)
        opt = cls(p, lr=0.1)
        with pytest.raises(ValueError, match="one parameter group"):
            opt.add_param_group({"params": q})
        assert opt.clips_in_step and opt.last_grad_norm is None and opt.table_uploads == 0
        with pytest.raises(RuntimeError, match="device route"):
            opt = cls(p, lr=0.1, fused=True)
            p[0].grad = torch.ones(3)
            opt.step()


def test_a_scheduler_acts_on_them_unchanged():
    for cls in (optim.ClipAdam, optim.ClipSGD):
        p = [torch.nn.Parameter(torch.ones(3))]
        opt = cls(p, lr=0.5, grad_norm_clip=1.0)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.1 ** e)
        p[0].grad = torch.ones(3)
        opt.step()
        sched.step()
        assert opt.param_groups[0]["lr"] == 0.5 * 0.1


def test_exports_validate_their_arguments_before_any_launch():
    """no device is touched: every call below returns before a launch (an error, or zero chunks, which is a no-op)"""
    import ctypes
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    table = (ctypes.c_int64 * 8)()
    state = (ctypes.c_float * 2)()
    coef = (ctypes.c_float * 1)(1.0)
    ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)                            # noqa: E731

    def adam(n=0, tensors=None, partial=None, max_norm=1.0, coef=None, state=None, wd=0.001, bc2=0.1):
        return lib.prcnn_optim_step_adam(tensors, tensors, n, partial, max_norm, coef, state, wd, 0.1, 0.999, 0.001, bc2, 1e-8, -0.002, None)

    def sgd(n=0, tensors=None, partial=None, max_norm=1.0, coef=None, state=None, wd=0.001, momentum=0.9):
        return lib.prcnn_optim_step_sgd(tensors, tensors, n, partial, max_norm, coef, state, wd, momentum, -0.002, None)
    for fn, name in ((adam, "prcnn_optim_step_adam"), (sgd, "prcnn_optim_step_sgd")):
        _cabi.check(fn(0, coef=ptr(coef)), name)                               # zero chunks: nothing to do
        _cabi.check(fn(0, state=ptr(state)), name)
        for kw, text in ((dict(n=-1, coef=ptr(coef)), "bad chunk count"), (dict(n=1, coef=ptr(coef)), "null table"),
                         (dict(n=0), "state must be given"), (dict(n=1, tensors=ptr(table), state=ptr(state)), "partial sums"),
                         (dict(n=0, state=ptr(state), max_norm=0.0), "max_norm must be > 0"),
                         (dict(n=0, coef=ptr(coef), wd=-1.0), "weight_decay must be >= 0")):
            with pytest.raises(_cabi.PointOpsError, match=name + ": .*" + text):
                _cabi.check(fn(**kw), name)
    with pytest.raises(_cabi.PointOpsError, match="beta2\\^t\\) must be > 0"):
        _cabi.check(adam(0, coef=ptr(coef), bc2=0.0), "prcnn_optim_step_adam")
    with pytest.raises(_cabi.PointOpsError, match="momentum must be >= 0"):
        _cabi.check(sgd(0, coef=ptr(coef), momentum=-0.5), "prcnn_optim_step_sgd")
    assert lib.prcnn_abi_version() == 12                                       # additive: the version stays


def test_packed_step_counters_stay_torchs_layout():
    """the device route keeps every parameter's `step` as a view of one flat tensor (ClipAdam._packed_steps): the views must behave
    as torch's own counters do -- its step() increments them, state_dict() carries them, stock torch continues from them"""
    params, grads = oc.case("clip", sizes=(5, 64, 257), steps=6)

    def run(ps, opt, steps, clip):
        for gs in steps:
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(g.copy())
            if clip:
                torch.nn.utils.clip_grad_norm_(ps, oc.MAX_NORM)
            opt.step()
    ref_ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    ref = mc.make_optimizer("adam", ref_ps, True)
    run(ref_ps, ref, grads, True)
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    opt = mc.make_optimizer("adam", ps, False)
    run(ps, opt, grads[:2], False)
    states = [opt.state[p] for p in ps]
    flat = opt._packed_steps(states)
    assert flat.tolist() == [2.0, 2.0, 2.0] and opt._packed_steps(states) is flat                # packed once
    assert all(st["step"].dim() == 0 and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" for st in states)
    run(ps, opt, grads[2:4], False)                                                              # torch's own step() moves the views
    assert flat.tolist() == [4.0, 4.0, 4.0] and opt._packed_steps(states) is flat
    sd = copy.deepcopy(opt.state_dict())
    assert [int(sd["state"][k]["step"]) for k in range(3)] == [4, 4, 4]
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    stock = mc.make_optimizer("adam", ps2, True)
    stock.load_state_dict(sd)
    run(ps2, stock, grads[4:], True)
    assert all(torch.equal(a, b) for a, b in zip(ps2, ref_ps))
    opt.load_state_dict(copy.deepcopy(stock.state_dict()))                                       # other counter objects: packed again
    again = opt._packed_steps([opt.state[p] for p in ps])
    assert again is not flat and again.tolist() == [6.0, 6.0, 6.0]
