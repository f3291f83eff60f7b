"""Run the REFERENCE's own adam_onecycle -- OptimWrapper(Adam(betas=(0.9, 0.99)), wd, true_wd=True, bn_wd=True) as
tools/train_rcnn.py:95-108 creates it, OneCycle as :135-138 does, stepped and clipped as tools/train_utils/train_utils.py:135 and
:188-190 do -- on the CPU over the seeded tensors of tests/optim_cases.py, and keep what it leaves.

Only used to GENERATE tests/golden/optim_ref.npz and optim_ref_noclip.npz (needs the reference tree; build container only).  The reference's modules are
imported, nothing of them is copied.  Recorded:
    sched_<N>            (N, 2) float64 (lr, mom) of every iteration of total_steps N = 10 and 7
    sched_default_steps / sched_default   a handful of iterations of a 10 000-step run and their (lr, mom)
    <case>_p / _m / _v   parameters, exp_avg, exp_avg_sq (flat float32) after optim_cases.STEPS steps; <case> = clip (norm above the
                         clip) | noclip (below)
    <case>_p64 / _m64 / _v64   the same run on float64 tensors (float32 inputs widened)
    <case>_norms         the norm clip_grad_norm_ returned at every step (float32 run)
    <case>_yard          E_p, E_m, E_v of the reference's float32 run against its float64 run (optim_cases.errors): the yardstick"""
import importlib.util
import os
import sys

import numpy as np
import torch

REFERENCE = os.environ.get("PRCNN_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
DEFAULT_TOTAL = 10000
DEFAULT_STEPS = (0, 1, 1234, 3999, 4000, 4001, 7777, 9999)


def available():
    return os.path.isfile(os.path.join(REFERENCE, "tools", "train_utils", "fastai_optim.py"))


def _modules():
    for p in (os.path.join(REFERENCE, "tools"), ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("prcnn_compat_adapters", os.path.join(TESTS, "compat", "usercustomize.py"))
    spec.loader.exec_module(importlib.util.module_from_spec(spec))
    from train_utils import learning_schedules_fastai as lsf
    from train_utils.fastai_optim import OptimWrapper
    return lsf, OptimWrapper


class _Leaf(torch.nn.Module):
    def __init__(self, arrays, dtype):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dtype)) for a in arrays])


def schedule(total_steps, steps, hyper):
    lsf, _ = _modules()
    opt = lsf.FakeOptim()
    sch = lsf.OneCycle(opt, total_steps, hyper["lr_max"], list(hyper["moms"]), hyper["div_factor"], hyper["pct_start"])
    out = []
    for s in steps:
        sch.step(s)
        out.append((float(opt.lr), float(opt.mom)))
    return np.array(out, np.float64)


def run_reference(params, grads, total_steps, hyper, max_norm, dtype):
    from functools import partial
    lsf, OptimWrapper = _modules()
    model = torch.nn.Sequential(_Leaf(params, dtype))
    opt = OptimWrapper.create(partial(torch.optim.Adam, betas=(0.9, hyper["betas2"]), eps=hyper["eps"]), 3e-3, [torch.nn.Sequential(model[0])],
                              wd=hyper["weight_decay"], true_wd=True, bn_wd=True)
    sch = lsf.OneCycle(opt, total_steps, hyper["lr_max"], list(hyper["moms"]), hyper["div_factor"], hyper["pct_start"])
    ps = list(model.parameters())
    norms = []
    for it, gs in enumerate(grads):
        sch.step(it)
        opt.zero_grad()
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(np.array(g)).to(dtype)
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)))
        opt.step()
    st = [opt.opt.state[p] for p in ps]
    return ([p.detach().numpy() for p in ps], [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st], norms)


def make_golden(path=None):
    _modules()
    import optim_cases as oc
    out = {}
    for n in (10, 7):
        out["sched_%d" % n] = schedule(n, range(n), oc.HYPER)
    out["sched_default_steps"] = np.array(DEFAULT_STEPS, np.int64)
    out["sched_default"] = schedule(DEFAULT_TOTAL, DEFAULT_STEPS, oc.HYPER)
    lr_sum = float(out["sched_10"][:oc.STEPS, 0].sum())
    for name in ("clip", "noclip"):
        params, grads = oc.case(name)
        p, m, v, norms = run_reference(params, grads, oc.TOTAL_STEPS, oc.HYPER, oc.MAX_NORM, torch.float32)
        p64, m64, v64, _ = run_reference(params, grads, oc.TOTAL_STEPS, oc.HYPER, oc.MAX_NORM, torch.float64)
        assert (min(norms) > 2 * oc.MAX_NORM) if name == "clip" else (max(norms) < 0.5 * oc.MAX_NORM), (name, norms)
        yard = oc.errors(p, m, v, p64, m64, v64, lr_sum)
        assert all(np.isfinite(y) and y > 0 for y in yard), (name, yard)
        print(name, "norms %.3f .. %.3f" % (min(norms), max(norms)), "E_p %.3e E_m %.3e E_v %.3e" % yard)
        for k, a in (("p", p), ("m", m), ("v", v)):
            out["%s_%s" % (name, k)] = oc.flat(a).astype(np.float32)
        for k, a in (("p64", p64), ("m64", m64), ("v64", v64)):
            out["%s_%s" % (name, k)] = oc.flat(a).astype(np.float64)
        out[name + "_norms"] = np.array(norms, np.float64)
        out[name + "_yard"] = np.array(yard, np.float64)
    # every fixture file stays under 1 MiB: the noclip run's arrays go to a file of their own
    path = path or os.path.join(HERE, "optim_ref.npz")
    np.savez_compressed(path, **{k: a for k, a in out.items() if not k.startswith("noclip_")})
    np.savez_compressed(path.replace(".npz", "_noclip.npz"), **{k: a for k, a in out.items() if k.startswith("noclip_")})
    print("wrote", path, "and its _noclip file")


if __name__ == "__main__":
    make_golden()
