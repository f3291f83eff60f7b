"""Shared pieces of the adam / sgd update tests (test_optim_modes_cpu.py, test_gpu_optim_modes.py): the scalars as the device
route forms them, the host build of csrc/optim_math.h (tests/optim_modes_host.cpp), and stock torch as the reference."""
import math
import os
import struct
import subprocess

import numpy as np

import optim_cases as oc

F32 = np.float32
LR, WD, BETAS, EPS, MOMENTUM = 0.002, 0.001, (0.9, 0.999), 1e-8, 0.9
MODES = {"adam": 1, "sgd": 2}


def adam_scalars(t, lr=LR, wd=WD, betas=BETAS, eps=EPS):
    """the seven float32 scalars of ClipAdam's step t (counted from 1)"""
    b1, b2 = betas
    return [F32(x) for x in (wd, 1 - b1, b2, 1 - b2, math.sqrt(1 - b2 ** t), eps, -(lr / (1 - b1 ** t)))]


def sgd_scalars(lr=LR, wd=WD, momentum=MOMENTUM):
    return [F32(x) for x in (wd, momentum, -lr)]


def scalars(mode, t, lr=LR, wd=WD, momentum=MOMENTUM):
    return adam_scalars(t, lr, wd) if mode == "adam" else sgd_scalars(lr, wd, momentum)


def build_host(workdir, sanitize):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "optim_modes_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(root, "tests", "hip_stub"), "-I", os.path.join(root, "pointrcnn_amd", "csrc"),
                    os.path.join(root, "tests", "optim_modes_host.cpp"), "-o", exe], check=True)
    return exe


def run_host(exe, workdir, mode, params, grads, step_scalars, coefs=None, max_norm=oc.MAX_NORM, has_grad=None, m=None, v=None):
    """tests/optim_modes_host.cpp over len(grads) steps; step_scalars[t]: scalars(mode, t + 1, ...); coefs[t]: the caller's coefficient
    or None = formed by the program.  -> (p, m, v lists, norms, coefs); sgd's momentum buffer is m"""
    sizes = [len(p) for p in params]
    has_grad = [1] * len(sizes) if has_grad is None else [int(h) for h in has_grad]
    m = [np.zeros(n, F32) for n in sizes] if m is None else m
    v = [np.zeros(n, F32) for n in sizes] if v is None else v
    fin, fout = os.path.join(str(workdir), "modes_in.bin"), os.path.join(str(workdir), "modes_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i", len(sizes), len(grads), 0 if coefs is None else 1, MODES[mode]))
        f.write(struct.pack("<f", max_norm if max_norm is not None else 0.0))
        f.write(np.asarray(sizes, np.int64).tobytes() + np.asarray(has_grad, np.int32).tobytes())
        for arrs in (params, m, v):
            f.write(oc.flat(arrs).astype(F32).tobytes())
        for t, gs in enumerate(grads):
            sc = list(step_scalars[t]) + [F32(0)] * (7 - len(step_scalars[t]))
            f.write(np.asarray(sc, F32).tobytes())
            f.write(struct.pack("<f", 0.0 if coefs is None else coefs[t]))
            f.write(oc.flat(gs).astype(F32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(fout, F32)
    n = sum(sizes)
    assert out.size == 3 * n + 2 * len(grads), out.size
    sp = (lambda a: oc.split(a, sizes)) if len(sizes) > 1 else (lambda a: [a])
    return sp(out[:n]), sp(out[n:2 * n]), sp(out[2 * n:3 * n]), out[3 * n:3 * n + len(grads)], out[3 * n + len(grads):]


def make_optimizer(mode, ps, stock, lr=LR, wd=WD, momentum=MOMENTUM, max_norm=oc.MAX_NORM, fused=False):
    import torch
    from pointrcnn_amd import optim
    if stock:
        return (torch.optim.Adam(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd) if mode == "adam" else
                torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=wd))
    return (optim.ClipAdam(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, grad_norm_clip=max_norm, fused=fused) if mode == "adam" else
            optim.ClipSGD(ps, lr=lr, momentum=momentum, weight_decay=wd, grad_norm_clip=max_norm, fused=fused))


def state_arrays(mode, opt, ps):
    """-> (m, v) lists of numpy arrays: exp_avg / exp_avg_sq, or momentum_buffer / zeros; zeros where a tensor has no state"""
    m, v = [], []
    for p in ps:
        st = opt.state.get(p, {})
        a = st.get("exp_avg" if mode == "adam" else "momentum_buffer")
        b = st.get("exp_avg_sq")
        m.append(np.zeros(p.numel(), p.detach().cpu().numpy().dtype) if a is None else a.detach().cpu().numpy().reshape(-1))
        v.append(np.zeros(p.numel(), p.detach().cpu().numpy().dtype) if b is None else b.detach().cpu().numpy().reshape(-1))
    return m, v


def run_torch(mode, params, grads, dtype, stock=True, max_norm=oc.MAX_NORM, none_grad=(), device="cpu", fused=False, **hyper):
    """stock clip_grad_norm_ + torch.optim.Adam / SGD (stock=True), or ClipAdam / ClipSGD, over numpy inputs
    -> (p, m, v lists of numpy arrays, [gradient norm per step or None])"""
    import torch
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(p)).to(dtype).to(device)) for p in params]
    opt = make_optimizer(mode, ps, stock, max_norm=max_norm, fused=fused, **hyper)
    norms = []
    for gs in grads:
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if i in none_grad else torch.from_numpy(np.array(g)).to(dtype).to(device)
        if stock:
            norm = None if max_norm is None else torch.nn.utils.clip_grad_norm_(ps, max_norm)
            opt.step()
        else:
            opt.step()
            norm = opt.last_grad_norm
        norms.append(None if norm is None else float(norm))
    m, v = state_arrays(mode, opt, ps)
    return [p.detach().cpu().numpy() for p in ps], m, v, norms
