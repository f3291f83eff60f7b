"""Shared inputs and yardsticks of the adam_onecycle tests (test_optim_cpu.py, test_gpu_optim.py) and of the fixture generator
tests/golden/ref_optim.py: seeded parameters and per-step gradients, the float64 evaluation, the error figures of the bar."""
import os
import struct
import subprocess

import numpy as np

from util import GOLDEN

F32 = np.float32
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 257, 4095, 4097, 8199)
STEPS, TOTAL_STEPS = 10, 10                    # ten steps of a ten-step cycle: the phase boundary is iteration 4
HYPER = dict(lr_max=0.002, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, weight_decay=0.001, betas2=0.99, eps=1e-8)
MAX_NORM = 1.0
# gradient scales: the norm over sum(SIZES) = 17 108 entries is about 131 * scale (times the per-tensor factor 0.5 .. 1.5)
GRAD_SCALE = {"clip": 0.05, "noclip": 0.002}
MARGIN = 8.0                                   # the device and the host twin may be 8 x the reference's own float32 error


def fixture():
    """tests/golden/optim_ref.npz and optim_ref_noclip.npz as one dict (every fixture file stays under 1 MiB)"""
    out = dict(np.load(os.path.join(GOLDEN, "optim_ref.npz")))
    out.update(np.load(os.path.join(GOLDEN, "optim_ref_noclip.npz")))
    return out


def case(name, sizes=SIZES, steps=STEPS, seed=7):
    """-> (params [float32 arrays], grads [steps][float32 arrays]); the same numbers for the same arguments, everywhere"""
    rng = np.random.default_rng(seed + (0 if name == "clip" else 1000))
    params = [rng.normal(0, 0.3, n).astype(F32) for n in sizes]
    grads = [[(rng.normal(0, GRAD_SCALE[name], n) * rng.uniform(0.5, 1.5)).astype(F32) for n in sizes] for _ in range(steps)]
    return params, grads


def flat(arrays):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays]) if len(arrays) else np.zeros(0)


def split(flat_array, sizes=SIZES):
    return np.split(np.asarray(flat_array), np.cumsum(sizes)[:-1])


def errors(p, m, v, p64, m64, v64, lr_sum, sizes=SIZES):
    """the bar's figures: E_p = max |p - p64| / (|p64| + sum_t lr_t) over all entries; E_m, E_v = the largest per-tensor
    max |x - x64| / max |x64| (tensors without elements or with an all-zero x64 add nothing)"""
    p, m, v = (np.asarray(flat(x) if isinstance(x, (list, tuple)) else x, np.float64) for x in (p, m, v))
    p64, m64, v64 = (np.asarray(flat(x) if isinstance(x, (list, tuple)) else x, np.float64) for x in (p64, m64, v64))
    e_p = float(np.max(np.abs(p - p64) / (np.abs(p64) + lr_sum))) if p.size else 0.0

    def per_tensor(x, x64):
        worst = 0.0
        for a, b in zip(split(x, sizes), split(x64, sizes)):
            if b.size and np.abs(b).max() > 0:
                worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
        return worst
    return e_p, per_tensor(m, m64), per_tensor(v, v64)


def run_composed(params, grads, total_steps, dtype, max_norm=MAX_NORM, device="cpu", fused=False, none_grad=()):
    """pointrcnn_amd.optim.OneCycleAdam over numpy inputs -> (p, m, v lists of numpy arrays, [last_grad_norm per step]);
    none_grad: indices of tensors that never receive a gradient"""
    import torch
    from pointrcnn_amd.optim import OneCycleAdam
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(p)).to(dtype).to(device)) for p in params]
    opt = OneCycleAdam(ps, total_steps, grad_norm_clip=max_norm, fused=fused, **HYPER)
    norms = []
    for gs in grads:
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if i in none_grad else torch.from_numpy(np.array(g)).to(dtype).to(device)
        opt.step()
        norms.append(None if opt.last_grad_norm is None else float(opt.last_grad_norm))
    st = [opt.state[p] for p in ps]
    return ([p.detach().cpu().numpy() for p in ps], [s["exp_avg"].cpu().numpy() for s in st],
            [s["exp_avg_sq"].cpu().numpy() for s in st], norms)


def lr_sum(total_steps, steps):
    from pointrcnn_amd.optim import one_cycle
    return sum(one_cycle(t, total_steps, HYPER["lr_max"], HYPER["moms"], HYPER["div_factor"], HYPER["pct_start"])[0] for t in range(steps))


def step_scalars(t, total_steps):
    """the seven float32 scalars of iteration t (counted from 1), as the device route forms them"""
    from pointrcnn_amd.optim import adam_scalars, one_cycle
    lr, mom = one_cycle(t - 1, total_steps, HYPER["lr_max"], HYPER["moms"], HYPER["div_factor"], HYPER["pct_start"])
    return [F32(s) for s in adam_scalars(lr, mom, HYPER["betas2"], t, HYPER["weight_decay"], HYPER["eps"])]


# ---------------------------------------------------------------------------------------------- tests/optim_host.cpp
def build_host(workdir, sanitize):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "optim_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(root, "tests", "hip_stub"), "-I", os.path.join(root, "pointrcnn_amd", "csrc"),
                    os.path.join(root, "tests", "optim_host.cpp"), "-o", exe], check=True)
    return exe


def run_host(exe, workdir, params, grads, scalars, coefs=None, max_norm=MAX_NORM, has_grad=None, m=None, v=None):
    """tests/optim_host.cpp over `len(grads)` steps.  scalars[t]: seven float32; coefs[t]: the caller's coefficient of step t, or
    None = the program forms norm and coef itself (float64 sum in element order).  -> (p, m, v lists, norms, coefs as float32)"""
    sizes = [len(p) for p in params]
    has_grad = [1] * len(sizes) if has_grad is None else [int(h) for h in has_grad]
    m = [np.zeros(n, F32) for n in sizes] if m is None else m
    v = [np.zeros(n, F32) for n in sizes] if v is None else v
    fin, fout = os.path.join(str(workdir), "optim_in.bin"), os.path.join(str(workdir), "optim_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", len(sizes), len(grads), 0 if coefs is None else 1))
        f.write(struct.pack("<f", max_norm if max_norm is not None else 0.0))
        f.write(np.asarray(sizes, np.int64).tobytes() + np.asarray(has_grad, np.int32).tobytes())
        for arrs in (params, m, v):
            f.write(flat(arrs).astype(F32).tobytes())
        for t, gs in enumerate(grads):
            f.write(np.asarray(scalars[t], F32).tobytes())
            f.write(struct.pack("<f", 0.0 if coefs is None else coefs[t]))
            f.write(flat(gs).astype(F32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(fout, F32)
    n = sum(sizes)
    assert out.size == 3 * n + 2 * len(grads), out.size
    sp = (lambda a: split(a, sizes)) if len(sizes) > 1 else (lambda a: [a])
    return sp(out[:n]), sp(out[n:2 * n]), sp(out[2 * n:3 * n]), out[3 * n:3 * n + len(grads)], out[3 * n + len(grads):]
