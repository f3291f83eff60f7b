"""CPU: the arithmetic header of the fused RPN loss (pointrcnn_amd/csrc/rpn_loss_math.h), compiled for the host by
tests/rpn_loss_math_host.cpp -- once plain, once with -fsanitize=address,undefined.

Label targets (bins, residuals, size targets): BIT FOR BIT what train_functions._bin_and_residual and the angle code of
get_reg_loss (get_ry_fine=False, row_mask form) give when torch runs them on the CPU in float32 -- on bin edges and one float32
step either side, beyond both clamp ends, angle-bin edges +- one step, negative / large / special angles and 10 000 random labels.

Per-row terms and derivatives (focal, 12-way softmax cross-entropy, smooth-L1, and a whole regression row) against float64
closed forms.  The error of a value is |err| / S with S the sum of the absolute values of the addends that form it (the
normalisation of test_gpu_train_stack_f64.py).  The bar is not fixed in advance: for every point it is 8 x the error the COMPOSED
float32 code (SigmoidFocalClassificationLoss / F.cross_entropy / F.smooth_l1_loss with autograd, torch CPU) has against the same
float64 closed form at that point, and never below 8 x 2^-24 (half a float32 ulp of S: what one correctly rounded float32
operation on S-sized operands may already be off by).  Worst figures over each family (composed, header):
    focal value and derivative 1 / 1 (at logit 20, target 1, float32 loses 1 - p entirely in both codes: the bar is per point
    for that reason); softmax value 4.4e-8 / 4.4e-8, derivative 4.05e-6 / 4.05e-6; smooth-L1 value 5.33e-6 / 5.33e-6 (the
    denormal 0.5 * 1e-20^2), derivative 0 / 0; whole row terms 7.9e-4 / 7.9e-4 (a smooth-L1 term of a residual within 1e-4 of its
    target, relative to the term), row derivatives 5.5e-7 / 5.8e-7 (S as in tests/test_gpu_rpn_loss.py).
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pointrcnn_amd import train_functions as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
CFG = tf.RPNLossConfig
F32 = np.float32
FLOOR = 2.0 ** -24
C = 76

@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rpn_loss_math") / "rpn_loss_math_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "rpn_loss_math_host.cpp"),
                    "-o", exe], check=True)
    work = os.path.dirname(exe)

    def run(mode, records, *extra):
        records = np.ascontiguousarray(records, dtype=F32)
        records.tofile(os.path.join(work, "in.bin"))
        r = subprocess.run([exe, mode, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")] + [str(e) for e in extra],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(os.path.join(work, "out.bin"), F32).reshape(len(records), -1)
    return run


def _steps(v):
    v = np.asarray(v, F32)
    return np.concatenate([v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))])


def label_families():
    rng = np.random.default_rng(20240607)
    fam = {}
    k = np.arange(0, 13)
    fam["xz bin edges"] = (_steps((k * 0.5 - 3).astype(F32)), None)
    fam["xz beyond scope"] = (np.array([-1e6, -10, -3.5, -3.0001, -3, 2.9985, 2.999, 2.9995, 3, 3.0001, 3.5, 10, 1e6], F32), None)
    k = np.arange(-14, 27)
    fam["ry bin edges"] = (None, _steps((k * math.pi / 6 - math.pi / 12).astype(F32)))
    special = [0.0, -0.0, math.pi, -math.pi, 2 * math.pi, -2 * math.pi, 4 * math.pi, -4 * math.pi, 7.0, -7.0, 100.0, -100.0, 1e-30,
               -1e-30, -1e-3, math.pi / 12, -math.pi / 12, 2 * math.pi - math.pi / 12]
    fam["ry special"] = (None, _steps(np.array(special, F32)))
    fam["random"] = (rng.uniform(-4, 4, 10000).astype(F32), rng.uniform(-3 * math.pi, 3 * math.pi, 10000).astype(F32))
    out = {}
    for name, (xz, ry) in fam.items():
        n = len(xz) if xz is not None else len(ry)
        lab = np.empty((n, 7), F32)
        lab[:, 0] = xz if xz is not None else rng.uniform(-4, 4, n)
        lab[:, 1] = rng.uniform(-1, 1, n)
        lab[:, 2] = xz[::-1] if xz is not None else rng.uniform(-4, 4, n)
        lab[:, 3:6] = rng.uniform(0.5, 6, (n, 3))
        lab[:, 6] = ry if ry is not None else rng.uniform(-7, 7, n)
        out[name] = lab
    return out


def torch_targets(lab):
    """the composed code's label targets, torch CPU, in lab's dtype"""
    xb, xr = tf._bin_and_residual(lab[:, 0], CFG.LOC_SCOPE, CFG.LOC_BIN_SIZE)
    zb, zr = tf._bin_and_residual(lab[:, 2], CFG.LOC_SCOPE, CFG.LOC_BIN_SIZE)
    ry = lab[:, 6]                                          # get_reg_loss, get_ry_fine=False with a row mask
    two_pi = 2 * math.pi
    apc = two_pi / CFG.NUM_HEAD_BIN
    shift = ((ry % two_pi) + apc / 2) % two_pi
    rb = torch.clamp((shift / apc).floor().long(), 0, CFG.NUM_HEAD_BIN - 1)
    rr = (shift - (rb.float() * apc + apc / 2)) / (apc / 2)
    anchor = torch.tensor(CFG.MEAN_SIZE, dtype=lab.dtype)
    return torch.stack([xb, zb, rb], 1), torch.cat([torch.stack([xr, zr, rr], 1), (lab[:, 3:6] - anchor) / anchor], 1)


def test_label_targets_equal_torch_cpu_float32_bit_for_bit(host):
    for name, lab in label_families().items():
        got = host("labels", lab)
        bins, res = torch_targets(torch.from_numpy(lab))
        assert np.array_equal(got[:, :3].view(np.int32), bins.numpy().astype(np.int32)), name
        want = res.numpy()
        same = got[:, 3:].view(np.uint32) == want.view(np.uint32)
        assert same.all(), "%s: %d residuals differ, first at %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    lab = label_families()["xz beyond scope"]
    bins = host("labels", lab)[:, :3].view(np.int32)
    assert bins[:, 0].min() == 0 and bins[:, 0].max() == 11             # both clamp ends are hit


def _check(name, got, ref, composed, S):
    """got / composed float32 results, ref float64, S the normalisation: per point |got - ref| / S <= 8 max(|composed - ref| / S, 2^-24)"""
    got, ref, composed, S = (np.asarray(a, np.float64) for a in (got, ref, composed, S))
    assert np.isfinite(got).all(), name
    S = np.where(S > 0, S, 1.0)
    e_got, e_cmp = np.abs(got - ref) / S, np.abs(composed - ref) / S
    print("%s: composed float32 %.3g, header %.3g (worst |err| / S)" % (name, e_cmp.max(), e_got.max()))
    bad = e_got > 8 * np.maximum(e_cmp, FLOOR)
    assert not bad.any(), "%s: %s" % (name, [(i, e_got[i], e_cmp[i]) for i in np.argwhere(bad)[:5]])


def test_focal_term_and_derivative_against_float64(host):
    gamma, alpha, w = CFG.FOCAL_GAMMA, CFG.FOCAL_ALPHA[0], 1.0 / 7.0
    xs = np.array([0, 1e-3, -1e-3, 20, -20, 100, -100, 0.7, -2.5], F32)
    rec = np.array([(x, t, w) for x in xs for t in (0.0, 1.0)], F32)
    got = host("focal", rec)
    x, t, wf = (rec[:, k].astype(np.float64) for k in range(3))
    lg = np.log1p(np.exp(-np.abs(x)))
    ce = np.maximum(x, 0) - x * t + lg
    p, omp = 1 / (1 + np.exp(-x)), 1 / (1 + np.exp(x))
    q = t * omp + (1 - t) * p
    a = t * alpha + (1 - t) * (1 - alpha)
    mod, dmod = q ** gamma, gamma * q ** (gamma - 1) * (1 - 2 * t) * p * omp
    dce = np.where(t > 0, -omp, p)
    ref_v, ref_d = mod * a * ce * wf, a * wf * (dmod * ce + mod * dce)
    S_v = a * wf * mod * (np.maximum(x, 0) + np.abs(x * t) + lg)
    S_d = a * wf * (np.abs(dmod * ce) + mod * (p + t))
    xt = torch.from_numpy(rec[:, 0].copy()).requires_grad_(True)
    per = tf.SigmoidFocalClassificationLoss(gamma=gamma, alpha=alpha)(xt, torch.from_numpy(rec[:, 1].copy()), torch.from_numpy(rec[:, 2].copy()))
    per.sum().backward()
    _check("focal value", got[:, 0], ref_v, per.detach().numpy(), S_v)
    _check("focal derivative", got[:, 1], ref_d, xt.grad.numpy(), S_d)


def test_softmax_cross_entropy_against_float64(host):
    rng = np.random.default_rng(5)
    rec = []
    for spike in (80.0, -80.0, None):
        for at in (0, 5, 11):
            for target in (at, (at + 3) % 12):
                z = rng.normal(0, 2, 12)
                if spike is not None:
                    z[at] = spike
                rec.append(list(z) + [target])
    rec = np.array(rec, F32)
    got = host("softmax", rec)
    z, tgt = rec[:, :12].astype(np.float64), rec[:, 12].astype(np.int64)
    m = z.max(1, keepdims=True)
    ls = np.log(np.exp(z - m).sum(1))
    zt = np.take_along_axis(z, tgt[:, None], 1)[:, 0]
    onehot = np.eye(12)[tgt]
    soft = np.exp(z - m - ls[:, None])
    zt32 = torch.from_numpy(rec[:, :12].copy()).requires_grad_(True)
    per = F.cross_entropy(zt32, torch.from_numpy(tgt), reduction="none")
    per.sum().backward()
    _check("softmax value", got[:, 0], ls - (zt - m[:, 0]), per.detach().numpy(), np.abs(ls) + np.abs(zt - m[:, 0]))
    _check("softmax derivative", got[:, 1:].ravel(), (soft - onehot).ravel(), zt32.grad.numpy().ravel(), (soft + onehot).ravel())


def test_smooth_l1_against_float64(host):
    one = np.array([1.0], F32)
    ds = np.concatenate([_steps(one), -_steps(one), np.array([0, 1e-20, 0.5, -0.5, 3, -3], F32)])
    rec = np.concatenate([np.stack([ds, np.zeros_like(ds)], 1), np.stack([ds + F32(0.5), np.full_like(ds, 0.5)], 1)]).astype(F32)
    got = host("sl1", rec)
    a, b = rec[:, 0].astype(np.float64), rec[:, 1].astype(np.float64)
    d = a - b
    small = np.abs(d) < 1
    at = torch.from_numpy(rec[:, 0].copy()).requires_grad_(True)
    per = F.smooth_l1_loss(at, torch.from_numpy(rec[:, 1].copy()), reduction="none")
    per.sum().backward()
    mag = np.abs(a) + np.abs(b)
    _check("smooth-L1 value", got[:, 0], np.where(small, 0.5 * d * d, np.abs(d) - 0.5), per.detach().numpy(), np.where(small, 0.5 * mag * mag, mag + 0.5))
    _check("smooth-L1 derivative", got[:, 1], np.where(small, d, np.sign(d)), at.grad.numpy(), np.where(small, mag, 1.0))


def test_whole_row_against_get_reg_loss_in_float64(host):
    """one foreground row through rl_reg_row against get_reg_loss itself (float64, one row per call): ties the bins and the column
    layout of the header to the function the fused route replaces"""
    rng = np.random.default_rng(11)
    n = 64
    lab = label_families()["random"][:n].copy()
    pred = rng.normal(0, 1.5, (n, C)).astype(F32)
    got = host("row", np.concatenate([pred, lab], 1))
    assert got.shape == (n, 8 + C)
    keys = ["loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res", "loss_y_offset", "loss_ry_bin", "loss_ry_res", "loss_size"]

    def run(dtype):
        vals, grads = [], []
        anchor = torch.tensor(CFG.MEAN_SIZE, dtype=dtype)
        for i in range(n):
            p = torch.from_numpy(pred[i:i + 1]).to(dtype).requires_grad_(True)
            loc, ang, size, d = tf.get_reg_loss(p, torch.from_numpy(lab[i:i + 1]).to(dtype), CFG.LOC_SCOPE, CFG.LOC_BIN_SIZE, CFG.NUM_HEAD_BIN,
                                                anchor, get_xz_fine=True, want_items=True)
            (loc + ang + 3 * size).backward()
            vals.append([float(d[k].detach() if torch.is_tensor(d[k]) else d[k]) * (3 if k == "loss_size" else 1) for k in keys])
            grads.append(p.grad[0].numpy().astype(np.float64))
        return np.array(vals), np.array(grads)
    ref_v, ref_g = run(torch.float64)
    cmp_v, cmp_g = run(torch.float32)
    # values relative to the term; derivatives per entry by the S of tests/test_gpu_rpn_loss.py (its docstring), every row foreground
    from test_gpu_rpn_loss import Case, scales
    c = Case.__new__(Case)
    c.C, c.npts, c.cls, c.lab = C, n, torch.zeros(1, n, 1), torch.ones(1, n, dtype=torch.long)
    c.reg, c.reg_lab = torch.from_numpy(pred).view(1, n, C), torch.from_numpy(lab).view(1, n, 7)
    S = scales(c)[1].reshape(n, C) * n                       # scales() holds the 1 / n of the mean; the rows here are single-row calls
    assert not ref_g[S == 0].any() and not got[:, 8:][S == 0].any()
    _check("row terms", got[:, :8].ravel(), ref_v.ravel(), cmp_v.ravel(), np.abs(ref_v).ravel())
    _check("row derivatives", got[:, 8:][S > 0], ref_g[S > 0], cmp_g[S > 0], S[S > 0])
    assert (np.abs(got[:, 8:]) > 0).sum(1).min() >= 12 * 3 + 3 + 1 + 3                       # every head contributes
