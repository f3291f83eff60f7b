"""CPU: the arithmetic header of the fused RCNN loss (pointrcnn_amd/csrc/rcnn_loss_math.h over rpn_loss_math.h), compiled for the
host by tests/rcnn_loss_math_host.cpp -- once plain, once with -fsanitize=address,undefined -- and run as a program.

Label targets (x / z / y bins and residuals, the fine angle target of get_ry_fine=True, size targets against MEAN_SIZE and against a
per-row anchor): BIT FOR BIT what train_functions._bin_and_residual and get_reg_loss's angle code give when torch runs them on the
CPU in float32 -- on every bin edge and one float32 step either side, beyond both clamp ends, at +-pi/2, +-3pi/2, 0, +-2pi (where
torch compares the float32 angle with the float32-rounded constant), at both ends of the shift clamp, negative and > 2pi angles and
10 000 random labels.  NaN and +-inf labels: every bin stays in its range.

The BCE term and a whole regression row against float64, with the error measure and the bar of tests/test_rpn_loss_math_cpu.py
(|err| / S, per point 8 x the composed float32 code's own error at that point, never below 8 x 2^-24).  Worst figures (composed,
header): BCE value 4.9 / 7.4e-8 and derivative 1 / 9.3e-8 (from |x| ~ 17 on float32 sigmoid(x) is 1 and the composed term is the clamp
100 with a zero derivative; the header keeps softplus and p - t); row terms 2.2e-4 / 2.2e-4 (a smooth-L1 term of a residual close to
its target, relative to the term), row derivatives 8.7e-7 / 8.7e-7.
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pointrcnn_amd import train_functions as tf
from pointrcnn_amd.rcnn import RCNNConfig as CFG
from test_rpn_loss_math_cpu import F32, _check, _steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
MEAN = tf.RPNLossConfig.MEAN_SIZE
NH = CFG.NUM_HEAD_BIN
APC = (math.pi / 2) / NH


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rcnn_loss_math") / "rcnn_loss_math_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "rcnn_loss_math_host.cpp"),
                    "-o", exe], check=True)
    work = os.path.dirname(exe)

    def run(mode, records, y_by_bin=0, size_on_roi=0):
        records = np.ascontiguousarray(records, dtype=F32)
        records.tofile(os.path.join(work, "in.bin"))
        r = subprocess.run([exe, mode, os.path.join(work, "in.bin"), os.path.join(work, "out.bin"), str(int(y_by_bin)), str(int(size_on_roi))],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(os.path.join(work, "out.bin"), F32).reshape(len(records), -1)
    return run


def label_families():
    """name -> (n, 10) float32 records [dx dy dz h w l ry, 3 anchor sizes]"""
    rng = np.random.default_rng(20240611)
    pi = math.pi
    fam = {}
    fam["xz and y bin edges"] = (_steps((np.arange(0, 7) * 0.5 - 1.5).astype(F32)), _steps((np.arange(0, 5) * 0.25 - 0.5).astype(F32)), None)
    fam["beyond scope"] = (np.array([-1e6, -10, -2, -1.5001, -1.5, 1.4985, 1.499, 1.4995, 1.5, 1.5001, 2, 10, 1e6], F32),
                           np.array([-1e6, -10, -1, -0.5001, -0.5, 0.4985, 0.499, 0.4995, 0.5, 0.5001, 1, 10, 1e6], F32), None)
    edges = np.arange(0, NH + 1) * APC - pi / 4                 # shift == k * apc, then the same edge through the flip and a turn
    fam["ry bin edges"] = (None, None, _steps(np.concatenate([edges + s for s in (0, pi, -pi, 2 * pi, -2 * pi, 3 * pi)]).astype(F32)))
    ends = [-pi / 4 + 1e-3, pi / 4 - 1e-3, -pi / 4, pi / 4]     # both ends of the shift clamp, and where the shift leaves [0, pi/2]
    special = [0.0, -0.0, pi / 2, -pi / 2, 3 * pi / 2, -3 * pi / 2, 2 * pi, -2 * pi, pi, -pi, 4 * pi, -4 * pi, 5 * pi / 2, -5 * pi / 2, 7.0,
               -7.0, 100.0, -100.0, 1e-30, -1e-30, -1e-3, 1e-3] + ends + [e + pi for e in ends] + [e - pi for e in ends]
    fam["ry special"] = (None, None, _steps(np.array(special, F32)))
    fam["random"] = (rng.uniform(-2, 2, 10000).astype(F32), rng.uniform(-0.8, 0.8, 10000).astype(F32),
                     rng.uniform(-3 * pi, 3 * pi, 10000).astype(F32))
    out = {}
    for name, (xz, y, ry) in fam.items():
        n = max(len(v) for v in (xz, y, ry) if v is not None)
        rec = np.empty((n, 10), F32)
        rec[:, 0] = np.resize(xz, n) if xz is not None else rng.uniform(-2, 2, n)
        rec[:, 1] = np.resize(y, n) if y is not None else rng.uniform(-0.8, 0.8, n)
        rec[:, 2] = np.resize(xz, n)[::-1] if xz is not None else rng.uniform(-2, 2, n)
        rec[:, 3:6] = rng.uniform(0.5, 6, (n, 3))
        rec[:, 6] = np.resize(ry, n) if ry is not None else rng.uniform(-7, 7, n)
        rec[:, 7:10] = rng.uniform(0.5, 6, (n, 3))
        out[name] = rec
    return out


def torch_targets(rec, size_on_roi):
    """the composed code's label targets, torch CPU, in rec's dtype: (n, 4) bins, (n, 7) residuals and size targets"""
    lab = rec[:, :7]
    xb, xr = tf._bin_and_residual(lab[:, 0], CFG.LOC_SCOPE, CFG.LOC_BIN_SIZE)
    zb, zr = tf._bin_and_residual(lab[:, 2], CFG.LOC_SCOPE, CFG.LOC_BIN_SIZE)
    yb, yr = tf._bin_and_residual(lab[:, 1], CFG.LOC_Y_SCOPE, CFG.LOC_Y_BIN_SIZE)
    ry = lab[:, 6]                                          # get_reg_loss, get_ry_fine=True with a row mask
    two_pi = 2 * math.pi
    apc = (math.pi / 2) / NH
    ry = ry % two_pi
    opposite = (ry > math.pi * 0.5) & (ry < math.pi * 1.5)
    ry = torch.where(opposite, (ry + math.pi) % two_pi, ry)
    shift = (ry + math.pi * 0.5) % two_pi
    shift = torch.clamp(shift - math.pi * 0.25, min=1e-3, max=math.pi * 0.5 - 1e-3)
    rb = torch.clamp((shift / apc).floor().long(), 0, NH - 1)
    rr = (shift - (rb.float() * apc + apc / 2)) / (apc / 2)
    anchor = rec[:, 7:10] if size_on_roi else torch.tensor(MEAN, dtype=rec.dtype)
    return torch.stack([xb, zb, yb, rb], 1), torch.cat([torch.stack([xr, zr, yr, rr], 1), (lab[:, 3:6] - anchor) / anchor], 1)


@pytest.mark.parametrize("size_on_roi", [0, 1], ids=["mean-size", "per-row-anchor"])
def test_label_targets_equal_torch_cpu_float32_bit_for_bit(host, size_on_roi):
    fams = label_families()
    for name, rec in fams.items():
        got = host("labels", rec, 1, size_on_roi)
        bins, res = torch_targets(torch.from_numpy(rec), size_on_roi)
        same = got[:, :4].view(np.int32) == bins.numpy().astype(np.int32)
        assert same.all(), "%s: %d bins differ, first at %s" % (name, (~same).sum(), np.argwhere(~same)[0])
        same = got[:, 4:].view(np.uint32) == res.numpy().view(np.uint32)
        assert same.all(), "%s: %d residuals differ, first at %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    bins = host("labels", fams["beyond scope"], 1, size_on_roi)[:, :4].view(np.int32)
    assert bins[:, 0].min() == 0 and bins[:, 0].max() == 5 and bins[:, 2].min() == 0 and bins[:, 2].max() == 3      # both clamp ends are hit
    bins = host("labels", fams["ry special"], 1, size_on_roi)[:, 3].view(np.int32)
    assert bins.min() == 0 and bins.max() == NH - 1
    edge = host("labels", np.array([[0, 0, 0, 1, 1, 1, math.pi / 2, 1, 1, 1]], F32), 1, size_on_roi)
    assert edge[0, 3].view(np.int32) == NH - 1                  # float32(pi/2) is not "> math.pi * 0.5" for torch: no flip, upper clamp


def test_non_finite_labels_keep_every_bin_in_range(host):
    bad = [float("nan"), float("inf"), float("-inf")]
    rec = label_families()["random"][:9 * 4].copy()
    for i in range(len(rec)):
        rec[i, (0, 1, 2, 6)[i % 4]] = bad[(i // 4) % 3]
    rec[-1, :7] = float("nan")
    for y_by_bin in (0, 1):
        bins = host("labels", rec, y_by_bin, 0)[:, :4].view(np.int32)
        for col, n in ((0, 6), (1, 6), (2, 4), (3, NH)):
            assert bins[:, col].min() >= 0 and bins[:, col].max() <= n - 1, (col, bins[:, col])
    pred = np.random.default_rng(3).normal(0, 1, (len(rec), 53)).astype(F32)
    got = host("row", np.concatenate([pred, rec], 1), 1, 1)      # and a whole row runs with them (ASan / UBSan: no wild index)
    assert got.shape == (len(rec), 9 + 53)


def test_bce_term_and_derivative_against_float64(host):
    xs = np.concatenate([np.linspace(-20, 20, 81), [1e-3, -1e-3, 0.5, -7.3, 16.6, -16.7, 17.5]]).astype(F32)
    rec = np.array([(x, t) for x in xs for t in (0.0, 1.0)], F32)
    got = host("bce", rec)
    x, t = rec[:, 0].astype(np.float64), rec[:, 1].astype(np.float64)
    lg = np.log1p(np.exp(-np.abs(x)))
    sp_pos, sp_neg = np.maximum(x, 0) + lg, np.maximum(-x, 0) + lg
    p, omp = 1 / (1 + np.exp(-x)), 1 / (1 + np.exp(x))
    ref_v = np.where(t > 0, sp_neg, sp_pos)
    ref_d = np.where(t > 0, -omp, p)
    xt = torch.from_numpy(rec[:, 0].copy()).requires_grad_(True)
    per = F.binary_cross_entropy(torch.sigmoid(xt), torch.from_numpy(rec[:, 1].copy()), reduction="none")
    per.sum().backward()
    _check("BCE value", got[:, 0], ref_v, per.detach().numpy(), ref_v)
    _check("BCE derivative", got[:, 1], ref_d, xt.grad.numpy(), p + t)
    far = host("bce", np.array([(x, t) for x in (90.0, -90.0, 150.0, -150.0) for t in (0.0, 1.0)], F32))
    assert np.isfinite(far).all() and (np.abs(far[:, 1]) <= 1).all() and (far[:, 0] >= 0).all() and far[:, 0].max() == 100.0
    assert far[0, 0] == 90.0 and far[0, 1] == 1.0 and abs(far[1, 0]) < 1e-38 and abs(far[1, 1]) < 1e-38      # x = 90 against t = 0, t = 1


@pytest.mark.parametrize("name", ["bce", "ybin", "roi"])
def test_whole_row_against_get_reg_loss_in_float64(host, name):
    """one regressed row through rc_reg_row against get_reg_loss(get_ry_fine=True) itself (float64, one row per call) for the default
    heads (y_by_bin False, MEAN_SIZE anchor), LOC_Y_BY_BIN (C = 53) and the per-row anchor: ties the bins and the column layout of the
    header to the function the fused route replaces"""
    from rcnn_loss_cases import CFGS, CHANNELS, Case, scales
    cfg, C = CFGS[name], CHANNELS[name]
    rng = np.random.default_rng(11)
    n = 64
    rec = label_families()["random"][:n].copy()
    rec[:, 7:10] = rec[:, 3:6] * rng.uniform(0.8, 1.25, (n, 3)).astype(F32)
    pred = rng.normal(0, 1.5, (n, C)).astype(F32)
    got = host("row", np.concatenate([pred, rec], 1), cfg.LOC_Y_BY_BIN, cfg.SIZE_RES_ON_ROI)
    assert got.shape == (n, 9 + C)
    keys = ["loss_x_bin", "loss_z_bin", "loss_x_res", "loss_z_res"] + (["loss_y_bin", "loss_y_res"] if cfg.LOC_Y_BY_BIN else ["loss_y_offset"])
    keys += ["loss_ry_bin", "loss_ry_res", "loss_size"]
    cols = [k for k in range(9) if cfg.LOC_Y_BY_BIN or k != 5]
    if not cfg.LOC_Y_BY_BIN:
        assert not got[:, 5].any()

    def run(dtype):
        vals, grads = [], []
        for i in range(n):
            p = torch.from_numpy(pred[i:i + 1]).to(dtype).requires_grad_(True)
            anchor = torch.from_numpy(rec[i:i + 1, 7:10]).to(dtype) if cfg.SIZE_RES_ON_ROI else torch.tensor(MEAN, dtype=dtype)
            loc, ang, size, d = tf.get_reg_loss(p, torch.from_numpy(rec[i:i + 1, :7]).to(dtype), cfg.LOC_SCOPE, cfg.LOC_BIN_SIZE, NH, anchor,
                                                get_xz_fine=True, get_y_by_bin=cfg.LOC_Y_BY_BIN, loc_y_scope=cfg.LOC_Y_SCOPE,
                                                loc_y_bin_size=cfg.LOC_Y_BIN_SIZE, get_ry_fine=True, want_items=True)
            (loc + ang + 3 * size).backward()
            vals.append([float(d[k].detach() if torch.is_tensor(d[k]) else d[k]) * (3 if k == "loss_size" else 1) for k in keys])
            grads.append(p.grad[0].numpy().astype(np.float64))
        return np.array(vals), np.array(grads)
    ref_v, ref_g = run(torch.float64)
    cmp_v, cmp_g = run(torch.float32)
    c = Case.__new__(Case)
    c.C, c.R, c.cls, c.lab, c.mask = C, n, torch.zeros(n, 1), torch.ones(n, dtype=torch.long), torch.ones(n, dtype=torch.long)
    c.reg, c.gt, c.roi = torch.from_numpy(pred), torch.from_numpy(rec[:, :7].copy()), torch.zeros(n, 7)
    c.roi[:, 3:6] = torch.from_numpy(rec[:, 7:10].copy())
    S = scales(c, name)[1] * n                               # scales() holds the 1 / n of the mean; the rows here are single-row calls
    assert not ref_g[S == 0].any() and not got[:, 9:][S == 0].any()
    _check("row terms", got[:, cols].ravel(), ref_v.ravel(), cmp_v.ravel(), np.abs(ref_v).ravel())
    _check("row derivatives", got[:, 9:][S > 0], ref_g[S > 0], cmp_g[S > 0], S[S > 0])
    heads = 6 * 2 + 2 + (4 + 1 if cfg.LOC_Y_BY_BIN else 1) + NH + 1 + 3
    assert (np.abs(got[:, 9:]) > 0).sum(1).min() >= heads                       # every head contributes
