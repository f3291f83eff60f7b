"""The double clip of csrc/quad_clip.h and its Python twin (tests/train_input_twin.py) against an exact rational reference
(tests/exact_quad.py) on adversarial box pairs (tests/quad_families.py); the sampler's fp32 separating-axis shortcut
(gta_separated, csrc/train_input.hip) restated in numpy fp32 against the same reference.  No GPU.

Bar for an IoU: |got - exact| <= 2^-23 * exact + 1e-12.  The result is one fp32 rounding (2^-24 relative; doubled because the fp32
heights enter both sides identically but round again in o * h) of a double computation whose own error is far smaller: the
shoelace products are of order x * z <= 38 * 69 = 2.6e3, so each rounds by <= 2.3e-13 m^2, about 1e-12 m^2 over a polygon, on
areas of 1 to 30 m^2: <= 1e-12 in the IoU only for the smallest boxes here, and typically 1e-14.

Measured with families(seed=0, n=24): 600 pairs, 373 with an exact IoU > 0, 175 with IoU == 0 and the bottoms closer than 1 mm,
32 with an IoU in (0, 1e-6).  The twin, worst over both IoUs (the host builds of quad_clip.h give the same figures but for the
slivers of the touch_* and corner_contact families, where they stay below 2e-13 absolute):

    family            near: rel  abs            far: rel  abs
    random            5.0e-08   2.6e-08        5.6e-08   2.9e-08
    same_heading      4.4e-08   2.0e-08        4.9e-08   2.9e-08
    touch_length      4.3e-08   2.7e-15        5.8e-07   2.4e-14
    touch_width       4.3e-08   1.8e-15        2.8e-07   1.3e-13
    identical         0         0              0         0
    nested            5.6e-08   1.4e-08        5.6e-08   1.4e-08
    turn_90           4.3e-08   2.3e-08        4.3e-08   2.7e-08
    turn_180          2.9e-08   2.9e-08        1.6e-08   1.6e-08
    corner_contact    1.0e-01   5.0e-18        1.0e+00   4.9e-14
    near_contact      2.8e-08   3.1e-10        3.5e-08   7.4e-10
    thin              3.7e-08   1.5e-08        4.4e-08   1.8e-08
    degenerate        0         0              0         0
    parking_rows      6.0e-08   1.5e-11

Every pair is inside the bar; the worst uses 48 % of it, and no decision at 1e-8 differs.  The large relative errors of the
touch_* and corner_contact rows belong to slivers (overlaps of a few ulps, IoU 1e-7 down to 1e-17): their absolute errors,
1e-13 and less, sit inside the 1e-12 term, which is what that term is for.
"""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import exact_quad as xq
import quad_families as qf
import train_input_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pointrcnn_amd", "csrc")
F32 = np.float32
THR = F32(1e-8)


def within_bar(got, want):
    """got fp32, want Fraction -> (ok, |got - want| as float)"""
    d = abs(Fraction(float(got)) - want)
    return d <= want / 2 ** 23 + Fraction(1, 10 ** 12), float(d)


def check_against_exact(name, got3, gotb, want):
    """got3, gotb: fp32 per pair; want: [(iou3d, bev) Fraction].  Prints the worst errors, then asserts the bar and the 1e-8 decision"""
    worst_rel = worst_abs = 0.0
    bad = []
    for i, (w3, wb) in enumerate(want):
        for g, w in ((got3[i], w3), (gotb[i], wb)):
            ok, d = within_bar(g, w)
            worst_abs = max(worst_abs, d)
            if w > 0:
                worst_rel = max(worst_rel, d / float(w))
            if not ok:
                bad.append((i, float(g), float(w), d))
        if (F32(got3[i]) < THR) != (F32(float(w3)) < THR):
            bad.append((i, "decision", float(got3[i]), float(w3)))
    print("%-22s worst rel %.2e abs %.2e" % (name, worst_rel, worst_abs))
    assert not bad, (name, bad[:5])


def test_exact_reference_self_test():
    assert xq.self_test()


def test_families_are_live():
    pos, close, sliver, total = qf.check_liveness()
    print("pairs %d: exact IoU > 0 %d, == 0 and closer than 1 mm %d, in (0, 1e-6) %d" % (total, pos, close, sliver))
    fams = qf.families()
    assert len(fams) == 25
    for name in qf.TOUCHING:                                   # the sampler can take these
        for where in ("near_", "far_"):
            qf.sampler_boxes(fams[where + name].a), qf.sampler_boxes(fams[where + name].b)


def test_twin_matches_exact_on_every_family():
    fams, ex = qf.families(), qf.exact()
    for name, f in fams.items():
        got = [tw.pair_iou(f.ca[i], f.cb[i]) for i in range(len(f.ca))]
        check_against_exact(name, [g[0] for g in got], [g[1] for g in got], ex[name])


def separated_fp32(ax, az, bx, bz):
    """gta_separated (csrc/train_input.hip) in numpy fp32: every product and sum rounded on its own, no FMA"""
    ax, az, bx, bz = (np.asarray(v, F32) for v in (ax, az, bx, bz))
    S = max(F32(1.0), np.abs(np.concatenate([ax, az, bx, bz])).max())
    for e in range(8):
        ex, ez = (ax, az) if e < 4 else (bx, bz)
        i = e & 3
        j = (i + 1) & 3
        nx, nz = -(ez[j] - ez[i]), ex[j] - ex[i]
        margin = F32(1e-5) * (np.abs(nx) + np.abs(nz)) * S
        pa = ax * nx + az * nz
        pb = bx * nx + bz * nz
        if pa.max() < pb.min() - margin or pb.max() < pa.min() - margin:
            return True
    return False


def test_separating_axis_shortcut_is_sound_and_still_useful():
    fams = qf.families()
    unsound = []
    far_apart = fired = overlapping = 0
    for name, f in fams.items():
        n = len(f.ca)
        for roll in range(4):                      # pair i, and three other partners from the same neighbourhood
            for i in range(n):
                ca, cb = f.ca[i], f.cb[(i + roll) % n]
                o, area_a, area_b = xq.exact_overlap(ca, cb)
                sep = separated_fp32(ca[:4, 0], ca[:4, 2], cb[:4, 0], cb[:4, 2])
                if o > 0:
                    overlapping += 1
                    if sep:
                        unsound.append((name, i, roll, float(o)))
                elif area_a > 0 and area_b > 0 and xq.quad_gap(ca, cb) > 1e-2:
                    far_apart += 1
                    fired += sep
    print("overlapping %d, apart by more than 1 cm %d of which the shortcut decides %d" % (overlapping, far_apart, fired))
    assert not unsound, unsound[:5]
    assert overlapping >= 500 and far_apart >= 200
    assert 2 * fired >= far_apart


def _host_compiler():
    for cc in ("g++", "c++", "clang++"):
        if shutil.which(cc):
            return [shutil.which(cc)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


@pytest.mark.parametrize("flags", [("-ffp-contract=off",), ("-ffp-contract=fast", "-march=native")], ids=["no-fma", "fma-native"])
def test_quad_clip_header_on_the_host_matches_exact(flags, tmp_path):
    """quad_clip.h itself (it is __host__ __device__), compiled with and without FMA contraction of the cross products"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "quad_clip_host")
    subprocess.run(cc + ["-O2", "-std=c++17", *flags, "-I", os.path.join(HERE, "hip_stub"), "-I", CSRC,
                         os.path.join(HERE, "quad_clip_host.cpp"), "-o", exe], check=True)
    fams, ex = qf.families(), qf.exact()
    names = list(fams)
    pairs = np.concatenate([np.concatenate([fams[k].ca.reshape(-1, 24), fams[k].cb.reshape(-1, 24)], 1) for k in names]).astype(F32)
    pairs.tofile(str(tmp_path / "in.bin"))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(str(tmp_path / "out.bin"), F32).reshape(-1, 2)
    assert len(got) == len(pairs)
    at = 0
    for k in names:
        n = len(fams[k].ca)
        check_against_exact(k, got[at:at + n, 0], got[at:at + n, 1], ex[k])
        at += n


def test_sampler_twin_takes_an_iou_callable():
    """gt_aug_sample(iou=...) with the twin's own IoU is the default, and the callable is what decides"""
    scene, db = qf.parking_scene(3, 40, 60)
    cfg = {"GT_EXTRA_NUM": 50, "GT_AUG_RAND_NUM": False, "GT_AUG_APPLY_PROB": 1.0, "GT_AUG_HARD_RATIO": 0.0, "PC_AREA_SCOPE": None,
           "TRY_TIMES": 60}
    args = (scene, (0.0, -1.0, 0.0, 1.65), db, np.zeros(len(db), F32), np.full(len(db), 50), cfg, 7, 0)
    base = tw.gt_aug_sample(*args, max_accept=64)
    same = tw.gt_aug_sample(*args, max_accept=64, iou=lambda a, b: tw.pair_iou(a, b)[0])
    exact = tw.gt_aug_sample(*args, max_accept=64, iou=lambda a, b: F32(float(xq.exact_iou(a, b)[0])))
    none = tw.gt_aug_sample(*args, max_accept=64, iou=lambda a, b: F32(1))
    for k in ("ids", "boxes", "y_shift"):
        assert np.array_equal(base[k], same[k]) and np.array_equal(base[k], exact[k]), k
    assert base["stats"] == same["stats"] == exact["stats"]
    assert 5 <= len(base["ids"]) < base["stats"][2] - 5           # both verdicts occur
    assert len(none["ids"]) == 0
