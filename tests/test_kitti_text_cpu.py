"""CPU: pointrcnn_amd/csrc/kitti_text_math.h through its host build tests/kitti_text_host.cpp (plain and with ASan + UBSan): the
"%.4f" conversion against Python's own, the result lines against pointrcnn_amd/kitti_output.py and against the reference's own writer
recorded in tests/golden/kitti_output_ref.npz.

Bounds: the float32 columns of a row may differ from kitti_output's numpy by 2e-6 relative (alpha only: numpy's trig against glibc's,
one unit in the last place of a float32 near pi is 2.4e-7), the image box by 1e-4 px (a last-place difference of cosf / sinf moves a
corner by ~1e-6 m, times the focal length over the depth: measured <= 1.4e-5 px on these scenes).  Against the fixture a field may
move by one unit of the fourth decimal, and at most 1 field in 100 may move at all."""
import ctypes
import os

import numpy as np
import pytest

import kitti_text_cases as kc
from pointrcnn_amd import kitti_output
from util import GOLDEN


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    work = tmp_path_factory.mktemp("kitti_text_host")
    return kc.build_host(work, request.param), work


def formatter_inputs():
    r = np.random.default_rng(11)
    parts = [np.array(kc.EDGE_VALUES, np.float64)]
    parts.append(r.uniform(-2.0 ** 31, 2.0 ** 31, 150_000))                                   # float64 across the domain
    parts.append(r.uniform(-2.0 ** 31, 2.0 ** 31, 150_000).astype(np.float32).astype(np.float64))
    parts.append((r.normal(0, 1, 150_000) * 10.0 ** r.uniform(-9, 3, 150_000)))                # dense near zero
    parts.append((r.normal(0, 1, 150_000) * 10.0 ** r.uniform(-9, 3, 150_000)).astype(np.float32).astype(np.float64))
    parts.append(r.uniform(-100, 1300, 100_000).astype(np.float32).astype(np.float64))        # what a result line holds
    # the exact ties (2j+1)/32 = k.xxxx5 with both signs, and their float64 and float32 neighbours
    j = np.concatenate([np.arange(0, 40_000), r.integers(0, 2 ** 35, 30_000)]).astype(np.float64)
    t = (2 * j + 1) / 32
    t = np.concatenate([t, -t])
    parts += [t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)]
    t32 = t[np.abs(t) < 2.0 ** 18].astype(np.float32)                                           # ties a float32 holds exactly
    assert np.array_equal(t32.astype(np.float64), t[np.abs(t) < 2.0 ** 18])
    parts += [np.nextafter(t32, np.float32(np.inf)).astype(np.float64), np.nextafter(t32, np.float32(-np.inf)).astype(np.float64)]
    x = np.concatenate(parts)
    return x[np.abs(x) < 2.0 ** 31]


def test_formatter_prints_what_python_prints(host):
    exe, work = host
    x = formatter_inputs()
    assert x.size >= 10 ** 6
    ln, rec = kc.run_fmt(exe, work, x)
    assert (ln > 0).all()
    want = [(" %.4f" % v).encode() for v in x.tolist()]
    got = [rec[i, :ln[i]].tobytes() for i in range(x.size)]
    bad = [i for i in range(x.size) if got[i] != want[i]]
    assert not bad, [(x[i].hex(), got[i], want[i]) for i in bad[:5]]
    by_value = dict(zip(x.tolist()[:len(kc.EDGE_VALUES)], got))
    assert by_value[1241.0] == b" 1241.0000" and by_value[-1e-5] == b" -0.0000" and by_value[2.0 ** 31 - 1] == b" 2147483647.0000"
    assert got[1] == b" -0.0000" and got[0] == b" 0.0000"
    assert max(ln) <= 17


def test_formatter_reports_what_it_cannot_print(host):
    exe, work = host
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 1e300, -1e19, np.nextafter(2.0 ** 31, 0), 5e-324, -5e-324])
    ln, rec = kc.run_fmt(exe, work, x)
    assert (ln[:8] == -1).all() and not rec[:8].any()
    assert [rec[i, :ln[i]].tobytes() for i in (8, 9, 10)] == [b" 2147483648.0000", b" 0.0000", b" -0.0000"]


BATCHES = {"seed1": dict(seeds=(1,)), "seed2": dict(seeds=(2,)), "seed5_n64": dict(seeds=(5,), n=64)}


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_lines_are_python_format_of_the_rows_and_rows_follow_kitti_output(host, name):
    exe, work = host
    batch = kc.make_batch(**BATCHES[name])
    out = kc.run_lines(exe, work, batch)
    assert out["status"].tolist() == [0]
    assert kc.frame_lines(out, 0) == kc.python_lines(out["rows"][0], out["valid"][0])
    b, sc, P2, (H, W) = batch["boxes"][0], batch["scores"][0], batch["P2"][0].reshape(3, 4), batch["img_hw"][0]
    ib = kitti_output.corners_to_image_boxes(kitti_output.box_corners(b), P2)
    ib[:, 0::2] = np.clip(ib[:, 0::2], 0, W - 1)
    ib[:, 1::2] = np.clip(ib[:, 1::2], 0, H - 1)
    valid = ((ib[:, 2] - ib[:, 0]) < W * 0.8) & ((ib[:, 3] - ib[:, 1]) < H * 0.8)
    assert np.array_equal(out["valid"][0].astype(bool), valid) and 0 < valid.sum() < valid.size
    rows = out["rows"][0]
    alpha = kitti_output.observation_angle(b).astype(np.float64)
    print("max |alpha - numpy| rel", float(np.max(np.abs(rows[:, 0] - alpha) / np.maximum(np.abs(alpha), 1.0))),
          "max image box diff px", float(np.max(np.abs(rows[:, 1:5] - ib))))
    assert np.all(np.abs(rows[:, 0] - alpha) <= 2e-6 * np.maximum(np.abs(alpha), 1.0))
    assert np.all(np.abs(rows[:, 1:5] - ib) <= 1e-4)
    assert np.array_equal(rows[:, 5:8], b[:, 3:6].astype(np.float64)) and np.array_equal(rows[:, 8:11], b[:, 0:3].astype(np.float64))
    assert np.array_equal(rows[:, 11], b[:, 6].astype(np.float64)) and np.array_equal(rows[:, 12], sc.astype(np.float64))
    assert kc.frame_lines(out, 0)[0].startswith("Car -1 -1 ")


def test_rows_are_the_numpy_arithmetic_with_the_host_libm_trig(host):
    """with glibc's cosf / sinf / atan2f (what ref_trig.h restates) in place of numpy's, the float32 parts agree to the bit"""
    exe, work = host
    libm = ctypes.CDLL("libm.so.6")
    for f in (libm.cosf, libm.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    libm.atan2f.restype, libm.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    batch = kc.make_batch((7,), n=2000)
    out = kc.run_lines(exe, work, batch)
    b = batch["boxes"][0]
    beta = np.array([libm.atan2f(float(z), float(x)) for x, z in zip(b[:, 0], b[:, 2])], np.float32)
    alpha = -np.sign(beta) * np.float32(np.pi) / np.float32(2) + beta + b[:, 6]
    assert alpha.dtype == np.float32 and np.array_equal(out["rows"][0][:, 0], alpha.astype(np.float64))
    c = np.array([libm.cosf(float(a)) for a in b[:, 6]], np.float32)[:, None]
    s = np.array([libm.sinf(float(a)) for a in b[:, 6]], np.float32)[:, None]
    h, w, l = b[:, 3:4], b[:, 4:5], b[:, 5:6]
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float32)
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float32)
    top = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.float32)
    xc, zc, yc = (l / np.float32(2)) * sx, (w / np.float32(2)) * sz, -h * top
    corners = np.stack([b[:, 0:1] + (xc * c + zc * s), b[:, 1:2] + yc, b[:, 2:3] + (xc * -s + zc * c)], axis=2).astype(np.float64)
    P = batch["P2"][0].reshape(3, 4)
    num = [(corners[..., 0] * P[r, 0] + corners[..., 1] * P[r, 1]) + corners[..., 2] * P[r, 2] + P[r, 3] for r in range(3)]
    u, v = num[0] / num[2], num[1] / num[2]
    H, W = batch["img_hw"][0]
    ib = np.stack([np.clip(u.min(1), 0, W - 1), np.clip(v.min(1), 0, H - 1), np.clip(u.max(1), 0, W - 1), np.clip(v.max(1), 0, H - 1)], axis=1)
    assert np.array_equal(out["rows"][0][:, 1:5], ib)
    assert np.array_equal(out["valid"][0].astype(bool), ((ib[:, 2] - ib[:, 0]) < W * 0.8) & ((ib[:, 3] - ib[:, 1]) < H * 0.8))


def compare_with_recorded(got, want, class_name="Car"):
    """the conditions against the reference's own lines -> (fields that differ, fields)"""
    assert len(got) == len(want)
    differ = total = 0
    for g, w in zip(got, want):
        gf, wf = g.split(" "), w.split(" ")
        assert gf[:3] == wf[:3] == [class_name, "-1", "-1"] and len(gf) == len(wf) == 16
        for a, b in zip(gf[3:], wf[3:]):
            total += 1
            if a != b:
                differ += 1
                assert abs(round(float(a) * 1e4) - round(float(b) * 1e4)) == 1, (a, b)
    return differ, total


def test_lines_against_the_reference_writer(host):
    exe, work = host
    g = np.load(os.path.join(GOLDEN, "kitti_output_ref.npz"))
    for seed in (1, 2):
        out = kc.run_lines(exe, work, kc.make_batch((seed,)))
        differ, total = compare_with_recorded(kc.frame_lines(out, 0), [str(x) for x in g["lines%d" % seed]])
        print("seed", seed, "fields that differ", differ, "of", total)
        assert total == 13 * len(g["lines%d" % seed]) and differ * 100 <= total


def test_lines_against_kitti_lines_on_a_large_frame(host):
    """2000 boxes through the numpy route (pinned to the reference's writer by the fixture above): the same conditions"""
    exe, work = host
    batch = kc.make_batch((7,), n=2000)
    out = kc.run_lines(exe, work, batch)
    want = kitti_output.kitti_lines(batch["boxes"][0], batch["scores"][0], batch["P2"][0].reshape(3, 4), batch["img_hw"][0])
    differ, total = compare_with_recorded(kc.frame_lines(out, 0), want)
    print("fields that differ", differ, "of", total)
    assert total > 20000 and differ * 100 <= total


def test_statuses_and_degenerate_frames(host):
    exe, work = host
    base = kc.make_batch((1, 2, 3, 4, 5))
    B, M = base["scores"].shape
    first = kc.run_lines(exe, work, base)
    kept = [np.flatnonzero(first["valid"][b]) for b in range(B)]
    dropped = [np.flatnonzero(first["valid"][b] == 0) for b in range(B)]
    assert all(len(k) and len(d) for k, d in zip(kept, dropped))
    batch = dict(base, num=np.array([0, M, M, M, M], np.int32), keep=np.tile(np.arange(M, dtype=np.int32), (B, 1)))
    batch["boxes"], batch["scores"] = base["boxes"].copy(), base["scores"].copy()
    batch["keep"][1, :len(dropped[1])] = dropped[1]                       # frame 1: only boxes the size test drops
    batch["num"][1] = len(dropped[1])
    batch["scores"][2, kept[2][3]] = np.nan                               # frame 2: a NaN score in a kept box
    batch["scores"][3, dropped[3][0]] = np.nan                            # frame 3: a NaN score in a dropped box
    batch["keep"][4, 5] = M                                               # frame 4: an index outside the frame
    out = kc.run_lines(exe, work, batch)
    assert out["status"].tolist() == [0, 0, 1, 0, 2]
    assert out["text_len"][[0, 1, 2, 4]].tolist() == [0, 0, 0, 0] and not out["text"][[0, 1, 2, 4]].any()
    assert not out["valid"][0].any() and not out["rows"][0].any()
    assert not out["valid"][1].any() and out["rows"][1, :len(dropped[1])].any()
    assert kc.frame_lines(out, 3) == kc.frame_lines(first, 3) and len(kc.frame_lines(out, 3)) == len(kept[3])
    # Pedestrian, a shuffled subset, and a num outside [0, M]
    r = np.random.default_rng(3)
    sub = r.permutation(M)[:17].astype(np.int32)
    keep = np.full((1, M), -1, np.int32)
    keep[0, :17] = sub
    out = kc.run_lines(exe, work, kc.make_batch((5,), class_name="Pedestrian", keep=keep, num=[17]))
    full = kc.run_lines(exe, work, kc.make_batch((5,), class_name="Pedestrian"))
    assert np.array_equal(out["rows"][0, :17], full["rows"][0][sub]) and not out["rows"][0, 17:].any()
    assert kc.frame_lines(out, 0) == kc.python_lines(full["rows"][0][sub], full["valid"][0][sub], "Pedestrian")
    assert kc.run_lines(exe, work, kc.make_batch((5,), num=[M + 1]))["status"].tolist() == [2]
    assert kc.run_lines(exe, work, kc.make_batch((5,), num=[-1]))["status"].tolist() == [2]


def test_a_corner_on_the_camera_plane_drops_the_box(host):
    exe, work = host
    batch = kc.make_batch((1,))
    batch["P2"][0, 11] = 0.0
    batch["boxes"][0, 7] = [0.0, 1.0, 0.0, 1.5, 2.0, 0.0, 0.0]            # l = 0, z = 0: every corner has depth 0 -> inf / NaN
    out = kc.run_lines(exe, work, batch)
    assert out["status"].tolist() == [0] and out["valid"][0, 7] == 0
    ref = kitti_output.kitti_lines(batch["boxes"][0], batch["scores"][0], batch["P2"][0].reshape(3, 4), batch["img_hw"][0])
    assert len(kc.frame_lines(out, 0)) == len(ref)


def test_export_binding_and_constants_agree():
    import re
    from pointrcnn_amd import _cabi, ops
    root = os.path.dirname(os.path.dirname(GOLDEN))
    header = open(os.path.join(root, "include", "prcnn_pointops.h")).read()
    m = re.search(r"^int prcnn_kitti_result_text\((.*?)\);", header, flags=re.S | re.M)
    assert m and len(m.group(1).split(",")) == len(_cabi.SIGNATURES["prcnn_kitti_result_text"][1]) == 15
    math_h = open(os.path.join(root, "pointrcnn_amd", "csrc", "kitti_text_math.h")).read()
    assert int(re.search(r"#define PRCNN_KITTI_LINE_MAX (\d+)", header).group(1)) == ops.KITTI_LINE_MAX == kc.LINE_MAX
    assert int(re.search(r"#define KT_LINE_MAX (\d+)", math_h).group(1)) == kc.LINE_MAX and ops.KITTI_FIELDS == kc.FIELDS
    lib = _cabi.lib()
    assert lib.prcnn_kitti_result_text(None, None, None, None, -1, 4, None, None, b"Car", None, None, None, None, None, None) == -1
    assert b"bad sizes" in lib.prcnn_last_error()
    assert lib.prcnn_kitti_result_text(None, None, None, None, 3, 0, None, None, b"Car", None, None, None, None, None, None) == 0
    assert lib.prcnn_kitti_result_text(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    # the unit is one of the bit-exact ones: compiled without contraction, like the rest of the library
    from pointrcnn_amd import build
    assert "-ffp-contract=off" in build.FLAGS and any(s.endswith("kitti_text.hip") for s in build.sources())
