"""CPU: the selection both RoI samplers share (pointrcnn_amd/csrc/roi_sample.h: candidate lists, slot plan, the draw without
replacement, the background picks) compiled for the host by tests/roi_sample_host.cpp -- once plain, once with
-fsanitize=address,undefined -- and run as a program, held EXACTLY to the two independent statements of that logic:

    online   the oracle (oracle/prcnn_oracle.c, its own generator, lists and case table): its max_overlaps in, counts / status / src out
    offline  the numpy twin (tests/rcnn_offline_twin.py): the row maxima and the column-argmax tail of its iou3d in, the same out

Everything the two kernels do differently around the header is an input of the driver, so each comparison runs the header the way
its kernel does."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import rcnn_offline_cases as rc
from util import GOLDEN

sys.path.insert(0, GOLDEN)
import ref_proposal_target as rpt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
F32 = np.float32
CFG = (0.55, 0.6, 0.45, 0.05, 0.5, 0.8)
ONLINE = dict(key_by_roi=1, fg_only_fills=1, streams=(10, 11, 12, 13))
OFFLINE = dict(key_by_roi=0, fg_only_fills=0, streams=(40, 41, 42, 43))      # 41 is never drawn from: fg_only_fills is 0
BOTH, FG_ONLY, BG_ONLY, NEITHER = range(4)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("roi_sample") / "roi_sample_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "roi_sample_host.cpp"), "-o", exe],
                   check=True)
    work = os.path.dirname(exe)

    def run(frames):
        """frames: dicts mo, tail, R, ng, seed, frame, cfg + ONLINE / OFFLINE -> per frame dict counts, status, kind, fs, bs, nh, src"""
        with open(os.path.join(work, "in.bin"), "wb") as f:
            for fr in frames:
                mo, tail = np.ascontiguousarray(fr["mo"], F32), np.ascontiguousarray(fr.get("tail", ()), np.int32)
                f.write(struct.pack("<12i", len(mo), len(tail), fr["R"], fr["ng"], fr["seed"], fr["frame"], fr["key_by_roi"],
                                    fr["fg_only_fills"], *fr["streams"]))
                f.write(struct.pack("<6d", *fr.get("cfg", CFG)) + mo.tobytes() + tail.tobytes())
        r = subprocess.run([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        words, out = np.fromfile(os.path.join(work, "out.bin"), np.int32), []
        for fr in frames:
            w, words = words[:9 + fr["R"]], words[9 + fr["R"]:]
            out.append(dict(counts=w[:4], status=int(w[4]), kind=int(w[5]), fs=int(w[6]), bs=int(w[7]), nh=int(w[8]), src=w[9:]))
        assert len(words) == 0
        return out
    return run


def live_gt(gt):
    """the rows of a padded ground truth up to its last row with a non-zero sum"""
    nz = np.flatnonzero(gt.sum(1) != 0)
    return int(nz[-1]) + 1 if len(nz) else 0


def online_frames(roi, gt, o, R, seed, cfg=CFG):
    return [dict(ONLINE, mo=o["max_overlaps"][b], R=R, ng=live_gt(gt[b]), seed=seed, frame=b, cfg=cfg) for b in range(len(roi))]


def assert_same(got, want_counts, want_status, want_src, tag):
    assert np.array_equal(got["counts"], want_counts), (tag, got["counts"], want_counts)
    assert got["status"] == want_status, (tag, got["status"], want_status)
    assert np.array_equal(got["src"], want_src), (tag, got["src"], want_src)
    # the plan is consistent with what it reports
    nfg, nbg = got["counts"][0], got["counts"][1] + got["counts"][2]
    if want_status != 2:
        assert got["kind"] == (BOTH if nfg and nbg else FG_ONLY if nfg else BG_ONLY if nbg else NEITHER), tag
        assert got["fs"] == got["counts"][3] and (got["fs"] + got["bs"] == (0 if want_status else len(want_src))) and 0 <= got["nh"] <= got["bs"], tag


_online = {}


def online_cases(cpu):
    """(tag, roi, gt, R, seed, cfg, oracle output), computed once"""
    if not _online:
        cases = []
        for seed in (1, 2, 3):
            roi, gt = rpt.scenes(seed)
            cases.append(("scenes(%d)" % seed, roi, gt, 64, 40 + seed, CFG))
        roi, gt = rpt.scenes(1)
        for fg_ratio in (0.5, 0.35):                   # test_slot_arithmetic_is_python_double_arithmetic
            cases.append(("R 20 ratios (%g, 0.7)" % fg_ratio, roi, gt, 20, 3, CFG[:4] + (fg_ratio, 0.7)))
        cases.append(("small frames",) + rpt.small_frames() + (8, 1, CFG))
        _online["v"] = [c + (cpu.proposal_target_sample(c[1], c[2], roi_per_image=c[3], cfgv=c[5], seed=c[4]),) for c in cases]
    return _online["v"]


def test_the_online_inputs_are_the_cases_they_are_named_after(cpu):
    cases = {c[0]: c[6] for c in online_cases(cpu)}
    assert cases["scenes(1)"]["counts"].tolist() == [[67, 105, 275, 32], [512, 0, 0, 64], [0, 4, 508, 0]]
    for seed in (1, 2, 3):                             # both / foreground only / background only
        c = cases["scenes(%d)" % seed]["counts"]
        assert (c[0, 0] > 32 and c[0, 1] > 0 and c[0, 2] > 0 and c[0, 3] == 32) and (c[1, 1] + c[1, 2] == 0 and c[1, 3] == 64) and c[2, 0] == 0
    o = cases["R 20 ratios (0.5, 0.7)"]
    assert o["counts"][0, 3] == 10 and int((o["max_overlaps"][0][o["src"][0][10:]] >= 0.05).sum()) == 7          # 10 * 0.7 = 7, not 6
    o = cases["R 20 ratios (0.35, 0.7)"]
    assert o["counts"][0, 3] == 7 and int((o["max_overlaps"][0][o["src"][0][7:]] >= 0.05).sum()) == int(13 * 0.7)
    o = cases["small frames"]
    assert o["counts"].tolist() == [list(c) for c in rpt.SMALL_COUNTS] and o["status"].tolist() == list(rpt.SMALL_STATUS)
    mo = o["max_overlaps"]
    assert abs(mo[1, 0] - 0.5168) < 1e-3 and abs(mo[2, 0] - 0.2921) < 1e-3
    assert (o["src"][[1, 4]] == -1).all() and (o["src"][[0, 2, 3, 5, 6]] >= 0).all()


def test_online_selection_equals_the_oracle(host, cpu):
    for tag, roi, gt, R, seed, cfg, o in online_cases(cpu):
        got = host(online_frames(roi, gt, o, R, seed, cfg))
        for b in range(len(roi)):
            assert_same(got[b], o["counts"][b], o["status"][b], o["src"][b], (tag, b))


def test_offline_selection_equals_the_twin(host):
    frames, want = [], []
    for name in rc.CASES:
        t = rc.twin_result(name, 3)
        iou = t["iou3d"]
        col, ra = iou.max(axis=0), iou.argmax(axis=0)
        frames.append(dict(OFFLINE, mo=iou.max(axis=1), tail=ra[col > 0], R=rc.CASES[name][1], ng=iou.shape[1], seed=rc.SEED, frame=3))
        want.append(t)
    got = host(frames)
    for name, g, t in zip(rc.CASES, got, want):
        assert_same(g, t["counts"], t["status"], t["src"], name)
    kinds = {g["kind"] for g in got}
    assert kinds == {BOTH, FG_ONLY, BG_ONLY}, kinds      # NEITHER: small frame 1 of the online test
