"""CPU: the workgroup table of the multi-problem launches (pointrcnn_amd/csrc/level_units.h), compiled for the host by
tests/level_units_host.cpp -- once plain, once with -fsanitize=address,undefined.

A launch that carries the grouped stacks of a whole set-abstraction level gives every problem a run of consecutive workgroups;
a workgroup finds (problem, local index, local count) and the problem's kernel body strides over its work units by the local
count.  Checked here, by walking every workgroup of every case: each unit of each problem is visited exactly once; no workgroup
falls outside its problem; a share never exceeds what the problem asked for; a capped grid is used in full; and no division --
by the problems' own grids or by weights (the resident slots of persistent bodies dealt by row bound) -- leaves a problem that
has work without a workgroup."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("level_units") / "level_units_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "level_units_host.cpp"), "-o", exe],
                   check=True)

    def run(cases):
        """cases: (cap, want, weight or None, units) -> one list of ints per case"""
        text = ""
        for cap, want, weight, units in cases:
            n = len(want)
            text += " ".join(str(int(v)) for v in [n, cap] + list(want) + list(weight if weight is not None else [-1] * n) + list(units)) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


def test_uncapped_launch_is_the_sum_of_the_problems_own_grids(host):
    cases = [(0, [7], None, [7]),
             (0, [10, 20], None, [10, 20]),
             (0, [2048, 1024, 8192, 4096], None, [300, 5, 0, 0]),          # SA2: the dense lists' workgroups find no unit
             (0, [512, 768, 512, 768], None, [5000, 4100, 3, 0]),           # SA1: persistent bodies, more units than workgroups
             (0, [0, 5, 0, 3], None, [0, 11, 0, 3]),                        # problems without rows take no workgroup
             (0, [0, 0], None, [0, 0]),
             (4096, [10, 20, 30], None, [10, 20, 30])]                      # a cap the sum stays under changes nothing
    got = host(cases)
    for (cap, want, _, _), g in zip(cases, got):
        assert g == [sum(want)] + list(want) + [1], (want, g)


def test_capped_grid_is_dealt_in_proportion_and_bodies_stride_across_it(host):
    cases = [(15, [10, 20], None, [10, 20]),
             (2048, [2048, 2048], None, [9000, 1]),                         # SA3 / SA4: two stacks under the single launch's cap
             (2048, [2048, 512], None, [2048 * 3, 700]),
             (512, [512, 512, 512, 512], [4, 8, 16, 32], [4700, 5300, 40, 0]),      # resident slots by row bound
             (512, [512, 3, 512, 512], [4, 8, 16, 32], [4700, 3, 40, 0]),           # a share clipped to what the problem wants
             (4, [100, 100, 100, 100], [1, 1000000, 1, 1], [100, 100, 100, 100]),   # cap == live problems: one workgroup each
             (5, [100, 0, 100, 100], [1, 7, 1000000, 1], [100, 0, 100, 100]),
             (6, [1, 1, 1, 50], None, [1, 1, 1, 5000])]
    got = host(cases)
    assert got[0] == [15, 6, 9, 1]
    assert got[1] == [2048, 1024, 1024, 1] and got[2][0] == 2048 and got[2][-1] == 1
    assert got[3] == [512, 37, 68, 136, 271, 1]                             # 1 + 508 w / 60 each, the three left over to the first
    assert got[4] == [512, 37 + 65, 3, 136, 271, 1]                         # ... what the clipped one leaves, too
    assert got[5] == [4, 1, 1, 1, 1, 1]
    assert got[6] == [5, 2, 0, 2, 1, 1]                                     # (2 * 10^6 / 1000002 rounds down to 1; the one left over goes to the first)
    assert got[7] == [6, 1, 1, 1, 3, 1]
    for (cap, want, _, _), g in zip(cases, got):
        assert g[0] == min(cap, sum(want)) and g[-1] == 1 and all(1 <= s <= w or (w == 0 and s == 0) for s, w in zip(g[1:-1], want)), (want, g)


def test_random_cases_visit_every_unit_once(host):
    rng = np.random.default_rng(20250611)
    cases = []
    for _ in range(400):
        n = int(rng.integers(1, 5))
        want = [int(v) for v in rng.choice([0, 1, 2, 3, 17, 256, 768, 2048], n)]
        live = sum(1 for w in want if w)
        cap = int(rng.choice([0, live, live + 1, 8, 512, 2048, 10000])) if live else 0
        cap = cap if cap == 0 or cap >= live else live
        weight = [int(v) for v in rng.choice([0, 1, 5, 1000, 1 << 33], n)] if rng.random() < 0.5 else None
        units = [int(rng.choice([0, 1, w, 3 * w + 1, 40 * w])) if w else 0 for w in want]
        cases.append((cap, want, weight, units))
    for (cap, want, _, _), g in zip(cases, host(cases)):
        assert g[-1] == 1 and g[0] == (sum(want) if cap == 0 else min(cap, sum(want))), (cap, want, g)


def test_refused_requests(host):
    cases = [(1, [5, 5], None, [5, 5]),                # a cap below the number of problems that have work
             (0, [-1], None, [0]),
             (8, [5, 5], [3, -2], [5, 5])]
    assert host(cases) == [[-1], [-1], [-1]]
