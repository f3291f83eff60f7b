"""CPU: the case table of the training SharedMLP (tests/train_stack_cases.py) reaches every kernel variant its host code can pick.

tests/train_launch_record.cpp includes mlp.hip -- and with it csrc/mlp_train.h -- as host code with the launch macro recording
instead of launching (tests/launch_record_prelude.h, shared with tests/mlp_launch_record.cpp).  `--sweep` walks
prcnn_train_stack_fwd / _bwd over rows 1 .. 2 M, widths 3 .. 512, all sources, pooled / padding-free, BatchNorm / none, input
gradient wanted / not and both native switches: the universe of reachable instantiations.  `--case` records one case of the table.
The union over the table must EQUAL the universe, so a variant added to the dispatch without a case fails here, before any GPU
time is spent; the direct wgrad kernel's run-time forms (unpooled / pooled / padding-free pooled x operand prologue on / off)
must all be there too.  Built and run once plain and once with -fsanitize=address,undefined, as tests/test_mlp_host_cpu.py does.

`--digest` is the full record: the five stack exports and prcnn_train_stack_work_bytes over the union of the three training
recorders' sweeps, the four settings of PRCNN_TRAIN_FWD_GENERIC x PRCNN_WGRAD_DIRECT, operand variants that flip every
alignment-dependent choice and an invalid call per check of the host code; per call the return code, the message, and per launch
the instantiation, grid, block, dynamic LDS and every argument (parameter structs field by field).  Its per-(switch setting, export,
source) digests must equal tests/golden/train_launch_digests.txt, recorded from the sources before the host code was given a
per-layer plan and one launch table each for forward, wgrad and dgrad: this recorder built with -I on a checkout of that commit's
pointrcnn_amd/csrc (the parameter structs and the exports are the same), `train_launch_record --digest > the golden file`.  A
change that means to alter a launch re-records the file the same way and says so; `--digest-dump` prints the records to compare."""
import os
import subprocess

import pytest

import train_stack_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

WGRAD_FORMS = {"train_wgrad_kernel pool=%d pro=%d" % (pool, pro) for pool in range(3) for pro in range(2)}
DIRECT_TILINGS = {"train_wgrad_kernel<%s>" % t for t in ("1, 1, 1, 1", "1, 2, 1, 1", "1, 2, 1, 2", "2, 1, 1, 1", "2, 2, 1, 1", "2, 2, 1, 2", "2, 1, 2, 1",
                                                           "2, 2, 2, 1", "2, 2, 2, 2")}
LDS_FORMS = {"train_wgrad_lds_kernel<%d, %s, %s>" % (p, m, pro) for p, m in ((0, "false"), (0, "true"), (1, "false"), (2, "true"))
             for pro in ("false", "true")}
WIDE = {"train_fwd_kernel<0, 2, true>", "train_fwd_kernel<0, 2, false>", "train_fwd_kernel<1, 2, false>", "train_fwd_kernel<2, 2, false>",
        "train_dgrad_kernel<2, 0>", "train_dgrad_kernel<2, 1>", "train_dgrad_kernel<2, 2>"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("sanitize", [False, True])
def test_the_case_table_reaches_every_variant(tmp_path, sanitize):
    exe = str(tmp_path / "train_launch_record")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "train_launch_record.cpp"), "-o", exe],
                   check=True)

    def record(args):
        run = subprocess.run([exe] + args, capture_output=True, text=True)
        return run.returncode, set(run.stdout.splitlines()), run.stderr[-2000:]

    rc, universe, err = record(["--sweep"])
    assert rc == 0, err
    assert WGRAD_FORMS | DIRECT_TILINGS | LDS_FORMS | WIDE <= universe, sorted((WGRAD_FORMS | DIRECT_TILINGS | LDS_FORMS | WIDE) - universe)
    reached = {}
    for case in T.CASES:
        rc, names, err = record(["--case"] + case.recorder_args())
        assert rc == 0 and names, (case.name, err)
        for n in names:
            reached.setdefault(n, []).append(case.name)
    missing, unknown = universe - set(reached), set(reached) - universe
    assert not missing, "variants no case of tests/train_stack_cases.py reaches: %s" % sorted(missing)
    assert not unknown, "variants the sweep of tests/train_launch_record.cpp does not reach: %s" % sorted(unknown)
    for n, cases in reached.items():                           # the direct 128 x 128 tiling is reached under PRCNN_WGRAD_DIRECT only
        assert n != "train_wgrad_kernel<2, 2, 2, 2>" or all("PRCNN_WGRAD_DIRECT" in T.BY_NAME[c].switches for c in cases), cases
    # nsample 256 does not fit the uint8 pooling slot: refused before anything is launched
    rc, names, err = record(["--case", "group", "1024", "256", "1", "1", "0", "0", "3", "4"])
    assert rc == 1 and not names and "bad pooling arguments" in err, (rc, names, err)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("sanitize", [False, True])
def test_every_call_launches_what_it_launched(tmp_path, sanitize):
    exe = str(tmp_path / "train_launch_record")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "train_launch_record.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe, "--digest"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "train_launch_digests.txt")) as f:
        want = f.read().splitlines()
    assert [g.rsplit(" ", 2)[0] for g in got[:-1]] == [w.rsplit(" ", 2)[0] for w in want[:-1]]          # the same groups, in order
    changed = [g.rsplit(" ", 2)[0] for g, w in zip(got, want) if g != w]
    assert not changed, "calls that no longer launch (or refuse) what they did: %s" % changed
    assert got[-1] == want[-1] and len(got) == len(want)


def test_seeded_cases_stay_out_of_the_decision_bands():
    """the share of ReLU decisions and arg-max slots float64 cannot tell, from the float64 reference alone (its own decisions): every
    seeded case far inside the 1e-3 the GPU test allows; and the plain float32 CPU evaluation's per-entry ratios, from which the GPU
    test's bars derive, are the recorded ones (within a factor of 2: BLAS builds differ in their blocking)"""
    worst = {"dW": 0.0, "dx": 0.0}
    for case in T.CASES:
        I = T.build_inputs(case)
        rows = T.Rows(case, I)
        ref = T.reference(case, I, rows)
        inside, slots, total = T.band_share(case, ref)
        assert inside + slots <= T.MAX_BAND_SHARE * total, (case.name, inside, slots, total)
        T.check_decisions(case, ref, ref.mask, ref.arg)
        ratios = T.cpu_f32_ratios(case, I, rows, ref)
        worst = {k: max(worst[k], ratios[k]) for k in worst}
    for k in worst:
        assert T.CPU_F32_RATIO[k] / 2 <= worst[k] <= T.CPU_F32_RATIO[k] * 2, (k, worst[k], T.CPU_F32_RATIO[k])


def test_the_table_holds_the_edges_the_kernels_tile_by():
    rows = {c.rows for c in T.CASES}
    assert {1, 2, 63, 64, 65, 127, 128, 129, 6016, 6017} <= rows
    for (r, per, splits), rem in ((T.SPLIT_BELOW, -1), (T.SPLIT_ON, 0), (T.SPLIT_ABOVE, 1)):
        assert r in rows and splits >= 3 and r % per == rem % per
    k0 = {c.chans[0] for c in T.CASES}
    nout = {n for c in T.CASES for n in c.chans[1:]}
    assert {3, 4, 5, 31, 33, 65, 99, 515} <= k0 and {4, 28, 36, 68, 132} <= nout
    assert any(not c.bn and c.bias for c in T.CASES) and any(not c.bn and not c.bias for c in T.CASES)
    assert any(c.shape.get("ns") == 255 for c in T.CASES if c.source == "group") and any(not c.need_x for c in T.CASES)
    for c in T.CASES:                                          # (no case beyond about 6 500 rows x 515 x 512)
        assert c.rows * max(a * b for a, b in zip(c.chans[:-1], c.chans[1:])) <= 6500 * 515 * 512, c.name
