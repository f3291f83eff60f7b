"""CPU: the opt-in split-bf16 training GEMMs (train_mlp.TRAIN_SPLIT -> prcnn_train_stack_fwd_split / _bwd_split) reach exactly
the kernels tests/train_split_cases.py says, layer by layer, and the fp32 entry points launch what they launched before.

tests/train_split_launch_record.cpp includes mlp.hip -- and csrc/mlp_train.h -- as host code with the launch macro recording
instead of launching (tests/launch_record_prelude.h), built once plain and once with -fsanitize=address,undefined:
  * `--case`: every forward / dgrad GEMM of every new case runs the instantiation EXPECT names -- the split kernels narrow and
    wide, dgrad over the three POOL stagers, the fp32 kernels on the ineligible layers;
  * `--sweep` (rows 1 .. 2 M, widths 3 .. 512, every source, through the split entry points) finds no split instantiation the
    case table misses, and none outside SPLIT_VARIANTS;
  * `--fp32-case`: prcnn_train_stack_fwd / _bwd record, for every switch-free case of tests/train_stack_cases.py, the launch
    sequence (kernel, grid, block) of tests/golden/train_stack_fp32_launches.txt -- recorded from the sources before the split
    entry points existed -- and the same set of kernels tests/train_launch_record.cpp records.
The float64 reference's own decision-band share of every new case stays <= MAX_BAND_SHARE (the GPU test asserts the same on the
device's decisions), and the Python side exists: the exports, their ctypes signatures, train_mlp.TRAIN_SPLIT."""
import ctypes
import os
import subprocess
import sys

import pytest

import train_split_cases as S
import train_stack_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_stack_fp32_launches.txt")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")


def _build(src, exe, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", src), "-o", exe], check=True)


def _lines(exe, args):
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, (args, run.stderr[-2000:])
    return run.stdout.splitlines()


@needs_hipcc
@pytest.mark.parametrize("sanitize", [False, True])
def test_every_layer_gets_the_kernel_the_table_names(tmp_path, sanitize):
    exe = str(tmp_path / "train_split_launch_record")
    _build("train_split_launch_record.cpp", exe, sanitize)
    universe = set(_lines(exe, ["--sweep"]))
    split_seen = {n for n in universe if n.startswith(("train_fwd_s_kernel", "train_dgrad_s_kernel"))}
    assert split_seen == S.SPLIT_VARIANTS, sorted(split_seen ^ S.SPLIT_VARIANTS)
    assert S.SPLIT_PACKERS <= universe
    reached = set()
    for case in S.CASES:
        fwd, dgrad, also = [], {}, set()
        for line in _lines(exe, ["--case"] + S.recorder_args(case)):
            kind, rest = line.split(" ", 1)
            if kind == "fwd":
                layer, name = rest.split(" ", 1)
                assert int(layer) == len(fwd)
                fwd.append(name)
            elif kind == "dgrad":
                layer, name = rest.split(" ", 1)
                assert int(layer) not in dgrad
                dgrad[int(layer)] = name
            else:
                also.add(rest)
        want_fwd, want_dgrad = S.EXPECT[case.name]
        assert fwd == want_fwd, (case.name, fwd)
        assert dgrad == want_dgrad, (case.name, dgrad)
        # the fp32 weight image is still packed for every layer; the split images come next to it
        assert "train_pack_kernel" in also
        assert ("pack_weight_split_kernel" in also) == any(n.startswith("train_fwd_s_") for n in fwd), case.name
        assert ("train_pack_split_t_kernel" in also) == any(n.startswith("train_dgrad_s_") for n in dgrad.values()), case.name
        reached |= set(fwd) | set(dgrad.values()) | also
        assert reached <= universe, sorted(reached - universe)
    missing = S.SPLIT_VARIANTS - reached
    assert not missing, "split variants no case of tests/train_split_cases.py reaches: %s" % sorted(missing)
    assert any(n.startswith("train_fwd_kernel") for n in reached) and any(n.startswith("train_dgrad_kernel") for n in reached)


@needs_hipcc
def test_the_fp32_entry_points_launch_what_they_launched(tmp_path):
    new, old = str(tmp_path / "train_split_launch_record"), str(tmp_path / "train_launch_record")
    _build("train_split_launch_record.cpp", new, False)
    _build("train_launch_record.cpp", old, False)
    golden, name = {}, None
    with open(GOLDEN) as f:
        for line in f.read().splitlines():
            if line.startswith("# "):
                name = line[2:]
                golden[name] = []
            else:
                golden[name].append(line)
    cases = [c for c in T.CASES if not c.switches]
    assert sorted(golden) == sorted(c.name for c in cases)
    for case in cases:
        got = _lines(new, ["--fp32-case"] + S.recorder_args(case))
        assert got == golden[case.name], case.name
        assert not any("_s_kernel" in line or "split" in line for line in got), case.name
        names_old = {n for n in _lines(old, ["--case"] + case.recorder_args()) if not n.startswith("train_wgrad_kernel pool=")}
        assert {line.split(" grid ")[0] for line in got} == names_old, case.name


def test_new_cases_stay_out_of_the_decision_bands():
    """the share of ReLU decisions and arg-max slots float64 cannot tell, from the float64 reference's own decisions"""
    for case in S.CASES:
        I = T.build_inputs(case)
        rows = T.Rows(case, I)
        ref = T.reference(case, I, rows)
        inside, slots, total = T.band_share(case, ref)
        assert inside + slots <= T.MAX_BAND_SHARE * total, (case.name, inside, slots, total)
        T.check_decisions(case, ref, ref.mask, ref.arg)
        assert case.rows * max(a * b for a, b in zip(case.chans[:-1], case.chans[1:])) <= 6500 * 515 * 512, case.name


def test_the_table_holds_the_edges():
    rows = {c.rows for c in S.CASES if c.source == "plain"}
    assert {1, 63, 64, 65, 127, 128, 129, 6016, 6017} <= rows
    edge = [c for c in S.CASES if c.name.startswith("s_rows_")]
    assert {c.chans[0] for c in edge} == {32, 64, 96}
    assert {4, 28, 32, 36, 68, 132} <= {n for c in edge for n in c.chans[1:]}
    assert any(not c.bn for c in S.CASES) and any(not c.need_x for c in S.CASES)
    assert {"group", "flat", "interp"} <= {c.source for c in S.CASES}
    assert not set(S.BY_NAME) & set(T.BY_NAME)                 # (the seeds come from the names)


def test_exports_signatures_and_the_python_attribute():
    from pointrcnn_amd import _cabi
    with open(os.path.join(ROOT, "include", "prcnn_pointops.h")) as f:
        header = f.read()
    for name, extra in (("prcnn_train_stack_fwd_split", "prcnn_train_stack_fwd"), ("prcnn_train_stack_bwd_split", "prcnn_train_stack_bwd")):
        assert "int %s(" % name in header
        ret, args = _cabi.SIGNATURES[name]
        ret0, args0 = _cabi.SIGNATURES[extra]
        assert ret is ret0 and len(args) == len(args0) + 1                  # what the twin takes + the table
        assert [a for a in args if a not in args0] == [ctypes.POINTER(ctypes.c_void_p)]
    assert _cabi.REQUIRED_ABI == 12
    env = {k: v for k, v in os.environ.items() if k != "PRCNN_TRAIN_SPLIT"}
    code = "from pointrcnn_amd import train_mlp; print(train_mlp.TRAIN_SPLIT)"
    for value, want in ((None, "0"), ("1", "6"), ("6", "6"), ("0", "0"), ("3", None), ("yes", None)):
        e = dict(env) if value is None else dict(env, PRCNN_TRAIN_SPLIT=value)
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
        if want is None:
            assert run.returncode != 0 and "PRCNN_TRAIN_SPLIT" in run.stderr, (value, run.stderr[-500:])
        else:
            assert run.returncode == 0 and run.stdout.strip() == want, (value, run.stdout, run.stderr[-500:])
