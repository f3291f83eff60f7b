"""CPU: the opt-in split-bf16 weight gradient of the wide training layers (train_mlp.TRAIN_SPLIT_WGRAD ->
prcnn_train_stack_bwd_wsplit -> train_wgrad_s_kernel) reaches exactly the kernels tests/train_wsplit_cases.py says, layer by
layer, and nothing else reaches the new kernel.

tests/train_wsplit_launch_record.cpp includes mlp.hip -- and csrc/mlp_train.h -- as host code with the launch macro recording
instead of launching (tests/launch_record_prelude.h), built once plain and once with -fsanitize=address,undefined as a stand-alone
program:
  * `--case wsplit`: the wgrad of every layer of every case is the instantiation EXPECT names -- all eight forms of
    train_wgrad_s_kernel on the wide layers, the direct kernels on the narrow ones -- and no layer runs train_wgrad_lds_kernel;
  * `--sweep wsplit` (rows 1 .. 2 M, widths 3 .. 515, every source) finds exactly WSPLIT_VARIANTS among the names starting with
    train_wgrad_s_kernel, all of them reached by the case table;
  * `--sweep split`, `--sweep fp32` and every case through those entry points: train_wgrad_s_kernel is never recorded, and each
    case launches train_wgrad_lds_kernel with the template arguments the new export gives train_wgrad_s_kernel.
The float64 reference's own decision-band share of every case stays <= MAX_BAND_SHARE (the GPU test asserts the same on the
device's decisions), and the Python side exists: the export in the header and _cabi.SIGNATURES with the parameter list of
prcnn_train_stack_bwd_split, ABI 12, train_mlp.TRAIN_SPLIT_WGRAD from PRCNN_TRAIN_SPLIT_WGRAD."""
import os
import re
import subprocess
import sys

import pytest

import train_split_cases as S
import train_stack_cases as T
import train_wsplit_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
NEW = "train_wgrad_s_kernel"


def _build(src, exe, sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", src), "-o", exe], check=True)


def _lines(exe, args):
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, (args, run.stderr[-2000:])
    return run.stdout.splitlines()


def _wgrads(exe, via, case):
    wgrad, also = [], set()
    for line in _lines(exe, ["--case", via] + WC.recorder_args(case)):
        kind, rest = line.split(" ", 1)
        if kind == "wgrad":
            layer, name = rest.split(" ", 1)
            assert int(layer) == len(wgrad)
            wgrad.append(name)
        else:
            also.add(rest)
    return wgrad, also


@needs_hipcc
@pytest.mark.parametrize("sanitize", [False, True])
def test_every_layer_gets_the_wgrad_kernel_the_table_names(tmp_path, sanitize):
    exe = str(tmp_path / "train_wsplit_launch_record")
    _build("train_wsplit_launch_record.cpp", exe, sanitize)
    universe = set(_lines(exe, ["--sweep", "wsplit"]))
    seen = {n for n in universe if n.startswith(NEW)}
    assert seen == WC.WSPLIT_VARIANTS, sorted(seen ^ WC.WSPLIT_VARIANTS)
    assert not any(n.startswith("train_wgrad_lds_kernel") for n in universe)        # (no switch set: every wide layer is taken)
    reached = set()
    for case in WC.CASES:
        wgrad, also = _wgrads(exe, "wsplit", case)
        assert wgrad == WC.EXPECT[case.name], (case.name, wgrad)
        assert "train_wgrad_reduce_kernel" in also and "bn_bwd_reduce_kernel" in also
        reached |= set(wgrad) | also
        assert reached <= universe, sorted(reached - universe)
        # through the two older entry points: the fp32 twin with the same template arguments, never the new kernel
        for via in ("split", "fp32"):
            old, also_old = _wgrads(exe, via, case)
            assert old == [n.replace(NEW, "train_wgrad_lds_kernel") for n in wgrad], (case.name, via, old)
            assert not any(NEW in n for n in also_old), (case.name, via)
    missing = WC.WSPLIT_VARIANTS - reached
    assert not missing, "split wgrad variants no case of tests/train_wsplit_cases.py reaches: %s" % sorted(missing)
    assert any(n.startswith("train_wgrad_kernel<") for n in reached)


@needs_hipcc
def test_the_older_entry_points_never_reach_the_new_kernel(tmp_path):
    exe = str(tmp_path / "train_wsplit_launch_record")
    _build("train_wsplit_launch_record.cpp", exe, False)
    for via in ("split", "fp32"):
        names = set(_lines(exe, ["--sweep", via]))
        assert any(n.startswith("train_wgrad_lds_kernel") for n in names), via
        assert not any(NEW in n for n in names), (via, sorted(n for n in names if NEW in n))


def test_new_cases_stay_out_of_the_decision_bands():
    """the share of ReLU decisions and arg-max slots float64 cannot tell, from the float64 reference's own decisions"""
    for case in WC.CASES:
        I = T.build_inputs(case)
        rows = T.Rows(case, I)
        ref = T.reference(case, I, rows)
        inside, slots, total = T.band_share(case, ref)
        assert inside + slots <= T.MAX_BAND_SHARE * total, (case.name, inside, slots, total)
        T.check_decisions(case, ref, ref.mask, ref.arg)
        assert case.rows * max(a * b for a, b in zip(case.chans[:-1], case.chans[1:])) <= 6500 * 515 * 512, case.name


def test_the_table_holds_the_edges():
    plain = [c for c in WC.CASES if c.source == "plain"]
    assert {1, 15, 16, 17, 31, 32, 33, 511, 512, 513, 1025} <= {c.rows for c in plain}
    widths = {(k, n) for c in WC.CASES for k, n in zip(c.chans[:-1], c.chans[1:])}
    assert {(68, 68), (128, 128), (132, 68), (68, 132), (96, 128)} <= widths and any(n == 196 for _, n in widths)
    assert {"group", "flat", "interp"} <= {c.source for c in WC.CASES}
    assert any(not c.bn for c in WC.CASES)
    assert any(c.source == "group" and c.chans[0] > 64 + 3 for c in WC.CASES)          # rotated [feat | dxyz] columns in a wide layer
    mixed = WC.EXPECT[WC.MIXED]
    assert all(mixed[l].startswith(NEW) for l in WC.MIXED_WIDE_LAYERS)
    assert all(mixed[l].startswith("train_wgrad_kernel<") for l in WC.MIXED_NARROW_LAYERS)
    assert set(WC.REPEAT_CASES) <= set(WC.BY_NAME)
    assert not set(WC.BY_NAME) & (set(T.BY_NAME) | set(S.BY_NAME))                     # (the seeds come from the names)


def test_export_signature_and_the_python_attribute():
    from pointrcnn_amd import _cabi
    with open(os.path.join(ROOT, "include", "prcnn_pointops.h")) as f:
        header = f.read()

    def params(name):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        return " ".join(m.group(1).split())
    assert params("prcnn_train_stack_bwd_wsplit") == params("prcnn_train_stack_bwd_split")
    assert _cabi.SIGNATURES["prcnn_train_stack_bwd_wsplit"] == _cabi.SIGNATURES["prcnn_train_stack_bwd_split"]
    assert _cabi.REQUIRED_ABI == 12
    with open(os.path.join(CSRC, "cabi_common.hip")) as f:
        assert "prcnn_abi_version(void) { return 12; }" in f.read()
    env = {k: v for k, v in os.environ.items() if k not in ("PRCNN_TRAIN_SPLIT", "PRCNN_TRAIN_SPLIT_WGRAD")}
    code = "from pointrcnn_amd import train_mlp; print(train_mlp.TRAIN_SPLIT_WGRAD, train_mlp.TRAIN_SPLIT)"
    for value, want in ((None, "0 0"), ("", "0 0"), ("1", "6 0"), ("6", "6 0"), ("0", "0 0"), ("3", None), ("yes", None)):
        e = dict(env) if value is None else dict(env, PRCNN_TRAIN_SPLIT_WGRAD=value)
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
        if want is None:
            assert run.returncode != 0 and "PRCNN_TRAIN_SPLIT_WGRAD" in run.stderr, (value, run.stderr[-500:])
        else:
            assert run.returncode == 0 and run.stdout.strip() == want, (value, run.stdout, run.stderr[-500:])
    # independent of PRCNN_TRAIN_SPLIT
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, PRCNN_TRAIN_SPLIT="1"), capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "0 6", (run.stdout, run.stderr[-500:])
