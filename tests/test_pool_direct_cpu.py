"""CPU: the host side of storing SA-level results by destination (prcnn_mlp_chain_group_multi_dst, prcnn_group_compact_pair_dst).

tests/pool_direct_host.cpp includes mlp.hip as host code with the launch macro recording instead of launching (the way
tests/mlp_launch_record.cpp does) and drives the old and the new multi export over the four RPN set-abstraction levels: without
destination lists the new export records the old one's launches, with them kernel instance, grid, block and LDS are unchanged.  It
also holds a plain C++ twin of the split's destination rule, checked on hand-made index rows.  A stand-alone program with its own
main: nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("sanitize", [False, True])
def test_destination_lists_change_no_launch(tmp_path, sanitize):
    exe = str(tmp_path / "pool_direct_host")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "pool_direct_host.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "0 failed", run.stdout[-4000:]
    # one launch per level, of the family the level is known to run on
    heads = {l.split(":")[0]: l for l in lines[:-1]}
    assert set(heads) == {"SA1", "SA2", "SA3", "SA4"}
    assert "sa0_multi_kernel" in heads["SA1"] and "chain_fast_multi_kernelILi3ELi2EE" in heads["SA2"]
    assert "stack2_multi_kernelILi2ELi2EE" in heads["SA3"] and "stack2_multi_kernelILi3ELi2EE" in heads["SA4"]


def test_the_new_exports_are_declared_where_the_old_ones_are():
    from pointrcnn_amd import _cabi
    header = open(os.path.join(ROOT, "include", "prcnn_pointops.h")).read()
    for name in ("prcnn_mlp_chain_group_multi_dst", "prcnn_group_compact_pair_dst", "prcnn_level_pool_residual"):
        assert name in _cabi.SIGNATURES and ("int %s(" % name) in header
    old, new = _cabi.SIGNATURES["prcnn_group_compact_pair"], _cabi.SIGNATURES["prcnn_group_compact_pair_dst"]
    assert len(new[1]) == len(old[1]) + 2                     # + rdst_a, rdst_b
    assert _cabi.SIGNATURES["prcnn_level_pool_residual"] == _cabi.SIGNATURES["prcnn_level_pool"]
    assert _cabi.REQUIRED_ABI == 12                            # additive: the version stays
