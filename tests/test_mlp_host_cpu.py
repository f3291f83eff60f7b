"""CPU: the host front-end of the fused MLPs (pointrcnn_amd/csrc/mlp_host.h).

tests/mlp_launch_record.cpp includes mlp.hip as host code with the launch macro recording instead of launching, and walks every
MLP export over a sweep of shapes, alignments and switches.  Its per-(switch setting, export) digests must equal
tests/golden/mlp_launch_digests.txt, recorded from the sources before the front-end was given one fill per operand mode and one
launch site: same kernel instance, grid, block, dynamic LDS, params, return code and message for every call.  The program also
checks prcnn_mlp_chain_supported against what the chain dispatch launches.  tests/golden/mlp_rejections.json holds invalid
calls with the code and message the library gave for them before that change."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("sanitize", [False, True])
def test_every_call_launches_what_it_launched_before(tmp_path, sanitize):
    exe = str(tmp_path / "mlp_launch_record")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "mlp_launch_record.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    want = open(os.path.join(GOLDEN, "mlp_launch_digests.txt")).read().splitlines()
    got = run.stdout.splitlines()
    assert want[-1].endswith(" 0 inconsistent") and len(want) == 241
    assert got[-1] == want[-1], got[-1]
    differ = [g for g, w in zip(got, want) if g != w]
    assert not differ, "launch records differ from the recorded ones in %d groups, first: %s" % (len(differ), differ[:5])


def _arg(v):
    """fixture argument -> ctypes: "A<i>" an aligned dummy pointer, "U<i>" one that is 4 bytes off, "F..." / "I..." host arrays"""
    if isinstance(v, str) and v[0] in "AU":
        return ctypes.c_void_p(0x10000 * (int(v[1:]) + 1) + (4 if v[0] == "U" else 0))
    if isinstance(v, dict):
        if "ptrs" in v:
            return (ctypes.c_void_p * len(v["ptrs"]))(*[_arg(p).value if p is not None else None for p in v["ptrs"]])
        return (ctypes.c_int * len(v["ints"]))(*v["ints"])
    return v


def test_invalid_calls_are_rejected_as_before():
    """every call fails its checks before anything is launched: the pointers are dummies"""
    from pointrcnn_amd import _cabi
    lib = _cabi.lib()
    cases = json.load(open(os.path.join(GOLDEN, "mlp_rejections.json")))
    assert len(cases) >= 60
    seen = set()
    for c in cases:
        keep = [_arg(a) for a in c["args"]]
        rc = getattr(lib, c["export"])(*keep)
        msg = lib.prcnn_last_error().decode() if rc == -1 else ""
        assert (rc, msg) == (c["rc"], c["message"]), (c["export"], c["what"], rc, msg)
        assert rc in (-1, -3), (c["export"], c["what"])
        seen.add(c["export"])
    assert seen == {"prcnn_mlp_rows", "prcnn_mlp_rows_split", "prcnn_mlp_rows_addinterp", "prcnn_mlp_rows_addinterp_split", "prcnn_mlp_group",
                    "prcnn_mlp_group_split", "prcnn_mlp_interp", "prcnn_mlp_chain_rows", "prcnn_mlp_chain_group", "prcnn_mlp_chain_interp",
                    "prcnn_mlp_chain_rows_split", "prcnn_mlp_chain_interp_split"}
