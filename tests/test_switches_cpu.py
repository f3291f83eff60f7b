"""CPU: the native A/B switches (pointrcnn_amd/csrc/switches.h) -- every call site's accessor against the getenv expression it
replaced, the snapshot as the loaded library reports it, the context manager that flips one in a running process, and the table
in INTEGRATION.md."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")


def table_names():
    text = open(os.path.join(CSRC, "switches.h")).read()
    names = ["PRCNN_" + m for m in re.findall(r"^\s*X\((\w+),\s*\"", text, flags=re.M)]
    assert len(names) == len(set(names)) >= 27
    return names


@pytest.mark.parametrize("sanitize", [False, True])
def test_every_call_site_reads_its_switch_as_the_getenv_expression_did(tmp_path, sanitize):
    exe = str(tmp_path / "switches_legacy_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "switches_legacy_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"^%d switches, \d+ call sites, 0 failures$" % len(table_names()), run.stdout, flags=re.M), run.stdout


def test_library_snapshot_and_the_context_manager():
    from pointrcnn_amd import _cabi
    from test_cabi_and_host import header_decls
    names = table_names()
    with _cabi.switches(**{n: None for n in names}):                      # a clean environment, whatever the caller's shell holds
        for n in names:
            assert _cabi.switch_get(n) == (False, 0), n
        with _cabi.switches(PRCNN_FPS_BATCH="1", PRCNN_NMS_PREFILTER="0"):
            assert os.environ["PRCNN_FPS_BATCH"] == "1" and os.environ["PRCNN_NMS_PREFILTER"] == "0"
            assert _cabi.switch_get("PRCNN_FPS_BATCH") == (True, 1)
            assert _cabi.switch_get("PRCNN_NMS_PREFILTER") == (True, 0)
            for n in names:
                if n not in ("PRCNN_FPS_BATCH", "PRCNN_NMS_PREFILTER"):
                    assert _cabi.switch_get(n) == (False, 0), n
        for n in names:
            assert _cabi.switch_get(n) == (False, 0) and n not in os.environ, n
        with pytest.raises(_cabi.PointOpsError, match="PRCNN_NO_SUCH_SWITCH"):
            _cabi.switch_get("PRCNN_NO_SUCH_SWITCH")
        with pytest.raises(_cabi.PointOpsError):
            with _cabi.switches(PRCNN_MLP_SPLIT="0"):                        # read in Python, not a switch of the library
                pass
        with pytest.raises(ZeroDivisionError):                               # the old values come back when the body raises
            with _cabi.switches(PRCNN_FPS_SLOTS="0"):
                1 / 0
        assert _cabi.switch_get("PRCNN_FPS_SLOTS") == (False, 0)
    lib = _cabi.lib()
    assert lib.prcnn_switch_get(b"PRCNN_NO_SUCH_SWITCH", None, None) == -1 and lib.prcnn_switch_get(None, None, None) == -1
    assert lib.prcnn_switch_get(b"PRCNN_FPS_SLOTS", None, None) == 0                     # null outputs are allowed
    # header == SIGNATURES == nm -D, at ABI 12
    decls = header_decls()
    assert "prcnn_switches_reload" in decls and "prcnn_switch_get" in decls
    assert sorted(decls) == sorted(_cabi.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.library_path()], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (prcnn_\w+)", out)) == set(decls)
    assert lib.prcnn_abi_version() == 12 and _cabi.REQUIRED_ABI == 12


def test_switch_table_is_documented_and_nothing_sets_a_switch_behind_the_snapshot():
    names = table_names()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index("### 3.1 Switches read inside the library"):doc.index("## 4. ")]
    assert sorted(re.findall(r"^\| `(PRCNN_\w+)` \|", section, flags=re.M)) == sorted(names)
    # only the switches implementation reads the environment
    for d in (CSRC, os.path.join(ROOT, "include")):
        for f in sorted(os.listdir(d)):
            if f != "switches.h":
                assert "getenv" not in open(os.path.join(d, f)).read(), f
    # a monkeypatch.setenv / os.environ[...] = / os.putenv of one of these names in a running process no longer reaches the library:
    # the code around it would run the default kernel twice and pass vacuously.  _cabi.switches(...) is the way.
    alt = "|".join(names)
    setters = re.compile(r"(?:setenv|putenv)\(\s*[\"'](?:%s)[\"']|environ\[\s*[\"'](?:%s)[\"']\s*\]\s*=(?!=)" % (alt, alt))
    for sub in ("tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith(".py"):
                    for no, line in enumerate(open(os.path.join(dirpath, f), errors="replace"), 1):
                        assert not setters.search(line), "%s:%d sets a native switch without _cabi.switches" % (os.path.join(dirpath, f), no)
