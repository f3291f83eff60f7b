"""CPU: the third split-bf16 opt-in of the training SharedMLP (train_mlp.TRAIN_SPLIT_ALL -> prcnn_train_stack_fwd_split_all /
_bwd_split_all) reaches exactly the kernels tests/train_split_all_cases.py says, layer by layer, with ONE split-packing launch per
call, and the five older exports reach none of the new kernels.

tests/train_split_all_launch_record.cpp includes mlp.hip -- and csrc/mlp_train.h -- as host code with the launch macro recording
instead of launching (tests/launch_record_prelude.h), built once plain and once with -fsanitize=address,undefined:
  * `--case`: every forward / dgrad GEMM of every case runs the instantiation EXPECT names; train_pack_split_all_kernel is launched
    as often as EXPECT says (once per call), the per-layer split packers never, train_pack_kernel still; the two forms that are
    narrow at a wide shape run ceil(blocks / 2) workgroups per tile; the wgrad_split flag moves the wide layers' wgrad and nothing else;
  * `--sweep` (rows 1 .. 2 M, widths 3 .. 515, every source, both flag values) finds exactly NEW_VARIANTS among the new kernels;
  * `--old-case`: prcnn_train_stack_fwd / _bwd, _fwd_split / _bwd_split and _bwd_wsplit record no new kernel and no new packer on any
    of these cases.  (That their launch sequences are what they were is tests/test_train_split_cpu.py's and
    tests/test_train_wsplit_cpu.py's, unchanged.)
The split image: a numpy twin of train_pack_split_all_kernel (`twin_planes`, `twin_bytes`; the GPU test compares the device's bytes
with it) -- the three bf16 planes sum back to the fp32 weight exactly, every padding element is +0 in every plane, the rotation is
train_pack_kernel's, the transposed form leaves the xyz columns out; where the width is a multiple of 32 the bytes are those of the
existing split (pack_weight_split_kernel's chain = 0 layout, restated here).  The packer's index arithmetic itself
(csrc/train_split_index.h) is walked by tests/train_split_index_host.cpp under -fsanitize=address,undefined.
Further: the float64 reference's own decision-band share of every case stays <= MAX_BAND_SHARE, the table holds the edges the
kernels have, and the Python side exists: the exports, their ctypes signatures, train_mlp.TRAIN_SPLIT_ALL."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import train_split_all_cases as A
import train_stack_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointrcnn_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _build(exe, sanitize):
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function", "-Wno-unused-value",
                    "-Wl,--unresolved-symbols=ignore-all"] + (SAN if sanitize else [])
                   + ["-I", CSRC, os.path.join(ROOT, "tests", "train_split_all_launch_record.cpp"), "-o", exe], check=True)


def _lines(exe, args):
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, (args, run.stderr[-2000:])
    return run.stdout.splitlines()


def _record(exe, case, wg):
    fwd, dgrad, grid_y, also, packs = [], {}, {}, set(), None
    for line in _lines(exe, ["--case", str(wg)] + A.recorder_args(case)):
        kind, rest = line.split(" ", 1)
        if kind in ("fwd", "dgrad"):
            layer, rest = rest.split(" ", 1)
            name, gy = rest.rsplit(" ", 1)
            grid_y[(case.name, kind, int(layer))] = int(gy)
            if kind == "fwd":
                assert int(layer) == len(fwd)
                fwd.append(name)
            else:
                assert int(layer) not in dgrad
                dgrad[int(layer)] = name
        elif kind == "packs":
            packs = tuple(int(x) for x in rest.split())
        else:
            also.add(rest)
    return fwd, dgrad, packs, also, grid_y


def _is_new(name):
    return name.startswith(("train_fwd_sa_kernel", "train_dgrad_sa_kernel", A.NEW_PACKER))


@needs_hipcc
@pytest.mark.parametrize("sanitize", [False, True])
def test_every_layer_gets_the_kernel_the_table_names(tmp_path, sanitize):
    exe = str(tmp_path / "train_split_all_launch_record")
    _build(exe, sanitize)
    universe = set(_lines(exe, ["--sweep"]))
    new_seen = {n for n in universe if n.startswith(("train_fwd_sa_kernel", "train_dgrad_sa_kernel"))}
    assert new_seen == A.NEW_VARIANTS, sorted(new_seen ^ A.NEW_VARIANTS)
    assert A.NEW_PACKER in universe and not (A.OLD_SPLIT_PACKERS & universe)
    reached = set()
    for case in A.CASES:
        fwd, dgrad, packs, also, grid_y = _record(exe, case, 0)
        want_fwd, want_dgrad, want_packs = A.EXPECT[case.name]
        assert fwd == want_fwd, (case.name, fwd)
        assert dgrad == want_dgrad, (case.name, dgrad)
        # one split-packing launch per call (none where the call splits nothing); the fp32 images are still packed for every layer
        assert packs == want_packs, (case.name, packs)
        split_f = any("_s_kernel" in n or "_sa_kernel" in n for n in fwd)
        split_b = any("_s_kernel" in n or "_sa_kernel" in n for n in dgrad.values())
        assert packs == (int(split_f), int(split_b)), case.name
        assert "train_pack_kernel" in also and not (A.OLD_SPLIT_PACKERS & also), (case.name, sorted(also))
        assert not any(n.startswith("train_wgrad_s_kernel") for n in also), case.name
        for key, want in A.NARROW_GRID_Y.items():
            if key[0] == case.name:
                assert grid_y[key] == want, (key, grid_y[key])
        # the flag: the same forward / dgrad kernels, the LDS-staged wgrad replaced by its split twin and nothing else
        fwd1, dgrad1, packs1, also1, _ = _record(exe, case, 1)
        assert (fwd1, dgrad1, packs1) == (fwd, dgrad, packs), case.name
        swap = lambda names: {n.replace("train_wgrad_lds_kernel", "train_wgrad_s_kernel") for n in names}      # noqa: E731
        assert also1 == swap(also) and not any(n.startswith("train_wgrad_lds_kernel") for n in also1), case.name
        reached |= set(fwd) | set(dgrad.values()) | also | also1
    assert reached <= universe | {n for n in reached if not _is_new(n)}
    missing = A.NEW_VARIANTS - reached
    assert not missing, "new variants no case of tests/train_split_all_cases.py reaches: %s" % sorted(missing)
    assert any(n.startswith("train_wgrad_s_kernel") for n in reached), "no case has a wide layer for the wgrad_split flag"


@needs_hipcc
def test_the_older_exports_reach_no_new_kernel(tmp_path):
    exe = str(tmp_path / "train_split_all_launch_record")
    _build(exe, False)
    for case in A.CASES:
        for via in ("fp32", "split", "wsplit"):
            names = _lines(exe, ["--old-case", via] + A.recorder_args(case))
            assert names and not [n for n in names if _is_new(n)], (case.name, via)
            if via == "fp32":
                assert not [n for n in names if "_s_kernel" in n or "split" in n], case.name


# ---- the split image, in numpy ---------------------------------------------------------------------------------------------------
def split3(x):
    """csrc/mlp.hip split3 on a float32 array -> three uint16 arrays (bf16 bit patterns): the top halves of x, of x - top(x) and of
    that remainder's remainder (both differences are exact in float32)"""
    x = np.ascontiguousarray(x, np.float32)
    top = lambda b: (b & np.uint32(0xFFFF0000)).view(np.float32)      # noqa: E731
    b0 = x.view(np.uint32)
    r1 = (x - top(b0)).astype(np.float32)
    b1 = r1.view(np.uint32)
    r2 = (r1 - top(b1)).astype(np.float32)
    b2 = r2.view(np.uint32)
    return [(b >> np.uint32(16)).astype(np.uint16) for b in (b0, b1, b2)]


def twin_source(W, rot, transposed):
    """the (image rows x reduction width) fp32 matrix an image holds, before padding: forward W with its columns rotated as
    train_pack_kernel rotates them (column k <- W[:, (k + rot) mod K]); transposed W[:, rot:]^T (the xyz columns left out)"""
    W = np.asarray(W, np.float32)
    return np.ascontiguousarray(W[:, rot:].T) if transposed else np.roll(W, -rot, axis=1)


def twin_planes(W, rot=0, transposed=False):
    """-> (3, NB * 32, KS * 16) uint16: the three bf16 planes of the zero-padded image, KS = 2 ceil(width / 32)"""
    M = twin_source(W, rot, transposed)
    rows, width = M.shape
    P = np.zeros((-(-rows // 32) * 32, -(-width // 32) * 32), np.float32)
    P[:rows, :width] = M
    return np.stack(split3(P))


def twin_bytes(planes):
    """the planes in the kernels' layout [column block][k-step][piece][lane][8 bf16]: lane (h, j) holds row 32 nb + j, k = 16 ks + 8 h + e"""
    _, R, Kp = planes.shape
    NB, KS = R // 32, Kp // 16
    v = planes.reshape(3, NB, 32, KS, 2, 8)                        # piece, nb, j, ks, h, e
    return np.ascontiguousarray(v.transpose(1, 3, 0, 4, 2, 5)).reshape(-1).view(np.uint8)          # nb, ks, piece, h, j, e


def existing_split_bytes(W):
    """pack_weight_split_kernel's chain = 0 image of a (Nout x K) weight, restated from its index arithmetic (KS = ceil(K / 16))"""
    W = np.asarray(W, np.float32)
    Nout, K = W.shape
    NB, KS = -(-Nout // 32), -(-K // 16)
    out = np.zeros((NB * KS * 3 * 64, 8), np.uint16)
    for nb in range(NB):
        for ks in range(KS):
            for lane in range(64):
                n, hh = nb * 32 + (lane & 31), lane >> 5
                k = ks * 16 + 8 * hh + np.arange(8)
                v = np.where((n < Nout) & (k < K), W[min(n, Nout - 1), np.minimum(k, K - 1)], np.float32(0)).astype(np.float32)
                for p, piece in enumerate(split3(v)):
                    out[((nb * KS + ks) * 3 + p) * 64 + lane] = piece
    return out.reshape(-1).view(np.uint8)


IMAGE_SHAPES = ((32, 36, 0), (64, 99, 3), (196, 128, 0))


@pytest.mark.parametrize("shape", IMAGE_SHAPES, ids=["%dx%d_rot%d" % s for s in IMAGE_SHAPES])
@pytest.mark.parametrize("transposed", [False, True])
def test_the_padded_image_twin(shape, transposed):
    Nout, K, rot = shape
    rng = np.random.default_rng(7 + Nout + K)
    W = (rng.standard_normal((Nout, K)) / np.sqrt(K)).astype(np.float32)
    W[0, 0], W[1, min(5, K - 1)], W[2, K - 1] = 0.0, np.float32(2.0 ** -100), np.float32(-3.0e4)      # zero, tiny, large
    planes = twin_planes(W, rot, transposed)
    M = twin_source(W, rot, transposed)
    rows, width = M.shape
    assert planes.shape == (3, -(-rows // 32) * 32, -(-width // 32) * 32) and planes.shape[2] % 32 == 0
    # the three planes sum back to the weight exactly (each bf16 piece widened is a float32; the sum is exact in float64)
    val = (planes.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64).sum(0)
    assert np.array_equal(val[:rows, :width], M.astype(np.float64))
    # every padding element is +0 in every plane (bit pattern 0: not -0, not a remainder)
    pad = np.ones(planes.shape[1:], bool)
    pad[:rows, :width] = False
    assert bool(pad.any()) == bool(rows % 32 or width % 32) and not planes[:, pad].any()      # (96 x 64, the transposed 64 x 99: no padding)
    # the rotation is train_pack_kernel's: image column kp reads W's column kp + rot below K - rot, kp - (K - rot) from there
    if not transposed:
        kp = np.arange(K)
        ko = np.where(kp < K - rot, kp + rot, kp - (K - rot))
        assert np.array_equal(M, W[:, ko])
    else:
        assert M.shape == (K - rot, Nout) and np.array_equal(M, W.T[rot:])
    # the byte layout: one 16-byte lane per (block, k-step, piece, lane), and -- where nothing is padded in k and nothing rotated --
    # the bytes of the existing split image
    img = twin_bytes(planes)
    assert img.size == planes.shape[1] // 32 * (planes.shape[2] // 16) * 3 * 1024
    if width % 32 == 0 and rot == 0:
        assert np.array_equal(img, existing_split_bytes(M))
    lane = img.view(np.uint16).reshape(planes.shape[1] // 32, planes.shape[2] // 16, 3, 2, 32, 8)
    assert np.array_equal(lane[1 if rows > 32 else 0, 1, 2, 1, 3], planes[2, (32 if rows > 32 else 0) + 3, 16 + 8: 16 + 16])


def test_the_packer_index_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "train_split_index_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + SAN
                   + ["-I", CSRC, os.path.join(ROOT, "tests", "train_split_index_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.stdout, run.stderr[-2000:])


def test_wsplit_bytes_counts_whole_chunks():
    from pointrcnn_amd import _cabi
    L = _cabi.lib()
    for nout, k in ((32, 32), (64, 128), (196, 512), (128, 64)):          # multiples of 32: what it returned before
        assert L.prcnn_wsplit_bytes(nout, k) == -(-nout // 32) * (k // 16) * 3 * 1024
    for nout, k in ((32, 36), (64, 99), (196, 100), (35, 33), (512, 515)):
        assert L.prcnn_wsplit_bytes(nout, k) == -(-nout // 32) * (-(-k // 32) * 2) * 3 * 1024
        W = np.zeros((nout, k), np.float32)
        assert L.prcnn_wsplit_bytes(nout, k) == twin_bytes(twin_planes(W)).size


def test_new_cases_stay_out_of_the_decision_bands():
    """the share of ReLU decisions and arg-max slots float64 cannot tell, from the float64 reference's own decisions"""
    for case in A.CASES:
        I = T.build_inputs(case)
        rows = T.Rows(case, I)
        ref = T.reference(case, I, rows)
        inside, slots, total = T.band_share(case, ref)
        assert inside + slots <= T.MAX_BAND_SHARE * total, (case.name, inside, slots, total)
        T.check_decisions(case, ref, ref.mask, ref.arg)
        assert case.rows * max(a * b for a, b in zip(case.chans[:-1], case.chans[1:])) <= 6500 * 515 * 512, case.name


def test_the_table_holds_the_edges():
    import train_split_cases as S
    edge = [c for c in A.CASES if c.name.startswith("a_rows_")]
    assert {c.rows for c in edge} == {1, 63, 64, 65, 127, 128, 129}
    split_k = {k for c in edge for f, k in zip(A.EXPECT[c.name][0], c.chans[:-1]) if f.startswith("train_fwd_sa_")}
    split_n = {c.chans[l + 1] for c in edge for l, d in A.EXPECT[c.name][1].items() if d.startswith("train_dgrad_sa_")}
    assert split_k >= {36, 100, 196} and split_n >= {36, 68, 100, 196}
    assert A.EXPECT["a_rows_129"][0][0].startswith("train_fwd_kernel") and BY("a_rows_129").chans[0] == 28
    assert A.EXPECT["a_rows_63"][1][1].startswith("train_dgrad_kernel") and BY("a_rows_63").chans[2] == 28
    for src in ("group", "flat"):
        ks = {c.chans[0]: A.EXPECT[c.name][0][0] for c in A.CASES if c.source == src}
        assert {19, 35, 61, 99} <= set(ks) and ks[19].startswith("train_fwd_kernel<1")
        assert all(ks[k].startswith("train_fwd_sa_kernel<1") for k in (35, 61, 99))
    assert {c.chans[0] for c in A.CASES if c.source == "interp" and c.shape["C1"] == 7} == {37, 72}
    deep = BY("a_deep")
    assert deep.chans[0] == 515 and deep.rows == 130
    assert any(not c.bn and c.rows > 1 for c in A.CASES) and any(not c.need_x for c in A.CASES)
    for name in ("a_group_wide", "a_flat_wide"):
        c = BY(name)
        assert c.chans == [35, 512, 64] and (c.shape["B"], c.shape["N"], c.shape["M"], c.shape["ns"]) == (2, 400, 50, 64)
    mixed = BY("a_mixed")
    assert mixed.chans[0] == 33 and A.EXPECT["a_mixed"][0] == [A.FF(0, 1, False), A.FA(0, 1), A.FA(0, 1)]
    assert not set(A.BY_NAME) & (set(T.BY_NAME) | set(S.BY_NAME))          # (the seeds come from the names)


def BY(name):
    return A.BY_NAME[name]


def test_exports_signatures_and_the_python_attribute():
    from pointrcnn_amd import _cabi
    with open(os.path.join(ROOT, "include", "prcnn_pointops.h")) as f:
        header = f.read()
    tab = ctypes.POINTER(ctypes.c_void_p)
    for name, twin, extra in (("prcnn_train_stack_fwd_split_all", "prcnn_train_stack_fwd_split", []),
                              ("prcnn_train_stack_bwd_split_all", "prcnn_train_stack_bwd_wsplit", [ctypes.c_int])):
        assert "int %s(" % name in header
        ret, args = _cabi.SIGNATURES[name]
        ret0, args0 = _cabi.SIGNATURES[twin]
        assert ret is ret0 and list(args) == list(args0) + extra and tab in args
        assert callable(getattr(_cabi.lib(), name))
    assert _cabi.REQUIRED_ABI == 12                                     # additive: the ABI number stays
    env = {k: v for k, v in os.environ.items() if not k.startswith("PRCNN_TRAIN_SPLIT")}
    code = "from pointrcnn_amd import train_mlp as t; print(t.TRAIN_SPLIT_ALL, t.TRAIN_SPLIT, t.TRAIN_SPLIT_WGRAD)"
    for value, want in ((None, "0 0 0"), ("1", "6 0 0"), ("6", "6 0 0"), ("0", "0 0 0"), ("3", None), ("yes", None)):
        e = dict(env) if value is None else dict(env, PRCNN_TRAIN_SPLIT_ALL=value)
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
        if want is None:
            assert run.returncode != 0 and "PRCNN_TRAIN_SPLIT_ALL" in run.stderr, (value, run.stderr[-500:])
        else:
            assert run.returncode == 0 and run.stdout.strip() == want, (value, run.stdout, run.stderr[-500:])
    # the other two variables keep their meaning next to it
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, PRCNN_TRAIN_SPLIT_ALL="1", PRCNN_TRAIN_SPLIT_WGRAD="1"),
                         capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "6 0 6", (run.stdout, run.stderr[-500:])
