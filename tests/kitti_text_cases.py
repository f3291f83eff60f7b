"""Shared inputs and helpers of the KITTI result-text tests (test_kitti_text_cpu.py, test_gpu_kitti_text.py): the host twin
tests/kitti_text_host.cpp, batches built from tests/golden/ref_kitti_output.cases, the formatter's edge values."""
import os
import struct
import subprocess
import sys

import numpy as np

from util import GOLDEN

sys.path.insert(0, GOLDEN)
from ref_kitti_output import cases  # noqa: E402

LINE_MAX = 256
FIELDS = 13
F32 = np.float32
# values every formatter test includes: signed zeros, a negative that rounds to zero, an integer, the top of the domain
EDGE_VALUES = [0.0, -0.0, -1e-5, 1e-5, 1241.0, 2.0 ** 31 - 1, -(2.0 ** 31 - 1), 0.00005, -0.00005, 0.99995, 9.99995, 2147483647.99999]


def build_host(workdir, sanitize):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "kitti_text_host" + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(root, "tests", "hip_stub"), "-I", os.path.join(root, "pointrcnn_amd", "csrc"),
                    os.path.join(root, "tests", "kitti_text_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode, workdir, payload):
    fin, fout = os.path.join(str(workdir), "kt_in.bin"), os.path.join(str(workdir), "kt_out.bin")
    with open(fin, "wb") as f:
        f.write(payload)
    r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    with open(fout, "rb") as f:
        return f.read()


def run_fmt(exe, workdir, values):
    """-> (lengths (n,) int, -1 outside the domain; records (n,17) uint8)"""
    x = np.ascontiguousarray(values, np.float64)
    out = np.frombuffer(_run(exe, "fmt", workdir, struct.pack("<q", x.size) + x.tobytes()), np.uint8).reshape(-1, 18)
    assert out.shape[0] == x.size
    ln = out[:, 0].astype(np.int64)
    ln[ln == 255] = -1
    return ln, out[:, 1:]


def run_lines(exe, workdir, batch):
    """batch: dict of make_batch -> dict text (B, M*256) u8, text_len, status (B) i32, rows (B,M,13) f64, valid (B,M) u8"""
    boxes, scores = batch["boxes"], batch["scores"]
    B, M = scores.shape
    keep, num = batch.get("keep"), batch.get("num")
    name = batch.get("class_name", "Car").encode()
    payload = struct.pack("<5i", B, M, int(keep is not None), int(num is not None), len(name)) + name.ljust(16, b"\0")
    payload += boxes.astype(F32).tobytes() + scores.astype(F32).tobytes()
    payload += (np.zeros((B, M), np.int32) if keep is None else keep.astype(np.int32)).tobytes()
    payload += (np.zeros((B,), np.int32) if num is None else num.astype(np.int32)).tobytes()
    payload += batch["P2"].astype(np.float64).tobytes() + batch["img_hw"].astype(np.int32).tobytes()
    raw = _run(exe, "lines", workdir, payload)
    o, out = 0, {}
    for key, dt, shape in (("text", np.uint8, (B, M * LINE_MAX)), ("text_len", np.int32, (B,)), ("status", np.int32, (B,)),
                           ("rows", np.float64, (B, M, FIELDS)), ("valid", np.uint8, (B, M))):
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[o:o + n], dt).reshape(shape).copy()
        o += n
    assert o == len(raw)
    return out


def make_batch(seeds, n=40, class_name="Car", keep=None, num=None):
    """one frame per seed from ref_kitti_output.cases; keep (B,M) / num (B) as given"""
    frames = [cases(s, n=n) for s in seeds]
    batch = {"boxes": np.stack([f[0] for f in frames]).astype(F32), "scores": np.stack([f[1] for f in frames]).astype(F32),
             "P2": np.stack([np.asarray(f[2], np.float64).reshape(12) for f in frames]),
             "img_hw": np.array([f[3] for f in frames], np.int32), "class_name": class_name}
    if keep is not None:
        batch["keep"] = np.asarray(keep, np.int32)
    if num is not None:
        batch["num"] = np.asarray(num, np.int32)
    return batch


def numpy_valid(batch, b):
    """the size test of frame b's boxes by kitti_output's numpy functions"""
    from pointrcnn_amd import kitti_output
    H, W = batch["img_hw"][b]
    ib = kitti_output.corners_to_image_boxes(kitti_output.box_corners(batch["boxes"][b]), batch["P2"][b].reshape(3, 4))
    ib[:, 0::2] = np.clip(ib[:, 0::2], 0, W - 1)
    ib[:, 1::2] = np.clip(ib[:, 1::2], 0, H - 1)
    return ((ib[:, 2] - ib[:, 0]) < W * 0.8) & ((ib[:, 3] - ib[:, 1]) < H * 0.8)


def frame_lines(out, b):
    """the text of frame b as a list of lines (without the newline)"""
    blob = out["text"][b, :int(out["text_len"][b])].tobytes().decode("ascii")
    assert blob == "" or blob.endswith("\n")
    return blob.split("\n")[:-1] if blob else []


def python_lines(rows, valid, class_name="Car"):
    """Python's own % on the kept rows"""
    fmt = class_name + " -1 -1" + " %.4f" * FIELDS
    return [fmt % tuple(r) for r, v in zip(rows.tolist(), valid.tolist()) if v]
