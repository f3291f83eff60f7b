"""Tensor-level host layer over the C ABI: argument checking, output allocation, stream plumbing.

PyTorch is used for device memory and streams only; every computation below is one call into
libprcnn_pointops.so on torch's CURRENT stream (so it composes with torch.cuda.graphs and side streams).
Shapes and argument meaning mirror the reference op surface (see each function's citation).
"""
import ctypes
import math
import os
import threading
import weakref

import torch

from . import _cabi

_INT = torch.int32
_F32 = torch.float32
# The spatially pruned FPS kernel (Morton pre-sort + exact bounding-box skip) for 2048 < N <= 16384.  Bit-identical
# results, ~35 % shorter serial chain.  With the neighbour searches on the grid the FPS chain is the longest dependency of
# a batch, so it is the default (+8 % RPN throughput at 3 batches in flight); PRCNN_FPS_PRUNED=0 selects the plain kernel.
FPS_PRUNED = os.environ.get("PRCNN_FPS_PRUNED", "1") == "1"
# A nested FPS level (a cloud that IS the sample set of the previous level, in sample order) is answered from the parent's indices
# by prcnn_fps_nested: positions 0, 1, 2, ... for every frame a device pass accepts, the plain kernels for the rest.  Same bits;
# PRCNN_FPS_NESTED=0 selects plain FPS at every level (A/B).
FPS_NESTED = os.environ.get("PRCNN_FPS_NESTED", "1") == "1"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name, dtype=_F32, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA(HIP) tensor: the HIP kernels are the only implementation" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError("%s must have %d dims, got shape %s" % (name, ndim, tuple(t.shape)))
    return t


def _p(t):
    return None if t is None else t.data_ptr()


def _tensor_key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version)


def _hintable(*tensors):
    """the nested-FPS hint may ride on these tensors: the switch is on and every one of them tracks a version counter.  A tensor made
    under torch.inference_mode() does not (reading _version raises, and an in-place write leaves no trace), so it never carries a hint
    and its FPS levels all take plain prcnn_fps."""
    return FPS_NESTED and not any(t.is_inference() for t in tensors)


# ------------------------------------------------------------------ PointNet++ operators
def furthest_point_sample(xyz, npoint, order="canonical"):
    """xyz (B,N,3) f32 -> idx (B,npoint) i32   [pointnet2_utils.furthest_point_sample]
    order: "canonical" (ties among equal running min-distances -> lowest point index; the tested contract) or "upstream"
    (the order the upstream CUDA kernel's thread layout produces, SURVEY Appendix A.1: argmin (k mod T, k)) -- they differ
    only on clouds with duplicate points / exact lattices; "upstream" is a comparison mode, not a fast path."""
    _chk(xyz, "xyz", ndim=3)
    B, N, _ = xyz.shape
    idx = torch.empty((B, npoint), dtype=_INT, device=xyz.device)
    if order != "canonical":
        if order != "upstream":
            raise ValueError("furthest_point_sample: order must be 'canonical' or 'upstream'")
        tmp = torch.empty((B, N), dtype=_F32, device=xyz.device)
        _cabi.check(_cabi.lib().prcnn_fps_order(_p(xyz), B, N, npoint, 1, _p(tmp), _p(idx), _stream()), "prcnn_fps_order")
        return idx
    # (B,N) 4-byte scratch: Morton-order permutation of the spatially pruned kernel (2048 < N <= 16384), or the
    # HBM-resident min-distance array (N > 16384); the small-N kernels need none
    tmp = torch.empty((B, N), dtype=_F32, device=xyz.device) if (N > 16384 or (N > 2048 and FPS_PRUNED)) else None
    L = _cabi.lib()
    # the modules hand each other tensors only, so the hint rides on them: gather_rows tags the sample set it writes with the
    # indices that made it (see there); any doubt -- another object, a view, a copy, an in-place write since -- means plain FPS
    parent = getattr(xyz, "_prcnn_fps_parent", None) if _hintable(xyz) else None
    if parent is not None:
        prev_idx, prev_version, key = parent
        if not (_hintable(prev_idx) and key == _tensor_key(xyz) and prev_idx._version == prev_version and prev_idx.device == xyz.device
                and tuple(prev_idx.shape) == (B, N) and npoint <= N <= 16384):
            parent = None
    if parent is not None:
        skip = torch.empty((B,), dtype=_INT, device=xyz.device)
        _cabi.check(L.prcnn_fps_nested(_p(xyz), _p(prev_idx), B, N, npoint, _p(tmp), _p(idx), _p(skip), _stream()), "prcnn_fps_nested")
    else:
        _cabi.check(L.prcnn_fps(_p(xyz), B, N, npoint, _p(tmp), _p(idx), _stream()), "prcnn_fps")
    # the identity (not the address: a new tensor can land where a dropped one was) and the state of the tensor these indices sample
    if _hintable(xyz, idx):
        idx._prcnn_fps_src = (weakref.ref(xyz), _tensor_key(xyz), idx._version)
    return idx


_ARITH = {"canonical": 0, "upstream": 1}
_ORDER = {"canonical": 0, "upstream": 1}


def furthest_point_sample_mode(xyz, npoint, order="canonical", arith="canonical"):
    """COMPARISON MODE (prcnn_fps_mode): FPS with a selectable tie order and squared-distance arithmetic -- "upstream" arithmetic is
    fma(dz,dz, fma(dy,dy, dx*dx)), what nvcc makes of the upstream kernel's expression.  Plain kernel, not a fast path."""
    _chk(xyz, "xyz", ndim=3)
    B, N, _ = xyz.shape
    idx = torch.empty((B, npoint), dtype=_INT, device=xyz.device)
    tmp = torch.empty((B, N), dtype=_F32, device=xyz.device)
    _cabi.check(_cabi.lib().prcnn_fps_mode(_p(xyz), B, N, npoint, _ORDER[order], _ARITH[arith], _p(tmp), _p(idx), _stream()), "prcnn_fps_mode")
    return idx


def ball_query_arith(radius, nsample, xyz, new_xyz, arith="upstream"):
    """COMPARISON MODE (prcnn_ball_query_arith): ball_query by a plain scan under the chosen squared-distance arithmetic"""
    _chk(xyz, "xyz", ndim=3); _chk(new_xyz, "new_xyz", ndim=3)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    idx = torch.empty((B, M, nsample), dtype=_INT, device=xyz.device)
    _cabi.check(_cabi.lib().prcnn_ball_query_arith(_p(xyz), _p(new_xyz), B, N, M, float(radius), nsample, _ARITH[arith], _p(idx), _stream()),
                "prcnn_ball_query_arith")
    return idx


def three_nn_arith(unknown, known, arith="upstream"):
    """COMPARISON MODE (prcnn_three_nn_arith): -> dist2 (B,n,3) SQUARED, idx (B,n,3) under the chosen squared-distance arithmetic"""
    _chk(unknown, "unknown", ndim=3); _chk(known, "known", ndim=3)
    B, n, _ = unknown.shape
    m = known.shape[1]
    d2 = torch.empty((B, n, 3), dtype=_F32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=_INT, device=unknown.device)
    _cabi.check(_cabi.lib().prcnn_three_nn_arith(_p(unknown), _p(known), B, n, m, _ARITH[arith], _p(d2), _p(idx), _stream()),
                "prcnn_three_nn_arith")
    return d2, idx


def fps_status():
    """Raise if a multi-workgroup furthest_point_sample launch (N > 16384) timed out waiting for a partner slice since the
    last check (its output then holds -1 indices).  Does not synchronise: call after the stream has (end of a step / test)."""
    _cabi.check(_cabi.lib().prcnn_fps_status(), "prcnn_fps_status")


def gather(features, idx):
    """features (B,C,N), idx (B,M) i32 -> (B,C,M)   [gather_operation]"""
    _chk(features, "features", ndim=3); _chk(idx, "idx", _INT, 2)
    B, C, N = features.shape
    M = idx.shape[1]
    out = torch.empty((B, C, M), dtype=_F32, device=features.device)
    _cabi.check(_cabi.lib().prcnn_gather(_p(features), _p(idx), B, C, N, M, _p(out), _stream()), "prcnn_gather")
    return out


def gather_grad(grad_out, idx, N):
    _chk(grad_out, "grad_out", ndim=3); _chk(idx, "idx", _INT, 2)
    B, C, M = grad_out.shape
    g = torch.zeros((B, C, N), dtype=_F32, device=grad_out.device)
    _cabi.check(_cabi.lib().prcnn_gather_grad(_p(grad_out), _p(idx), B, C, N, M, _p(g), _stream()), "prcnn_gather_grad")
    return g


def gather_rows(in_cl, idx):
    """in_cl (B,N,C) channels-last (row stride may exceed C), idx (B,M) i32 -> (B,M,C)"""
    _chk(idx, "idx", _INT, 2)
    B, N, C = in_cl.shape
    M = idx.shape[1]
    out = torch.empty((B, M, C), dtype=_F32, device=in_cl.device)
    _cabi.check(_cabi.lib().prcnn_gather_rows(_p(in_cl), _row_stride(in_cl), _p(idx), B, N, M, C, _p(out), _stream()),
                "prcnn_gather_rows")
    src = getattr(idx, "_prcnn_fps_src", None) if (C == 3 and _hintable(in_cl, idx, out)) else None
    if src is not None and src[0]() is in_cl and src[1] == _tensor_key(in_cl) and src[2] == idx._version:
        # `out` is the canonical FPS sample set of in_cl in sample order: a later furthest_point_sample(out, m <= M) may answer from idx
        out._prcnn_fps_parent = (idx, idx._version, _tensor_key(out))
    return out


# Frames with at least this many points are searched through a per-frame grid (csrc/grid.hip) instead of a full scan:
# identical results, ~N/30 of the distance evaluations.  PRCNN_GRID_SEARCH=0 forces the scans (A/B, debugging).
GRID_MIN_POINTS = 2048 if os.environ.get("PRCNN_GRID_SEARCH", "1") != "0" else 1 << 62
THREE_NN_GRID_MIN = int(os.environ.get("PRCNN_THREE_NN_GRID_MIN", "1024")) if GRID_MIN_POINTS < (1 << 62) else 1 << 62   # known points
DENSE_SCAN = os.environ.get("PRCNN_DENSE_SCAN", "1") != "0"      # dense frames fall back to the scan (A/B switch, same results)
BQ_GRID_CELLS = int(os.environ.get("PRCNN_BQ_GRID_CELLS", "128"))       # cells per axis of the ball-query grid (64 | 128)


class Grid:
    """points of B frames binned into per-frame 64x64 x-z grids (prcnn_grid_build)"""

    def __init__(self, xyz, min_cell=0.0, cells_per_axis=64):
        _chk(xyz, "xyz", ndim=3)
        self.B, self.N = xyz.shape[0], xyz.shape[1]
        L = _cabi.lib()
        nbytes = L.prcnn_grid_bytes(self.B, self.N)
        self.buf = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=xyz.device)
        _cabi.check(L.prcnn_grid_build(_p(xyz), self.B, self.N, float(min_cell), int(cells_per_axis), _p(self.buf), nbytes, _stream()),
                    "prcnn_grid_build")


def ball_query_grid(grid, new_xyz, radius_a, nsample_a, radius_b=0.0, nsample_b=0, xyz=None):
    """== ball_query / ball_query2 on a Grid of the source points.  xyz: the points the grid was built from -- frames the grid
    build flags as dense are then answered by the index-order scan (same results, see prcnn_ball_query2_grid)"""
    _chk(new_xyz, "new_xyz", ndim=3)
    B, M = new_xyz.shape[0], new_xyz.shape[1]
    if B != grid.B:
        raise ValueError("ball_query_grid: %d frames of centroids vs %d frames in the grid" % (B, grid.B))
    ia = torch.empty((B, M, nsample_a), dtype=_INT, device=new_xyz.device)
    ib = torch.empty((B, M, nsample_b), dtype=_INT, device=new_xyz.device) if nsample_b else None
    _cabi.check(_cabi.lib().prcnn_ball_query2_grid(_p(grid.buf), _p(xyz), _p(new_xyz), B, grid.N, M, float(radius_a), nsample_a, _p(ia),
                                                   float(radius_b), nsample_b, _p(ib), _stream()), "prcnn_ball_query2_grid")
    return (ia, ib) if nsample_b else ia


def ball_query(radius, nsample, xyz, new_xyz):
    """xyz (B,N,3), new_xyz (B,M,3) -> idx (B,M,nsample) i32   [ball_query]"""
    _chk(xyz, "xyz", ndim=3); _chk(new_xyz, "new_xyz", ndim=3)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    if N >= GRID_MIN_POINTS and B > 0 and M > 0:
        return ball_query_grid(Grid(xyz, radius, BQ_GRID_CELLS), new_xyz, radius, nsample, xyz=xyz if DENSE_SCAN else None)
    idx = torch.empty((B, M, nsample), dtype=_INT, device=xyz.device)
    _cabi.check(_cabi.lib().prcnn_ball_query(_p(xyz), _p(new_xyz), B, N, M, float(radius), nsample, _p(idx), _stream()),
                "prcnn_ball_query")
    return idx


def ball_query2(radius_a, nsample_a, radius_b, nsample_b, xyz, new_xyz):
    """two radii in one scan -> (idx_a, idx_b)"""
    _chk(xyz, "xyz", ndim=3); _chk(new_xyz, "new_xyz", ndim=3)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    if N >= GRID_MIN_POINTS and B > 0 and M > 0:
        return ball_query_grid(Grid(xyz, max(radius_a, radius_b), BQ_GRID_CELLS), new_xyz, radius_a, nsample_a, radius_b, nsample_b,
                               xyz=xyz if DENSE_SCAN else None)
    ia = torch.empty((B, M, nsample_a), dtype=_INT, device=xyz.device)
    ib = torch.empty((B, M, nsample_b), dtype=_INT, device=xyz.device)
    _cabi.check(_cabi.lib().prcnn_ball_query2(_p(xyz), _p(new_xyz), B, N, M, float(radius_a), nsample_a, _p(ia),
                                              float(radius_b), nsample_b, _p(ib), _stream()), "prcnn_ball_query2")
    return ia, ib


def group(features, idx):
    """features (B,C,N), idx (B,M,ns) -> (B,C,M,ns)   [grouping_operation]"""
    _chk(features, "features", ndim=3); _chk(idx, "idx", _INT, 3)
    B, C, N = features.shape
    _, M, ns = idx.shape
    out = torch.empty((B, C, M, ns), dtype=_F32, device=features.device)
    _cabi.check(_cabi.lib().prcnn_group(_p(features), _p(idx), B, C, N, M, ns, _p(out), _stream()), "prcnn_group")
    return out


def group_grad(grad_out, idx, N):
    _chk(grad_out, "grad_out", ndim=4); _chk(idx, "idx", _INT, 3)
    B, C, M, ns = grad_out.shape
    g = torch.zeros((B, C, N), dtype=_F32, device=grad_out.device)
    _cabi.check(_cabi.lib().prcnn_group_grad(_p(grad_out), _p(idx), B, C, N, M, ns, _p(g), _stream()), "prcnn_group_grad")
    return g


def three_nn(unknown, known, want_weight=False):
    """unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3), idx (B,n,3) i32 [, weight (B,n,3)]"""
    _chk(unknown, "unknown", ndim=3); _chk(known, "known", ndim=3)
    B, n, _ = unknown.shape
    m = known.shape[1]
    d2 = torch.empty((B, n, 3), dtype=_F32, device=unknown.device)
    idx = torch.empty((B, n, 3), dtype=_INT, device=unknown.device)
    w = torch.empty((B, n, 3), dtype=_F32, device=unknown.device) if want_weight else None
    if m >= THREE_NN_GRID_MIN and B > 0 and n > 0:
        g = Grid(known, 0.0)
        _cabi.check(_cabi.lib().prcnn_three_nn_grid(_p(g.buf), _p(unknown), B, n, m, _p(d2), _p(idx), _p(w), _stream()),
                    "prcnn_three_nn_grid")
        return (d2, idx, w) if want_weight else (d2, idx)
    _cabi.check(_cabi.lib().prcnn_three_nn(_p(unknown), _p(known), B, n, m, _p(d2), _p(idx), _p(w), _stream()),
                "prcnn_three_nn")
    return (d2, idx, w) if want_weight else (d2, idx)


def three_interpolate(features, idx, weight):
    """features (B,C,m), idx (B,n,3), weight (B,n,3) -> (B,C,n)"""
    _chk(features, "features", ndim=3); _chk(idx, "idx", _INT, 3); _chk(weight, "weight", ndim=3)
    B, C, m = features.shape
    n = idx.shape[1]
    out = torch.empty((B, C, n), dtype=_F32, device=features.device)
    _cabi.check(_cabi.lib().prcnn_three_interp(_p(features), _p(idx), _p(weight), B, C, m, n, _p(out), _stream()),
                "prcnn_three_interp")
    return out


def three_interpolate_grad(grad_out, idx, weight, m):
    _chk(grad_out, "grad_out", ndim=3); _chk(idx, "idx", _INT, 3); _chk(weight, "weight", ndim=3)
    B, C, n = grad_out.shape
    g = torch.zeros((B, C, m), dtype=_F32, device=grad_out.device)
    ws = torch.empty((B, m, C), dtype=_F32, device=grad_out.device)        # channels-last accumulator (see the header)
    _cabi.check(_cabi.lib().prcnn_three_interp_grad(_p(grad_out), _p(idx), _p(weight), B, C, n, m, _p(g), _p(ws), _stream()),
                "prcnn_three_interp_grad")
    return g


# ------------------------------------------------------------------ fused per-point MLP layers
class PackedLinear:
    """One 1x1-conv layer with (eval-mode) BatchNorm folded in, packed for the MFMA kernel.

    weight: (Nout, K) f32 device tensor in torch conv layout; bias: (Nout) or None.
    k_rot: leading input channels moved to the end of K (3 for grouped [dxyz, feat] layers).
    """

    def __init__(self, weight, bias=None, relu=True, k_rot=0):
        _chk(weight, "weight", ndim=2)
        self.nout, self.k = weight.shape
        self.relu = bool(relu)
        L = _cabi.lib()
        self.wpack = torch.empty((L.prcnn_wpack_floats(self.nout, self.k),), dtype=_F32, device=weight.device)
        _cabi.check(L.prcnn_pack_weight(_p(weight), self.nout, self.k, k_rot, _p(self.wpack), _stream()),
                    "prcnn_pack_weight")
        self._w = weight if k_rot == 0 else None         # kept for the split-bf16 variant's own weight image (built on first use)
        self._wsplit = None
        # bias is kept zero-padded to a multiple of 32 entries (the chain kernel reads whole 32-channel blocks)
        self.bias = None
        if bias is not None:
            _chk(bias.contiguous(), "bias", ndim=1)
            self.bias = torch.zeros(((self.nout + 31) // 32 * 32,), dtype=_F32, device=weight.device)
            self.bias[: self.nout] = bias


    def wsplit(self, chain=0):
        """the pre-split bf16 weight image of the split-bf16 variant (prcnn_pack_weight_split; chain = 1: the chain kernel's
        image), or None when the layer does not qualify (K a multiple of 32, no rotated input channels)"""
        if self._wsplit is None:
            self._wsplit = {}
        if chain not in self._wsplit and self._w is not None and self.k % 32 == 0:
            L = _cabi.lib()
            img = torch.empty((L.prcnn_wsplit_bytes(self.nout, self.k),), dtype=torch.uint8, device=self._w.device)
            _cabi.check(L.prcnn_pack_weight_split(_p(self._w.contiguous()), self.nout, self.k, int(chain), _p(img), _stream()),
                        "prcnn_pack_weight_split")
            self._wsplit[chain] = img
        return self._wsplit.get(chain)


# Arithmetic of the fused inference MLPs' plain-row layers, heads and hoisted FP0 (everything that reaches prcnn_mlp_rows*,
# the two-layer head chains and the interpolating chain):
#   6 (default) -- split-bf16, six terms: every fp32 operand cut EXACTLY into three bf16 pieces, six bf16 MFMA products per fp32
#                  product, fp32 accumulate; drops partial products below 2^-24 |x||w|: fp32-grade results (measured 2.9e-7 of
#                  sum |x||w| against float64, the fp32-MFMA kernel 3.0e-7), rows with non-finite values recomputed on the fp32
#                  pipe.  Qualified by the whole GPU suite, which runs every test under both arithmetics (tests/conftest.py
#                  `mlp_mode`), and by bench.py's max_diff_vs_f32_mfma on uniform, lidar and saturated clouds (contract 1e-5).
#   0           -- fp32 MFMA (v_mfma_f32_32x32x2_f32) throughout: PRCNN_MLP_SPLIT=0.
#   3           -- three terms (drops below 2^-16 |x||w|): OUTSIDE the 1e-5 contract, dev / trade-off measurements only.
# The choice never depends on row counts (a frame's bits are the same in a batch of 1 and of 32 -- with one exception: FINITE rows that
# share a 64-row block (32 in the chain kernels) with a row holding inf / NaN are recomputed with it on the fp32 pipe and carry the
# fp32-MFMA kernel's bits, within the same 1e-5 contract).  Training kernels are fp32 MFMA.
MLP_SPLIT_TERMS = int(os.environ.get("PRCNN_MLP_SPLIT", "6") or 0)
if MLP_SPLIT_TERMS not in (0, 3, 6):
    raise RuntimeError("PRCNN_MLP_SPLIT=%r: 6 (default) / 3 split-bf16 terms, 0 = fp32 MFMA" % os.environ.get("PRCNN_MLP_SPLIT"))

_MODE_ROWS, _MODE_GROUP, _MODE_INTERP = 0, 1, 2
_chain_ok = {}


def chain_supported(mode, layers, pool_ns=0):
    """True when the register-resident chain kernel has an instance for this stack of PackedLinear layers."""
    key = (mode, tuple(l.nout for l in layers), pool_ns)
    hit = _chain_ok.get(key)
    if hit is None:
        arr = (ctypes.c_int * len(layers))(*[l.nout for l in layers])
        hit = bool(_cabi.lib().prcnn_mlp_chain_supported(mode, len(layers), arr, pool_ns)) if 1 <= len(layers) <= 3 else False
        _chain_ok[key] = hit
    return hit


class _ChainArgs:
    """host arrays (wpack*, bias*, nout, relu) describing a stack of PackedLinear layers.  Holds the layers themselves:
    the raw pointers below stay valid and the id()s of the cache key cannot be recycled while this object lives."""

    def __init__(self, layers):
        n = len(layers)
        self.n = n
        self.layers = tuple(layers)
        self.wpack = (ctypes.c_void_p * n)(*[l.wpack.data_ptr() for l in layers])
        self.bias = (ctypes.c_void_p * n)(*[(l.bias.data_ptr() if l.bias is not None else None) for l in layers])
        self.nout = (ctypes.c_int * n)(*[l.nout for l in layers])
        self.relu = (ctypes.c_int * n)(*[int(l.relu) for l in layers])


def _chain_args(layers):
    key = tuple(id(l) for l in layers)
    hit = getattr(layers[0], "_chain_cache", None)
    if hit is None or hit[0] != key:
        hit = (key, _ChainArgs(layers))
        layers[0]._chain_cache = hit
    return hit[1]


def _row_stride(x):
    """row stride (in elements) of a channels-last rows view (..., K): the stride of the innermost leading dim of
    size > 1 (size-1 dims carry arbitrary strides); the caller guarantees uniform striding (pt_utils._rows_view)."""
    for size, stride in zip(reversed(x.shape[:-1]), reversed(x.stride()[:-1])):
        if size != 1:
            return stride
    return x.shape[-1]


def _out_buf(out, rows, nout, device):
    """-> buffer, ld_out, col_off: a fresh (rows, nout) buffer, or out = (buffer, col_off) of a wider channels-last one"""
    if out is None:
        return torch.empty((rows, nout), dtype=_F32, device=device), nout, 0
    buf, col_off = out
    return buf, _row_stride(buf), col_off


# what a layer wrapper and its chain twin share: shapes read off the operands, the output buffer (last: the layer that writes it)
def _rows_prelude(name, x, last, out, pool_ns):
    if x.stride(-1) != 1:
        raise RuntimeError("%s: last dim must be contiguous" % name)
    K = x.shape[-1]
    rows = x.numel() // K
    return (K, rows, _row_stride(x)) + _out_buf(out, rows // pool_ns if pool_ns else rows, last.nout, x.device)


def _group_prelude(xyz, idx, feat_cl, last, out, pool_ns, act):
    B, N, _ = xyz.shape
    _, M, ns = idx.shape
    C = 0 if feat_cl is None else feat_cl.shape[-1]
    ld_feat = 0 if feat_cl is None else _row_stride(feat_cl)
    rows = B * M * ns
    return (B, N, M, ns, C, ld_feat) + ((None, None) if act is None else tuple(act)) + _out_buf(out, rows // pool_ns if pool_ns else rows, last.nout, xyz.device)


def _interp_prelude(known_cl, idx3, skip_cl, last, out):
    B, m, C2 = known_cl.shape
    n = idx3.shape[1]
    C1 = 0 if skip_cl is None else skip_cl.shape[-1]
    ld_skip = 0 if skip_cl is None else _row_stride(skip_cl)
    return (B, n, m, C2, C1, ld_skip) + _out_buf(out, B * n, last.nout, known_cl.device)


def mlp_chain_rows(x, layers, out=None, pool_ns=0, seg=None):
    """whole stack on channels-last rows in one kernel (see mlp_rows for the layout contract; seg as there)"""
    K, rows, ld_in, buf, ld_out, col_off = _rows_prelude("mlp_chain_rows", x, layers[-1], out, pool_ns)
    a = _chain_args(layers)
    seg_cnt, seg_rows = (None, 0) if seg is None else (seg[0], int(seg[1]))
    if (MLP_SPLIT_TERMS and not pool_ns and seg is None and a.n == 2 and K == 128 and layers[0].nout == 128
            and (layers[1].nout == 1 or 64 < layers[1].nout <= 128) and layers[0].wsplit(1) is not None and layers[1].wsplit(1) is not None):
        if getattr(a, "wchain", None) is None:                 # (host array of the two chain images, kept with the cached args)
            a.wchain = (ctypes.c_void_p * 2)(layers[0].wsplit(1).data_ptr(), layers[1].wsplit(1).data_ptr())
        rc = _cabi.lib().prcnn_mlp_chain_rows_split(_p(x), ld_in, rows, K, a.wchain, a.wpack, a.bias, a.nout, a.relu,
                                                    MLP_SPLIT_TERMS, _p(buf), ld_out, col_off, _stream())
        if rc != _cabi.EUNSUPPORTED:
            _cabi.check(rc, "prcnn_mlp_chain_rows_split")
            return buf
    _cabi.check(_cabi.lib().prcnn_mlp_chain_rows(_p(x), ld_in, rows, K, a.n, a.wpack, a.bias, a.nout, a.relu, _p(buf),
                                                 ld_out, col_off, pool_ns, _p(seg_cnt), seg_rows, _stream()), "prcnn_mlp_chain_rows")
    return buf


def mlp_chain_group(xyz, new_xyz, idx, feat_cl, layers, out=None, pool_ns=0, act=None, groups_dev=None):
    B, N, M, ns, C, ld_feat, awx, ab, buf, ld_out, col_off = _group_prelude(xyz, idx, feat_cl, layers[-1], out, pool_ns, act)
    a = _chain_args(layers)
    _cabi.check(_cabi.lib().prcnn_mlp_chain_group(_p(xyz), _p(new_xyz), _p(idx), _p(feat_cl), ld_feat, B, N, M, ns, C, _p(awx), _p(ab), a.n,
                                                  a.wpack, a.bias, a.nout, a.relu, _p(buf), ld_out, col_off, pool_ns,
                                                  _p(groups_dev), _stream()), "prcnn_mlp_chain_group")
    return buf


def mlp_chain_group_multi(problems):
    """Up to four mlp_chain_group problems -- dicts of its arguments (xyz, new_xyz, idx, feat_cl, layers, out, pool_ns, act,
    groups_dev; out is required) -- in ONE launch, heaviest first.  False, with nothing launched, when the library has no kernel
    for the combination (PRCNN_EUNSUPPORTED): the caller issues them one by one.
    A problem that also has the key dst = (int32 device list, out2, col_off2) stores by destination (prcnn_mlp_chain_group_multi_dst;
    out2, the level's output rows, is one tensor for all of them): an un-pooled problem row r to row list[r] of out2 where
    list[r] >= 0 and to its own out otherwise, a pooled one group g to row list[g]."""
    by_dst = [pr["dst"] for pr in problems if pr.get("dst") is not None]
    out2 = by_dst[0][1] if by_dst else None
    if any(d[1] is not out2 for d in by_dst):
        raise RuntimeError("mlp_chain_group_multi: the problems that store by destination must share one output")
    arr = (_cabi.ChainGroupProblem * len(problems))()
    for q, pr in zip(arr, problems):
        layers = pr["layers"]
        B, N, M, ns, C, ld_feat, awx, ab, buf, ld_out, col_off = _group_prelude(pr["xyz"], pr["idx"], pr.get("feat_cl"), layers[-1], pr["out"],
                                                                                pr.get("pool_ns", 0), pr.get("act"))
        a = _chain_args(layers)
        q.xyz, q.new_xyz, q.idx, q.feat_cl, q.act_wx, q.act_bias = (_p(pr["xyz"]), _p(pr.get("new_xyz")), _p(pr["idx"]), _p(pr.get("feat_cl")),
                                                                    _p(awx), _p(ab))
        q.wpack, q.bias = ctypes.cast(a.wpack, ctypes.c_void_p), ctypes.cast(a.bias, ctypes.c_void_p)
        q.nout, q.relu = ctypes.cast(a.nout, ctypes.c_void_p), ctypes.cast(a.relu, ctypes.c_void_p)
        q.out, q.groups_dev = _p(buf), _p(pr.get("groups_dev"))
        q.ld_feat, q.B, q.N, q.M, q.nsample, q.C, q.nlayers = ld_feat, B, N, M, ns, C, a.n
        q.ld_out, q.col_off, q.pool_ns = ld_out, col_off, pr.get("pool_ns", 0)
    if out2 is None:
        rc = _cabi.lib().prcnn_mlp_chain_group_multi(len(problems), arr, _stream())
    else:
        dst = (ctypes.c_void_p * len(problems))(*[_p(pr["dst"][0]) if pr.get("dst") is not None else None for pr in problems])
        col2 = (ctypes.c_int * len(problems))(*[int(pr["dst"][2]) if pr.get("dst") is not None else 0 for pr in problems])
        rc = _cabi.lib().prcnn_mlp_chain_group_multi_dst(len(problems), arr, dst, _p(out2), _row_stride(out2), col2, _stream())
    if rc == _cabi.EUNSUPPORTED:
        return False
    _cabi.check(rc, "prcnn_mlp_chain_group_multi_dst" if out2 is not None else "prcnn_mlp_chain_group_multi")
    return True


def mlp_chain_interp(known_cl, idx3, w3, skip_cl, layers, out=None, act_bias=None):
    B, n, m, C2, C1, ld_skip, buf, ld_out, col_off = _interp_prelude(known_cl, idx3, skip_cl, layers[-1], out)
    a = _chain_args(layers)
    if (MLP_SPLIT_TERMS and skip_cl is None and act_bias is not None and a.n == 1 and C2 == 128 and layers[0].nout == 128
            and layers[0].wsplit(1) is not None):
        l0 = layers[0]
        rc = _cabi.lib().prcnn_mlp_chain_interp_split(_p(known_cl), _row_stride(known_cl), _p(idx3), _p(w3), B, n, m, C2, _p(act_bias),
                                                      _p(l0.wsplit(1)), _p(l0.wpack), _p(l0.bias), l0.nout, int(l0.relu), MLP_SPLIT_TERMS, _p(buf),
                                                      ld_out, col_off, _stream())
        if rc != _cabi.EUNSUPPORTED:
            _cabi.check(rc, "prcnn_mlp_chain_interp_split")
            return buf
    _cabi.check(_cabi.lib().prcnn_mlp_chain_interp(_p(known_cl), _row_stride(known_cl), _p(idx3), _p(w3), _p(skip_cl), ld_skip,
                                                   B, n, m, C2, C1, _p(act_bias), a.n, a.wpack, a.bias, a.nout, a.relu, _p(buf),
                                                   ld_out, col_off, _stream()), "prcnn_mlp_chain_interp")
    return buf


def mlp_rows(x, lin, out=None, pool_ns=0, rows_dev=None, rows_unit=1, seg=None):
    """x (..., K) channels-last rows (last dim contiguous, uniform row stride) -> (rows[/pool_ns], Nout).
    out = (buffer, col_off) writes into a wider channels-last buffer instead of allocating.
    rows_dev (1,) int32 device tensor: only the first rows_dev * rows_unit rows are processed (device-side count).
    seg = (seg_cnt (nseg,) int32 device tensor, seg_rows): segment-prefix live rows -- of every run of seg_rows rows only the
    first seg_cnt[s] are live (roipool3d wrap-copies); tiles in a segment's dead tail are skipped, their outputs unwritten."""
    K, rows, ld_in, buf, ld_out, col_off = _rows_prelude("mlp_rows", x, lin, out, pool_ns)
    if MLP_SPLIT_TERMS and ld_in % 4 == 0 and (seg is None or (rows_dev is None and not pool_ns)) and lin.wsplit() is not None:
        _cabi.check(_cabi.lib().prcnn_mlp_rows_split(_p(x), ld_in, rows, K, _p(lin.wpack), _p(lin.wsplit()), MLP_SPLIT_TERMS,
                                                     _p(lin.bias), lin.nout, int(lin.relu), _p(buf), ld_out, col_off, int(pool_ns), _p(rows_dev),
                                                     int(rows_unit), _p(None if seg is None else seg[0]), 0 if seg is None else int(seg[1]),
                                                     _stream()), "prcnn_mlp_rows_split")
        return buf
    _cabi.check(_cabi.lib().prcnn_mlp_rows(_p(x), ld_in, rows, K, _p(lin.wpack), _p(lin.bias), lin.nout, int(lin.relu),
                                           _p(buf), ld_out, col_off, pool_ns, _p(rows_dev), int(rows_unit),
                                           _p(None if seg is None else seg[0]), 0 if seg is None else int(seg[1]), _stream()), "prcnn_mlp_rows")
    return buf


def mlp_group(xyz, new_xyz, idx, feat_cl, lin, out=None, pool_ns=0, act=None, groups_dev=None):
    """First SA layer fused with ball-query grouping.  xyz (B,N,3), new_xyz (B,M,3) or None (GroupAll),
    idx (B,M,ns) i32, feat_cl (B,N,C) channels-last or None -> (B*M*ns[/pool_ns], Nout).
    act = (act_wx (C,3), act_bias (C)) selects the HOISTED form: feat_cl is Z = W_f.feat per source point and `lin` is
    the SECOND layer (see include/prcnn_pointops.h)."""
    B, N, M, ns, C, ld_feat, awx, ab, buf, ld_out, col_off = _group_prelude(xyz, idx, feat_cl, lin, out, pool_ns, act)
    if MLP_SPLIT_TERMS and act is not None and C % 32 == 0 and ld_feat % 4 == 0 and lin.wsplit() is not None:
        # the hoisted grouped layer on the split-bf16 kernel (round 5; PRCNN_GROUP_SPLIT=0 inside the library is the A/B switch)
        _cabi.check(_cabi.lib().prcnn_mlp_group_split(_p(xyz), _p(new_xyz), _p(idx), _p(feat_cl), ld_feat, B, N, M, ns, C, _p(awx), _p(ab),
                                                      _p(lin.wpack), _p(lin.wsplit()), MLP_SPLIT_TERMS, _p(lin.bias), lin.nout, int(lin.relu),
                                                      _p(buf), ld_out, col_off, pool_ns, _p(groups_dev), _stream()), "prcnn_mlp_group_split")
        return buf
    _cabi.check(_cabi.lib().prcnn_mlp_group(_p(xyz), _p(new_xyz), _p(idx), _p(feat_cl), ld_feat, B, N, M, ns, C, _p(awx), _p(ab),
                                            _p(lin.wpack), _p(lin.bias), lin.nout, int(lin.relu), _p(buf), ld_out,
                                            col_off, pool_ns, _p(groups_dev), _stream()), "prcnn_mlp_group")
    return buf


def mlp_interp(known_cl, idx3, w3, skip_cl, lin, out=None, act_bias=None):
    """First FP layer fused with three_interpolate + skip concat.  known_cl (B,m,C2), idx3/w3 (B,n,3),
    skip_cl (B,n,C1) or None -> (B*n, Nout).  act_bias (C2) selects the HOISTED form (skip_cl must be None): known_cl
    is Y = W.known per known point, the row is relu(interp(Y) + act_bias) and `lin` is the second layer."""
    B, n, m, C2, C1, ld_skip, buf, ld_out, col_off = _interp_prelude(known_cl, idx3, skip_cl, lin, out)
    _cabi.check(_cabi.lib().prcnn_mlp_interp(_p(known_cl), _row_stride(known_cl), _p(idx3), _p(w3), _p(skip_cl), ld_skip,
                                             B, n, m, C2, C1, _p(act_bias), _p(lin.wpack), _p(lin.bias), lin.nout,
                                             int(lin.relu), _p(buf), ld_out, col_off, _stream()), "prcnn_mlp_interp")
    return buf


def mlp_rows_addinterp(skip_cl, lin_b, y_cl, idx3, w3, out=None):
    """Hoisted FP first layer with skip features: act(skip . W_b^T + bias + interp(y_cl)); skip_cl (B,n,C1),
    y_cl (B,m,Nout) = W_a.known, idx3/w3 (B,n,3) -> (B*n, Nout)."""
    B, n, C1 = skip_cl.shape
    m = y_cl.shape[1]
    buf, ld_out, col_off = _out_buf(out, B * n, lin_b.nout, skip_cl.device)
    if MLP_SPLIT_TERMS and _row_stride(skip_cl) % 4 == 0 and lin_b.wsplit() is not None:
        _cabi.check(_cabi.lib().prcnn_mlp_rows_addinterp_split(_p(skip_cl), _row_stride(skip_cl), C1, _p(lin_b.wpack), _p(lin_b.wsplit()),
                                                               MLP_SPLIT_TERMS, _p(lin_b.bias), lin_b.nout, int(lin_b.relu), _p(y_cl),
                                                               _row_stride(y_cl), _p(idx3), _p(w3), B, n, m, _p(buf), ld_out, col_off,
                                                               _stream()), "prcnn_mlp_rows_addinterp_split")
        return buf
    _cabi.check(_cabi.lib().prcnn_mlp_rows_addinterp(_p(skip_cl), _row_stride(skip_cl), C1, _p(lin_b.wpack), _p(lin_b.bias),
                                                     lin_b.nout, int(lin_b.relu), _p(y_cl), _row_stride(y_cl), _p(idx3),
                                                     _p(w3), B, n, m, _p(buf), ld_out, col_off, _stream()),
                "prcnn_mlp_rows_addinterp")
    return buf


def maxpool_rows(x, ns, out=None):
    """x (rows, C) -> (rows/ns, C): max over every ns consecutive rows (generic nsample fallback)."""
    rows, C = x.shape
    rows_out = rows // ns
    buf, ld_out, col_off = _out_buf(out, rows_out, C, x.device)
    _cabi.check(_cabi.lib().prcnn_maxpool_rows(_p(x), x.stride(0), rows_out, ns, C, _p(buf), ld_out, col_off, _stream()),
                "prcnn_maxpool_rows")
    return buf


# ------------------------------------------------------------------ roipool3d
ROIPOOL_BINS = os.environ.get("PRCNN_ROIPOOL_BINS", "1") != "0"        # binned point selection (A/B switch; same results)
ROIPOOL_BINS_MIN_BOXES = 8


def _roipool_work(B, N, M, dev):
    """scratch for the binned point selection of roipool3d (None: linear scan -- few RoIs, or N beyond the LDS bitmap)"""
    if not ROIPOOL_BINS or M < ROIPOOL_BINS_MIN_BOXES:
        return None, 0
    nbytes = _cabi.lib().prcnn_roipool3d_work_bytes(B, N)
    if nbytes == 0:
        return None, 0
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def roipool3d(xyz, boxes3d_enlarged, pts_feature, sampled_pt_num, want_index=False):
    """xyz (B,N,3), boxes (B,M,7) already enlarged, pts_feature (B,N,C) -> pooled (B,M,S,3+C), empty (B,M) i32
    [roipool3d_cuda.forward, lib/utils/roipool3d/src/roipool3d.cpp:48-79]
    want_index: also -> idx (B,M,S) i32, the frame-local source point of every pooled row (-1 in the rows of an empty RoI), and
    distinct (B,M) i32 = min(points in the box, S) (prcnn_roipool3d_index; pooled and empty are the same bytes)"""
    _chk(xyz, "xyz", ndim=3); _chk(boxes3d_enlarged, "boxes3d", ndim=3); _chk(pts_feature, "pts_feature", ndim=3)
    B, N, _ = xyz.shape
    M, C = boxes3d_enlarged.shape[1], pts_feature.shape[2]
    pooled = torch.empty((B, M, sampled_pt_num, 3 + C), dtype=_F32, device=xyz.device)
    empty = torch.empty((B, M), dtype=_INT, device=xyz.device)
    work, nbytes = _roipool_work(B, N, M, xyz.device)
    if want_index:
        idx = torch.empty((B, M, sampled_pt_num), dtype=_INT, device=xyz.device)
        distinct = torch.empty((B, M), dtype=_INT, device=xyz.device)
        _cabi.check(_cabi.lib().prcnn_roipool3d_index_ws(_p(xyz), _p(boxes3d_enlarged), _p(pts_feature), B, N, M, C, sampled_pt_num,
                                                         _p(pooled), _p(empty), _p(idx), _p(distinct), _p(work), nbytes, _stream()),
                    "prcnn_roipool3d_index")
        return pooled, empty, idx, distinct
    _cabi.check(_cabi.lib().prcnn_roipool3d_ws(_p(xyz), _p(boxes3d_enlarged), _p(pts_feature), B, N, M, C, sampled_pt_num,
                                               _p(pooled), _p(empty), _p(work), nbytes, _stream()), "prcnn_roipool3d")
    return pooled, empty


def roipool3d_grad(gpooled, idx, distinct, N, C=None, col0=0, out=None):
    """The pooling's gradient with respect to the per-point features (prcnn_roipool3d_grad; the reference has none):
    gfeat[b, p, c] = sum over (m, s) with idx[b, m, s] == p of gpooled[b, m, s, col0 + c], float32, ascending (m, s), no atomics.
    gpooled: (B, M, S, W) or (B * M, S, W) fp32 rows of unit last stride and one row stride (a column slice of a wider tensor is
    taken as it is); idx (B,M,S) / distinct (B,M) i32 from roipool3d(..., want_index=True); C: columns summed (default W - col0).
    out: (B, N, >= C) rows to write the C columns into (default: a fresh (B, N, C) tensor) -> gfeat"""
    _chk(idx, "idx", _INT, 3); _chk(distinct, "distinct", _INT, 2)
    B, M, S = idx.shape
    if tuple(distinct.shape) != (B, M):
        raise ValueError("roipool3d_grad: distinct must be (B, M) = %s, got %s" % ((B, M), tuple(distinct.shape)))
    if not (isinstance(gpooled, torch.Tensor) and gpooled.is_cuda and gpooled.dtype == _F32):
        raise RuntimeError("roipool3d_grad: gpooled must be a fp32 device tensor")
    g = gpooled.view(B, M, S, gpooled.shape[-1]) if gpooled.dim() == 3 and gpooled.shape[0] == B * M and gpooled.shape[1] == S else gpooled
    if g.dim() != 4 or tuple(g.shape[:3]) != (B, M, S):
        raise ValueError("roipool3d_grad: gpooled must be (B, M, S, W) or (B * M, S, W) with idx (B, M, S) = %s, got %s"
                         % ((B, M, S), tuple(gpooled.shape)))
    W = g.shape[3]
    C = W - col0 if C is None else int(C)
    ld_g = g.stride(2) if S > 1 else (g.stride(1) if M > 1 else max(g.stride(0), W))
    if B * M * S > 0 and (g.stride(3) != 1 or (M > 1 and g.stride(1) != S * ld_g) or (B > 1 and g.stride(0) != M * S * ld_g)):
        raise RuntimeError("roipool3d_grad: gpooled rows must have unit last stride and one row stride")
    if col0 < 0 or C < 1 or col0 + C > W:
        raise ValueError("roipool3d_grad: columns [%d, %d) outside the %d of gpooled" % (col0, col0 + C, W))
    dev = idx.device
    if out is None:
        out = torch.empty((B, N, C), dtype=_F32, device=dev)
    elif not (out.is_cuda and out.dtype == _F32 and out.dim() == 3 and out.shape[0] == B and out.shape[1] == N and out.shape[2] >= C
              and out.is_contiguous()):
        raise ValueError("roipool3d_grad: out must be a contiguous (B, N, >= C) fp32 device tensor")
    L = _cabi.lib()
    nbytes = L.prcnn_roipool3d_grad_work_bytes(B, N, M, S)
    work = torch.empty((max(nbytes, 4),), dtype=torch.uint8, device=dev)
    _cabi.check(L.prcnn_roipool3d_grad(_p(g), ld_g, col0, _p(idx), _p(distinct), B, N, M, S, C, _p(out), out.shape[2], _p(work), nbytes,
                                       _stream()), "prcnn_roipool3d_grad")
    return out


def roipool3d_canonical(xyz, pool_boxes3d, rois, extras, feat_cl, sampled_pt_num, out_feat=None, want_distinct=False):
    """Fused lib/net/rcnn_net.py:127-154: pool [extras..., feat] per RoI and move the pooled xyz into the RoI's
    canonical frame, writing each consumer's operand directly.
    xyz (B,N,3); pool_boxes3d (B,M,7) enlarged; rois (B,M,7) or None; extras: list of <= 2 (B,N) tensors;
    feat_cl (B,N,C) channels-last rows (unit last stride).  out_feat = (buffer (B*M*S, W), col): write the C pooled
    features at that column of a wider rows buffer (default: a fresh (B*M*S, C) tensor).
    want_distinct: also return distinct (B,M) i32 = number of distinct rows per RoI (the rest are wrap-copies); the feature
    rows of the copies are then NOT written (see prcnn_roipool3d_canonical).
    -> pts (B*M, S, 3+len(extras)), feat buffer, empty (B,M) i32 [, distinct]"""
    _chk(xyz, "xyz", ndim=3); _chk(pool_boxes3d, "pool_boxes3d", ndim=3)
    B, N, _ = xyz.shape
    if not (isinstance(feat_cl, torch.Tensor) and feat_cl.is_cuda and feat_cl.dtype == _F32 and feat_cl.dim() == 3
            and feat_cl.stride(-1) == 1 and feat_cl.stride(0) == N * feat_cl.stride(1)):
        raise RuntimeError("roipool3d_canonical: feat must be a (B,N,C) fp32 device tensor of uniformly strided rows")
    M, C, S = pool_boxes3d.shape[1], feat_cl.shape[2], int(sampled_pt_num)
    ex = [e.contiguous() for e in extras]
    if len(ex) > 2:
        raise ValueError("roipool3d_canonical: at most 2 scalar channels")
    for e in ex:
        _chk(e, "extra", ndim=2)
    P = 3 + len(ex)
    dev = xyz.device
    pts = torch.empty((B * M, S, P), dtype=_F32, device=dev)
    if out_feat is None:
        fbuf, col = torch.empty((B * M * S, C), dtype=_F32, device=dev), 0
    else:
        fbuf, col = out_feat
        if fbuf.dim() != 2 or fbuf.shape[0] != B * M * S or fbuf.stride(1) != 1 or col + C > fbuf.shape[1]:
            raise ValueError("roipool3d_canonical: out_feat buffer must be (B*M*S, >= col + C) rows")
    empty = torch.empty((B, M), dtype=_INT, device=dev)
    distinct = torch.empty((B, M), dtype=_INT, device=dev) if want_distinct else None
    if rois is not None:
        _chk(rois, "rois", ndim=3)
    work, nbytes = _roipool_work(B, N, M, dev)
    _cabi.check(_cabi.lib().prcnn_roipool3d_canonical_ws(
        _p(xyz), _p(pool_boxes3d), _p(rois), _p(ex[0]) if ex else None, _p(ex[1]) if len(ex) > 1 else None, _p(feat_cl),
        _row_stride(feat_cl), B, N, M, C, S, _p(pts), P, fbuf.data_ptr() + 4 * col, fbuf.stride(0), _p(empty), _p(distinct),
        _p(work), nbytes, _stream()), "prcnn_roipool3d_canonical")
    return (pts, fbuf, empty, distinct) if want_distinct else (pts, fbuf, empty)


def rpn_labels(pts, gt_boxes3d, num_gt=None, extra_width=0.2):
    """KittiRCNNDataset.generate_rpn_training_labels (kitti_rcnn_dataset.py:365-394) for a whole batch on the device.
    pts (B,N,3), gt_boxes3d (B,G,7), num_gt (B) i32 or None -> cls_label (B,N) i32 {-1,0,1}, reg_label (B,N,7)"""
    _chk(pts, "pts", ndim=3); _chk(gt_boxes3d, "gt_boxes3d", ndim=3)
    B, N, _ = pts.shape
    G = gt_boxes3d.shape[1]
    if gt_boxes3d.shape[0] != B or gt_boxes3d.shape[2] != 7:
        raise ValueError("rpn_labels: gt_boxes3d must be (%d, G, 7)" % B)
    if num_gt is not None:
        _chk(num_gt, "num_gt", _INT, 1)
    cls = torch.empty((B, N), dtype=_INT, device=pts.device)
    reg = torch.empty((B, N, 7), dtype=_F32, device=pts.device)
    _cabi.check(_cabi.lib().prcnn_rpn_labels(_p(pts), _p(gt_boxes3d), _p(num_gt), B, N, G, float(extra_width), _p(cls), _p(reg),
                                             _stream()), "prcnn_rpn_labels")
    return cls, reg


# what csrc/rpn_loss.hip holds per row: RL_MAX_BINS (csrc/rpn_loss_math.h) bins per head and RL_MAX_C (csrc/rpn_loss.hip) channels, a
# multiple of 4.  train_functions routes a configuration beyond them to the composed loss; the exports answer PRCNN_EUNSUPPORTED.
RPN_LOSS_MAX_BINS = 16
RPN_LOSS_MAX_C = 96


def rpn_loss_cfg(cfg):
    """an RPNLossConfig-like object -> prcnn_rpn_loss_cfg_t (what csrc/rpn_loss.hip accepts of it is decided there)"""
    kinds = {"SigmoidFocalLoss": 0, "DiceLoss": 1, "BinaryCrossEntropy": 2}
    alpha = cfg.FOCAL_ALPHA[0]
    return _cabi.RpnLossCfg(loc_scope=float(cfg.LOC_SCOPE), loc_bin_size=float(cfg.LOC_BIN_SIZE),
                            mean_size=(ctypes.c_double * 3)(*[float(v) for v in cfg.MEAN_SIZE]), gamma=float(cfg.FOCAL_GAMMA),
                            alpha=0.0 if alpha is None else float(alpha),
                            loss_weight=(ctypes.c_double * 2)(float(cfg.LOSS_WEIGHT[0]), float(cfg.LOSS_WEIGHT[1])),
                            num_head_bin=int(cfg.NUM_HEAD_BIN), xz_fine=int(bool(cfg.LOC_XZ_FINE)), y_by_bin=0, ry_fine=0,
                            loss_cls=kinds.get(cfg.LOSS_CLS, -1), has_alpha=int(alpha is not None))


def rpn_loss_channels(cfg):
    """channels of an rpn_reg row under cfg: (4 or 2) * nb + 1 + 2 * NUM_HEAD_BIN + 3"""
    nb = int(cfg.LOC_SCOPE / cfg.LOC_BIN_SIZE) * 2
    return (4 if cfg.LOC_XZ_FINE else 2) * nb + 1 + 2 * int(cfg.NUM_HEAD_BIN) + 3


def _uniform_rows(x):
    """x (..., K) -> (x or a contiguous copy, row stride): the rows of x in flat order sit at one stride (what the heads hand over:
    contiguous, or a channels-last view of a wider buffer); any other layout is copied"""
    K = x.shape[-1]
    if K == 1 or x.stride(-1) == 1:
        ld, expect, ok = _row_stride(x), None, True
        for size, stride in zip(reversed(x.shape[:-1]), reversed(x.stride()[:-1])):
            if size != 1:
                expect = stride if expect is None else expect
                ok = ok and stride == expect
                expect = expect * size
        if ok and ld >= K:
            return x, ld
    x = x.contiguous()
    return x, K


def _rpn_loss_work(npts, device):
    return torch.empty((_cabi.lib().prcnn_rpn_loss_workspace_bytes(npts) + 7) // 8, dtype=torch.int64, device=device)


def _rpn_loss_label(cls_label):
    if cls_label.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("rpn_loss: rpn_cls_label must be int32 or int64, got %s" % cls_label.dtype)
    if not cls_label.is_cuda:
        raise RuntimeError("rpn_loss: rpn_cls_label must be a CUDA(HIP) tensor")
    return cls_label.contiguous(), int(cls_label.dtype == torch.int64)


def rpn_loss_counts(cls_label):
    """cls_label (...) i32 / i64 -> counts (4) i32 = this process's {#(label > 0), #(label >= 0), #foreground, 0} and
    norm (2) f32 = {1 / max(pos, 1), 1}, the single-process normalisers (a data-parallel caller overwrites them, see
    train_functions.get_rpn_loss).  Nothing is read back."""
    label, is64 = _rpn_loss_label(cls_label)
    npts = label.numel()
    counts = torch.empty((4,), dtype=_INT, device=label.device)
    norm = torch.empty((2,), dtype=_F32, device=label.device)
    work = _rpn_loss_work(npts, label.device)
    _cabi.check(_cabi.lib().prcnn_rpn_loss_counts(_p(label), is64, npts, _p(counts), _p(norm), _p(work), work.numel() * 8, _stream()),
                "prcnn_rpn_loss_counts")
    return counts, norm


def _rpn_loss_prelude(rpn_cls, rpn_reg, cls_label, reg_label, counts, norm):
    for name, t in (("rpn_cls", rpn_cls), ("rpn_reg", rpn_reg)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == _F32):
            raise RuntimeError("rpn_loss: %s must be a float32 CUDA(HIP) tensor" % name)
    C = rpn_reg.shape[-1]
    npts = rpn_reg.numel() // C
    if rpn_cls.numel() != npts or cls_label.numel() != npts:
        raise ValueError("rpn_loss: rpn_cls / rpn_cls_label must have %d rows" % npts)
    _chk(reg_label, "rpn_reg_label")
    if reg_label.numel() != npts * 7 or reg_label.shape[-1] != 7:
        raise ValueError("rpn_loss: rpn_reg_label must be (..., 7) with %d rows" % npts)
    _chk(counts, "counts", _INT, 1)
    if norm is not None:                               # None: the *_kind exports' single-process normalisers, read from counts
        _chk(norm, "norm", _F32, 1)
    label, is64 = _rpn_loss_label(cls_label)
    cls_rows, ld_cls = _uniform_rows(rpn_cls.reshape(rpn_cls.shape + (1,)) if rpn_cls.dim() == 1 else rpn_cls)
    reg_rows, ld_reg = _uniform_rows(rpn_reg)
    return (_p(cls_rows), ld_cls, _p(reg_rows), ld_reg, _p(label), is64, _p(reg_label), npts, C), (cls_rows, reg_rows, label)


def rpn_loss_forward(rpn_cls, rpn_reg, cls_label, reg_label, cfg, counts, norm):
    """rpn_cls (B,N,1), rpn_reg (B,N,C) f32 (views whose rows sit at ONE stride -- contiguous, or channels-last columns of a wider
    buffer, what the heads hand over -- are read in place; any other layout costs a contiguous copy, a second pass over the
    tensor, see _uniform_rows), cls_label (B,N) i32 / i64, reg_label (B,N,7),
    cfg (rpn_loss_cfg), counts / norm (rpn_loss_counts) -> terms (9) f32: loss, loss_cls, loss_reg, loss_loc, loss_angle,
    loss_size, cls_pos, cls_neg, fg_sum.  Two launches, nothing read back."""
    args, keep = _rpn_loss_prelude(rpn_cls, rpn_reg, cls_label, reg_label, counts, norm)
    terms = torch.empty((9,), dtype=_F32, device=rpn_reg.device)
    work = _rpn_loss_work(args[7], rpn_reg.device)
    _cabi.check(_cabi.lib().prcnn_rpn_loss_forward(*args, ctypes.byref(cfg), _p(counts), _p(norm), _p(terms), _p(work), work.numel() * 8,
                                                   _stream()), "prcnn_rpn_loss_forward")
    return terms


def rpn_loss_backward(rpn_cls, rpn_reg, cls_label, reg_label, cfg, counts, norm, grad_out):
    """the inputs of rpn_loss_forward + grad_out (a float32 device scalar) -> grad_out * d loss / d rpn_cls, d loss / d rpn_reg,
    contiguous, in the inputs' shapes; one launch that writes every entry once"""
    args, keep = _rpn_loss_prelude(rpn_cls, rpn_reg, cls_label, reg_label, counts, norm)
    _chk(grad_out, "grad_out")
    if grad_out.numel() != 1:
        raise ValueError("rpn_loss_backward: grad_out must be a scalar")
    dcls = torch.empty(rpn_cls.shape, dtype=_F32, device=rpn_cls.device)
    dreg = torch.empty(rpn_reg.shape, dtype=_F32, device=rpn_reg.device)
    _cabi.check(_cabi.lib().prcnn_rpn_loss_backward(*args, ctypes.byref(cfg), _p(counts), _p(norm), _p(grad_out), _p(dcls), _p(dreg),
                                                    _stream()), "prcnn_rpn_loss_backward")
    return dcls, dreg


def rpn_loss_cls_sums(rpn_cls, cls_label):
    """DiceLoss: rpn_cls (B,N,1) f32, cls_label (B,N) i32 / i64 -> (2) f64 on the device: the sums of min(sigmoid(x), t) and of
    max(sigmoid(x), t) over the rows with label >= 0.  Two launches, nothing read back; a data-parallel caller all-reduces the
    result in place before rpn_loss_forward_kind / rpn_loss_backward_kind read it."""
    if not (isinstance(rpn_cls, torch.Tensor) and rpn_cls.is_cuda and rpn_cls.dtype == _F32):
        raise RuntimeError("rpn_loss: rpn_cls must be a float32 CUDA(HIP) tensor")
    label, is64 = _rpn_loss_label(cls_label)
    npts = label.numel()
    if rpn_cls.numel() != npts:
        raise ValueError("rpn_loss: rpn_cls / rpn_cls_label must have %d rows" % npts)
    cls_rows, ld_cls = _uniform_rows(rpn_cls.reshape(rpn_cls.shape + (1,)) if rpn_cls.dim() == 1 else rpn_cls)
    sums = torch.empty((2,), dtype=torch.float64, device=label.device)
    work = _rpn_loss_work(npts, label.device)
    _cabi.check(_cabi.lib().prcnn_rpn_loss_cls_sums(_p(cls_rows), ld_cls, _p(label), is64, npts, _p(sums), _p(work), work.numel() * 8,
                                                    _stream()), "prcnn_rpn_loss_cls_sums")
    return sums


def _rpn_loss_kind_args(cfg, cls_sums, fg_weight):
    if cfg.loss_cls == 1:
        _chk(cls_sums, "cls_sums", torch.float64, 1)
        if cls_sums.numel() != 2:
            raise ValueError("rpn_loss: cls_sums must hold the two sums of rpn_loss_cls_sums")
    return _p(cls_sums) if cfg.loss_cls == 1 else None, float(fg_weight)


def rpn_loss_forward_kind(rpn_cls, rpn_reg, cls_label, reg_label, cfg, counts, norm, cls_sums=None, fg_weight=1.0):
    """rpn_loss_forward for every RPN.LOSS_CLS (cfg.loss_cls 0 focal: the same launches; 1 DiceLoss; 2 BinaryCrossEntropy).
    cls_sums: DiceLoss, the (2) f64 of rpn_loss_cls_sums; fg_weight: BinaryCrossEntropy, RPN.FG_WEIGHT.  norm None (DiceLoss,
    BinaryCrossEntropy): the single-process normalisers, formed from counts on the device.  terms[6:8] are 0 for those two kinds."""
    args, keep = _rpn_loss_prelude(rpn_cls, rpn_reg, cls_label, reg_label, counts, norm)
    sums_p, fg_weight = _rpn_loss_kind_args(cfg, cls_sums, fg_weight)
    terms = torch.empty((9,), dtype=_F32, device=rpn_reg.device)
    work = _rpn_loss_work(args[7], rpn_reg.device)
    _cabi.check(_cabi.lib().prcnn_rpn_loss_forward_kind(*args, ctypes.byref(cfg), _p(counts), _p(norm), _p(terms), _p(work),
                                                        work.numel() * 8, sums_p, fg_weight, _stream()), "prcnn_rpn_loss_forward_kind")
    return terms


def rpn_loss_backward_kind(rpn_cls, rpn_reg, cls_label, reg_label, cfg, counts, norm, grad_out, cls_sums=None, fg_weight=1.0):
    """rpn_loss_backward for every RPN.LOSS_CLS, arguments as rpn_loss_forward_kind; one launch that writes every entry once"""
    args, keep = _rpn_loss_prelude(rpn_cls, rpn_reg, cls_label, reg_label, counts, norm)
    sums_p, fg_weight = _rpn_loss_kind_args(cfg, cls_sums, fg_weight)
    _chk(grad_out, "grad_out")
    if grad_out.numel() != 1:
        raise ValueError("rpn_loss_backward_kind: grad_out must be a scalar")
    dcls = torch.empty(rpn_cls.shape, dtype=_F32, device=rpn_cls.device)
    dreg = torch.empty(rpn_reg.shape, dtype=_F32, device=rpn_reg.device)
    _cabi.check(_cabi.lib().prcnn_rpn_loss_backward_kind(*args, ctypes.byref(cfg), _p(counts), _p(norm), _p(grad_out), _p(dcls), _p(dreg),
                                                         sums_p, fg_weight, _stream()), "prcnn_rpn_loss_backward_kind")
    return dcls, dreg


# what csrc/rcnn_loss.hip takes: RC_MAX_C channels per row (any count up to it), RC_MAX_ROWS rows, RL_MAX_BINS bins per head.
# train_functions routes a configuration beyond them to the composed loss; the exports answer PRCNN_EUNSUPPORTED.
RCNN_LOSS_MAX_C = 56
RCNN_LOSS_MAX_ROWS = 1 << 24
RCNN_LOSS_TERMS = 23


def rcnn_loss_cfg(cfg, mean_size):
    """an RCNNConfig-like object + CLS_MEAN_SIZE -> prcnn_rcnn_loss_cfg_t (loss kinds numbered as rpn_loss_cfg; what
    csrc/rcnn_loss.hip accepts is decided there)"""
    kinds = {"SigmoidFocalLoss": 0, "DiceLoss": 1, "BinaryCrossEntropy": 2}
    alpha = cfg.FOCAL_ALPHA[0]
    return _cabi.RcnnLossCfg(loc_scope=float(cfg.LOC_SCOPE), loc_bin_size=float(cfg.LOC_BIN_SIZE), loc_y_scope=float(cfg.LOC_Y_SCOPE),
                             loc_y_bin_size=float(cfg.LOC_Y_BIN_SIZE), mean_size=(ctypes.c_double * 3)(*[float(v) for v in mean_size]),
                             gamma=float(cfg.FOCAL_GAMMA), alpha=0.0 if alpha is None else float(alpha),
                             num_head_bin=int(cfg.NUM_HEAD_BIN), y_by_bin=int(bool(cfg.LOC_Y_BY_BIN)),
                             size_res_on_roi=int(bool(cfg.SIZE_RES_ON_ROI)), loss_cls=kinds.get(cfg.LOSS_CLS, -1),
                             has_alpha=int(alpha is not None))


def rcnn_loss_channels(cfg):
    """channels of an rcnn_reg row under cfg: 4 * nb + (2 * nby or 1) + 2 * NUM_HEAD_BIN + 3"""
    nb = int(cfg.LOC_SCOPE / cfg.LOC_BIN_SIZE) * 2
    nby = int(cfg.LOC_Y_SCOPE / cfg.LOC_Y_BIN_SIZE) * 2
    return 4 * nb + (2 * nby if cfg.LOC_Y_BY_BIN else 1) + 2 * int(cfg.NUM_HEAD_BIN) + 3


def _rcnn_loss_ints(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.int32, torch.int64)):
        raise RuntimeError("rcnn_loss: %s must be an int32 or int64 CUDA(HIP) tensor" % name)
    return t.contiguous(), int(t.dtype == torch.int64)


def _rcnn_loss_work(R, device):
    return torch.empty((_cabi.lib().prcnn_rcnn_loss_workspace_bytes(R) + 7) // 8, dtype=torch.int64, device=device)


def _rcnn_loss_prelude(rcnn_cls, rcnn_reg, cls_label, reg_valid_mask, roi_boxes3d, gt_of_rois):
    for name, t in (("rcnn_cls", rcnn_cls), ("rcnn_reg", rcnn_reg)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == _F32):
            raise RuntimeError("rcnn_loss: %s must be a float32 CUDA(HIP) tensor" % name)
    C = rcnn_reg.shape[-1]
    R = rcnn_reg.numel() // C
    if rcnn_cls.numel() != R or cls_label.numel() != R or reg_valid_mask.numel() != R:
        raise ValueError("rcnn_loss: rcnn_cls / cls_label / reg_valid_mask must have %d rows" % R)
    _chk(roi_boxes3d, "roi_boxes3d"); _chk(gt_of_rois, "gt_of_rois")
    for name, t in (("roi_boxes3d", roi_boxes3d), ("gt_of_rois", gt_of_rois)):
        if t.numel() != R * 7 or t.shape[-1] != 7:
            raise ValueError("rcnn_loss: %s must be (..., 7) with %d rows" % (name, R))
    label, label64 = _rcnn_loss_ints(cls_label, "cls_label")
    mask, mask64 = _rcnn_loss_ints(reg_valid_mask, "reg_valid_mask")
    cls_rows, ld_cls = _uniform_rows(rcnn_cls.reshape(rcnn_cls.shape + (1,)) if rcnn_cls.dim() == 1 else rcnn_cls)
    reg_rows, ld_reg = _uniform_rows(rcnn_reg)
    args = (_p(cls_rows), ld_cls, _p(reg_rows), ld_reg, _p(label), label64, _p(mask), mask64, _p(roi_boxes3d), _p(gt_of_rois), R, C)
    return args, (cls_rows, reg_rows, label, mask)


def rcnn_loss_forward(rcnn_cls, rcnn_reg, cls_label, reg_valid_mask, roi_boxes3d, gt_of_rois, cfg, finalize=True):
    """rcnn_cls (R,1), rcnn_reg (R,C) f32 (views whose rows sit at ONE stride are read in place, see _uniform_rows; C is any count
    up to RCNN_LOSS_MAX_C), cls_label (R) and reg_valid_mask (R) i32 / i64, roi_boxes3d (R,7), gt_of_rois (R,7), cfg (rcnn_loss_cfg)
    -> counts (4) i32 {#(label > 0), #(label >= 0), #(mask > 0), sum of mask}, terms (RCNN_LOSS_TERMS) f32 or None, work.
    finalize=True: the single-process loss, one launch up to 256 rows and two beyond.  finalize=False (data-parallel callers): the
    counts and the unnormalised sums in work only, one launch; rcnn_loss_finalize follows.  Nothing is read back."""
    args, keep = _rcnn_loss_prelude(rcnn_cls, rcnn_reg, cls_label, reg_valid_mask, roi_boxes3d, gt_of_rois)
    dev = rcnn_reg.device
    counts = torch.empty((4,), dtype=_INT, device=dev)
    terms = torch.empty((RCNN_LOSS_TERMS,), dtype=_F32, device=dev) if finalize else None
    work = _rcnn_loss_work(args[10], dev)
    _cabi.check(_cabi.lib().prcnn_rcnn_loss_forward(*args, ctypes.byref(cfg), int(bool(finalize)), _p(counts), _p(terms), _p(work),
                                                    work.numel() * 8, _stream()), "prcnn_rcnn_loss_forward")
    return counts, terms, work


def rcnn_loss_finalize(R, C, cfg, counts, norm, work):
    """the sums rcnn_loss_forward(finalize=False) left in work + counts + norm (2) f32 {classification scale, regression scale} (or
    None: the single-process normalisers) -> terms (RCNN_LOSS_TERMS) f32; one launch"""
    _chk(counts, "counts", _INT, 1)
    if norm is not None:
        _chk(norm, "norm", _F32, 1)
    terms = torch.empty((RCNN_LOSS_TERMS,), dtype=_F32, device=counts.device)
    _cabi.check(_cabi.lib().prcnn_rcnn_loss_finalize(R, C, ctypes.byref(cfg), _p(counts), _p(norm), _p(terms), _p(work), work.numel() * 8,
                                                     _stream()), "prcnn_rcnn_loss_finalize")
    return terms


def rcnn_loss_backward(rcnn_cls, rcnn_reg, cls_label, reg_valid_mask, roi_boxes3d, gt_of_rois, cfg, counts, norm, grad_out):
    """the inputs of rcnn_loss_forward + its counts, the norm given to rcnn_loss_finalize (or None) and grad_out (a float32 device
    scalar) -> grad_out * d loss / d rcnn_cls, d loss / d rcnn_reg, contiguous, in the inputs' shapes; one launch that writes every
    entry once"""
    args, keep = _rcnn_loss_prelude(rcnn_cls, rcnn_reg, cls_label, reg_valid_mask, roi_boxes3d, gt_of_rois)
    _chk(counts, "counts", _INT, 1); _chk(grad_out, "grad_out")
    if norm is not None:
        _chk(norm, "norm", _F32, 1)
    if grad_out.numel() != 1:
        raise ValueError("rcnn_loss_backward: grad_out must be a scalar")
    dcls = torch.empty(rcnn_cls.shape, dtype=_F32, device=rcnn_cls.device)
    dreg = torch.empty(rcnn_reg.shape, dtype=_F32, device=rcnn_reg.device)
    _cabi.check(_cabi.lib().prcnn_rcnn_loss_backward(*args, ctypes.byref(cfg), _p(counts), _p(norm), _p(grad_out), _p(dcls), _p(dreg),
                                                     _stream()), "prcnn_rcnn_loss_backward")
    return dcls, dreg


def gt_aug_edit(pts, intensity, boxes3d, new_pts, new_intensity, num_pts=None, num_boxes=None, num_new=None, extra_h=2.0,
                want_removed=False):
    """The point work of KittiRCNNDataset.apply_gt_aug_to_one_scene (kitti_rcnn_dataset.py:484-507) for a batch of scenes.
    pts (B,N,3), intensity (B,N) or None, boxes3d (B,K,7) accepted objects (tested with h + extra_h), new_pts (B,P,3),
    new_intensity (B,P) or None; num_* (B) i32 live counts or None.
    -> out_pts (B,N+P,3), out_intensity (B,N+P) or None, count (B) i32 [, removed (B,N) i32]: surviving scene points in their
    original order, then the new points; rows past count are zero."""
    _chk(pts, "pts", ndim=3); _chk(boxes3d, "boxes3d", ndim=3); _chk(new_pts, "new_pts", ndim=3)
    B, N, _ = pts.shape
    K, P = boxes3d.shape[1], new_pts.shape[1]
    if boxes3d.shape[0] != B or boxes3d.shape[2] != 7 or new_pts.shape[0] != B or new_pts.shape[2] != 3:
        raise ValueError("gt_aug_edit: boxes3d must be (%d, K, 7), new_pts (%d, P, 3)" % (B, B))
    if (intensity is None) != (new_intensity is None):
        raise ValueError("gt_aug_edit: intensity and new_intensity go together")
    if intensity is not None:
        _chk(intensity, "intensity", ndim=2); _chk(new_intensity, "new_intensity", ndim=2)
        if tuple(intensity.shape) != (B, N) or tuple(new_intensity.shape) != (B, P):
            raise ValueError("gt_aug_edit: intensity must be (B, N), new_intensity (B, P)")
    for name, t in (("num_pts", num_pts), ("num_boxes", num_boxes), ("num_new", num_new)):
        if t is not None:
            _chk(t, name, _INT, 1)
            if t.shape[0] != B:
                raise ValueError("gt_aug_edit: %s must be (%d,)" % (name, B))
    dev = pts.device
    out_pts = torch.empty((B, N + P, 3), dtype=_F32, device=dev)
    out_int = torch.empty((B, N + P), dtype=_F32, device=dev) if intensity is not None else None
    count = torch.empty((B,), dtype=_INT, device=dev)
    removed = torch.empty((B, N), dtype=_INT, device=dev) if want_removed else None
    _cabi.check(_cabi.lib().prcnn_gt_aug_edit(_p(pts), _p(intensity), _p(num_pts), _p(boxes3d), _p(num_boxes), float(extra_h),
                                              _p(new_pts), _p(new_intensity), _p(num_new), B, N, K, P, _p(out_pts), _p(out_int),
                                              _p(count), _p(removed), _stream()), "prcnn_gt_aug_edit")
    return (out_pts, out_int, count, removed) if want_removed else (out_pts, out_int, count)


def corner_iou3d(corners_a, corners_b, need_bev=False):
    """kitti_utils.get_iou3d (lib/utils/kitti_utils.py:195-235): corners_a (N,8,3), corners_b (M,8,3) -> iou3d (N,M)
    [, iou_bev (N,M) when need_bev].  Exact double clip of the bottom quads in place of shapely (csrc/quad_clip.h)."""
    _chk(corners_a, "corners_a", ndim=3); _chk(corners_b, "corners_b", ndim=3)
    if tuple(corners_a.shape[1:]) != (8, 3) or tuple(corners_b.shape[1:]) != (8, 3):
        raise ValueError("corner_iou3d: corners must be (N, 8, 3) and (M, 8, 3)")
    N, M = corners_a.shape[0], corners_b.shape[0]
    iou3d = torch.empty((N, M), dtype=_F32, device=corners_a.device)
    bev = torch.empty((N, M), dtype=_F32, device=corners_a.device) if need_bev else None
    _cabi.check(_cabi.lib().prcnn_corner_iou3d(_p(corners_a), N, _p(corners_b), M, _p(iou3d), _p(bev), _stream()), "prcnn_corner_iou3d")
    return (iou3d, bev) if need_bev else iou3d


def gt_aug_sample(gt_boxes3d, num_gt, planes, db_boxes, db_alpha, db_npts, easy_idx, hard_idx, extra_num=15, rand_num=True,
                  apply_prob=1.0, hard_ratio=0.6, area_scope=None, try_times=100, max_accept=16, seed=0):
    """The sampling loop of KittiRCNNDataset.apply_gt_aug_to_one_scene (kitti_rcnn_dataset.py:414-497) for a batch, one launch.
    gt_boxes3d (B,G,7) non-DontCare labels, num_gt (B) i32 or None, planes (B,4) f64 road planes; db_boxes (D,7), db_alpha (D),
    db_npts (D) i32, easy_idx (E) / hard_idx (H) i32 database ids (used when hard_ratio > 0); area_scope = 6 floats or None.
    -> dict: count (B) i32, db_id (B,K) i32, boxes3d (B,K,7) placed boxes, alpha (B,K), y_shift (B,K) f64, stats (B,4) i32
    (applied, extra_gt_num, counted tries, tries started), status (B) i32: 0 ok, 1 the reference raises, 2 more than max_accept
    accepted, 3 an easy / hard entry outside [0, D) (include/prcnn_pointops.h)"""
    _chk(gt_boxes3d, "gt_boxes3d", ndim=3); _chk(planes, "planes", torch.float64, 2)
    _chk(db_boxes, "db_boxes", ndim=2); _chk(db_alpha, "db_alpha", ndim=1); _chk(db_npts, "db_npts", _INT, 1)
    B, G, C = gt_boxes3d.shape
    D = db_boxes.shape[0]
    if C != 7 or tuple(planes.shape) != (B, 4):
        raise ValueError("gt_aug_sample: gt_boxes3d must be (B, G, 7), planes (B, 4)")
    if db_boxes.shape[1] != 7 or db_alpha.shape[0] != D or db_npts.shape[0] != D:
        raise ValueError("gt_aug_sample: db_boxes (D, 7), db_alpha (D,), db_npts (D,) disagree")
    if num_gt is not None:
        _chk(num_gt, "num_gt", _INT, 1)
        if num_gt.shape[0] != B:
            raise ValueError("gt_aug_sample: num_gt must be (%d,)" % B)
    for name, t in (("easy_idx", easy_idx), ("hard_idx", hard_idx)):
        if t is not None:
            _chk(t, name, _INT, 1)
    if hard_ratio > 0 and (easy_idx is None or hard_idx is None):
        raise ValueError("gt_aug_sample: hard_ratio > 0 needs the easy and hard lists")
    dev = gt_boxes3d.device
    for name, t in (("num_gt", num_gt), ("planes", planes), ("db_boxes", db_boxes), ("db_alpha", db_alpha), ("db_npts", db_npts),
                    ("easy_idx", easy_idx), ("hard_idx", hard_idx)):
        if t is not None and t.device != dev:
            raise RuntimeError("gt_aug_sample: %s is on %s, gt_boxes3d on %s" % (name, t.device, dev))
    # ids outside [0, D) in the easy / hard lists are caught by the kernel (status 3) without a host read of the lists
    if not 1 <= max_accept <= 64 or G + max_accept > 256:
        raise ValueError("gt_aug_sample: max_accept must be 1..64 with G + max_accept <= 256 (G=%d)" % G)
    K = int(max_accept)
    out = {"count": torch.empty((B,), dtype=_INT, device=dev), "db_id": torch.empty((B, K), dtype=_INT, device=dev),
           "boxes3d": torch.empty((B, K, 7), dtype=_F32, device=dev), "alpha": torch.empty((B, K), dtype=_F32, device=dev),
           "y_shift": torch.empty((B, K), dtype=torch.float64, device=dev), "stats": torch.empty((B, 4), dtype=_INT, device=dev),
           "status": torch.empty((B,), dtype=_INT, device=dev)}
    cfg4 = (ctypes.c_double * 4)(float(extra_num), 1.0 if rand_num else 0.0, float(apply_prob), float(hard_ratio))
    scope = None if area_scope is None else (ctypes.c_double * 6)(*[float(v) for v in area_scope])
    E = 0 if easy_idx is None else easy_idx.shape[0]
    H = 0 if hard_idx is None else hard_idx.shape[0]
    _cabi.check(_cabi.lib().prcnn_gt_aug_sample(
        _p(gt_boxes3d), _p(num_gt), _p(planes), B, G, _p(db_boxes), _p(db_alpha), _p(db_npts), D, _p(easy_idx), E, _p(hard_idx), H,
        ctypes.cast(cfg4, ctypes.c_void_p), None if scope is None else ctypes.cast(scope, ctypes.c_void_p), int(try_times), K, int(seed) & 0xFFFFFFFF, _p(out["count"]), _p(out["db_id"]), _p(out["boxes3d"]),
        _p(out["alpha"]), _p(out["y_shift"]), _p(out["stats"]), _p(out["status"]), _stream()), "prcnn_gt_aug_sample")
    return out


def pts_in_boxes3d(pts, boxes3d):
    """pts (N,3), boxes3d (M,7) -> flags (M,N) i32"""
    _chk(pts, "pts", ndim=2); _chk(boxes3d, "boxes3d", ndim=2)
    N, M = pts.shape[0], boxes3d.shape[0]
    flags = torch.empty((M, N), dtype=_INT, device=pts.device)
    _cabi.check(_cabi.lib().prcnn_pts_in_boxes3d(_p(pts), _p(boxes3d), N, M, _p(flags), _stream()), "prcnn_pts_in_boxes3d")
    return flags


# ------------------------------------------------------------------ iou3d
def boxes_overlap_bev(boxes_a, boxes_b, out=None):
    _chk(boxes_a, "boxes_a", ndim=2); _chk(boxes_b, "boxes_b", ndim=2)
    na, nb = boxes_a.shape[0], boxes_b.shape[0]
    if out is None:
        out = torch.empty((na, nb), dtype=_F32, device=boxes_a.device)
    _cabi.check(_cabi.lib().prcnn_boxes_overlap_bev(_p(boxes_a), na, _p(boxes_b), nb, _p(out), _stream()),
                "prcnn_boxes_overlap_bev")
    return out


def boxes_iou_bev(boxes_a, boxes_b, out=None):
    _chk(boxes_a, "boxes_a", ndim=2); _chk(boxes_b, "boxes_b", ndim=2)
    na, nb = boxes_a.shape[0], boxes_b.shape[0]
    if out is None:
        out = torch.empty((na, nb), dtype=_F32, device=boxes_a.device)
    _cabi.check(_cabi.lib().prcnn_boxes_iou_bev(_p(boxes_a), na, _p(boxes_b), nb, _p(out), _stream()),
                "prcnn_boxes_iou_bev")
    return out


def ref_trig(fn, a, b=None):
    """csrc/ref_trig.h on the device, element-wise: fn in {"sinf", "cosf", "atan2f"} (atan2f(a, b)); float32 tensors"""
    _chk(a, "a")
    out = torch.empty_like(a)
    _cabi.check(_cabi.lib().prcnn_ref_trig(_p(a), _p(b), a.numel(), ["sinf", "cosf", "atan2f"].index(fn), _p(out), _stream()), "prcnn_ref_trig")
    return out


def boxes_iou3d(boxes_a, boxes_b):
    """boxes_a (N,7), boxes_b (M,7) [x, y, z, h, w, l, ry] -> 3-D IoU (N,M)   [iou3d_utils.boxes_iou3d_gpu, iou3d_utils.py:20-53]"""
    _chk(boxes_a, "boxes_a", ndim=2); _chk(boxes_b, "boxes_b", ndim=2)
    out = torch.empty((boxes_a.shape[0], boxes_b.shape[0]), dtype=_F32, device=boxes_a.device)
    _cabi.check(_cabi.lib().prcnn_boxes_iou3d(_p(boxes_a), boxes_a.shape[0], _p(boxes_b), boxes_b.shape[0], _p(out), _stream()),
                "prcnn_boxes_iou3d")
    return out


# the eight outputs both RoI samplers share
def _roi_sample_outputs(B, M, R, dev):
    return {"rois": torch.empty((B, R, 7), dtype=_F32, device=dev), "gt_of_rois": torch.empty((B, R, 7), dtype=_F32, device=dev),
            "roi_iou": torch.empty((B, R), dtype=_F32, device=dev), "src": torch.empty((B, R), dtype=_INT, device=dev),
            "max_overlaps": torch.empty((B, M), dtype=_F32, device=dev), "gt_assignment": torch.empty((B, M), dtype=_INT, device=dev),
            "counts": torch.empty((B, 4), dtype=_INT, device=dev), "status": torch.empty((B,), dtype=_INT, device=dev)}


# -> cfg6 (doubles: the ratios must arrive as Python computes with them) as a pointer, aug_method as the C ABI's number
def _roi_sample_cfg(thresholds, fg_ratio, hard_bg_ratio, aug_method):
    cfg6 = (ctypes.c_double * 6)(*[float(v) for v in tuple(thresholds) + (fg_ratio, hard_bg_ratio)])
    return ctypes.cast(cfg6, ctypes.c_void_p), {"multiple": 0, "single": 1}[aug_method]


def proposal_target_sample(roi_boxes3d, gt_boxes3d, roi_per_image=64, thresholds=(0.55, 0.6, 0.45, 0.05), fg_ratio=0.5, hard_bg_ratio=0.8,
                           aug_times=10, aug_method="multiple", seed=0):
    """ProposalTargetLayer.sample_rois_for_rcnn for the whole batch in one launch (lib/rpn/proposal_target_layer.py:75-250).
    roi_boxes3d (B,M,7), gt_boxes3d (B,G,>=7, zero rows at the end); thresholds = (REG_FG, CLS_FG, CLS_BG, CLS_BG_LO).
    -> dict: rois, gt_of_rois (B,R,7), roi_iou (B,R), src (B,R) i32, max_overlaps (B,M), gt_assignment (B,M) i32, counts (B,4), status (B)"""
    _chk(roi_boxes3d, "roi_boxes3d", ndim=3); _chk(gt_boxes3d, "gt_boxes3d", ndim=3)
    B, M, _ = roi_boxes3d.shape
    G, gc = gt_boxes3d.shape[1], gt_boxes3d.shape[2]
    R, dev = int(roi_per_image), roi_boxes3d.device
    o = _roi_sample_outputs(B, M, R, dev)
    cfg6, method = _roi_sample_cfg(thresholds, fg_ratio, hard_bg_ratio, aug_method)
    _cabi.check(_cabi.lib().prcnn_proposal_target_sample(_p(roi_boxes3d), _p(gt_boxes3d), B, M, G, gc, R, cfg6,
                                                         int(aug_times), method, seed & 0xFFFFFFFF,
                                                         _p(o["rois"]), _p(o["gt_of_rois"]), _p(o["roi_iou"]), _p(o["src"]),
                                                         _p(o["max_overlaps"]), _p(o["gt_assignment"]), _p(o["counts"]), _p(o["status"]),
                                                         _stream()), "prcnn_proposal_target_sample")
    return o


def rcnn_offline_sample(roi_boxes3d, num_roi, gt_boxes3d, num_gt, roi_per_image=64, thresholds=(0.55, 0.6, 0.45, 0.05), fg_ratio=0.5,
                        hard_bg_ratio=0.8, aug_times=10, aug_method="multiple", seed=0, frame_ids=None):
    """The sampling part of KittiRCNNDataset.get_rcnn_training_sample_batch (lib/datasets/kitti_rcnn_dataset.py:890-957) for a batch
    (`--train_mode rcnn_offline`, RCNN.ROI_SAMPLE_JIT False).  roi_boxes3d (B,M,7) with num_roi (B) i32, gt_boxes3d (B,G,7) with
    num_gt (B) i32; thresholds = (REG_FG, CLS_FG, CLS_BG, CLS_BG_LO); frame_ids (B) i32 = the id of every frame in the random table
    (default: its position in the batch).
    -> dict: iou3d (B,M,G) corner IoU, rois, gt_of_rois (B,R,7), roi_iou (B,R) the noise loop's last IoU, src (B,R) i32,
    max_overlaps (B,M), gt_assignment (B,M) i32, counts (B,4), status (B): 0 ok, 1 the reference raises, 2 no label
    (include/prcnn_pointops.h)"""
    _chk(roi_boxes3d, "roi_boxes3d", ndim=3); _chk(gt_boxes3d, "gt_boxes3d", ndim=3)
    _chk(num_roi, "num_roi", _INT, 1); _chk(num_gt, "num_gt", _INT, 1)
    B, M, _ = roi_boxes3d.shape
    G = gt_boxes3d.shape[1]
    if roi_boxes3d.shape[2] != 7 or gt_boxes3d.shape[0] != B or gt_boxes3d.shape[2] != 7 or num_roi.shape[0] != B or num_gt.shape[0] != B:
        raise ValueError("rcnn_offline_sample: roi_boxes3d (B, M, 7), gt_boxes3d (B, G, 7), num_roi (B,), num_gt (B,) disagree")
    if aug_method not in ("multiple", "single"):
        raise ValueError("rcnn_offline_sample: REG_AUG_METHOD %r is not supported ('multiple' or 'single')" % (aug_method,))
    dev = roi_boxes3d.device
    if frame_ids is not None:
        _chk(frame_ids, "frame_ids", _INT, 1)
        if frame_ids.shape[0] != B:
            raise ValueError("rcnn_offline_sample: frame_ids must be (%d,)" % B)
    for name, t in (("num_roi", num_roi), ("gt_boxes3d", gt_boxes3d), ("num_gt", num_gt), ("frame_ids", frame_ids)):
        if t is not None and t.device != dev:
            raise RuntimeError("rcnn_offline_sample: %s is on %s, roi_boxes3d on %s" % (name, t.device, dev))
    R = int(roi_per_image)
    o = dict(iou3d=torch.empty((B, M, G), dtype=_F32, device=dev), **_roi_sample_outputs(B, M, R, dev))
    cfg6, method = _roi_sample_cfg(thresholds, fg_ratio, hard_bg_ratio, aug_method)
    _cabi.check(_cabi.lib().prcnn_rcnn_offline_sample(
        _p(roi_boxes3d), _p(num_roi), _p(gt_boxes3d), _p(num_gt), _p(frame_ids), B, M, G, R, cfg6,
        int(aug_times), method, int(seed) & 0xFFFFFFFF, _p(o["iou3d"]), _p(o["rois"]), _p(o["gt_of_rois"]),
        _p(o["roi_iou"]), _p(o["src"]), _p(o["max_overlaps"]), _p(o["gt_assignment"]), _p(o["counts"]), _p(o["status"]), _stream()),
        "prcnn_rcnn_offline_sample")
    return o


AUG_METHOD_BITS = {"rotation": 1, "scaling": 2, "flip": 4}


def rcnn_offline_finish(pooled, sample, pooled_empty_flag, thresholds=(0.55, 0.6, 0.45), aug_methods=("rotation", "scaling", "flip"),
                        flip_prob=0.5, rot_range=18, seed=0, frame_ids=None):
    """Everything of get_rcnn_training_sample_batch after pooling (kitti_rcnn_dataset.py:976-1010), one launch.  pooled (B,R,S,W) or
    (B*R,S,W) contiguous, xyz in its first three columns, REWRITTEN IN PLACE (per-RoI rotate / scale / flip, canonical transform);
    sample: rcnn_offline_sample's dict; pooled_empty_flag (B,R) i32; thresholds = (REG_FG, CLS_FG, CLS_BG); aug_methods: the entries of
    AUG_METHOD_LIST, () when AUG_DATA is off.
    -> dict roi_boxes3d, gt_boxes3d (B,R,7) the augmented boxes, gt_boxes3d_ct (B,R,7), cls_label, reg_valid_mask (B,R) i32"""
    _chk(pooled, "pooled"); _chk(pooled_empty_flag, "pooled_empty_flag", _INT, 2)
    rois, gts, iou, status = sample["rois"], sample["gt_of_rois"], sample["roi_iou"], sample["status"]
    B, R, _ = rois.shape
    if not pooled.is_contiguous() or pooled.dim() not in (3, 4) or pooled.numel() % (B * R) or pooled.shape[-1] < 3 or \
            pooled.numel() // (B * R) != pooled.shape[-2] * pooled.shape[-1] or tuple(pooled_empty_flag.shape) != (B, R):
        raise ValueError("rcnn_offline_finish: pooled must be contiguous (B, R, S, W >= 3) rows for the sample's (%d, %d) slots" % (B, R))
    S, W = pooled.shape[-2], pooled.shape[-1]
    if frame_ids is not None:
        _chk(frame_ids, "frame_ids", _INT, 1)
    dev = pooled.device
    o = {"roi_boxes3d": torch.empty((B, R, 7), dtype=_F32, device=dev), "gt_boxes3d": torch.empty((B, R, 7), dtype=_F32, device=dev),
         "gt_boxes3d_ct": torch.empty((B, R, 7), dtype=_F32, device=dev), "cls_label": torch.empty((B, R), dtype=_INT, device=dev),
         "reg_valid_mask": torch.empty((B, R), dtype=_INT, device=dev)}
    cfg5 = (ctypes.c_double * 5)(*[float(v) for v in tuple(thresholds) + (flip_prob, rot_range)])
    _cabi.check(_cabi.lib().prcnn_rcnn_offline_finish(
        _p(pooled), W, B, R, S, _p(rois), _p(gts), _p(iou), _p(pooled_empty_flag), _p(status), _p(frame_ids),
        ctypes.cast(cfg5, ctypes.c_void_p), sum(AUG_METHOD_BITS[m] for m in set(aug_methods)), int(seed) & 0xFFFFFFFF, _p(o["roi_boxes3d"]),
        _p(o["gt_boxes3d"]), _p(o["gt_boxes3d_ct"]), _p(o["cls_label"]), _p(o["reg_valid_mask"]), _stream()), "prcnn_rcnn_offline_finish")
    return o


def nms_sorted(boxes_sorted, thresh, rotated=True, max_keep=0):
    """Greedy NMS over boxes already sorted by descending score, fully on device.
    -> keep (N) int64 (first num entries valid), num (1) int32.  No host sync.
    max_keep > 0 stops the sweep once that many boxes are kept (the proposal layer only uses the first
    RPN_POST_NMS_TOP_N of them, lib/rpn/proposal_layer.py:112): same leading entries, a fraction of the work."""
    _chk(boxes_sorted, "boxes", ndim=2)
    N = boxes_sorted.shape[0]
    L = _cabi.lib()
    keep = torch.empty((max(N, 1),), dtype=torch.int64, device=boxes_sorted.device)
    num = torch.empty((1,), dtype=_INT, device=boxes_sorted.device)
    wsb = L.prcnn_nms_workspace_bytes(N)
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=boxes_sorted.device)
    _cabi.check(L.prcnn_nms(_p(boxes_sorted), N, float(thresh), 0 if rotated else 1, int(max_keep), _p(keep), _p(num),
                            _p(ws), wsb, _stream()), "prcnn_nms")
    return keep, num


_NMS_STAGE = threading.local()


def nms_sorted_to_host(boxes_sorted, thresh, rotated, keep_cpu):
    """The shape the reference's pybind functions force (iou3d.cpp:73-120: `keep` is a CPU int64 tensor, the return value the number of
    kept boxes): greedy NMS over boxes sorted by descending score, the kept indices copied into `keep_cpu[:n]`, -> n (host int).
    ONE host synchronisation: the kept indices and their count leave the device in one asynchronous copy into a pinned staging buffer
    (one per host thread and device) queued behind the sweep, the host waits for the stream once and copies the n entries."""
    _chk(boxes_sorted, "boxes", ndim=2)
    N = boxes_sorted.shape[0]
    if N == 0:
        return 0
    dev = boxes_sorted.device
    stages = getattr(_NMS_STAGE, "buf", None)
    if stages is None:
        stages = _NMS_STAGE.buf = {}
    stage = stages.get(dev.index)
    if stage is None or stage.numel() < N + 1:
        stage = stages[dev.index] = torch.empty((max(2 * N, 8192) + 1,), dtype=torch.int64).pin_memory()
    L = _cabi.lib()
    wsb = L.prcnn_nms_workspace_bytes(N)
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=dev)
    out = torch.empty((N + 1,), dtype=torch.int64, device=dev)          # [0, N): kept indices, [N]: their count (low int32)
    stream = torch.cuda.current_stream(dev)
    _cabi.check(L.prcnn_nms(_p(boxes_sorted), N, float(thresh), 0 if rotated else 1, 0, _p(out), _p(out) + 8 * N,
                            _p(ws), wsb, stream.cuda_stream), "prcnn_nms")
    stage[:N + 1].copy_(out, non_blocking=True)
    stream.synchronize()
    n = int(stage[N:N + 1].view(torch.int32)[0])
    if n:
        keep_cpu[:n].copy_(stage[:n])
    return n


# ---------------------------------------------------------------------------------------------------------
# proposal stage
# ---------------------------------------------------------------------------------------------------------
def decode_bbox_target(roi, pred_reg, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True,
                       get_y_by_bin=False, loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False, y_to_bottom=False):
    """lib/utils/bbox_transform.py:24-121 as one kernel.  roi (N,3|7), pred_reg (N,C) -> (N,7).
    anchor_size: 3 host floats (h, w, l)."""
    _chk(roi, "roi", ndim=2)
    _chk(pred_reg, "pred_reg", ndim=2)
    if roi.shape[0] != pred_reg.shape[0]:
        raise ValueError("decode_bbox_target: %d rois vs %d regression rows" % (roi.shape[0], pred_reg.shape[0]))
    N, C = pred_reg.shape
    out = torch.empty((N, 7), dtype=torch.float32, device=pred_reg.device)
    anchor = (ctypes.c_float * 3)(*[float(a) for a in anchor_size])
    _cabi.check(_cabi.lib().prcnn_decode_bbox_target(
        _p(roi), roi.shape[1], _p(pred_reg), N, C, float(loc_scope), float(loc_bin_size), int(num_head_bin),
        ctypes.cast(anchor, ctypes.c_void_p), int(bool(get_xz_fine)), int(bool(get_y_by_bin)), float(loc_y_scope),
        float(loc_y_bin_size), int(bool(get_ry_fine)), int(bool(y_to_bottom)), _p(out), _stream()), "prcnn_decode_bbox_target")
    return out


def proposal_layer(scores, boxes3d, pre, post, nms_thresh, rotated=False, ranges=(0.0, 40.0, 80.0)):
    """lib/rpn/proposal_layer.py:35-141 for the whole batch, no host sync.
    scores (B,N) raw, boxes3d (B,N,7) decoded; pre/post = (area 1, area 2) top-n; ranges=None -> score based.
    -> rois (B, post[0]+post[1], 7), roi_scores (B, post[0]+post[1]) zero padded, count (B) int32."""
    _chk(scores, "scores", ndim=2)
    _chk(boxes3d, "boxes3d", ndim=3)
    B, N = scores.shape
    if tuple(boxes3d.shape) != (B, N, 7):
        raise ValueError("proposal_layer: boxes3d must be (%d, %d, 7), got %s" % (B, N, tuple(boxes3d.shape)))
    L = _cabi.lib()
    tot = int(post[0]) + int(post[1])
    dev = scores.device
    rois = torch.empty((B, tot, 7), dtype=torch.float32, device=dev)
    roi_scores = torch.empty((B, tot), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=_INT, device=dev)
    wsb = L.prcnn_proposal_workspace_bytes(B, N, max(pre), max(post))
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=dev)
    r = ranges if ranges is not None else (0.0, 0.0, 0.0)
    _cabi.check(L.prcnn_proposal_layer(_p(scores), _p(boxes3d), B, N, int(ranges is not None), float(r[0]), float(r[1]),
                                       float(r[2]), int(pre[0]), int(pre[1]), int(post[0]), int(post[1]), float(nms_thresh),
                                       0 if rotated else 1, _p(rois), _p(roi_scores), _p(count), _p(ws), wsb, _stream()),
                "prcnn_proposal_layer")
    return rois, roi_scores, count


def nms_batched(boxes3d, scores, valid=None, thresh=0.1, rotated=True, max_keep=0):
    """tools/eval_rcnn.py:600-614 for the whole batch: per frame select valid rows, order by score, greedy NMS.
    boxes3d (B,M,7), scores (B,M), valid (B,M) bool/uint8 or None -> keep (B,max_keep) int32 (-1 padded), num (B)."""
    _chk(boxes3d, "boxes3d", ndim=3)
    _chk(scores, "scores", ndim=2)
    B, M = scores.shape
    if tuple(boxes3d.shape) != (B, M, 7):
        raise ValueError("nms_batched: boxes3d must be (%d, %d, 7), got %s" % (B, M, tuple(boxes3d.shape)))
    if valid is not None:
        if tuple(valid.shape) != (B, M) or not valid.is_cuda:
            raise ValueError("nms_batched: valid must be a (%d, %d) device tensor" % (B, M))
        valid = valid.to(torch.uint8).contiguous()
    mk = M if max_keep <= 0 or max_keep > M else int(max_keep)
    L = _cabi.lib()
    dev = scores.device
    keep = torch.empty((B, max(mk, 1)), dtype=_INT, device=dev)
    num = torch.empty((B,), dtype=_INT, device=dev)
    wsb = L.prcnn_nms_batched_workspace_bytes(B, M)
    ws = torch.empty((max(wsb, 8),), dtype=torch.uint8, device=dev)
    _cabi.check(L.prcnn_nms_batched(_p(boxes3d), _p(scores), _p(valid) if valid is not None else None, B, M, float(thresh),
                                    0 if rotated else 1, mk, _p(keep), _p(num), _p(ws), wsb, _stream()), "prcnn_nms_batched")
    return keep[:, :mk], num


# ---------------------------------------------------------------------------------------------------------
# KITTI evaluation kernels (host logic in pointrcnn_amd/kitti_eval.py)
# ---------------------------------------------------------------------------------------------------------
def rotate_iou_eval(boxes, query_boxes, criterion=-1):
    """rotate_iou.py:287-329 rotate_iou_gpu_eval: (N,5), (K,5) [cx, cy, dx, dy, angle] -> (N,K)"""
    _chk(boxes, "boxes", ndim=2); _chk(query_boxes, "query_boxes", ndim=2)
    N, K = boxes.shape[0], query_boxes.shape[0]
    out = torch.zeros((N, K), dtype=_F32, device=boxes.device)
    _cabi.check(_cabi.lib().prcnn_rotate_iou_eval(_p(boxes), N, _p(query_boxes), K, int(criterion), _p(out), _stream()),
                "prcnn_rotate_iou_eval")
    return out


def kitti_overlaps(metric, dt, dt_off, gt, gt_off, ov_off, total):
    """per-frame overlap blocks (rows = dt, columns = gt) of all frames, flat float64 (see include/prcnn_pointops.h)"""
    F = dt_off.shape[0] - 1
    out = torch.zeros((max(int(total), 1),), dtype=torch.float64, device=dt_off.device)
    _cabi.check(_cabi.lib().prcnn_kitti_overlaps(int(metric), _p(dt), _p(dt_off), _p(gt), _p(gt_off), _p(ov_off), F, _p(out), _stream()),
                "prcnn_kitti_overlaps")
    return out[:int(total)]


def kitti_statistics(overlaps, ov_off, gt_datas, gt_off, dt_datas, dt_off, ign_gt, ign_det, dc, dc_off, metric, min_overlap,
                     thresholds, compute_fp, compute_aos):
    """compute_statistics_jit for every (frame, threshold) -> res (F,T,4) f64, matched (G) f64"""
    F, T = gt_off.shape[0] - 1, thresholds.shape[0]
    dev = gt_off.device
    res = torch.zeros((F, T, 4), dtype=torch.float64, device=dev)
    G = gt_datas.shape[0]
    matched = torch.full((max(G, 1),), float("nan"), dtype=torch.float64, device=dev)
    max_det = int((dt_off[1:] - dt_off[:-1]).max().item()) if F > 0 else 0
    _cabi.check(_cabi.lib().prcnn_kitti_statistics(_p(overlaps), _p(ov_off), _p(gt_datas), _p(gt_off), _p(dt_datas), _p(dt_off),
                                                   _p(ign_gt), _p(ign_det), _p(dc), _p(dc_off), F, max_det, int(metric),
                                                   float(min_overlap), _p(thresholds), T, int(compute_fp), int(compute_aos), _p(res),
                                                   _p(matched), _stream()), "prcnn_kitti_statistics")
    return res, matched[:G]


# ---------------------------------------------------------------------------------------------------------
# padding-free grouping (csrc/dedup.hip)
# ---------------------------------------------------------------------------------------------------------
_split_log = None      # bench.py's instrumented pass sets this to a list to read the device-side list lengths afterwards


class GroupSplit:
    """The G = B*M groups of one ball query split on the device (prcnn_group_compact) into a flat list of the real rows of
    the sparse groups (at most sparse_max hits) and the list of dense groups.  All tensors are worst-case sized; counts
    (3,) int32 holds [flat rows, dense groups, sparse groups]."""

    def __init__(self, idx, new_xyz, N, sparse_max, valid_n=None, counts=None):
        """counts: a (3,) int32 view to use instead of a fresh tensor -- the lists are then allocated only and the caller splits
        (GroupSplit.pair)"""
        _chk(idx, "idx", _INT, 3)
        _chk(new_xyz, "new_xyz", ndim=3)
        B, M, ns = idx.shape
        G, dev = B * M, idx.device
        T = max(1, min(int(sparse_max), ns))
        self.G, self.ns, self.T, self.max_rows = G, ns, T, G * T
        e = lambda shape, dt=_INT: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
        self.ridx, self.rnx = e((1, G * T, 1)), e((1, G * T, 3), _F32)
        self.slist, self.soff, self.scnt = e((G,)), e((G,)), e((G,))
        self.idxn, self.nxn, self.listn = e((1, G, ns)), e((1, G, 3), _F32), e((G,))
        self.counts = e((3,)) if counts is None else counts
        if valid_n is not None and (valid_n.dtype != _INT or valid_n.numel() != B or not valid_n.is_contiguous()):
            raise RuntimeError("valid_n must be a contiguous (B,) int32 tensor")
        if counts is None:
            _cabi.check(_cabi.lib().prcnn_group_compact(_p(idx), _p(new_xyz), B, N, M, ns, T, _p(valid_n), _p(self.ridx), _p(self.rnx), _p(self.slist),
                                                        _p(self.soff), _p(self.scnt), _p(self.idxn), _p(self.nxn), _p(self.listn),
                                                        _p(self.counts), _stream()), "prcnn_group_compact")
        self.rows, self.count_dense, self.count_sparse = self.counts[0:1], self.counts[1:2], self.counts[2:3]
        if _split_log is not None:
            _split_log.append(self)

    def _lists(self):
        return (ctypes.c_void_p * 8)(*[_p(t) for t in (self.ridx, self.rnx, self.slist, self.soff, self.scnt, self.idxn, self.nxn, self.listn)])

    @staticmethod
    def pair(idx_a, sparse_max_a, idx_b, sparse_max_b, new_xyz, N, rdst=False):
        """both scales of an MSG level split by one counter clear and one launch (prcnn_group_compact_pair): two GroupSplits whose
        counts are the halves of one (6,) tensor.  rdst: each also gets .rdst, sized like ridx -- per flat row the group id when the
        row is its group's only one, else -1 (prcnn_group_compact_pair_dst)"""
        if idx_a.shape[:2] != idx_b.shape[:2]:
            raise RuntimeError("GroupSplit.pair: the two index tensors must share (B, M)")
        counts = torch.empty((6,), dtype=_INT, device=idx_a.device)
        a = GroupSplit(idx_a, new_xyz, N, sparse_max_a, counts=counts[0:3])
        b = GroupSplit(idx_b, new_xyz, N, sparse_max_b, counts=counts[3:6])
        B, M, _ = idx_a.shape
        if rdst:
            a.rdst, b.rdst = torch.empty_like(a.ridx), torch.empty_like(b.ridx)
            _cabi.check(_cabi.lib().prcnn_group_compact_pair_dst(_p(idx_a), a.ns, a.T, _p(idx_b), b.ns, b.T, _p(new_xyz), B, N, M, a._lists(), b._lists(),
                                                                 _p(a.rdst), _p(b.rdst), _p(counts), _stream()), "prcnn_group_compact_pair_dst")
            return a, b
        _cabi.check(_cabi.lib().prcnn_group_compact_pair(_p(idx_a), a.ns, a.T, _p(idx_b), b.ns, b.T, _p(new_xyz), B, N, M, a._lists(), b._lists(),
                                                         _p(counts), _stream()), "prcnn_group_compact_pair")
        return a, b


def segmax_scatter(src, sp, dst, col_off):
    """dst[g, col_off : col_off + C] = max over the flat result rows of every sparse group g of the GroupSplit sp"""
    C = src.shape[-1]
    _cabi.check(_cabi.lib().prcnn_segmax_scatter(_p(src), src.stride(-2), _p(sp.slist), _p(sp.soff), _p(sp.scnt), _p(sp.count_sparse),
                                                 sp.G, C, _p(dst), dst.stride(-2), int(col_off), _stream()), "prcnn_segmax_scatter")


def scatter_rows(src, rows_list, count, dst, col_off):
    """dst[rows_list[r], col_off : col_off + C] = src[r] for r < count (count: (1,) int32 device tensor)"""
    C = src.shape[-1]
    _cabi.check(_cabi.lib().prcnn_scatter_rows(_p(src), src.stride(-2), _p(rows_list), _p(count), rows_list.shape[0], C, _p(dst),
                                               dst.stride(-2), int(col_off), _stream()), "prcnn_scatter_rows")


def level_pool(problems, dst, residual=False):
    """The pooling launches of one level as one (prcnn_level_pool).  problems: up to four of (src, sp, col_off, "flat") -- what
    segmax_scatter(src, sp, dst, col_off) does -- or (src, sp, col_off, "dense") -- scatter_rows(src, sp.listn, sp.count_dense, dst,
    col_off); they must write disjoint cells of dst.  residual: flat problems only, and only their groups of two or more rows are
    pooled (prcnn_level_pool_residual) -- the one-row groups were stored by destination (mlp_chain_group_multi with dst)."""
    n = len(problems)
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    src, ld, lst, off, cnt, count, cap, C, col = P(), I(), P(), P(), P(), P(), I(), I(), I()
    for q, (s, sp, c0, kind) in enumerate(problems):
        flat = kind == "flat"
        src[q], ld[q], C[q], col[q], cap[q] = _p(s), s.stride(-2), s.shape[-1], int(c0), sp.G
        lst[q], count[q] = (_p(sp.slist), _p(sp.count_sparse)) if flat else (_p(sp.listn), _p(sp.count_dense))
        off[q], cnt[q] = (_p(sp.soff), _p(sp.scnt)) if flat else (None, None)
    name = "prcnn_level_pool_residual" if residual else "prcnn_level_pool"
    _cabi.check(getattr(_cabi.lib(), name)(n, src, ld, lst, off, cnt, count, cap, C, col, _p(dst), dst.stride(-2), _stream()), name)


# what the wrappers of the passes over raw frames share (the native side of it is csrc/scene_common.h)
def _frames(raw, offsets, calib, *img_hw):
    """raw (total,4) f32, offsets (B+1) i64, calib (B,24) f32 and, where the pass takes one, img_hw (B,2) i32 -> (B, total, device)"""
    _chk(raw, "raw", ndim=2)
    _chk(calib, "calib", ndim=2)
    for hw in img_hw:
        _chk(hw, "img_hw", _INT, 2)
    if offsets.dtype != torch.int64 or not offsets.is_contiguous() or offsets.device != raw.device:
        raise RuntimeError("offsets must be a contiguous int64 tensor on the device of raw")
    B = offsets.shape[0] - 1
    if raw.shape[1] != 4 or calib.shape[1] != 24 or any(hw.shape[1] != 2 for hw in img_hw):
        raise RuntimeError("expected raw (total,4), calib (B,24), img_hw (B,2)")
    if calib.shape[0] != B or any(hw.shape[0] != B for hw in img_hw):
        raise RuntimeError("calib / img_hw must have one row per frame")
    return B, raw.shape[0], raw.device


def _scope(scope):
    """PC_AREA_SCOPE as the library takes it: 6 doubles [x0 x1 y0 y1 z0 z1], or NULL for no range crop"""
    return None if scope is None else (ctypes.c_double * 6)(*[float(v) for v in scope])


def _sample_outputs(B, npoints, dev):
    """-> xyz (B,npoints,3), src (B,npoints) i32, nvalid (B) i32, status (B) i32: what every npoints draw writes"""
    return (torch.empty((B, npoints, 3), dtype=_F32, device=dev), torch.empty((B, npoints), dtype=_INT, device=dev),
            torch.empty((B,), dtype=_INT, device=dev), torch.empty((B,), dtype=_INT, device=dev))


# ---------------------------------------------------------------------------------------------------------
# RPN input builder (csrc/scene.hip)
# ---------------------------------------------------------------------------------------------------------
SCENE_SMALL_MAX = 16384       # npoints up to here: the one-workgroup form of the draw (csrc/scene_common.h)
SCENE_LARGE_MAX = 65536       # npoints up to here: the large exports (the shuffle sorted through HBM)


def _large_npoints(name, npoints):
    """the domain of the large exports, held before any allocation or launch"""
    if not 1 <= int(npoints) <= SCENE_LARGE_MAX:
        raise _cabi.PointOpsError("%s: npoints=%d (1..%d)" % (name, int(npoints), SCENE_LARGE_MAX))


def scene_prepare(raw, offsets, max_points_per_frame, calib, img_hw, scope, npoints, seed, large=None, workspace=None):
    """raw (total,4) f32 scans back to back, offsets (B+1) i64, calib (B,24) f32 [M 4x3 | P2 3x4], img_hw (B,2) i32 -- all on
    the device; scope: 6 host floats [x0 x1 y0 y1 z0 z1] or None.  large: True = prcnn_scene_prepare_large (npoints 1..65536),
    False = prcnn_scene_prepare (1..16384), None = the large export when npoints > 16384.
    -> pts_rect (B,npoints,3), intensity - 0.5 (B,npoints), src index (B,npoints) i32, nvalid (B) i32, status (B) i32
    [lib/datasets/kitti_rcnn_dataset.py:246-310 for a whole batch; see prcnn_scene_prepare]"""
    if large is None:
        large = int(npoints) > SCENE_SMALL_MAX
    if large:
        _large_npoints("scene_prepare", npoints)
    B, total, dev = _frames(raw, offsets, calib, img_hw)
    L = _cabi.lib()
    if large:
        need, fn, name = int(L.prcnn_scene_large_workspace_bytes(total, B, int(npoints))), L.prcnn_scene_prepare_large, "prcnn_scene_prepare_large"
    else:
        need, fn, name = int(L.prcnn_scene_workspace_bytes(total, B)), L.prcnn_scene_prepare, "prcnn_scene_prepare"
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if workspace is None else workspace
    xyz, src, nvalid, status = _sample_outputs(B, npoints, dev)
    inten = torch.empty((B, npoints), dtype=_F32, device=dev)
    _cabi.check(fn(_p(raw), _p(offsets), B, total, int(max_points_per_frame), _p(calib), _p(img_hw), _scope(scope),
                   int(npoints), int(seed) & 0xFFFFFFFF, _p(xyz), _p(inten), _p(src), _p(nvalid), _p(status), _p(ws),
                   ws.numel(), _stream()), name)
    return xyz, inten, src, nvalid, status


# ---------------------------------------------------------------------------------------------------------
# RPN training batch (csrc/train_scene.hip)
# ---------------------------------------------------------------------------------------------------------
AUG_METHODS = ("rotation", "scaling", "flip")


def train_scene_prepare(raw, offsets, max_points_per_frame, calib, img_hw, scope, npoints, seed, gt_boxes3d, gt_alpha, num_gt=None,
                        accepted=None, db=None, aug_methods=AUG_METHODS, aug_prob=(1.0, 1.0, 0.5), aug_rot_range=18,
                        use_intensity=False, workspace=None, large=False):
    """get_rpn_sample's TRAIN path between the GT-augmentation sampling loop and the label generation, for a whole batch
    (prcnn_train_scene_prepare).  raw .. seed as scene_prepare; gt_boxes3d (B,G,7), gt_alpha (B,G), num_gt (B) i32 or None: the
    training labels; accepted = gt_aug_sample's dict or None (GT_AUG_ENABLED false), db = the packed database (an object with
    points (P,3), intensity (P,), offsets (D+1,) i64, size, max_points: kitti_input.GTDatabase); aug_methods = the names of
    cfg.AUG_METHOD_LIST that run (() = cfg.AUG_DATA false), aug_prob = cfg.AUG_METHOD_PROB, aug_rot_range = cfg.AUG_ROT_RANGE.
    -> dict pts_rect (B,npoints,3), pts_input (the same tensor, or (B,npoints,4) when use_intensity), pts_features (B,npoints,1),
    gt_boxes3d (B,G+K,7), num_gt (B), src, nvalid, status, aug (B,8) f64 -- see include/prcnn_pointops.h.
    large: True = prcnn_train_scene_prepare_large (npoints 1..65536); the default keeps prcnn_train_scene_prepare (1..16384)."""
    if large:
        _large_npoints("train_scene_prepare", npoints)
    B, total, dev = _frames(raw, offsets, calib, img_hw)
    _chk(gt_boxes3d, "gt_boxes3d", ndim=3); _chk(gt_alpha, "gt_alpha", ndim=2)
    G = gt_boxes3d.shape[1]
    if tuple(gt_boxes3d.shape) != (B, G, 7) or tuple(gt_alpha.shape) != (B, G):
        raise ValueError("train_scene_prepare: gt_boxes3d must be (%d, G, 7), gt_alpha (%d, G)" % (B, B))
    if num_gt is not None:
        _chk(num_gt, "num_gt", _INT, 1)
        if num_gt.shape[0] != B:
            raise ValueError("train_scene_prepare: num_gt must be (%d,)" % B)
    unknown = [m for m in aug_methods if m not in AUG_METHODS]
    if unknown:
        raise ValueError("train_scene_prepare: unknown augmentation %r" % unknown)
    K, D, db_max = 0, 0, 0
    acc = [None] * 6
    dbt = [None] * 3
    if accepted is not None:
        if db is None:
            raise ValueError("train_scene_prepare: accepted objects need the database they came from")
        K, D, db_max = accepted["db_id"].shape[1], int(db.size), int(db.max_points)
        acc = [_chk(accepted["count"], "count", _INT, 1), _chk(accepted["db_id"], "db_id", _INT, 2),
               _chk(accepted["boxes3d"], "boxes3d", ndim=3), _chk(accepted["alpha"], "alpha", ndim=2),
               _chk(accepted["y_shift"], "y_shift", torch.float64, 2), _chk(accepted["status"], "status", _INT, 1)]
        if acc[0].shape[0] != B or tuple(acc[2].shape) != (B, K, 7) or tuple(acc[3].shape) != (B, K) or tuple(acc[4].shape) != (B, K):
            raise ValueError("train_scene_prepare: the accepted objects must describe %d frames" % B)
        dbt = [_chk(db.points, "db.points", ndim=2), _chk(db.intensity, "db.intensity", ndim=1), db.offsets]
        if dbt[2].dtype != torch.int64 or dbt[2].shape[0] != D + 1 or dbt[1].shape[0] != dbt[0].shape[0]:
            raise ValueError("train_scene_prepare: db.offsets must be (D+1,) int64, db.intensity one value per point")
    L = _cabi.lib()
    if large:
        need, fn, name = int(L.prcnn_train_scene_large_workspace_bytes(total, B, K, db_max, int(npoints))), L.prcnn_train_scene_prepare_large, \
            "prcnn_train_scene_prepare_large"
    else:
        need, fn, name = int(L.prcnn_train_scene_workspace_bytes(total, B, K, db_max)), L.prcnn_train_scene_prepare, "prcnn_train_scene_prepare"
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if workspace is None else workspace
    xyz, src, nvalid, status = _sample_outputs(B, npoints, dev)
    pin = torch.empty((B, npoints, 4), dtype=_F32, device=dev) if use_intensity else None
    feat = torch.empty((B, npoints), dtype=_F32, device=dev)
    out_gt = torch.empty((B, G + K, 7), dtype=_F32, device=dev)
    out_ng = torch.empty((B,), dtype=_INT, device=dev)
    aug = torch.empty((B, 8), dtype=torch.float64, device=dev)
    hi = math.pi / aug_rot_range
    cfg = (ctypes.c_double * 10)(*([1.0 if m in aug_methods else 0.0 for m in AUG_METHODS] + [float(p) for p in aug_prob] +
                                   [-hi, hi, 0.95, 1.05]))
    _cabi.check(fn(
        _p(raw), _p(offsets), B, total, int(max_points_per_frame), _p(calib), _p(img_hw), _scope(scope), int(npoints),
        int(seed) & 0xFFFFFFFF, _p(gt_boxes3d), _p(gt_alpha), _p(num_gt), G, _p(acc[0]), _p(acc[1]), _p(acc[2]), _p(acc[3]), _p(acc[4]), _p(acc[5]), K,
        _p(dbt[0]), _p(dbt[1]), _p(dbt[2]), D, db_max, cfg, _p(xyz), _p(pin), _p(feat), _p(src), _p(nvalid), _p(status), _p(out_gt),
        _p(out_ng), _p(aug), _p(ws), ws.numel(), _stream()), name)
    return {"pts_rect": xyz, "pts_input": pin if use_intensity else xyz, "pts_features": feat.unsqueeze(-1), "gt_boxes3d": out_gt,
            "num_gt": out_ng, "src": src, "nvalid": nvalid, "status": status, "aug": aug}


# ---------------------------------------------------------------------------------------------------------
# GT-augmentation database builder (csrc/gt_database.hip)
# ---------------------------------------------------------------------------------------------------------
def gt_database_build(raw, offsets, max_points_per_frame, calib, boxes3d, num_boxes):
    """raw (total,4) f32, offsets (B+1) i64, calib (B,24) f32 as scene_prepare; boxes3d (B,G,7) f32 + num_boxes (B) i32: the kept
    labels of every frame (G <= 128) -- all on the device.
    -> npts (B,G) i32, offsets (B*G+1) i64 (exclusive scan of npts: objects frame-major, then label order), points (P,3) rect
    coordinates, intensity (P), src (P) i32 raw index in the frame; each object's points in ascending raw index
    [tools/generate_gt_database.py:50-84 for a batch of frames; see prcnn_gt_database_count / prcnn_gt_database_fill].
    One host read (P) between the two passes."""
    B, total, dev = _frames(raw, offsets, calib)
    _chk(boxes3d, "boxes3d", ndim=3)
    _chk(num_boxes, "num_boxes", _INT, 1)
    G = boxes3d.shape[1]
    if tuple(boxes3d.shape) != (B, G, 7) or num_boxes.shape[0] != B:
        raise ValueError("gt_database_build: boxes3d must be (%d, G, 7), num_boxes (%d,)" % (B, B))
    L = _cabi.lib()
    mp = int(max_points_per_frame)
    ws = torch.empty((int(L.prcnn_gt_database_workspace_bytes(mp, B, G)),), dtype=torch.uint8, device=dev)
    npts = torch.empty((B, G), dtype=_INT, device=dev)
    _cabi.check(L.prcnn_gt_database_count(_p(raw), _p(offsets), B, total, mp, _p(calib), _p(boxes3d), _p(num_boxes), G, _p(npts), _p(ws),
                                          ws.numel(), _stream()), "prcnn_gt_database_count")
    off = torch.zeros((B * G + 1,), dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(npts.reshape(-1), 0, dtype=torch.int64)
    P = int(off[-1])                                    # the one host read: the outputs are sized by the data
    points = torch.empty((P, 3), dtype=_F32, device=dev)
    inten = torch.empty((P,), dtype=_F32, device=dev)
    src = torch.empty((P,), dtype=_INT, device=dev)
    _cabi.check(L.prcnn_gt_database_fill(_p(raw), _p(offsets), B, total, mp, _p(calib), _p(boxes3d), _p(num_boxes), G, _p(off), P, _p(points),
                                         _p(inten), _p(src), _p(ws), ws.numel(), _stream()), "prcnn_gt_database_fill")
    return npts, off, points, inten, src


# ---------------------------------------------------------------------------------------------------------
# Offline GT-augmented scenes, the train_aug split (csrc/aug_scene.hip)
# ---------------------------------------------------------------------------------------------------------
AUG_SCENE_MAX_ACCEPT = 15            # cnt <= extra_gt_num + 1 <= 15 (csrc/aug_scene_math.h)


def aug_scene_sample(gt_boxes3d, num_gt, planes, frame_ids, db_boxes, db_npts, area_scope, seed=0, max_accept=AUG_SCENE_MAX_ACCEPT):
    """The sampling loop of AugSceneGenerator.aug_one_scene (tools/generate_aug_scene.py:157-219) for a batch, one launch.
    gt_boxes3d (B,G,7) non-DontCare labels, num_gt (B) i32 or None, planes (B,4) f64, frame_ids (B) i32 the new sample ids
    ((epoch + 1) * 10000 + sample_id: the key of the random table), db_boxes (D,7), db_npts (D) i32, area_scope 6 floats.
    -> dict: count (B) i32, db_id (B,K) i32 (-1 past count), boxes3d (B,K,7) placed and unenlarged, y_shift (B,K) f64, stats (B,3) i32
    (extra_gt_num, cnt, tries spent), status (B) i32: 0 ok, 1 the reference raises, 2 a bound was exceeded (include/prcnn_pointops.h)"""
    _chk(gt_boxes3d, "gt_boxes3d", ndim=3); _chk(planes, "planes", torch.float64, 2); _chk(frame_ids, "frame_ids", _INT, 1)
    _chk(db_boxes, "db_boxes", ndim=2); _chk(db_npts, "db_npts", _INT, 1)
    B, G, C = gt_boxes3d.shape
    D, K = db_boxes.shape[0], int(max_accept)
    if C != 7 or tuple(planes.shape) != (B, 4) or frame_ids.shape[0] != B:
        raise ValueError("aug_scene_sample: gt_boxes3d must be (B, G, 7), planes (B, 4), frame_ids (B,)")
    if db_boxes.shape[1] != 7 or db_npts.shape[0] != D:
        raise ValueError("aug_scene_sample: db_boxes (D, 7) and db_npts (D,) disagree")
    if num_gt is not None:
        _chk(num_gt, "num_gt", _INT, 1)
        if num_gt.shape[0] != B:
            raise ValueError("aug_scene_sample: num_gt must be (%d,)" % B)
    dev = gt_boxes3d.device
    for name, t in (("num_gt", num_gt), ("planes", planes), ("frame_ids", frame_ids), ("db_boxes", db_boxes), ("db_npts", db_npts)):
        if t is not None and t.device != dev:
            raise RuntimeError("aug_scene_sample: %s is on %s, gt_boxes3d on %s" % (name, t.device, dev))
    if area_scope is None or len(area_scope) != 6:
        raise ValueError("aug_scene_sample: area_scope must be 6 floats [x0 x1 y0 y1 z0 z1]")
    out = {"count": torch.empty((B,), dtype=_INT, device=dev), "db_id": torch.empty((B, max(K, 0)), dtype=_INT, device=dev),
           "boxes3d": torch.empty((B, max(K, 0), 7), dtype=_F32, device=dev),
           "y_shift": torch.empty((B, max(K, 0)), dtype=torch.float64, device=dev),
           "stats": torch.empty((B, 3), dtype=_INT, device=dev), "status": torch.empty((B,), dtype=_INT, device=dev)}
    _cabi.check(_cabi.lib().prcnn_aug_scene_sample(
        _p(gt_boxes3d), _p(num_gt), _p(planes), _p(frame_ids), B, G, _p(db_boxes), _p(db_npts), D, ctypes.cast(_scope(area_scope), ctypes.c_void_p),
        K, int(seed) & 0xFFFFFFFF, _p(out["count"]), _p(out["db_id"]), _p(out["boxes3d"]), _p(out["y_shift"]), _p(out["stats"]),
        _p(out["status"]), _stream()), "prcnn_aug_scene_sample")
    return out


def aug_scene_build(raw, offsets, max_points_per_frame, calib, img_hw, scope, accepted, db_points, db_intensity, db_offsets, guard_rows=0):
    """The augmented clouds of AugSceneGenerator.aug_one_epoch_scene (tools/generate_aug_scene.py:240-248, :205-231) for a batch.
    raw .. scope as scene_prepare; accepted = aug_scene_sample's dict; db_points (P,3), db_intensity (P), db_offsets (D+1) i64.
    -> rows (B) i32, offsets (B+1) i64 (their exclusive scan), out (total,4) [x y z intensity], src (total) i32: per frame the valid
    points outside every accepted box (h + 2) in raw order (src = raw index), then the accepted objects' points with y - y_shift
    (src = -1 - database row).  One host read (the total) between the two passes.  guard_rows: extra rows allocated behind the
    output, which the fill must leave alone (tests)."""
    B, total, dev = _frames(raw, offsets, calib, img_hw)
    cnt, ids, boxes = _chk(accepted["count"], "count", _INT, 1), _chk(accepted["db_id"], "db_id", _INT, 2), _chk(accepted["boxes3d"], "boxes3d", ndim=3)
    shift, status = _chk(accepted["y_shift"], "y_shift", torch.float64, 2), _chk(accepted["status"], "status", _INT, 1)
    K = ids.shape[1]
    if cnt.shape[0] != B or ids.shape[0] != B or tuple(boxes.shape) != (B, K, 7) or tuple(shift.shape) != (B, K) or status.shape[0] != B:
        raise ValueError("aug_scene_build: the accepted objects must describe %d frames" % B)
    _chk(db_points, "db_points", ndim=2); _chk(db_intensity, "db_intensity", ndim=1)
    if db_offsets.dtype != torch.int64 or not db_offsets.is_contiguous() or db_offsets.device != dev or db_offsets.dim() != 1 or db_offsets.shape[0] < 1:
        raise ValueError("aug_scene_build: db_offsets must be a contiguous (D+1,) int64 tensor on the device of raw")
    if db_points.shape[1] != 3 or db_intensity.shape[0] != db_points.shape[0]:
        raise ValueError("aug_scene_build: db_points (P, 3) needs one intensity per point")
    D, PT = db_offsets.shape[0] - 1, db_points.shape[0]
    L = _cabi.lib()
    mp = int(max_points_per_frame)
    ws = torch.empty((int(L.prcnn_aug_scene_workspace_bytes(mp, B)),), dtype=torch.uint8, device=dev)
    rows = torch.empty((B,), dtype=_INT, device=dev)
    sc = _scope(scope)
    _cabi.check(L.prcnn_aug_scene_count(_p(raw), _p(offsets), B, total, mp, _p(calib), _p(img_hw), sc, _p(cnt), _p(ids), _p(boxes), _p(status), K,
                                        _p(db_offsets), D, PT, _p(rows), _p(ws), ws.numel(), _stream()), "prcnn_aug_scene_count")
    off = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(rows, 0, dtype=torch.int64)
    if B and int(rows.min()) < 0:                       # host read
        raise RuntimeError("aug_scene_build: a frame holds more rows than an int32 counts")
    n = int(off[-1])                                    # the outputs are sized by the data
    out = torch.empty((n + int(guard_rows), 4), dtype=_F32, device=dev)
    src = torch.empty((n + int(guard_rows),), dtype=_INT, device=dev)
    if guard_rows:
        out[n:] = -12345.0
        src[n:] = -12345
    _cabi.check(L.prcnn_aug_scene_fill(_p(raw), _p(offsets), B, total, mp, _p(calib), _p(img_hw), sc, _p(cnt), _p(ids), _p(boxes), _p(shift),
                                       _p(status), K, _p(db_points), _p(db_intensity), _p(db_offsets), D, PT, _p(off), n, _p(out), _p(src),
                                       _p(ws), ws.numel(), _stream()), "prcnn_aug_scene_fill")
    return rows, off, out, src


# ---------------------------------------------------------------------------------------------------------
# Evaluation statistics (csrc/eval_stats.hip)
# ---------------------------------------------------------------------------------------------------------
EVAL_STATS_MAX_GT = 128
EVAL_STATS_STATE_BYTES = 160             # PRCNN_EVAL_STATS_STATE_BYTES: int64 counters[16], double sums[4]
EVAL_TRIM = {"joint": 0, "rcnn": 0, "rpn": 1}


def eval_stats_workspace(S, B, G, device):
    """-> (gt_max (S,B,G) f32, num_gt (B) i32): views of one prcnn_eval_stats_workspace_bytes buffer"""
    ws = torch.empty((int(_cabi.lib().prcnn_eval_stats_workspace_bytes(S, B, G)),), dtype=torch.uint8, device=device)
    n = S * B * G * 4
    return ws[:n].view(_F32).view(S, B, G), ws[n:n + B * 4].view(_INT)


def eval_gt_max_iou(boxes, gt_boxes3d, trim_mode=0, out=None):
    """`boxes_iou3d_gpu(boxes[k], gt[k]).max(dim=0)` for every frame of one or two box sets in one launch [tools/eval_rcnn.py:190-191,
    :551-563].  boxes: a (B,M,7) tensor or a sequence of one or two of them (RoIs, decoded boxes); gt_boxes3d (B,G,>=7), zero rows at the
    end; trim_mode 0 (joint / rcnn: nothing may remain) or 1 (rpn: row 0 always stays); out: an eval_stats_workspace pair.
    -> gt_max (S,B,G), NaN where a column holds a NaN, -1 past num_gt; num_gt (B) i32"""
    sets = [boxes] if isinstance(boxes, torch.Tensor) else list(boxes)
    if len(sets) not in (1, 2):
        raise ValueError("eval_gt_max_iou: one or two box sets, got %d" % len(sets))
    for t in sets:
        _chk(t, "boxes", ndim=3)
    _chk(gt_boxes3d, "gt_boxes3d", ndim=3)
    B, M = sets[0].shape[:2]
    G, gc = gt_boxes3d.shape[1], gt_boxes3d.shape[2]
    if any(tuple(t.shape) != (B, M, 7) for t in sets) or gt_boxes3d.shape[0] != B:
        raise ValueError("eval_gt_max_iou: every box set must be (%d, %d, 7) and gt_boxes3d (%d, G, >= 7)" % (B, M, B))
    gt_max, num_gt = out if out is not None else eval_stats_workspace(len(sets), B, G, gt_boxes3d.device)
    _cabi.check(_cabi.lib().prcnn_eval_gt_max_iou(_p(sets[0]), _p(sets[1]) if len(sets) == 2 else None, len(sets), B, M, _p(gt_boxes3d), G, gc,
                                                  int(trim_mode), _p(gt_max), _p(num_gt), _stream()), "prcnn_eval_gt_max_iou")
    return gt_max, num_gt


def eval_stats_accumulate(state, gt_max, num_gt, B, det_num=None, seg=None, cls_label=None, seg_mode=0, pred_class=None, gt_iou=None,
                          cls_fg=0.6, cls_bg=0.45, refine_thresh=0.7):
    """add one batch into `state` (EVAL_STATS_STATE_BYTES uint8 on the device; see prcnn_eval_stats_accumulate): recall counts from
    gt_max (S,B,G) / num_gt (both None: no recall part), det_num (B) i32, the segmentation IoU from seg (B,N) f32 and cls_label (B,N)
    i32 | i64, the RCNN classification accuracy from pred_class (B,R) u8 and gt_iou (B,R).  One launch, one workgroup."""
    _chk(state, "state", torch.uint8, 1)
    if state.numel() < EVAL_STATS_STATE_BYTES:
        raise ValueError("eval_stats_accumulate: state holds %d bytes, %d are needed" % (state.numel(), EVAL_STATS_STATE_BYTES))
    S = G = N = R = 0
    if gt_max is not None:
        _chk(gt_max, "gt_max", ndim=3); _chk(num_gt, "num_gt", _INT, 1)
        S, G = gt_max.shape[0], gt_max.shape[2]
        if gt_max.shape[1] != B or num_gt.shape[0] != B:
            raise ValueError("eval_stats_accumulate: gt_max must be (S, %d, G) and num_gt (%d,)" % (B, B))
    if det_num is not None and tuple(_chk(det_num, "det_num", _INT, 1).shape) != (B,):
        raise ValueError("eval_stats_accumulate: det_num must be (%d,)" % B)
    is64 = 0
    if seg is not None:
        _chk(seg, "seg", ndim=2)
        N = seg.shape[1]
        if seg.shape[0] != B:
            raise ValueError("eval_stats_accumulate: seg must be (%d, N)" % B)
    if cls_label is not None:
        if not (cls_label.is_cuda and cls_label.dtype in (torch.int32, torch.int64) and cls_label.is_contiguous()):
            raise RuntimeError("eval_stats_accumulate: cls_label must be a contiguous int32 or int64 CUDA(HIP) tensor")
        is64 = int(cls_label.dtype == torch.int64)
        if seg is not None and tuple(cls_label.shape) != tuple(seg.shape):
            raise ValueError("eval_stats_accumulate: cls_label must be shaped as seg")
    if pred_class is not None:
        _chk(pred_class, "pred_class", torch.uint8, 2)
        R = pred_class.shape[1]
        if pred_class.shape[0] != B:
            raise ValueError("eval_stats_accumulate: pred_class must be (%d, R)" % B)
    if gt_iou is not None and pred_class is not None and tuple(_chk(gt_iou, "gt_iou", ndim=2).shape) != tuple(pred_class.shape):
        raise ValueError("eval_stats_accumulate: gt_iou must be shaped as pred_class")
    _cabi.check(_cabi.lib().prcnn_eval_stats_accumulate(_p(gt_max), _p(num_gt), S, B, G, _p(det_num), _p(seg), _p(cls_label), is64, N,
                                                        int(seg_mode), _p(pred_class), _p(gt_iou), R, float(cls_fg), float(cls_bg),
                                                        float(refine_thresh), _p(state), _stream()), "prcnn_eval_stats_accumulate")


# ------------------------------------------------------------------ adam_onecycle parameter update (csrc/optim.hip)
OPTIM_CHUNK = 4096                       # PRCNN_OPTIM_CHUNK: elements per chunk, one workgroup each
OPTIM_SCALARS = ("decay", "one_minus_beta1", "beta2", "one_minus_beta2", "bias2_sqrt", "eps", "neg_step")


def optim_chunk_rows(numels):
    """the chunk table of tensors with these element counts, as a list of (tensor, first element) rows: every element of every
    tensor exactly once, in order; a tensor without elements has no row"""
    return [(t, first) for t, n in enumerate(numels) for first in range(0, int(n), OPTIM_CHUNK)]


def _optim_tables(tensors, chunks):
    _chk(tensors, "tensors", torch.int64, 2); _chk(chunks, "chunks", torch.int64, 2)
    if tensors.shape[1] != 5 or chunks.shape[1] != 2:
        raise ValueError("optim: tensors must be (T, 5) [param, grad, exp_avg, exp_avg_sq, numel] and chunks (C, 2) [tensor, first], "
                         "got %s and %s" % (tuple(tensors.shape), tuple(chunks.shape)))
    if chunks.shape[0] and not tensors.shape[0]:
        raise ValueError("optim: %d chunks of an empty tensor table" % chunks.shape[0])
    return chunks.shape[0]


def optim_grad_norm(tensors, chunks, partial=None):
    """tensors (T,5) i64 and chunks (C,2) i64 on the device (prcnn_optim_tensor_t / prcnn_optim_chunk_t rows; the caller vouches for
    the addresses in them) -> partial (C) f64, the sum of grad^2 over every chunk.  One launch, nothing read back."""
    C = _optim_tables(tensors, chunks)
    if partial is None:
        partial = torch.empty((C,), dtype=torch.float64, device=tensors.device)
    elif tuple(_chk(partial, "partial", torch.float64, 1).shape) != (C,):
        raise ValueError("optim_grad_norm: partial must be (%d,)" % C)
    _cabi.check(_cabi.lib().prcnn_optim_grad_norm(_p(tensors), _p(chunks), C, _p(partial), _stream()), "prcnn_optim_grad_norm")
    return partial


def _optim_update(who, fn, names, tensors, chunks, scalars, partial, max_norm, coef, state):
    C = _optim_tables(tensors, chunks)
    if len(scalars) != len(names):
        raise ValueError("%s: scalars must be the %d values %s" % (who, len(names), ", ".join(names)))
    if coef is not None:
        if _chk(coef, "coef").numel() != 1:
            raise ValueError("%s: coef must hold one float" % who)
        state = None
    else:
        if partial is None or tuple(_chk(partial, "partial", torch.float64, 1).shape) != (C,):
            raise ValueError("%s: without coef, partial must be the (%d,) float64 result of optim_grad_norm" % (who, C))
        if state is None:
            state = torch.zeros((2,), dtype=_F32, device=tensors.device)
        elif _chk(state, "state", _F32, 1).numel() != 2:
            raise ValueError("%s: state must be (2,) float32" % who)
    _cabi.check(getattr(_cabi.lib(), fn)(_p(tensors), _p(chunks), C, _p(partial), float(max_norm), _p(coef), _p(state),
                                         *[float(s) for s in scalars], _stream()), fn)
    return state


def optim_step(tensors, chunks, scalars, partial=None, max_norm=1.0, coef=None, state=None):
    """clip coefficient + decay + Adam over every chunk in one launch.  scalars: the seven OPTIM_SCALARS (optim.adam_scalars).
    coef None: the coefficient is formed from `partial` (optim_grad_norm) and max_norm, and {norm, coef} go to state (2) f32;
    coef (1) f32 on the device: it is used as it is.  -> state (None with a caller's coef).  Nothing is read back."""
    return _optim_update("optim_step", "prcnn_optim_step", OPTIM_SCALARS, tensors, chunks, scalars, partial, max_norm, coef, state)


OPTIM_ADAM_SCALARS = ("weight_decay",) + OPTIM_SCALARS[1:]
OPTIM_SGD_SCALARS = ("weight_decay", "momentum", "neg_lr")


def optim_step_adam(tensors, chunks, scalars, partial=None, max_norm=1.0, coef=None, state=None):
    """torch.optim.Adam with L2 decay (TRAIN.OPTIMIZER adam; optim.ClipAdam) over every chunk in one launch: as optim_step, but
    scalars are the seven OPTIM_ADAM_SCALARS (weight_decay is added to the gradient, nothing is decayed) and a tensor without a
    gradient is not touched."""
    return _optim_update("optim_step_adam", "prcnn_optim_step_adam", OPTIM_ADAM_SCALARS, tensors, chunks, scalars, partial, max_norm,
                         coef, state)


def optim_step_sgd(tensors, chunks, scalars, partial=None, max_norm=1.0, coef=None, state=None):
    """torch.optim.SGD with momentum (TRAIN.OPTIMIZER sgd; optim.ClipSGD) over every chunk in one launch.  scalars: the three
    OPTIM_SGD_SCALARS.  The momentum buffer is column exp_avg of `tensors`; exp_avg_sq is not read, and with momentum 0 neither
    is.  A tensor without a gradient is not touched."""
    return _optim_update("optim_step_sgd", "prcnn_optim_step_sgd", OPTIM_SGD_SCALARS, tensors, chunks, scalars, partial, max_norm,
                         coef, state)


# ------------------------------------------------------------------ KITTI result text (csrc/kitti_text.hip)
KITTI_LINE_MAX = 256                     # PRCNN_KITTI_LINE_MAX: bytes reserved per candidate line
KITTI_FIELDS = 13


def kitti_result_text(boxes, scores, P2, img_hw, keep=None, num=None, class_name="Car", out=None, want_rows=False):
    """the result-file text of a batch [tools/eval_rcnn.py:69-94 save_kitti_format]: boxes (B,M,7), scores (B,M), P2 (B,12) f64,
    img_hw (B,2) i32 [H, W]; candidate j < num[b] is box keep[b,j] (keep None: box j; num None: all M).  out: (text, text_len, status)
    to write into.  -> text (B, M * KITTI_LINE_MAX) u8, text_len (B) i32, status (B) i32 [, rows (B,M,13) f64, valid (B,M) u8 with
    want_rows].  One launch, nothing read back."""
    _chk(boxes, "boxes", ndim=3); _chk(scores, "scores", ndim=2)
    B, M = boxes.shape[:2]
    if boxes.shape[2] != 7 or tuple(scores.shape) != (B, M):
        raise ValueError("kitti_result_text: boxes must be (B, M, 7) and scores (B, M), got %s and %s" % (tuple(boxes.shape), tuple(scores.shape)))
    if tuple(_chk(P2, "P2", torch.float64, 2).shape) != (B, 12) or tuple(_chk(img_hw, "img_hw", _INT, 2).shape) != (B, 2):
        raise ValueError("kitti_result_text: P2 must be (%d, 12) float64 and img_hw (%d, 2) int32" % (B, B))
    if keep is not None and tuple(_chk(keep, "keep", _INT, 2).shape) != (B, M):
        raise ValueError("kitti_result_text: keep must be (%d, %d)" % (B, M))
    if num is not None and tuple(_chk(num, "num", _INT, 1).shape) != (B,):
        raise ValueError("kitti_result_text: num must be (%d,)" % B)
    name = class_name.encode()
    dev = boxes.device
    if out is None:
        out = (torch.empty((B, M * KITTI_LINE_MAX), dtype=torch.uint8, device=dev), torch.zeros((B,), dtype=_INT, device=dev),
               torch.zeros((B,), dtype=_INT, device=dev))
    text, text_len, status = out
    if tuple(_chk(text, "text", torch.uint8, 2).shape) != (B, M * KITTI_LINE_MAX) or tuple(_chk(text_len, "text_len", _INT, 1).shape) != (B,) \
            or tuple(_chk(status, "status", _INT, 1).shape) != (B,):
        raise ValueError("kitti_result_text: out must be text (%d, %d) u8, text_len (%d,) and status (%d,) i32" % (B, M * KITTI_LINE_MAX, B, B))
    rows = valid = None
    if want_rows:
        rows = torch.zeros((B, M, KITTI_FIELDS), dtype=torch.float64, device=dev)
        valid = torch.zeros((B, M), dtype=torch.uint8, device=dev)
    _cabi.check(_cabi.lib().prcnn_kitti_result_text(_p(boxes), _p(scores), _p(keep), _p(num), B, M, _p(P2), _p(img_hw), name, _p(text),
                                                    _p(text_len), _p(status), _p(rows), _p(valid), _stream()), "prcnn_kitti_result_text")
    return (text, text_len, status, rows, valid) if want_rows else (text, text_len, status)


# ---- training heads: Dropout keyed by a counter + the output layer (csrc/head_tail.hip) ----------------------------------------
HEAD_TAIL_PART_ROWS = 512      # rows per partial tile of head_tail_backward (csrc/head_tail.hip HT_BWD_ROWS)


def head_tail_supported(R, K, N, p):
    """the domain of prcnn_head_tail_fwd / _bwd (include/prcnn_pointops.h); outside it the caller takes the composed path"""
    return R >= 1 and K % 32 == 0 and 32 <= K <= 256 and 1 <= N <= 96 and R * K <= 2 ** 32 and 0.0 <= p < 1.0


def _head_tail_key(key):
    seed, stream, call, p = key
    return int(seed) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF, float(p)


def head_tail_forward(x, w, b, key):
    """out (R, N) = drop(x) w^T + b, the mask a pure function of key = (seed, stream, call, p) and the entry's position
    (train_mlp.head_keep_mask).  x (R, K), w (N, K), b (N,) or None.  One launch."""
    _chk(x, "x", ndim=2); _chk(w, "w", ndim=2)
    R, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or (b is not None and tuple(_chk(b, "b", ndim=1).shape) != (N,)):
        raise ValueError("head_tail_forward: x (R, K), w (N, K), b (N,); got %s, %s, %s" % (tuple(x.shape), tuple(w.shape), None if b is None else tuple(b.shape)))
    seed, stream, call, p = _head_tail_key(key)
    out = torch.empty((R, N), dtype=_F32, device=x.device)
    _cabi.check(_cabi.lib().prcnn_head_tail_fwd(_p(x), _p(w), _p(b), _p(out), R, K, N, seed, stream, call, p, _stream()), "prcnn_head_tail_fwd")
    return out


def head_tail_backward(x, w, g, key, want_gx=True, want_gw=True, want_gb=True):
    """-> (gx (R, K), gw (N, K), gb (N,)), None where not wanted, from one pass over x and g plus a fixed-order reduce of the partial
    tiles.  g (R, N) is taken as it is when its rows are uniformly strided (a column slice of a wider buffer)."""
    _chk(x, "x", ndim=2); _chk(w, "w", ndim=2)
    R, K = x.shape
    N = w.shape[0]
    if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == _F32 and tuple(g.shape) == (R, N)) or w.shape[1] != K:
        raise ValueError("head_tail_backward: x (R, K), w (N, K) and a float32 device g (R, N) expected")
    if (N > 1 and g.stride(1) != 1) or (R > 1 and g.stride(0) < N):
        g = g.contiguous()
    ldg = g.stride(0) if R > 1 else N
    seed, stream, call, p = _head_tail_key(key)
    L = _cabi.lib()
    dev = x.device
    gx = torch.empty((R, K), dtype=_F32, device=dev) if want_gx else None
    gw = torch.empty((N, K), dtype=_F32, device=dev) if want_gw else None
    gb = torch.empty((N,), dtype=_F32, device=dev) if want_gb else None
    work, nbytes = None, 0
    if want_gw or want_gb:
        nbytes = L.prcnn_head_tail_work_bytes(R, K, N)
        work = torch.empty((max(nbytes, 4) // 4,), dtype=_F32, device=dev)
    _cabi.check(L.prcnn_head_tail_bwd(_p(x), _p(w), _p(g), ldg, _p(gx), _p(gw), _p(gb), _p(work), nbytes, R, K, N, seed, stream, call, p,
                                      _stream()), "prcnn_head_tail_bwd")
    return gx, gw, gb


def dropout_rows(x, key):
    """drop(x) on (R, K) rows with the mask of key = (seed, stream, call, p); its backward is the same call on the gradient"""
    _chk(x, "x", ndim=2)
    R, K = x.shape
    seed, stream, call, p = _head_tail_key(key)
    out = torch.empty_like(x)
    _cabi.check(_cabi.lib().prcnn_dropout_rows(_p(x), _p(out), R, K, seed, stream, call, p, _stream()), "prcnn_dropout_rows")
    return out
