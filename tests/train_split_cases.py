"""The cases of the opt-in split-bf16 training GEMMs (train_mlp.TRAIN_SPLIT; csrc/mlp_train.h: train_fwd_s_kernel,
train_dgrad_s_kernel), built with train_stack_cases.Case and shared by tests/test_train_split_cpu.py (which kernel every layer
gets, recorded on the CPU by tests/train_split_launch_record.cpp) and tests/test_gpu_train_split.py (every case against float64).

Eligibility, per layer (prcnn_train_stack_fwd_split / _bwd_split decide on the host):
  forward   the layer reads plain rows (every layer l > 0, layer 0 of a plain source) and its K % 32 == 0
  dgrad     the layer's N % 32 == 0 (and its input takes a gradient)
Everything else -- grouped / interpolated first layers, K or N off the multiple -- keeps the fp32 kernel of the default path.
The wide forms (WNB = 2) follow the fp32 kernels' rule: >= 4 column blocks and ceil(rows / 128) * ceil(blocks / 4) >= 192.

`EXPECT[name]` = (forward kernels in layer order, {layer: dgrad kernel}): written down from the rules above, confirmed by the
recorder.  The shapes are the smallest that reach each variant; none beyond the cap of tests/train_stack_cases.py."""
from train_stack_cases import Case


def FS(wnb):
    return "train_fwd_s_kernel<%d>" % wnb


def FF(mode, wnb, fast):
    return "train_fwd_kernel<%d, %d, %s>" % (mode, wnb, "true" if fast else "false")


def DS(wnb, pool):
    return "train_dgrad_s_kernel<%d, %d>" % (wnb, pool)


def DF(wnb, pool):
    return "train_dgrad_kernel<%d, %d>" % (wnb, pool)


CASES = [
    # ---- row edges of the 64-row statistics slab and the 128-row tile, over K in {32, 64, 96} and N in {4, 28, 32, 36, 68, 132}
    Case("s_rows_1", "plain", [32, 32, 4], bn=False, R=1),                      # (one row: no BatchNorm, as plain_one_row_nobn)
    Case("s_rows_63", "plain", [64, 32, 28], R=63),
    Case("s_rows_64", "plain", [96, 36, 32], R=64),
    Case("s_rows_65", "plain", [32, 68, 32, 4], R=65),
    Case("s_rows_127", "plain", [64, 132, 32], R=127),
    Case("s_rows_128", "plain", [96, 32, 32, 36], R=128),
    Case("s_rows_129", "plain", [32, 64, 96, 32], R=129),
    # ---- mixed stack: layer 0 (K = 33) forward and the dgrad of the N = 36 layer stay on fp32
    Case("s_mixed", "plain", [33, 32, 64, 36], R=129),
    Case("s_deep", "plain", [512, 32], R=130),                                  # sixteen chunks of reduction
    Case("s_nobn", "plain", [64, 32, 32], bn=False, R=300),
    Case("s_no_x", "plain", [32, 32, 32], R=100, need_x=False),                 # no dgrad for layer 0
    Case("s_group_pooled", "group", [16, 32, 64], pool=True, B=2, N=100, M=12, ns=8),          # POOL 1 stager
    Case("s_flat", "flat", [11, 32, 32, 64], B=2, N=150, M=12, ns=16),                         # POOL 2 stager, weighted statistics
    Case("s_interp", "interp", [37, 32, 32], B=2, n=333, m=70, C1=7),
    # ---- wide forms: 48 tiles x 16 blocks is the first wide launch at width 512, 47 tiles the last narrow one
    Case("s_wide_6017", "plain", [128, 512, 128], R=6017),
    Case("s_narrow_6016", "plain", [128, 512, 128], R=6016),
    Case("s_group_wide", "group", [16, 512, 64], pool=True, B=2, N=400, M=50, ns=64),          # wide pooled dgrad (POOL 1)
    Case("s_flat_wide", "flat", [16, 512, 64], B=2, N=400, M=50, ns=64),                       # ... and POOL 2
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

EXPECT = {
    "s_rows_1": ([FS(1), FS(1)], {1: DF(1, 0), 0: DS(1, 0)}),
    "s_rows_63": ([FS(1), FS(1)], {1: DF(1, 0), 0: DS(1, 0)}),
    "s_rows_64": ([FS(1), FF(0, 1, True)], {1: DS(1, 0), 0: DF(1, 0)}),
    "s_rows_65": ([FS(1), FF(0, 1, True), FS(1)], {2: DF(1, 0), 1: DS(1, 0), 0: DF(1, 0)}),
    "s_rows_127": ([FS(1), FF(0, 1, True)], {1: DS(1, 0), 0: DF(1, 0)}),
    "s_rows_128": ([FS(1), FS(1), FS(1)], {2: DF(1, 0), 1: DS(1, 0), 0: DS(1, 0)}),
    "s_rows_129": ([FS(1), FS(1), FS(1)], {2: DS(1, 0), 1: DS(1, 0), 0: DS(1, 0)}),
    "s_mixed": ([FF(0, 1, False), FS(1), FS(1)], {2: DF(1, 0), 1: DS(1, 0), 0: DS(1, 0)}),
    "s_deep": ([FS(1)], {0: DS(1, 0)}),
    "s_nobn": ([FS(1), FS(1)], {1: DS(1, 0), 0: DS(1, 0)}),
    "s_no_x": ([FS(1), FS(1)], {1: DS(1, 0)}),
    "s_group_pooled": ([FF(1, 1, False), FS(1)], {1: DS(1, 1), 0: DS(1, 0)}),
    "s_flat": ([FF(1, 1, False), FS(1), FS(1)], {2: DS(1, 2), 1: DS(1, 0), 0: DS(1, 0)}),
    "s_interp": ([FF(2, 1, False), FS(1)], {1: DS(1, 0), 0: DS(1, 0)}),
    "s_wide_6017": ([FS(2), FS(1)], {1: DS(2, 0), 0: DS(1, 0)}),
    "s_narrow_6016": ([FS(1), FS(1)], {1: DS(1, 0), 0: DS(1, 0)}),
    "s_group_wide": ([FF(1, 2, False), FS(1)], {1: DS(2, 1), 0: DS(1, 0)}),
    "s_flat_wide": ([FF(1, 2, False), FS(1)], {1: DS(2, 2), 0: DS(1, 0)}),
}
assert set(EXPECT) == set(BY_NAME)
# every split instantiation the host code can pick
SPLIT_VARIANTS = {FS(1), FS(2)} | {DS(w, p) for w in (1, 2) for p in (0, 1, 2)}
SPLIT_PACKERS = {"pack_weight_split_kernel", "train_pack_split_t_kernel"}
# run twice for bit-identical results: the wide plain stack and the padding-free stack
REPEAT_CASES = ("s_wide_6017", "s_flat")


def recorder_args(case):
    """arguments of `train_split_launch_record --case / --fp32-case` (no native switches)"""
    return [case.source, str(case.rows), str(case.pool_ns), str(int(case.bn)), str(int(case.need_x))] + [str(c) for c in case.chans]
