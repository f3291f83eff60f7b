"""The cases of the opt-in split-bf16 weight gradient of the wide training layers (train_mlp.TRAIN_SPLIT_WGRAD; csrc/mlp_train.h:
train_wgrad_s_kernel through prcnn_train_stack_bwd_wsplit), built with train_stack_cases.Case and shared by
tests/test_train_wsplit_cpu.py (which wgrad kernel every layer gets, recorded on the CPU by tests/train_wsplit_launch_record.cpp)
and tests/test_gpu_train_wsplit.py (every case against float64).

Eligibility, per layer (the host code decides): the layer gets train_wgrad_s_kernel exactly where the fp32 entry points launch
train_wgrad_lds_kernel -- K > 64 and N > 64 (wgrad_plan: WK == WN == 2), the layer's input rows 16-byte aligned with a stride that is
a multiple of 4, PRCNN_WGRAD_DIRECT not set.  Every narrower layer keeps its direct kernel train_wgrad_kernel<KQ, NQ, WK, WN>.
The template arguments <POOL, MULT, PRO> are the fp32 kernel's: POOL 0 = G per row, 1 = pooled over fixed groups (the last layer
of a pooled stack), 2 = over the groups of padding-free rows; MULT = padding-free rows; PRO = the layer reads the previous layer's
saved y (every layer l > 0).

The kernel stages 16 rows at a time and wgrad_plan deals the rows out in ranges of >= 512 rows rounded up to 32 (one range up to
512 rows, two of 288 at 513, three of 352 at 1025), so the row counts are the edges of a chunk (15, 16, 17, 31, 32, 33), one row,
and the edges of the range split (511, 512, 513, 1025); the widths are one tile with both tails masked (68, 68), the exact tile
(128, 128: the unguarded store), a second tile in either dimension (132, 68), (68, 132), and (96, 128), (128, 196).

`EXPECT[name]` = the wgrad kernel of every layer, in layer order: written down from the rules above, confirmed by the recorder."""
from train_stack_cases import Case


def WS(pool, mult, pro):
    return "train_wgrad_s_kernel<%d, %s, %s>" % (pool, "true" if mult else "false", "true" if pro else "false")


def WD(kq, nq, wk, wn):
    return "train_wgrad_kernel<%d, %d, %d, %d>" % (kq, nq, wk, wn)


CASES = [
    # ---- rows inside one range, over the widths
    Case("w_rows_1", "plain", [68, 68, 68], bn=False, R=1),                     # (one row: no BatchNorm, as plain_one_row_nobn)
    Case("w_rows_15", "plain", [128, 128], R=15),
    Case("w_rows_16", "plain", [132, 68, 132], R=16),
    Case("w_rows_17", "plain", [68, 132, 68], R=17),
    Case("w_rows_31", "plain", [96, 128, 196], R=31),
    Case("w_rows_32", "plain", [128, 128, 128], R=32),
    Case("w_rows_33", "plain", [68, 68], R=33),
    # ---- rows around the range split
    Case("w_rows_511", "plain", [96, 128], R=511),
    Case("w_rows_512", "plain", [128, 128], R=512),
    Case("w_rows_513", "plain", [68, 132, 196], R=513),
    Case("w_rows_1025", "plain", [132, 68, 128], R=1025),
    # ---- the pooled and padding-free forms, gathered first layers
    Case("w_group_first", "group", [70, 132], pool=True, B=2, N=120, M=10, ns=16),                # <1,false,false>: K = C + 3, rotated columns
    Case("w_group_pooled", "group", [16, 96, 128], pool=True, B=2, N=200, M=20, ns=16),          # <1,false,true>
    # (C = 16 feature columns: a multiple of 4, so the scatter of the row gradients takes its gather form and the input gradient is
    # repeatable too -- with C % 4 != 0 prcnn_flat_rows_grad_ws falls back to float atomics, whatever the wgrad arithmetic)
    Case("w_flat", "flat", [19, 96, 128, 160], B=2, N=200, M=20, ns=16),                          # <0,true,true>, <2,true,true>
    Case("w_flat_first", "flat", [99, 68, 32], B=2, N=150, M=12, ns=16),                          # <0,true,false>
    Case("w_flat_one_layer", "flat", [70, 132], B=2, N=120, M=10, ns=16),                         # <2,true,false>
    Case("w_interp", "interp", [96, 132, 68], B=2, n=333, m=70, C1=16),
    # ---- one mixed stack: narrow layers (direct wgrad kernels) around a wide one
    Case("w_mixed", "plain", [32, 128, 128, 32], R=600),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

EXPECT = {
    "w_rows_1": [WS(0, False, False), WS(0, False, True)],
    "w_rows_15": [WS(0, False, False)],
    "w_rows_16": [WS(0, False, False), WS(0, False, True)],
    "w_rows_17": [WS(0, False, False), WS(0, False, True)],
    "w_rows_31": [WS(0, False, False), WS(0, False, True)],
    "w_rows_32": [WS(0, False, False), WS(0, False, True)],
    "w_rows_33": [WS(0, False, False)],
    "w_rows_511": [WS(0, False, False)],
    "w_rows_512": [WS(0, False, False)],
    "w_rows_513": [WS(0, False, False), WS(0, False, True)],
    "w_rows_1025": [WS(0, False, False), WS(0, False, True)],
    "w_group_first": [WS(1, False, False)],
    "w_group_pooled": [WD(1, 2, 1, 2), WS(1, False, True)],
    "w_flat": [WD(1, 2, 1, 2), WS(0, True, True), WS(2, True, True)],
    "w_flat_first": [WS(0, True, False), WD(2, 1, 2, 1)],
    "w_flat_one_layer": [WS(2, True, False)],
    "w_interp": [WS(0, False, False), WS(0, False, True)],
    "w_mixed": [WD(1, 2, 1, 2), WS(0, False, True), WD(2, 1, 2, 1)],
}
assert set(EXPECT) == set(BY_NAME)
# every instantiation of the split wgrad kernel the host code can pick
WSPLIT_VARIANTS = {WS(0, False, False), WS(0, False, True), WS(0, True, False), WS(0, True, True),
                   WS(1, False, False), WS(1, False, True), WS(2, True, False), WS(2, True, True)}
# run twice for bit-identical results: a plain wide stack crossing two range boundaries, and the padding-free stack
REPEAT_CASES = ("w_rows_1025", "w_flat")
MIXED = "w_mixed"
MIXED_WIDE_LAYERS, MIXED_NARROW_LAYERS = (1,), (0, 2)


def recorder_args(case):
    """arguments of `train_wsplit_launch_record --case / --other-case` (no native switches)"""
    return [case.source, str(case.rows), str(case.pool_ns), str(int(case.bn)), str(int(case.need_x))] + [str(c) for c in case.chans]
