"""The cases of the third split-bf16 opt-in of the training SharedMLP (train_mlp.TRAIN_SPLIT_ALL; csrc/mlp_train.h:
train_fwd_sa_kernel, train_dgrad_sa_kernel, train_pack_split_all_kernel), built with train_stack_cases.Case and shared by
tests/test_train_split_all_cpu.py (which kernel every layer gets, recorded on the CPU by tests/train_split_all_launch_record.cpp)
and tests/test_gpu_train_split_all.py (every case against float64).

Eligibility through prcnn_train_stack_fwd_split_all / _bwd_split_all, per layer (the host decides):
  forward, plain rows (every layer l > 0, layer 0 of a plain source)
        K % 32 == 0 (and K >= 32)                 train_fwd_s_kernel<WNB>, as under TRAIN_SPLIT
        else K >= 32 and K % 4 == 0               train_fwd_sa_kernel<0, WNB>
        else (K < 32, or K % 4 != 0: unaligned rows)      the fp32 kernel of the default path
  forward, layer 0 of a group / flat (mode 1) or interp (mode 2) source
        K >= 32                                   train_fwd_sa_kernel<mode, WNB>, any C; interp: WNB = 1 on the narrow grid always
        else                                      train_fwd_kernel<mode, WNB, false>
  dgrad of a layer with N outputs (its input takes a gradient), POOL 0 rows / 1 fixed groups / 2 padding-free groups (last layer)
        N % 32 == 0 (and N >= 32)                 train_dgrad_s_kernel<WNB, POOL>, as under TRAIN_SPLIT
        else N >= 32                              train_dgrad_sa_kernel<WNB, POOL>; POOL != 0: WNB = 1 on the narrow grid always
        else                                      train_dgrad_kernel<WNB, POOL>
The wide forms (WNB = 2) follow the fp32 kernels' rule: >= 4 column blocks and ceil(rows / 128) * ceil(blocks / 4) >= 192; a form
that is narrow "always" runs ceil(blocks / 2) workgroups per tile instead.  One train_pack_split_all_kernel launch per call builds
every split image the call uses (none when no layer of the call is split); the per-layer split packers are not launched.

`EXPECT[name]` = (forward kernels in layer order, {layer: dgrad kernel}, (packing launches of the forward call, of the backward
call)): written down from the rules above, confirmed by the recorder.  The shapes are the smallest that reach each variant; none
beyond the cap of tests/train_stack_cases.py."""
from train_split_cases import DF, DS, FF, FS
from train_stack_cases import Case


def FA(mode, wnb):
    return "train_fwd_sa_kernel<%d, %d>" % (mode, wnb)


def DA(wnb, pool):
    return "train_dgrad_sa_kernel<%d, %d>" % (wnb, pool)


GRP = dict(B=2, N=100, M=12, ns=8)
FLT = dict(B=2, N=150, M=12, ns=16)
CASES = [
    # ---- row edges of the 64-row statistics slab and the 128-row tile, over ragged K in {36, 100, 196} and N in {36, 68, 100, 196}
    Case("a_rows_1", "plain", [36, 36, 4], bn=False, R=1),                      # (one row: no BatchNorm, as plain_one_row_nobn)
    Case("a_rows_63", "plain", [100, 68, 28], R=63),                            # N = 28: its dgrad stays fp32
    Case("a_rows_64", "plain", [196, 100, 32], R=64),
    Case("a_rows_65", "plain", [36, 196, 36, 4], R=65),
    Case("a_rows_127", "plain", [100, 196, 32], R=127),
    Case("a_rows_128", "plain", [196, 36, 68, 100], R=128),
    Case("a_rows_129", "plain", [28, 36, 100, 196], R=129),                     # K = 28: its forward stays fp32
    # ---- mixed stack: layer 0 (K = 33: rows of 33 floats are not 16-byte pieces) stays fp32, the ragged layers after it are split
    Case("a_mixed", "plain", [33, 36, 68, 36], R=129),
    Case("a_nobn", "plain", [100, 36, 68], bn=False, R=300),
    # ---- grouped first layers, nsample-padded and pooled: K = C + 3, C = 58 is the unaligned one; K = 19 stays fp32
    Case("a_group_35", "group", [35, 36, 64], pool=True, **GRP),
    Case("a_group_61", "group", [61, 32, 36], pool=True, **GRP),                # ragged pooled dgrad (POOL 1)
    Case("a_group_99", "group", [99, 64, 100], pool=True, **GRP),
    Case("a_group_19", "group", [19, 36, 32], pool=True, **GRP),
    Case("a_no_x", "group", [35, 36, 36], pool=True, need_x=False, **GRP),      # no dgrad for layer 0
    Case("a_deep", "group", [515, 36], pool=True, B=1, N=100, M=13, ns=10),     # seventeen chunks of reduction at 130 rows
    # ---- the same on padding-free rows: weighted statistics, the live row count on the device
    Case("a_flat_35", "flat", [35, 36, 64], **FLT),
    Case("a_flat_61", "flat", [61, 32, 36], **FLT),                             # ragged pooled dgrad (POOL 2)
    Case("a_flat_99", "flat", [99, 64, 100], **FLT),
    Case("a_flat_19", "flat", [19, 36, 32], **FLT),
    # ---- interpolated first layers: C2 = 30 (a 4-group straddles known | skip) and C2 = 65
    Case("a_interp_37", "interp", [37, 36, 32], B=2, n=333, m=70, C1=7),
    Case("a_interp_72", "interp", [72, 100, 36], B=2, n=333, m=70, C1=7),
    # ---- wide forms: 50 tiles x 16 blocks (grouped), 48 x 16 (plain), and the forms that take the narrow grid at a wide shape
    Case("a_group_wide", "group", [35, 512, 64], pool=True, B=2, N=400, M=50, ns=64),
    Case("a_flat_wide", "flat", [35, 512, 64], B=2, N=400, M=50, ns=64),
    Case("a_wide_6017", "plain", [132, 512, 132], R=6017),                      # wide ragged forward, wide ragged dgrad
    Case("a_group_wide_rag", "group", [35, 512, 68], pool=True, B=2, N=400, M=50, ns=64),      # ragged pooled dgrad at a wide shape: narrow
    Case("a_interp_wide", "interp", [64, 512], B=2, n=3010, m=200, C1=16),      # interpolated forward at a wide shape: narrow
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

EXPECT = {
    "a_rows_1": ([FA(0, 1), FA(0, 1)], {1: DF(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_rows_63": ([FA(0, 1), FA(0, 1)], {1: DF(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_rows_64": ([FA(0, 1), FA(0, 1)], {1: DS(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_rows_65": ([FA(0, 1), FA(0, 1), FA(0, 1)], {2: DF(1, 0), 1: DA(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_rows_127": ([FA(0, 1), FA(0, 1)], {1: DS(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_rows_128": ([FA(0, 1), FA(0, 1), FA(0, 1)], {2: DA(1, 0), 1: DA(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_rows_129": ([FF(0, 1, True), FA(0, 1), FA(0, 1)], {2: DA(1, 0), 1: DA(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_mixed": ([FF(0, 1, False), FA(0, 1), FA(0, 1)], {2: DA(1, 0), 1: DA(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_nobn": ([FA(0, 1), FA(0, 1)], {1: DA(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_group_35": ([FA(1, 1), FA(0, 1)], {1: DS(1, 1), 0: DA(1, 0)}, (1, 1)),
    "a_group_61": ([FA(1, 1), FS(1)], {1: DA(1, 1), 0: DS(1, 0)}, (1, 1)),
    "a_group_99": ([FA(1, 1), FS(1)], {1: DA(1, 1), 0: DS(1, 0)}, (1, 1)),
    "a_group_19": ([FF(1, 1, False), FA(0, 1)], {1: DS(1, 1), 0: DA(1, 0)}, (1, 1)),
    "a_no_x": ([FA(1, 1), FA(0, 1)], {1: DA(1, 1)}, (1, 1)),
    "a_deep": ([FA(1, 1)], {0: DA(1, 1)}, (1, 1)),
    "a_flat_35": ([FA(1, 1), FA(0, 1)], {1: DS(1, 2), 0: DA(1, 0)}, (1, 1)),
    "a_flat_61": ([FA(1, 1), FS(1)], {1: DA(1, 2), 0: DS(1, 0)}, (1, 1)),
    "a_flat_99": ([FA(1, 1), FS(1)], {1: DA(1, 2), 0: DS(1, 0)}, (1, 1)),
    "a_flat_19": ([FF(1, 1, False), FA(0, 1)], {1: DS(1, 2), 0: DA(1, 0)}, (1, 1)),
    "a_interp_37": ([FA(2, 1), FA(0, 1)], {1: DS(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_interp_72": ([FA(2, 1), FA(0, 1)], {1: DA(1, 0), 0: DA(1, 0)}, (1, 1)),
    "a_group_wide": ([FA(1, 2), FS(1)], {1: DS(2, 1), 0: DS(1, 0)}, (1, 1)),
    "a_flat_wide": ([FA(1, 2), FS(1)], {1: DS(2, 2), 0: DS(1, 0)}, (1, 1)),
    "a_wide_6017": ([FA(0, 2), FS(1)], {1: DA(2, 0), 0: DS(1, 0)}, (1, 1)),
    "a_group_wide_rag": ([FA(1, 2), FS(1)], {1: DA(1, 1), 0: DS(1, 0)}, (1, 1)),
    "a_interp_wide": ([FA(2, 1)], {0: DS(1, 0)}, (1, 1)),
}
assert set(EXPECT) == set(BY_NAME)
# grid.y of the two forms that are narrow at a wide shape: ceil(blocks / 2), not ceil(blocks / 4)
NARROW_GRID_Y = {("a_group_wide_rag", "dgrad", 1): 8, ("a_interp_wide", "fwd", 0): 8}
# every new instantiation the host code can pick (the wide interpolated forward and the wide pooled ragged dgrads do not exist)
NEW_VARIANTS = {FA(0, 1), FA(0, 2), FA(1, 1), FA(1, 2), FA(2, 1), DA(1, 0), DA(2, 0), DA(1, 1), DA(1, 2)}
NEW_PACKER = "train_pack_split_all_kernel"
OLD_SPLIT_PACKERS = {"pack_weight_split_kernel", "train_pack_split_t_kernel"}
# run twice for bit-identical results: the wide grouped stack and its padding-free twin
REPEAT_CASES = ("a_group_wide", "a_flat_wide")


def recorder_args(case):
    """the case's words of `train_split_all_launch_record --case WG / --old-case VIA` (no native switches)"""
    return [case.source, str(case.rows), str(case.pool_ns), str(int(case.bn)), str(int(case.need_x))] + [str(c) for c in case.chans]
