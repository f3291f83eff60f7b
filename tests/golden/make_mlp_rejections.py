"""Records tests/golden/mlp_rejections.json: invalid calls of every MLP export with the return code and prcnn_last_error() text a
given build of the library answers them with.  Every call fails its checks before anything is launched; the pointers are dummies.

    python tests/golden/make_mlp_rejections.py /path/to/libprcnn_pointops.so

The fixture was recorded from the library as it stood before the MLP host front-end moved to csrc/mlp_host.h."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P2 = lambda *p: {"ptrs": list(p)}          # noqa: E731
I2 = lambda *i: {"ints": list(i)}          # noqa: E731

LAYER_OUT = [("wpack", "A10"), ("bias", None), ("Nout", 64), ("relu", 1), ("out", "A11"), ("ld_out", 64), ("col_off", 0)]
CHAIN_OUT = [("nlayers", 2), ("wpack", P2("A10", "A12")), ("bias", P2("A13", None)), ("nout", I2(128, 128)), ("relu", I2(1, 1)), ("out", "A11"),
             ("ld_out", 128), ("col_off", 0)]
GROUP_IN = [("xyz", "A0"), ("new_xyz", "A1"), ("idx", "A2"), ("feat_cl", "A3"), ("ld_feat", 32), ("B", 2), ("N", 1024), ("M", 64), ("nsample", 16),
            ("C", 32), ("act_wx", None), ("act_bias", None)]
INTERP_IN = [("known_cl", "A0"), ("ld_known", 64), ("idx3", "A1"), ("w3", "A2"), ("skip_cl", "A3"), ("ld_skip", 32), ("B", 2), ("n", 128), ("m", 64),
             ("C2", 64), ("C1", 32), ("act_bias", None)]
ROWS_TAIL = [("pool_ns", 0), ("rows_dev", None), ("rows_unit", 1), ("seg_cnt", None), ("seg_rows", 0), ("stream", None)]
ADDY = [("y_cl", "A4"), ("ld_y", 64), ("idx3", "A5"), ("w3", "A6"), ("B", 2), ("n", 128), ("m", 64)]
SPLIT = [("wsplit", "A14"), ("terms", 6)]


def _split_after_wpack(sig):
    i = [n for n, _ in sig].index("wpack") + 1
    return sig[:i] + SPLIT + sig[i:]


SIGS = {
    "prcnn_mlp_rows": [("in", "A0"), ("ld_in", 32), ("rows", 256), ("K", 32)] + LAYER_OUT + ROWS_TAIL,
    "prcnn_mlp_rows_addinterp": [("in", "A0"), ("ld_in", 32), ("K", 32)] + LAYER_OUT[:4] + ADDY + LAYER_OUT[4:] + [("stream", None)],
    "prcnn_mlp_group": GROUP_IN + LAYER_OUT + [("pool_ns", 16), ("groups_dev", None), ("stream", None)],
    "prcnn_mlp_interp": INTERP_IN + LAYER_OUT + [("stream", None)],
    "prcnn_mlp_chain_rows": [("in", "A0"), ("ld_in", 128), ("rows", 256), ("K", 128)] + CHAIN_OUT + [("pool_ns", 0), ("seg_cnt", None), ("seg_rows", 0),
                                                                                                    ("stream", None)],
    "prcnn_mlp_chain_group": GROUP_IN + CHAIN_OUT + [("pool_ns", 16), ("groups_dev", None), ("stream", None)],
    "prcnn_mlp_chain_interp": INTERP_IN + CHAIN_OUT + [("stream", None)],
    "prcnn_mlp_chain_rows_split": [("in", "A0"), ("ld_in", 128), ("rows", 256), ("K", 128), ("wchain", P2("A14", "A15")), ("wpack", P2("A10", "A12")),
                                   ("bias", P2("A13", None)), ("nout", I2(128, 128)), ("relu", I2(1, 0)), ("terms", 6), ("out", "A11"), ("ld_out", 128),
                                   ("col_off", 0), ("stream", None)],
    "prcnn_mlp_chain_interp_split": [("known_cl", "A0"), ("ld_known", 128), ("idx3", "A1"), ("w3", "A2"), ("B", 8), ("n", 128), ("m", 64), ("C2", 128),
                                     ("act_bias", "A3"), ("wchain", "A14"), ("wpack", "A10"), ("bias", None), ("Nout", 128), ("relu", 1), ("terms", 6),
                                     ("out", "A11"), ("ld_out", 128), ("col_off", 0), ("stream", None)],
}
for twin in ("prcnn_mlp_rows", "prcnn_mlp_rows_addinterp", "prcnn_mlp_group"):
    SIGS[twin + "_split"] = _split_after_wpack(SIGS[twin])

LAYER_COMMON = [("null weight image", {"wpack": None}), ("null output", {"out": None}), ("unaligned weight image", {"wpack": "U10"}),
                ("ld_out too small", {"ld_out": 32}), ("no output channels", {"Nout": 0, "ld_out": 64})]
ROWS = [("null input", {"in": None}), ("bad strides", {"ld_in": 16}), ("pool_ns=20", {"pool_ns": 20}), ("rows not a multiple of pool_ns", {"rows": 100, "pool_ns": 16}),
        ("seg_rows not a multiple of 128", {"seg_cnt": "A7", "seg_rows": 100}), ("segments with pooling", {"seg_cnt": "A7", "seg_rows": 128, "pool_ns": 16}),
        ("segments with a device row count", {"seg_cnt": "A7", "seg_rows": 128, "rows_dev": "A8"}), ("negative rows", {"rows": -128}),
        ("doubly invalid: null input and pool_ns=20", {"in": None, "pool_ns": 20}), ("doubly invalid: bad strides and bad segments", {"ld_in": 16, "seg_cnt": "A7", "seg_rows": 100}),
        ("doubly invalid: bad segments and pool_ns=20", {"seg_cnt": "A7", "seg_rows": 100, "pool_ns": 20})]
UNALIGNED_SPLIT = [("unaligned split image", {"wsplit": "U14"})]          # (not for the grouped export: without the hoisted form it takes the fp32 kernel)
SPLIT_COMMON = [("null split image", {"wsplit": None}), ("terms=4", {"terms": 4}),
                ("doubly invalid: terms=4 and ld_out too small", {"terms": 4, "ld_out": 32})]
ADDINTERP = [("null addend", {"y_cl": None}), ("no points", {"n": 0}), ("ld_y too small", {"ld_y": 32}), ("doubly invalid: null indices and no points", {"idx3": None, "n": 0})]
GROUP = [("null xyz", {"xyz": None}), ("features missing", {"feat_cl": None}), ("ld_feat too small", {"ld_feat": 16}), ("act_wx without act_bias", {"act_wx": "A7"}),
         ("hoisted form with C % 4 != 0", {"C": 30, "act_wx": "A7", "act_bias": "A8"}), ("unaligned act_bias", {"act_wx": "A7", "act_bias": "U8"}),
         ("doubly invalid: null idx and ld_out too small", {"idx": None, "ld_out": 8})]
INTERP = [("null known", {"known_cl": None}), ("skip features missing", {"skip_cl": None}), ("ld_known too small", {"ld_known": 32}),
          ("hoisted form with skip features", {"act_bias": "A7"}), ("hoisted form, unaligned act_bias", {"act_bias": "U7", "skip_cl": None, "C1": 0, "ld_skip": 0}),
          ("hoisted form with C2 % 4 != 0", {"act_bias": "A7", "skip_cl": None, "C1": 0, "ld_skip": 0, "C2": 62}),
          ("doubly invalid: null weights and ld_out too small", {"w3": None, "ld_out": 8})]
CHAIN_COMMON = [("nlayers=4", {"nlayers": 4}), ("null layer arrays", {"wpack": None}), ("layer 1 weight image missing", {"wpack": P2("A10", None)}),
                ("unaligned bias", {"bias": P2("U13", None)}), ("layer too wide", {"nout": I2(128, 600), "ld_out": 600}), ("ld_out too small", {"ld_out": 64}),
                ("no instance for the widths", {"nout": I2(128, 64), "ld_out": 64})]

CASES = {
    "prcnn_mlp_rows": ROWS + LAYER_COMMON + [("pool_ns=20 and no weights", {"pool_ns": 20, "wpack": None})],
    "prcnn_mlp_rows_split": ROWS + LAYER_COMMON + SPLIT_COMMON + UNALIGNED_SPLIT,
    "prcnn_mlp_rows_addinterp": ADDINTERP + LAYER_COMMON,
    "prcnn_mlp_rows_addinterp_split": ADDINTERP + SPLIT_COMMON + UNALIGNED_SPLIT + [("null weight image", {"wpack": None})],
    "prcnn_mlp_group": GROUP + LAYER_COMMON + [("pool_ns=20", {"pool_ns": 20, "nsample": 20}),
                                               ("doubly invalid: pool_ns=20 and act_wx alone", {"pool_ns": 20, "act_wx": "A7"})],
    "prcnn_mlp_group_split": GROUP + SPLIT_COMMON + [("no features", {"C": 0, "feat_cl": None}), ("pool_ns=20", {"pool_ns": 20, "nsample": 20})],
    "prcnn_mlp_interp": INTERP + LAYER_COMMON,
    "prcnn_mlp_chain_rows": CHAIN_COMMON + [("null input", {"in": None}), ("pool_ns=20", {"pool_ns": 20}), ("pool_ns=64", {"pool_ns": 64}),
                                            ("seg_rows not a multiple of 128", {"seg_cnt": "A7", "seg_rows": 100}),
                                            ("rows not a multiple of pool_ns", {"rows": 100, "pool_ns": 16}),
                                            ("doubly invalid: null input and nlayers=4", {"in": None, "nlayers": 4}),
                                            ("doubly invalid: nlayers=4 and pool_ns=20", {"nlayers": 4, "pool_ns": 20})],
    "prcnn_mlp_chain_group": CHAIN_COMMON + [("null xyz", {"xyz": None}), ("ld_feat too small", {"ld_feat": 16}), ("pool_ns != nsample", {"pool_ns": 32}),
                                             ("act_wx without act_bias", {"act_wx": "A7"}), ("hoisted form with C % 4 != 0", {"C": 30, "act_wx": "A7", "act_bias": "A8"}),
                                             ("doubly invalid: pool_ns != nsample and act_wx alone", {"pool_ns": 32, "act_wx": "A7"})],
    "prcnn_mlp_chain_interp": CHAIN_COMMON + [("null known", {"known_cl": None}), ("no known channels", {"C2": 0}), ("hoisted form with skip features", {"act_bias": "A7"}),
                                              ("doubly invalid: nlayers=4 and hoisted form with skip features", {"nlayers": 4, "act_bias": "A7"})],
    "prcnn_mlp_chain_rows_split": [("null input", {"in": None}), ("terms=4", {"terms": 4}), ("layer 1 fp32 image missing", {"wpack": P2("A10", None)}),
                                   ("unsupported K", {"K": 96}), ("unaligned input", {"in": "U0"}), ("ld_out too small", {"ld_out": 64}),
                                   ("doubly invalid: terms=4 and layer 1 fp32 image missing", {"terms": 4, "wpack": P2("A10", None)}),
                                   ("unsupported K and ld_out too small", {"K": 96, "ld_out": 64})],
    "prcnn_mlp_chain_interp_split": [("null act_bias", {"act_bias": None}), ("unaligned fp32 image", {"wpack": "U10"}), ("terms=4", {"terms": 4}), ("no points", {"n": 0}),
                                     ("ld_out too small", {"ld_out": 64}), ("unsupported C2", {"C2": 64}), ("unaligned known", {"known_cl": "U0"}),
                                     ("doubly invalid: terms=4 and no points", {"terms": 4, "n": 0})],
}


def main(path):
    os.environ["PRCNN_POINTOPS_LIB"] = path
    from pointrcnn_amd import _cabi
    from test_mlp_host_cpu import _arg
    lib = _cabi.lib()
    out = []
    for export, cases in CASES.items():
        for what, change in cases:
            names = [n for n, _ in SIGS[export]]
            assert set(change) <= set(names), (export, what)
            args = [change.get(n, v) for n, v in SIGS[export]]
            keep = [_arg(a) for a in args]
            rc = getattr(lib, export)(*keep)
            assert rc in (-1, -3), (export, what, rc)
            out.append({"export": export, "what": what, "args": args, "rc": rc, "message": lib.prcnn_last_error().decode() if rc == -1 else ""})
    with open(os.path.join(ROOT, "tests", "golden", "mlp_rejections.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in out) + "\n]\n")
    print(len(out), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
