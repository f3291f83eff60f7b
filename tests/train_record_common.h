// What the stand-alone recorders of the training SharedMLP share (tests/train_launch_record.cpp, train_split_launch_record.cpp,
// train_wsplit_launch_record.cpp): mlp.hip -- and with it csrc/mlp_train.h -- included as host code with the launch macro recording
// (tests/launch_record_prelude.h), the record of a launch's arguments, the dummy descriptors of one stack and the five stack exports
// called on them.  The pointers are dummies, never dereferenced.
// TRAIN_SPLIT_RECORD_FP32_ONLY: builds against a source without the split entry points.
#pragma once
#include "launch_record_prelude.h"
#include <cxxabi.h>
#include <set>
#include <type_traits>

// ---- the record of a launch: head (prelude), then -- with g_fields set -- every argument: a parameter struct field by field (never
// its raw bytes: TrainBwd is not zero-initialised), a loose argument as a number.  The direct wgrad kernel's pooling form and operand
// prologue are run-time branches: its record always carries the tag " ~pool=<0 rows | 1 fixed groups | 2 padding-free groups> pro=<0|1>"
struct TrainFwd;
struct TrainBwd;
struct TrainWgrad;
struct TrainDgrad;
struct TrainDgradS;
static bool g_fields = false;
static unsigned long pv(const void* p) { return (unsigned long)reinterpret_cast<uintptr_t>(p); }
static void rec_arg(const TrainFwd& T);
static void rec_arg(const TrainBwd& T);
static void rec_arg(const TrainWgrad& W);
static void rec_arg(const TrainDgrad& D);
static void rec_arg(const TrainDgradS& S);
static void rec_tag(const TrainWgrad& W);
template <class T> static void rec_tag(const T&) {}
template <class T> static void rec_arg(const T& v) {
    if constexpr (std::is_pointer_v<T> || std::is_null_pointer_v<T>) recf(" %lx", pv(v));
    else if constexpr (std::is_floating_point_v<T>) recf(" %g", (double)v);
    else if constexpr (std::is_integral_v<T>) recf(" %lld", (long long)v);
    else recf(" ?");          // a struct of an export these recorders do not call
}
template <class A0, class... R> static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const A0& a0, const R&... rest) {
    rec_head(k, g, b, lds);
    if (g_fields) { rec_arg(a0); (rec_arg(rest), ...); }
    rec_tag(a0);
}

#ifndef MLP_SOURCE
#define MLP_SOURCE "mlp.hip"
#endif
#include MLP_SOURCE

static void rec_params(const MlpParams& P) {          // (as tests/mlp_launch_record.cpp prints it)
    recf(" P{rows %ld K %d KB %d NB %d wpack %lx bias %lx Nout %d relu %d out %lx ld_out %d col_off %d pool_ns %d in %lx ld_in %d", P.rows, P.K, P.KB, P.NB,
         pv(P.wpack), pv(P.bias), P.Nout, P.relu, pv(P.out), P.ld_out, P.col_off, P.pool_ns, pv(P.in), P.ld_in);
    recf(" xyz %lx new_xyz %lx idx %lx feat %lx ld_feat %d N %d M %d ns %d C %d", pv(P.xyz), pv(P.new_xyz), pv(P.idx), pv(P.feat), P.ld_feat, P.N, P.M, P.ns, P.C);
    recf(" known %lx idx3 %lx w3 %lx skip %lx ld_known %d ld_skip %d n %d m %d C2 %d C1 %d vec %d,%d", pv(P.known), pv(P.idx3), pv(P.w3), pv(P.skip), P.ld_known,
         P.ld_skip, P.n, P.m, P.C2, P.C1, P.vec_a, P.vec_b);
    recf(" act %d wx %lx ab %lx addY %lx ldY %d rows_dev %lx unit %d seg %lx,%d xcd_tpf %d wgm_cols %d addy_phase %d wsplit %lx terms %d}", P.act, pv(P.act_wx),
         pv(P.act_bias), pv(P.addY), P.ldY, pv(P.rows_dev), P.rows_unit, pv(P.seg_cnt), P.seg_rows, P.xcd_tpf, P.wgm_cols, P.addy_phase, pv(P.wsplit), P.split_terms);
}
static void rec_params(const ChainParams&) {}
static void rec_arg(const TrainFwd& T) {
    rec_params(T.P);
    recf(" F{pro %lx,%lx a_dump %lx ld_dump %d part %lx ld_part %d mult %lx slab_w %lx}", pv(T.pro_scale), pv(T.pro_shift), pv(T.a_dump), T.ld_dump, pv(T.part),
         T.ld_part, pv(T.mult), pv(T.slab_w));
}
static void rec_arg(const TrainBwd& T) {
    recf(" B{rows %ld N %d G %lx ldG %d arg %lx pool_ns %d y %lx ld_y %d cst %lx ld_c %d rows_dev %lx mult %lx row_grp %lx seg_off %lx}", T.rows, T.N, pv(T.G), T.ldG,
         pv(T.arg), T.pool_ns, pv(T.y), T.ld_y, pv(T.cst), T.ld_c, pv(T.rows_dev), pv(T.mult), pv(T.row_grp), pv(T.seg_off));
}
static void rec_arg(const TrainWgrad& W) {
    rec_arg(W.B);
    recf(" W{a %lx lda %d K %d pro %lx,%lx rows_per_split %ld part %lx}", pv(W.a), W.lda, W.K, pv(W.pro_scale), pv(W.pro_shift), W.rows_per_split, pv(W.part));
}
static void rec_tag(const TrainWgrad& W) { recf(" ~pool=%d pro=%d", W.B.pool_ns == 0 ? 0 : W.B.pool_ns > 0 ? 1 : 2, W.pro_scale ? 1 : 0); }
static void rec_arg(const TrainDgrad& D) {
    rec_arg(D.B);
    recf(" D{wpack %lx KB %d NB %d Kin %d out %lx ld_out %d}", pv(D.wpack), D.KB, D.NB, D.Kin, pv(D.out), D.ld_out);
}
#ifndef TRAIN_SPLIT_RECORD_FP32_ONLY
static void rec_arg(const TrainDgradS& S) {
    rec_arg(S.D);
    recf(" S{wsplit %lx}", pv(S.wsplit));
}
#endif

// dummy pointers: A(i) 16-byte aligned
template <class T = float> static T* A(int i) { return reinterpret_cast<T*>((uintptr_t)0x100000 * (i + 1)); }

// "KName<&train_wgrad_kernel<1, 1, 1, 1>(TrainWgrad)>" or "KName<&(void train_x<...>(T))>" -> "train_wgrad_kernel<1, 1, 1, 1>"
static std::string pretty(const std::string& mangled) {
    int st = 0;
    char* d = abi::__cxa_demangle(mangled.c_str(), nullptr, nullptr, &st);
    std::string s = (st == 0 && d) ? d : mangled;
    free(d);
    const size_t amp = s.find('&');
    const size_t par = s.rfind('(');
    if (amp == std::string::npos || par == std::string::npos || par <= amp) return s;
    s = s.substr(amp + 1, par - amp - 1);
    if (s.compare(0, 1, "(") == 0) s.erase(0, 1);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    return s;
}

struct Launch { std::string name, shape, tag; };          // kernel instantiation, "grid x,y,z block x,y,z", the wgrad tag (or nothing)
static int g_failed = 0;
static bool starts(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

// the launches of the call in flight, in order
static std::vector<Launch> harvest(int rc) {
    std::vector<Launch> out;
    if (rc != PRCNN_OK) { g_failed++; fprintf(stderr, "call failed (%d):%s\n", rc, g_rec.c_str()); }
    size_t p = 0;
    while ((p = g_rec.find(" | ", p)) != std::string::npos) {
        p += 3;
        const size_t e = g_rec.find(" grid ", p);
        if (e == std::string::npos) break;
        size_t end = g_rec.find(" lds ", e), nxt = g_rec.find(" | ", e);
        if (nxt == std::string::npos) nxt = g_rec.size();
        if (end == std::string::npos) end = nxt;
        const size_t tag = g_rec.find(" ~", e);
        out.push_back({pretty(g_rec.substr(p, e - p)), g_rec.substr(e + 1, end - e - 1), tag < nxt ? g_rec.substr(tag + 2, nxt - tag - 2) : std::string()});
    }
    g_rec.clear();
    g_launches = 0;
    return out;
}

struct Case { int source; long rows; int pool_ns, bn, need_x, nl; int chans[9]; };          // source: 0 plain, 1 group, 2 interp, 3 flat
static int source_of(const std::string& s) { return s == "plain" ? 0 : s == "group" ? 1 : s == "interp" ? 2 : s == "flat" ? 3 : -1; }

// one stack as pointrcnn_amd/train_mlp.py would call it: the source, the layers, a split image for every layer's forward (ws) and
// dgrad (wst), and the loose arguments of the exports
struct Stack {
    prcnn_train_src_t S;
    prcnn_train_layer_t L[8];
    void *ws[8], *wst[8], *work;
    size_t work_bytes;
    int nl, ns, ldd, ld_out, col_off, ld_gout, ld_gin;
    float *dump, *out, *gout, *gin;
    uint8_t* arg;
};
static void build_stack(const Case& c, Stack& s) {
    s = Stack();
    prcnn_train_src_t& S = s.S;
    const int K0 = c.chans[0];
    S.rows = c.rows; S.K = K0;
    const int ns = c.pool_ns > 1 ? c.pool_ns : 1;
    if (c.source == 0) {
        S.mode = MODE_PLAIN; S.in = A(0); S.ld_in = (K0 + 3) / 4 * 4;
    } else if (c.source == 1) {
        S.mode = MODE_GROUP; S.xyz = A(1); S.new_xyz = A(2); S.idx = A<int32_t>(3); S.feat = K0 > 3 ? A(4) : nullptr; S.ld_feat = (K0 - 3 + 3) / 4 * 4;
        S.B = 1; S.N = 4096; S.M = (int)(c.rows / ns); S.ns = ns; S.C = K0 - 3;
    } else if (c.source == 3) {
        S.mode = MODE_GROUP; S.xyz = A(1); S.new_xyz = A(2); S.idx = A<int32_t>(3); S.feat = K0 > 3 ? A(4) : nullptr; S.ld_feat = (K0 - 3 + 3) / 4 * 4;
        S.B = 1; S.N = 4096; S.M = (int)c.rows; S.ns = 1; S.C = K0 - 3;
        S.mult = A(5); S.rows_dev = A<int32_t>(6); S.norm_rows = c.rows; S.seg_off = A<int32_t>(7); S.seg_cnt = A<int32_t>(8); S.row_grp = A<int32_t>(9);
        S.groups = (int)(c.rows / ns);
    } else {
        S.mode = MODE_INTERP; S.known = A(1); S.idx3 = A<int32_t>(2); S.w3 = A(3);
        S.C1 = K0 > 4 ? K0 / 4 : 0; S.C2 = K0 - S.C1;
        S.skip = S.C1 ? A(4) : nullptr; S.ld_known = (S.C2 + 3) / 4 * 4; S.ld_skip = (S.C1 + 3) / 4 * 4;
        S.B = 1; S.n = (int)c.rows; S.m = 64;
    }
    const int kin0 = (c.source == 1 || c.source == 3) ? K0 - 3 : K0;
    const bool need_x = c.need_x && kin0 > 0;
    prcnn_train_layer_t* L = s.L;
    for (int l = 0; l < c.nl; l++) {
        L[l].Nout = c.chans[l + 1];
        L[l].W = A(20 + l); L[l].y = A(30 + l); L[l].cst = A(40 + l); L[l].ld_c = (L[l].Nout + 127) / 128 * 128; L[l].wpack = A(50 + l);
        L[l].wpack_t = (l > 0 || need_x) ? A(60 + l) : nullptr;
        L[l].dW = A(70 + l);
        if (c.bn) { L[l].gamma = A(80 + l); L[l].beta = A(90 + l); L[l].dgamma = A(100 + l); L[l].dbeta = A(110 + l); L[l].running_mean = A(120 + l); L[l].running_var = A(130 + l); }
        else if (l % 2 == 0) { L[l].beta = A(90 + l); L[l].dbeta = A(110 + l); }          // Conv with bias / without, alternating
        L[l].eps = 1e-5f; L[l].momentum = 0.1f;
        s.ws[l] = A<void>(140 + l); s.wst[l] = A<void>(150 + l);
    }
    const bool gathered = c.source != 0;
    s.nl = c.nl; s.ns = ns; s.work = A<void>(200); s.work_bytes = (size_t)1 << 62;
    s.dump = gathered ? A(10) : nullptr; s.ldd = gathered ? (K0 + 3) / 4 * 4 : 0;
    s.arg = (ns > 1 || c.source == 3) ? A<uint8_t>(12) : nullptr;
    s.out = A(11); s.gout = A(13); s.ld_out = s.ld_gout = c.chans[c.nl];
    s.gin = need_x ? A(14) : nullptr; s.ld_gin = need_x ? (kin0 + 3) / 4 * 4 : 0;
}

// via: the pair of entry points.  VIA_FP32 prcnn_train_stack_fwd + _bwd, VIA_SPLIT _fwd_split + _bwd_split, VIA_WSPLIT _fwd_split + _bwd_wsplit
enum Via { VIA_FP32 = 0, VIA_SPLIT = 1, VIA_WSPLIT = 2 };
static int call_fwd(const Stack& s, int via) {
#ifndef TRAIN_SPLIT_RECORD_FP32_ONLY
    if (via != VIA_FP32) return prcnn_train_stack_fwd_split(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.out, s.ld_out, s.col_off, s.arg, s.ws, s.work, s.work_bytes, nullptr);
#endif
    return prcnn_train_stack_fwd(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.out, s.ld_out, s.col_off, s.arg, s.work, s.work_bytes, nullptr);
}
static int call_bwd(const Stack& s, int via) {
#ifndef TRAIN_SPLIT_RECORD_FP32_ONLY
    if (via == VIA_SPLIT) return prcnn_train_stack_bwd_split(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, s.wst, s.work, s.work_bytes, nullptr);
    if (via == VIA_WSPLIT) return prcnn_train_stack_bwd_wsplit(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, s.wst, s.work, s.work_bytes, nullptr);
#endif
    return prcnn_train_stack_bwd(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, s.work, s.work_bytes, nullptr);
}
// forward, then (no backward without a forward) backward: the launches of each
static void run_stack(const Case& c, int via, std::vector<Launch>& fwd, std::vector<Launch>& bwd) {
    Stack s;
    build_stack(c, s);
    const int rc = call_fwd(s, via);
    fwd = harvest(rc);
    bwd.clear();
    if (rc == PRCNN_OK) bwd = harvest(call_bwd(s, via));
}

// the case of a command line: SOURCE ROWS POOL_NS BN NEED_X, `skip` further words, K0 N1 [N2 ...]; false: not a case
static bool parse_case(int argc, char** argv, int at, int skip, Case& c) {
    c = Case();
    c.source = source_of(argv[at]);
    if (c.source < 0) { fprintf(stderr, "unknown source %s\n", argv[at]); return false; }
    c.rows = atol(argv[at + 1]); c.pool_ns = atoi(argv[at + 2]); c.bn = atoi(argv[at + 3]); c.need_x = atoi(argv[at + 4]);
    c.nl = argc - (at + 6 + skip);
    if (c.nl > 8) { fprintf(stderr, "at most 8 layers\n"); return false; }
    for (int i = 0; i <= c.nl; i++) c.chans[i] = atoi(argv[at + 5 + skip + i]);
    return true;
}
