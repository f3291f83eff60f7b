/*
 * prcnn_pointops.h -- C ABI of libprcnn_pointops.so, the MI355X (gfx950) implementation of
 * PointRCNN's point-ops hot path (PointNet++ set-abstraction / feature-propagation operators,
 * roipool3d, iou3d).
 *
 * This is the drop-in boundary: what the reference binds through its three pybind modules
 * (`pointnet2_cuda` [un-vendored submodule, .gitmodules:1-4], `iou3d_cuda`
 * lib/utils/iou3d/src/iou3d.cpp:174-179, `roipool3d_cuda` lib/utils/roipool3d/src/roipool3d.cpp:198-203)
 * is exactly this set of entry points.  INTEGRATION.md shows the ctypes binding
 * (pointrcnn_amd/_cabi.py is that binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in `_host` or the FUNCTION is named
 *     prcnn_host_* (host pointers only, no HIP call inside: safe in forked dataloader workers);
 *   - tensors are dense row-major fp32 / int32 / int64 exactly as the reference op surface lays
 *     them out; the caller allocates every output (reference: iou3d_utils.py:14,32,68;
 *     roipool3d_utils.py:21-23); callees keep no reference to any buffer after return;
 *   - `stream` is a hipStream_t (NULL = the null stream).  All work is enqueued on it and the call
 *     returns without synchronising (the reference launches on the legacy default stream and
 *     nms_* blocks on a D2H copy: iou3d.cpp:93-94 -- the sync lives in the Python shim only);
 *   - return value: 0 on success, <0 on error (never exit(): contrast iou3d.cpp:13-21);
 *     prcnn_last_error() returns a thread-local message for the last failing call;
 *   - every entry point is re-entrant and may be called concurrently from several host threads, each on its own
 *     device (the reference's nn.DataParallel convention).  The only process-wide state is a per-(kernel, device)
 *     "dynamic-LDS limit already raised" bit, updated atomically (csrc/common.h PrcnnLdsLimit), and the snapshot of the
 *     environment switches, published through one atomic pointer (csrc/switches.h).
 *
 * Arithmetic contract (shared bit-for-bit with oracle/prcnn_oracle.c):
 *   - squared distances are ((dx*dx + dy*dy) + dz*dz) with individually rounded fp32 operations (no FMA; the library is built
 *     with -ffp-contract=off);
 *   - box trigonometry of roipool3d / pts_in_boxes3d / labels / GT-aug / overlap / IoU / NMS / proposal NMS / RoI sampling is the
 *     REFERENCE'S HOST ARITHMETIC (oracle trig_mode 2): glibc 2.35's float sinf / cosf / atan2f restated operation by operation
 *     (csrc/ref_trig.h; prcnn_ref_trig exposes it), because the reference calls cos / sin / atan2 on floats
 *     (iou3d_kernel.cu:56,104-106,135-136; roipool3d.cpp:89); polygon vertices are ordered by that atan2f, as the reference's
 *     bubble sort orders them (iou3d_kernel.cu:188-196).  Results are bit-identical to the reference's own sources compiled for
 *     the host (oracle/_ref, oracle trig_mode 0), near-threshold pairs and on-the-face points included
 *     (tests/test_gpu_parity_residuals.py);
 *   - decode_bbox_target and the canonical transform of roipool3d keep cos / sin evaluated in double and rounded once to fp32
 *     (oracle trig_mode 1): their reference is torch's vectorised cos / sin, pinned to 2.4e-7, not glibc's scalar routines;
 *   - MLP layers: fp32 accumulation on the matrix pipe, either fp32 MFMA or the exact three-way bf16 split with six products per
 *     fp32 product (fp32-grade: |err| <= ~3e-7 * sum_k |x_k||w_k| per output element, measured against float64, for both).
 */
#ifndef PRCNN_POINTOPS_H
#define PRCNN_POINTOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* prcnn_stream_t; /* hipStream_t */

#define PRCNN_OK 0
#define PRCNN_EINVAL (-1)       /* bad argument (shape, null pointer, unsupported size) */
#define PRCNN_EHIP (-2)         /* HIP runtime / launch failure */
#define PRCNN_EUNSUPPORTED (-3) /* valid request this build has no kernel for */

int prcnn_abi_version(void);   /* 12: + prcnn_switches_reload, prcnn_switch_get (the PRCNN_* kernel switches are read once, through one table);
                                 * still 12 (additive): + prcnn_kitti_result_text (the KITTI result files' text formatted on the device);
                                 * still 12 (additive): + prcnn_aug_scene_sample, prcnn_aug_scene_workspace_bytes, prcnn_aug_scene_count,
                                 * prcnn_aug_scene_fill (the offline GT-augmented scenes, the train_aug split, generated on the device);
                                 * still 12 (additive): + prcnn_optim_chunk_elems, prcnn_optim_grad_norm, prcnn_optim_step (the adam_onecycle
                                 * parameter update: clip, decay and Adam over all tensors in two launches);
                                 * still 12 (additive): + prcnn_optim_step_adam, prcnn_optim_step_sgd (TRAIN.OPTIMIZER adam and sgd on the
                                 * same tables and launches);
                                 * still 12 (additive): + prcnn_head_tail_fwd, prcnn_head_tail_work_bytes, prcnn_head_tail_bwd,
                                 * prcnn_dropout_rows (the training heads' Dropout + output layer, the mask keyed by a counter);
                                 * still 12 (additive): + prcnn_eval_gt_max_iou, prcnn_eval_stats_accumulate, prcnn_eval_stats_workspace_bytes
                                 * (recall, segmentation IoU and RCNN accuracy of the evaluation loops counted on the device);
                                 * still 12 (additive): + prcnn_rcnn_offline_sample, prcnn_rcnn_offline_finish (RCNN offline training batches);
                                 * still 12 (additive): + prcnn_fps_nested (a nested FPS level answered from the parent's sample order);
                                 * still 12 (additive, no caller breaks): + prcnn_gt_database_workspace_bytes, prcnn_gt_database_count,
                                 * prcnn_gt_database_fill (the GT-augmentation database built on the device);
                                 * still 12 (additive): + prcnn_rpn_loss_workspace_bytes, prcnn_rpn_loss_counts, prcnn_rpn_loss_forward,
                                 * prcnn_rpn_loss_backward (the RPN training loss and its gradient in device passes);
                                 * still 12 (additive): + prcnn_rpn_loss_cls_sums, prcnn_rpn_loss_forward_kind, prcnn_rpn_loss_backward_kind
                                 * (the same for RPN.LOSS_CLS = DiceLoss and BinaryCrossEntropy);
                                 * still 12 (additive): + prcnn_rcnn_loss_workspace_bytes, prcnn_rcnn_loss_forward, prcnn_rcnn_loss_finalize,
                                 * prcnn_rcnn_loss_backward (the RCNN training loss and its gradient in device passes);
                                 * still 12 (additive): + prcnn_scene_prepare_large, prcnn_scene_large_workspace_bytes,
                                 * prcnn_train_scene_prepare_large, prcnn_train_scene_large_workspace_bytes (both input builders up to
                                 * 65536 points per frame: the shuffle sorted through HBM);
                                 * 11: + prcnn_train_scene_workspace_bytes, prcnn_train_scene_prepare (the RPN training batch on the device);
                                 * 10: + prcnn_corner_iou3d, prcnn_gt_aug_sample (GT-augmentation sampling loop on the device);
                                 * 9: + prcnn_fps_mode, prcnn_ball_query_arith, prcnn_three_nn_arith (comparison mode: the squared distance as nvcc contracts the
                                 * upstream expression); prcnn_nms_workspace_bytes grew by one flag byte per 64 x 64 tile; 8: + prcnn_mlp_group_split;
                                 * 7: split-bf16 chain entry points take the fp32 pack images too (fp32 recomputation of rows with non-finite values); 6: + prcnn_fps_status, training-mode SharedMLP (prcnn_train_*), prcnn_boxes_iou3d, prcnn_proposal_target_sample, prcnn_ref_trig (box trigonometry = the reference's host libm, bit for bit); 5: + prcnn_gt_aug_edit;
                                 * 4: + prcnn_host_* (host twins of the reference's *_cpu entry points), prcnn_build_id,
                                 * prcnn_fps_order (upstream tie order), prcnn_rpn_labels,
                                 * prcnn_ball_query2_grid takes xyz (dense-frame scan fallback);
                                 * 3: + padding-free grouping (rows_dev / groups_dev, prcnn_group_compact, ...), RoI duplicate
                                 * elimination (seg_cnt / seg_rows, distinct, valid_n), prcnn_scene_prepare */
const char* prcnn_last_error(void);
/* hex digest of the kernel sources + compile flags this library was built from (the Python binding compares it with the
 * sources it sits next to and refuses / rebuilds a stale library instead of silently loading it) */
const char* prcnn_build_id(void);
/* The PRCNN_* environment variables that select between kernels (csrc/switches.h lists them, INTEGRATION.md describes them)
 * are read ONCE, on the first call that consults one; later changes of the environment are not seen.
 * prcnn_switches_reload() reads them again and publishes the new values for every later call, from any thread; a call that
 * runs concurrently reads each switch from the old or the new set, never a torn value.  The caller must not change the
 * environment while this function runs (the C library does not allow it to be written while another thread reads it). */
int prcnn_switches_reload(void);
/* the library's current view of one switch, by variable name: *set = present, *num = atol of its value (0 if unset); either
 * pointer may be null.  PRCNN_EINVAL for a name that is not a switch of this library.  For tests; no product path calls it. */
int prcnn_switch_get(const char* name, int* set, long* num);

/* ---------------------------------------------------------------------------------------------
 * PointNet++ operators.  Replace pointnet2_cuda.* [UPSTREAM sshaoshuai/Pointnet2.PyTorch, not in
 * tree]; reference call sites: lib/net/pointnet2_msg.py:27-34,44,61,66-68, lib/net/rcnn_net.py:33-41.
 * ------------------------------------------------------------------------------------------- */

/* furthest_point_sampling_wrapper(B,N,npoint,xyz,temp,idx): xyz (B,N,3) -> idx (B,npoint) i32.
 * Start index 0, ties -> lowest point index.  `tmp` (B,N) 4-byte scratch (upstream's `temp` argument):
 *   N > 16384           required: HBM-resident running min-distances;
 *   2048 < N <= 16384   optional: when given, selects the spatially pruned kernel (Morton pre-sort into `tmp`, exact
 *                       bounding-box skip; bit-identical results); NULL = the register-resident kernel;
 *   N <= 2048           ignored.
 * Domain: FINITE coordinates.  The kernels order distances through integer compares of their bit patterns and bare
 * v_min/v_max (the file is built with -ffinite-math-only); a cloud holding NaN / Inf has no farthest point under any rule
 * and the indices returned for it are unspecified (always within [0, N)).  Callers with unvalidated input filter first
 * (prcnn_scene_prepare drops non-finite raw points). */
int prcnn_fps(const float* xyz, int B, int N, int npoint, float* tmp, int32_t* idx, prcnn_stream_t stream);

/* prcnn_fps for a NESTED level: xyz (B,N,3) must be gather(parent cloud, prev_idx), where prev_idx (B,N) i32 is what prcnn_fps
 * returned for the parent cloud with npoint = N (canonical tie order).  FPS is greedy, so the first npoint samples of such a cloud
 * are positions 0, 1, 2, ... unless the parent ran out of distinct points or a coordinate is non-finite / huge.  A device pass
 * decides that per frame (every |coordinate| < 1e4 and prev_idx[b][1 .. npoint-1] != 0; csrc/fps.hip states why that suffices):
 * a frame that passes gets idx[b][j] = j and skip[b] = 1, every other frame gets skip[b] = 0 and runs the kernels of prcnn_fps.
 * Same indices as prcnn_fps(xyz, ...) bit for bit, no host synchronisation (safe inside a graph capture).
 * Requires npoint <= N <= 16384; `tmp` as for prcnn_fps; skip (B) i32 is written, not read, by the caller. */
int prcnn_fps_nested(const float* xyz, const int32_t* prev_idx, int B, int N, int npoint, float* tmp, int32_t* idx, int32_t* skip,
                     prcnn_stream_t stream);

/* N > 16384 runs one frame on several cooperating workgroups whose wait for each other is bounded (a hang would take the
 * GPU down); a workgroup that gave up fills the rest of its frame's output with -1 and marks a host-visible word.
 * prcnn_fps_status() returns PRCNN_EHIP (and clears the mark) if that happened since the last check, PRCNN_OK otherwise;
 * it does not synchronise -- call it after the stream has.  prcnn_fps itself checks the mark before every such launch. */
int prcnn_fps_status(void);

/* Same, with a selectable rule for ties among equal running min-distances (they only occur on clouds with duplicate
 * points or exact lattices):
 *   PRCNN_FPS_ORDER_CANONICAL  lowest point index (== prcnn_fps; the contract every other test pins);
 *   PRCNN_FPS_ORDER_UPSTREAM   the order the upstream CUDA kernel's thread layout produces: argmin (k mod T, k) with
 *                              T = min(1024, largest power of two <= N) -- for index-by-index
 *                              comparison against an upstream build; `tmp` (B,N) is required; not a fast path. */
#define PRCNN_FPS_ORDER_CANONICAL 0
#define PRCNN_FPS_ORDER_UPSTREAM 1
int prcnn_fps_order(const float* xyz, int B, int N, int npoint, int order, float* tmp, int32_t* idx, prcnn_stream_t stream);

/* COMPARISON MODE of the three index operators: selectable squared-distance arithmetic (and, for FPS, tie order).
 *   PRCNN_ARITH_CANONICAL  three individually rounded products summed left to right -- the contract of prcnn_fps / prcnn_ball_query* /
 *                          prcnn_three_nn* and of every test that pins an index;
 *   PRCNN_ARITH_UPSTREAM   fma(dz,dz, fma(dy,dy, dx*dx)): what nvcc's default -fmad=true makes of the upstream kernels'
 *                          (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)  (sshaoshuai/Pointnet2.PyTorch, not in the reference tree:
 *                          .gitmodules:1-4) -- for index-by-index comparison against an upstream build, and for measuring how often
 *                          the two arithmetics disagree (tools/arith_disagreement.py).
 * Plain kernels (one workgroup per frame / one thread per query), bit-identical to the oracle's prcnn_cpu_fps_mode /
 * prcnn_cpu_ball_query_arith / prcnn_cpu_three_nn_arith in both arithmetics; not a fast path, used by no module.
 * prcnn_fps_mode: `tmp` (B,N) f32 is required.  prcnn_three_nn_arith returns SQUARED distances and no weights. */
#define PRCNN_ARITH_CANONICAL 0
#define PRCNN_ARITH_UPSTREAM 1
int prcnn_fps_mode(const float* xyz, int B, int N, int npoint, int order, int arith, float* tmp, int32_t* idx, prcnn_stream_t stream);
int prcnn_ball_query_arith(const float* xyz, const float* new_xyz, int B, int N, int M, float radius, int nsample, int arith,
                           int32_t* idx, prcnn_stream_t stream);
int prcnn_three_nn_arith(const float* unknown, const float* known, int B, int n, int m, int arith, float* dist2, int32_t* idx,
                         prcnn_stream_t stream);

/* gather_points_wrapper(B,C,N,npoint,feat,idx,out): out[b,c,m] = feat[b,c,idx[b,m]] */
int prcnn_gather(const float* feat, const int32_t* idx, int B, int C, int N, int M, float* out, prcnn_stream_t stream);
/* gather_points_grad_wrapper: grad_feat (B,C,N) += scatter(grad_out (B,C,M)); grad_feat pre-zeroed by caller */
int prcnn_gather_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M, float* grad_feat,
                      prcnn_stream_t stream);

/* channels-last twin of gather: out[b,m,0:C] = in_cl[b, idx[b,m], 0:C]; in_cl rows have stride ld_in floats.
 * (new_xyz = xyz[fps_idx] without the two transposes upstream needs around gather_operation.) */
int prcnn_gather_rows(const float* in_cl, int ld_in, const int32_t* idx, int B, int N, int M, int C, float* out,
                      prcnn_stream_t stream);

/* ball_query_wrapper(B,N,M,radius,nsample,new_xyz,xyz,idx): idx (B,M,nsample) i32; first <=nsample
 * points with d2 < radius^2 in ascending index order, padded with the first hit; no hit -> zeros. */
int prcnn_ball_query(const float* xyz, const float* new_xyz, int B, int N, int M, float radius, int nsample,
                     int32_t* idx, prcnn_stream_t stream);
/* Two radii in ONE scan of xyz (the MSG level's two groupers share new_xyz): same results as two
 * prcnn_ball_query calls. */
int prcnn_ball_query2(const float* xyz, const float* new_xyz, int B, int N, int M, float radius_a, int nsample_a,
                      int32_t* idx_a, float radius_b, int nsample_b, int32_t* idx_b, prcnn_stream_t stream);

/* group_points_wrapper(B,C,N,npoint,nsample,feat,idx,out): out[b,c,m,s] = feat[b,c,idx[b,m,s]] */
int prcnn_group(const float* feat, const int32_t* idx, int B, int C, int N, int M, int nsample, float* out,
                prcnn_stream_t stream);
int prcnn_group_grad(const float* grad_out, const int32_t* idx, int B, int C, int N, int M, int nsample,
                     float* grad_feat, prcnn_stream_t stream);

/* three_nn_wrapper(B,n,m,unknown,known,dist2,idx): 3 nearest known points per unknown point, SQUARED
 * distances (the Python wrapper takes the sqrt, as upstream does), strict-< insertion (ties keep the
 * earlier index).  `weight` (B,n,3), optional (NULL to skip): the FP module's normalised
 * inverse-distance weights w_k = r_k / (r_0+r_1+r_2), r_k = 1/(sqrt(dist2_k)+1e-8). */
int prcnn_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                   float* weight, prcnn_stream_t stream);

/* three_interpolate_wrapper(B,C,m,n,feat,idx,weight,out): out[b,c,i] = (w0*f[i0] + w1*f[i1]) + w2*f[i2] */
int prcnn_three_interp(const float* feat, const int32_t* idx, const float* weight, int B, int C, int m, int n,
                       float* out, prcnn_stream_t stream);
/* three_interpolate_grad_wrapper: grad_feat (B,C,m) += scatter(grad_out (B,C,n) * weight); grad_feat pre-zeroed by the caller.
 * workspace: (B*m*C) floats of scratch or NULL.  With a workspace the scatter runs through a channels-last accumulator (the 64
 * lanes of a wave add to 64 consecutive channels of one known point: one or two cache lines per atomic instruction instead of
 * 64) and is transposed into grad_feat afterwards; NULL selects the direct kernel. */
int prcnn_three_interp_grad(const float* grad_out, const int32_t* idx, const float* weight, int B, int C, int n,
                            int m, float* grad_feat, float* workspace, prcnn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused per-point MLP layers (new; replaces the SharedMLP = Conv2d1x1+BN+ReLU (+max_pool2d) chain
 * that upstream runs through cuDNN on a materialised (B,C+3,npoint,nsample) tensor; specs at
 * lib/net/pointnet2_msg.py:20-45, lib/net/rpn.py:20-46, lib/net/rcnn_net.py:23-41).
 *
 * All activations are CHANNELS-LAST rows: a row is one point (or one (centroid,sample) pair) and
 * holds its channels contiguously.  One call = one layer:
 *      out[row, col_off + n] = act( sum_k A[row,k] * W[n,k] + bias[n] ),   n < Nout
 * computed with fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate).
 * BatchNorm (eval) is folded into W/bias by the caller.  `wpack` is W re-laid for the MFMA operand
 * order by prcnn_pack_weight.  If pool_ns > 0 the epilogue max-reduces every pool_ns consecutive
 * rows (max_pool2d(kernel=[1,nsample])) and writes rows/pool_ns rows; pool_ns must be 16, 32 or 64.
 * `ld_*` are row strides in floats.
 * ------------------------------------------------------------------------------------------- */

/* floats needed for the packed image of a (Nout,K) weight */
size_t prcnn_wpack_floats(int Nout, int K);
/* w: (Nout,K) row-major (torch conv weight).  k_rot: the first k_rot input channels of W are moved
 * to the END of the packed K order (grouped rows are laid out [features(C), dxyz(3)] while torch's
 * QueryAndGroup order is [dxyz(3), features(C)]: pass k_rot=3 for those layers, 0 otherwise). */
int prcnn_pack_weight(const float* w, int Nout, int K, int k_rot, float* wpack, prcnn_stream_t stream);

/* A = in (rows, K), row stride ld_in.
 * rows_dev (device i32, may be NULL) / rows_unit: DEVICE-side row count -- the kernel processes
 * min(rows, *rows_dev * rows_unit) rows and the launch (sized for `rows`) exits early past that; used with the
 * compact group lists of prcnn_group_compact, whose lengths are only known on the device. */
int prcnn_mlp_rows(const float* in, int ld_in, int64_t rows, int K, const float* wpack, const float* bias, int Nout,
                   int relu, float* out, int ld_out, int col_off, int pool_ns, const int32_t* rows_dev, int rows_unit,
                   const int32_t* seg_cnt, int seg_rows, prcnn_stream_t stream);
/* seg_cnt (device i32, may be NULL) / seg_rows: SEGMENT-PREFIX LIVE ROWS -- rows come in segments of seg_rows rows
 * (a multiple of 128 dividing rows) and only the first seg_cnt[s] rows of segment s are ever read by anyone: roipool3d
 * pads an RoI holding fewer points than it samples with copies of its first rows (prcnn_roipool3d_canonical's
 * `distinct` output).  128-row tiles lying entirely in the dead tail of their segment are skipped; their output rows are
 * left unwritten. */

/* A row (b,m,s) = [ feat_cl[b, idx[b,m,s], 0:C],  xyz[b, idx[b,m,s]] - new_xyz[b,m] ]  (K = C+3;
 * C may be 0 with feat_cl NULL).  new_xyz NULL => GroupAll semantics (no centroid subtraction).
 * rows = B*M*nsample.
 * HOISTED FIRST LAYER (act_wx, act_bias non-NULL; both NULL = the classic form above): grouping is a linear gather
 * and the first conv of a SharedMLP is linear, so W.[feat[idx]; dxyz] = (W_f.feat)[idx] + W_x.dxyz.  The caller
 * computes Z = W_f.feat once per SOURCE point (N rows instead of M*nsample) with prcnn_mlp_rows and passes it as
 * feat_cl (C = width of that first layer, C % 4 == 0); act_wx is (C,3) row-major = the dxyz columns of the first
 * layer's weight, act_bias (C, padded to x4) its bias.  The A row is then relu(Z[idx] + act_wx.dxyz + act_bias),
 * K = C, and wpack/bias describe the SECOND layer.  Same result up to fp32 reassociation. */
int prcnn_mlp_group(const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl, int ld_feat,
                    int B, int N, int M, int nsample, int C, const float* act_wx, const float* act_bias,
                    const float* wpack, const float* bias, int Nout, int relu, float* out, int ld_out, int col_off,
                    int pool_ns, const int32_t* groups_dev, prcnn_stream_t stream);   /* groups_dev: device count of groups
                    (<= B*M) actually present, or NULL -- see prcnn_mlp_rows / prcnn_group_compact */

/* A row (b,i) = [ sum_j w3[b,i,j] * known_cl[b, idx3[b,i,j], 0:C2],  skip_cl[b,i,0:C1] ]  (K = C2+C1;
 * C1 may be 0 with skip_cl NULL).  rows = B*n.
 * HOISTED FIRST LAYER (act_bias non-NULL, requires C1 == 0): interpolation is linear, so W.interp(x) = interp(W.x).
 * The caller computes Y = W.known once per KNOWN point (m rows instead of n) and passes it as known_cl (C2 = width
 * of that layer); the A row is relu(interp(Y) + act_bias) and wpack/bias describe the second layer. */
int prcnn_mlp_interp(const float* known_cl, int ld_known, const int32_t* idx3, const float* w3, const float* skip_cl,
                     int ld_skip, int B, int n, int m, int C2, int C1, const float* act_bias, const float* wpack,
                     const float* bias, int Nout, int relu, float* out, int ld_out, int col_off,
                     prcnn_stream_t stream);

/* Hoisted FP first layer WITH skip features: out[row,n] = act( sum_k in[row,k]*W_b[n,k] + bias[n]
 *                                                             + sum_j w3[row,j] * y_cl[b*m + idx3[row,j], n] )
 * where `in` are the skip features (K = C1), W_b the skip columns of the first layer's weight and
 * y_cl = W_a.known (B*m rows, ld_y floats apart) the interpolated part computed per known point.  rows = B*n. */
int prcnn_mlp_rows_addinterp(const float* in, int ld_in, int K, const float* wpack, const float* bias, int Nout,
                             int relu, const float* y_cl, int ld_y, const int32_t* idx3, const float* w3, int B, int n,
                             int m, float* out, int ld_out, int col_off, prcnn_stream_t stream);

/* Split-bf16 VARIANT of the two plain-row layer calls above (never the default arithmetic; the caller opts in per call).
 * Every fp32 operand is cut exactly into three bf16 pieces (x = x0 + x1 + x2) and each fp32 product is rebuilt from `terms`
 * bf16 MFMA products with fp32 accumulation: terms = 6 keeps everything above 2^-24 |x||w| (fp32-grade results), terms = 3
 * everything above 2^-16 |x||w|.  wsplit: prcnn_wsplit_bytes(Nout, K) bytes written by prcnn_pack_weight_split from the
 * (Nout, K) row-major fp32 weight.  The split kernel needs K % 32 == 0 and 16-byte aligned input rows; any other shape runs
 * the fp32 kernel on `wpack`, exactly as prcnn_mlp_rows / prcnn_mlp_rows_addinterp would.  Non-finite values: a wave that finds
 * a non-finite accumulator (an infinite or NaN input value, an overflowing product) recomputes its rows with fp32 MFMAs on
 * `wpack` -- those outputs are the fp32 kernels' own (inf stays inf, NaN only where IEEE arithmetic gives NaN).
 * pool_ns / rows_dev / rows_unit / seg_cnt / seg_rows: as for prcnn_mlp_rows.  A supported shape runs the split kernel whatever
 * its row count (the arithmetic of a layer does not depend on the batch size).
 * prcnn_pack_weight_split: chain = 0 writes the image of the two layer calls, chain = 1 the image of prcnn_mlp_chain_rows_split
 * (same size).  prcnn_mlp_chain_rows_split: the two-layer plain-row chain (prcnn_mlp_chain_rows with nlayers = 2) for K = 128,
 * nout = {128, 1} or {128, 65..128} -- the RPN heads; wchain / bias / nout / relu are HOST arrays of length 2, wchain[l] the
 * chain = 1 image of layer l (wchain[1] unused when nout[1] == 1: that output is a dot product on wpack[1]); wpack: HOST array
 * of the two layers' fp32 prcnn_pack_weight images (the single-channel output and the fp32 recomputation of rows with
 * non-finite values read them).  Any other shape: PRCNN_EUNSUPPORTED, issue prcnn_mlp_chain_rows.
 * (The reference computes these layers as fp32 cuDNN convolutions, [U] pytorch_utils.py SharedMLP) */
size_t prcnn_wsplit_bytes(int Nout, int K);
int prcnn_pack_weight_split(const float* w, int Nout, int K, int chain, void* wsplit, prcnn_stream_t stream);
int prcnn_mlp_rows_split(const float* in, int ld_in, int64_t rows, int K, const float* wpack, const void* wsplit, int terms,
                         const float* bias, int Nout, int relu, float* out, int ld_out, int col_off, int pool_ns,
                         const int32_t* rows_dev, int rows_unit, const int32_t* seg_cnt, int seg_rows, prcnn_stream_t stream);
int prcnn_mlp_chain_rows_split(const float* in, int ld_in, int64_t rows, int K, const void* const* wchain, const float* const* wpack,
                               const float* const* bias, const int* nout, const int* relu, int terms, float* out, int ld_out,
                               int col_off, prcnn_stream_t stream);
/* hoisted FP0 on the split chain kernel: rows relu(interp(known_cl) + act_bias), C2 = 128 and no skip features, through ONE
 * 128 -> 128 layer (prcnn_mlp_chain_interp with nlayers = 1, C1 = 0, act_bias given); wchain: the chain = 1 image, wpack: the
 * layer's fp32 prcnn_pack_weight image (rows with non-finite values).  Other shapes: PRCNN_EUNSUPPORTED. */
int prcnn_mlp_chain_interp_split(const float* known_cl, int ld_known, const int32_t* idx3, const float* w3, int B, int n, int m,
                                 int C2, const float* act_bias, const void* wchain, const float* wpack, const float* bias, int Nout,
                                 int relu, int terms, float* out, int ld_out, int col_off, prcnn_stream_t stream);
int prcnn_mlp_rows_addinterp_split(const float* in, int ld_in, int K, const float* wpack, const void* wsplit, int terms,
                                   const float* bias, int Nout, int relu, const float* y_cl, int ld_y, const int32_t* idx3,
                                   const float* w3, int B, int n, int m, float* out, int ld_out, int col_off,
                                   prcnn_stream_t stream);
/* prcnn_mlp_group's HOISTED form (act_wx / act_bias given) on the split-bf16 layer kernel: the gathered row relu(Z[idx] + act_wx.dxyz +
 * act_bias) is activated on its way into the split.  wsplit: the layer's prcnn_pack_weight_split image (chain = 0), terms 3 / 6; wpack: its
 * fp32 image (rows holding inf / NaN are redone on the fp32 pipe).  Needs C % 32 == 0 and 16-byte aligned feature rows; any other shape
 * (or act_wx NULL) runs the fp32 layer kernel exactly as prcnn_mlp_group does.  Replaces the same reference code as prcnn_mlp_group. */
int prcnn_mlp_group_split(const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl, int ld_feat, int B, int N,
                          int M, int nsample, int C, const float* act_wx, const float* act_bias, const float* wpack,
                          const void* wsplit, int terms, const float* bias, int Nout, int relu, float* out, int ld_out, int col_off,
                          int pool_ns, const int32_t* groups_dev, prcnn_stream_t stream);

/* Register-resident layer CHAIN: up to 3 consecutive layers (a whole SharedMLP) in ONE kernel; one wave owns 32
 * rows and carries them through every layer inside the register file (the MFMA accumulator layout of layer l is
 * the B-operand layout of layer l+1), so intermediate activations touch neither LDS nor HBM and a gathered /
 * interpolated input row is built once.  Same arithmetic as the per-layer calls (fp32 MFMA, fp32 accumulate).
 * wpack[l], bias[l], nout[l], relu[l] are HOST arrays of length nlayers; every bias[l] (device, may be NULL) must
 * hold 32*ceil(nout[l]/32) floats (zero padded).  Limits: nout[l] <= 128; pool_ns in {0,16,32} (group variant:
 * pool_ns == nsample or 0).  Only a fixed set of width combinations is instantiated: ask
 * prcnn_mlp_chain_supported first, or handle PRCNN_EUNSUPPORTED by issuing the per-layer calls.
 * mode: 0 = rows, 1 = group, 2 = interp.  act_wx / act_bias: hoisted first layer, as for prcnn_mlp_group /
 * prcnn_mlp_interp (the chain then starts at the second layer).
 * One more shape (round 2): mode 1, TWO layers wider than 128 (nout[l] <= 384 / 512), un-pooled, nsample 1, hoisted first
 * layer with C <= 256 -- the flat row lists of the wide set-abstraction levels -- runs as a 32-row two-layer stack through
 * LDS (same bits as the per-layer calls); prcnn_mlp_chain_supported answers 1 for it from the widths alone, the call itself
 * returns PRCNN_EUNSUPPORTED if the other conditions are not met. */
int prcnn_mlp_chain_supported(int mode, int nlayers, const int* nout, int pool_ns);
int prcnn_mlp_chain_rows(const float* in, int ld_in, int64_t rows, int K, int nlayers, const float* const* wpack,
                         const float* const* bias, const int* nout, const int* relu, float* out, int ld_out,
                         int col_off, int pool_ns, const int32_t* seg_cnt, int seg_rows, prcnn_stream_t stream);
                         /* seg_cnt / seg_rows: as for prcnn_mlp_rows */
int prcnn_mlp_chain_group(const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl,
                          int ld_feat, int B, int N, int M, int nsample, int C, const float* act_wx,
                          const float* act_bias, int nlayers,
                          const float* const* wpack, const float* const* bias, const int* nout, const int* relu,
                          float* out, int ld_out, int col_off, int pool_ns, const int32_t* groups_dev, prcnn_stream_t stream);
int prcnn_mlp_chain_interp(const float* known_cl, int ld_known, const int32_t* idx3, const float* w3,
                           const float* skip_cl, int ld_skip, int B, int n, int m, int C2, int C1,
                           const float* act_bias, int nlayers, const float* const* wpack, const float* const* bias, const int* nout, const int* relu,
                           float* out, int ld_out, int col_off, prcnn_stream_t stream);

/* Up to four prcnn_mlp_chain_group problems in ONE launch (the grouped stacks of one set-abstraction level: both radii, flat and
 * dense list).  Every field is prcnn_mlp_chain_group's argument of that name.  Each problem is decided as a call of its own
 * would be; the launch exists when all of them resolve to the same kernel family (the SA-level-0 register kernel, the
 * straight-line chain or the two-layer stack) and that combination is instantiated -- otherwise PRCNN_EUNSUPPORTED and nothing
 * is launched: issue the problems one by one.  Same bits as the separate calls (same body on the same rows). */
typedef struct prcnn_chain_group_problem {
    const float* xyz; const float* new_xyz; const int32_t* idx; const float* feat_cl;
    const float* act_wx; const float* act_bias;
    const float* const* wpack; const float* const* bias; const int* nout; const int* relu;
    float* out; const int32_t* groups_dev;
    int ld_feat, B, N, M, nsample, C, nlayers, ld_out, col_off, pool_ns;
} prcnn_chain_group_problem_t;
int prcnn_mlp_chain_group_multi(int nprob, const prcnn_chain_group_problem_t* prob, prcnn_stream_t stream);
/* The same launch, storing by destination: dst (host array over the problems; NULL, or NULL entries: that problem stores to its
 * own out as above) names where problem q's result rows go in the level output out2 (ld_out2 floats per row, problem q's columns
 * at col_off2[q]).  Un-pooled problem: dst[q][row] >= 0 -> row dst[q][row] of out2, < 0 -> row `row` of the problem's out
 * (prcnn_group_compact_pair_dst's rdst).  Pooled problem: group g -> row dst[q][g] of out2 (the dense list's listn); its out is
 * not written.  Same kernels, grids and arithmetic as prcnn_mlp_chain_group_multi. */
int prcnn_mlp_chain_group_multi_dst(int nprob, const prcnn_chain_group_problem_t* prob, const int32_t* const* dst, float* out2, int ld_out2,
                                    const int* col_off2, prcnn_stream_t stream);

/* out[r, col_off + c] = max over ns consecutive rows of in (generic nsample fallback for pooling) */
int prcnn_maxpool_rows(const float* in, int ld_in, int64_t rows_out, int ns, int C, float* out, int ld_out,
                       int col_off, prcnn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * roipool3d.  Replaces roipool3d_cuda.forward (roipool3d.cpp:48-79 -> roipool3d_kernel.cu:209-237).
 * xyz (B,N,3), boxes3d (B,M,7) [x,y(bottom),z,h,w,l,ry] ALREADY enlarged (roipool3d_utils.py:19),
 * feat (B,N,C) -> pooled (B,M,S,3+C), empty (B,M) i32.  One pass, no B*N*M temporary, no allocation.
 * Every output element is written (empty boxes get zero rows), so `pooled` need not be pre-zeroed.
 * ------------------------------------------------------------------------------------------- */
int prcnn_roipool3d(const float* xyz, const float* boxes3d, const float* feat, int B, int N, int M, int C, int S,
                    float* pooled, int32_t* empty, prcnn_stream_t stream);
/* The same operator with a caller-provided scratch buffer (>= prcnn_roipool3d_work_bytes(B, N) device bytes; 0 = this N has no
 * binned form): the frame's points are first bucketed into x-z bins, and each RoI tests only the points of the bins its footprint
 * touches instead of all N (identical selection: same membership test, ascending index order).  work == NULL or too small:
 * the linear scan of prcnn_roipool3d.  Worth it from a handful of RoIs per frame upwards. */
size_t prcnn_roipool3d_work_bytes(int B, int N);
int prcnn_roipool3d_ws(const float* xyz, const float* boxes3d, const float* feat, int B, int N, int M, int C, int S, float* pooled,
                       int32_t* empty, void* work, size_t work_bytes, prcnn_stream_t stream);

/* The same two operators, also reporting the selection (pooled and empty are the bytes prcnn_roipool3d / _ws write):
 *   idx (B,M,S) i32: the frame-local source point, in [0, N), of every pooled row; every row of an empty RoI holds -1;
 *   distinct (B,M) i32: min(points in the box, S), 0 for an empty RoI.  idx[b,m,s] == idx[b,m,s % distinct] (roipool3d.cpp:171-177). */
int prcnn_roipool3d_index(const float* xyz, const float* boxes3d, const float* feat, int B, int N, int M, int C, int S,
                          float* pooled, int32_t* empty, int32_t* idx, int32_t* distinct, prcnn_stream_t stream);
int prcnn_roipool3d_index_ws(const float* xyz, const float* boxes3d, const float* feat, int B, int N, int M, int C, int S, float* pooled,
                             int32_t* empty, int32_t* idx, int32_t* distinct, void* work, size_t work_bytes, prcnn_stream_t stream);

/* Gradient of the pooling with respect to the per-point features (the reference's roipool3d has no backward):
 *   gfeat[b, p, c] = sum over (m, s) with idx[b, m, s] == p of gpooled[b, m, s, col0 + c]
 * gpooled: (B, M, S) rows of stride ld_g >= col0 + C floats; idx, distinct: as prcnn_roipool3d_index wrote them (entries outside
 * [0, N) and slots >= distinct of an RoI's first wrap period are ignored); gfeat: (B, N) rows of stride ld_out >= C, columns
 * [0, C) written.  work: prcnn_roipool3d_grad_work_bytes(B, N, M, S) device bytes (0: outside the domain), 4-byte aligned.
 * A gather: no float atomics, no memset; every gfeat element is written exactly once (a point no row refers to gets 0); a point's
 * addends are added in float32 from zero in ascending (m, s); two calls give the same bytes; rows of empty RoIs are never read.
 * Domain: 1 <= C <= 256, N <= 65536, S <= 512, M S < 2^31 -- PRCNN_EUNSUPPORTED beyond it, PRCNN_EINVAL for a bad shape, stride,
 * null pointer or workspace; nothing is launched or written then. */
size_t prcnn_roipool3d_grad_work_bytes(int B, int N, int M, int S);
int prcnn_roipool3d_grad(const float* gpooled, int64_t ld_g, int col0, const int32_t* idx, const int32_t* distinct, int B, int N, int M,
                         int S, int C, float* gfeat, int ld_out, void* work, size_t work_bytes, prcnn_stream_t stream);

/* point-in-box flags on the device: flags (M,N) i32 (device twin of roipool3d.cpp:97-125) */
int prcnn_pts_in_boxes3d(const float* pts, const float* boxes3d, int N, int M, int32_t* flags, prcnn_stream_t stream);

/* RPN training labels for a whole batch on the device (KittiRCNNDataset.generate_rpn_training_labels,
 * lib/datasets/kitti_rcnn_dataset.py:365-394): pts (B,N,3), gt_boxes3d (B,G,7) [x,y(bottom),z,h,w,l,ry], num_gt (B) i32 or
 * NULL (all G rows valid) -> cls_label (B,N) i32 in {-1 ignore, 0 background, 1 foreground}, reg_label (B,N,7)
 * [dx, dy, dz, h, w, l, ry] (zero rows for non-foreground points).  extra_width = 0.2 in the reference.  Boxes are applied in
 * order, later boxes overwrite earlier ones exactly as the reference's loop does.  G <= 128.  The in-box test is the analytic
 * one of roipool3d WITHOUT its 10 m centre-distance gate (the reference's hull test has none: a box with a half extent over
 * 10 m keeps all its points); it can differ from the hull test only for points within rounding distance of a face. */
int prcnn_rpn_labels(const float* pts, const float* gt_boxes3d, const int32_t* num_gt, int B, int N, int G, float extra_width,
                     int32_t* cls_label, float* reg_label, prcnn_stream_t stream);

/* GT-augmentation scene edit for a batch of scenes on the device -- the point work of
 * KittiRCNNDataset.apply_gt_aug_to_one_scene (lib/datasets/kitti_rcnn_dataset.py:484-489 one pts_in_boxes3d_cpu scan of the
 * scene per accepted object, :501-507 boolean-mask copy + concatenate).  pts (B,N,3), intensity (B,N) or NULL, boxes3d (B,K,7)
 * = the accepted objects' boxes [x,y(bottom),z,h,w,l,ry] (K <= 64), tested with h + extra_h (2.0 in the reference);
 * new_pts (B,P,3) / new_intensity (B,P) = the pasted objects' points, already concatenated in paste order.  num_pts / num_boxes /
 * num_new: (B) i32 live counts or NULL (all rows live).  Output: out_pts (B,N+P,3), out_intensity (B,N+P) or NULL: the scene
 * points outside every box IN THEIR ORIGINAL ORDER, then the new points; rows >= out_count[b] are zero.  out_count (B) i32;
 * removed (B,N) i32 or NULL: 1 where a scene point was dropped (the complement of the reference's src_pts_flag).
 * In-box test == prcnn_pts_in_boxes3d.  The sampling loop that decides which objects are pasted and where is prcnn_gt_aug_sample. */
int prcnn_gt_aug_edit(const float* pts, const float* intensity, const int32_t* num_pts, const float* boxes3d,
                      const int32_t* num_boxes, float extra_h, const float* new_pts, const float* new_intensity,
                      const int32_t* num_new, int B, int N, int K, int P, float* out_pts, float* out_intensity,
                      int32_t* out_count, int32_t* removed, prcnn_stream_t stream);

/* kitti_utils.get_iou3d (lib/utils/kitti_utils.py:195-235) on corner sets: corners_a (N,8,3), corners_b (M,8,3) in rect coords
 * (kitti_utils.boxes3d_to_corners3d order) -> iou3d (N,M), iou_bev (N,M) or NULL (the need_bev=True branch).  Heights in fp32 from
 * the corners as numpy forms them (min_h = -(sum of y over corners 0:4, left to right) / 4, max_h over 4:8); a pair with no height
 * overlap is 0.  The bottom quads (corners 0:4 in (x, z)) are clipped against each other in DOUBLE (exact convex clip, in place of
 * shapely's intersection) and the ratios are formed in double and stored as fp32.  A quad that is not strictly convex (degenerate,
 * self-intersecting) gives 0, as the reference's is_valid branch does.  Can differ from shapely only when an IoU is within
 * rounding of a decision threshold, i.e. for boxes that touch.  csrc/quad_clip.h. */
int prcnn_corner_iou3d(const float* corners_a, int N, const float* corners_b, int M, float* iou3d, float* iou_bev, prcnn_stream_t stream);

/* The sampling loop of KittiRCNNDataset.apply_gt_aug_to_one_scene (lib/datasets/kitti_rcnn_dataset.py:414-497) and the
 * apply-probability draw before it (:279), for a whole batch in one launch, one workgroup per frame, no host round trip.
 *   gt_boxes3d (B,G,7) the frame's non-DontCare labels [x,y(bottom),z,h,w,l,ry] (filtrate_dc_objects), num_gt (B) i32 or NULL;
 *   planes (B,4) f64 device: road plane a b c d, normal facing up and unit length (kitti_dataset.get_road_plane);
 *   db_boxes (D,7), db_alpha (D), db_npts (D) i32: the packed GT database; easy_idx (E) / hard_idx (H) i32: database ids of the
 *   easy (> 100 points) and hard lists, used when GT_AUG_HARD_RATIO > 0 (otherwise the draw is over all D entries);
 *   cfg4: four DOUBLES in HOST memory: GT_EXTRA_NUM, GT_AUG_RAND_NUM (0/1), GT_AUG_APPLY_PROB, GT_AUG_HARD_RATIO;
 *   scope: six doubles in HOST memory = PC_AREA_SCOPE (check_pc_range on the database centre) or NULL (PC_REDUCE_BY_RANGE false);
 *   try_times = 100 in the reference; K = bound on accepted objects per frame (1..64, G + K <= 256).
 * Per try: easy/hard draw, index draw, range check (skipped, not counted), < 5 points (skipped, not counted), the move onto the
 * road plane in double (new y rounded to fp32), w and l + 0.5, cnt += 1, collision test of the enlarged box against the list
 * (accepted iff every iou3d < 1e-8, prcnn_corner_iou3d arithmetic).  The list starts as the scene boxes with w, l + 0.5; every
 * accepted enlarged box is appended.  The loop ends when cnt > extra_gt_num or the tries run out: cnt counts tries that reached
 * the collision test, not accepted objects.
 * Output: count (B) i32; db_id (B,K) i32 (-1 past count), boxes3d (B,K,7) the placed UNENLARGED boxes, alpha (B,K), y_shift (B,K)
 * f64 = move_height (a pasted point's y becomes fp32(double(y) - y_shift)); stats (B,4) i32 = applied, extra_gt_num, cnt, tries
 * started; status (B): 0 ok, 1 = the reference raises for this frame (randint on an empty list or with GT_EXTRA_NUM <= 10, max of
 * an empty IoU array), 2 = more than K objects would be accepted (the first K are returned), 3 = an easy / hard list entry is
 * not a database id in [0, D) (the loop stops there).
 * Random calls: the counter-based table of csrc/train_input.hip (streams 30-33). */
int prcnn_gt_aug_sample(const float* gt_boxes3d, const int32_t* num_gt, const double* planes, int B, int G, const float* db_boxes, const float* db_alpha, const int32_t* db_npts, int D, const int32_t* easy_idx, int E, const int32_t* hard_idx, int H, const double* cfg4, const double* scope, int try_times, int K, uint32_t seed, int32_t* count, int32_t* db_id, float* boxes3d, float* alpha, double* y_shift, int32_t* stats, int32_t* status, prcnn_stream_t stream);

/* HOST twins of the reference's two CPU entry points (roipool3d.cpp:97-125 pts_in_boxes3d_cpu, :127-195 roipool3d_cpu),
 * which its dataloader calls inside forked worker processes (kitti_rcnn_dataset.py:487,582,625,843,970).  Host pointers,
 * no HIP call, bit-identical to the reference's CPU arithmetic (double half-extent compares, inclusive bounds).
 *   pts (N,3), boxes3d (M,7) -> flags (M,N) int64;
 *   pts (N,3), boxes3d (M,7), feat (N,C) -> pooled_pts (M,S,3), pooled_feat (M,S,C), empty (M) int64; rows of an empty
 *   box are left untouched (the caller zero-initialises them, roipool3d_utils.py:77-79). */
int prcnn_host_pts_in_boxes3d(const float* pts, const float* boxes3d, int64_t N, int64_t M, int64_t* flags);
int prcnn_host_roipool3d(const float* pts, const float* boxes3d, const float* feat, int64_t N, int64_t M, int64_t C, int64_t S,
                         float* pooled_pts, float* pooled_feat, int64_t* empty);

/* ---------------------------------------------------------------------------------------------
 * iou3d.  Replace iou3d_cuda.{boxes_overlap_bev_gpu,boxes_iou_bev_gpu,nms_gpu,nms_normal_gpu}
 * (iou3d.cpp:31,52,73,123).  BEV boxes are (N,5) [x1,y1,x2,y2,ry].
 * ------------------------------------------------------------------------------------------- */
int prcnn_boxes_overlap_bev(const float* boxes_a, int Na, const float* boxes_b, int Nb, float* out,
                            prcnn_stream_t stream);
int prcnn_boxes_iou_bev(const float* boxes_a, int Na, const float* boxes_b, int Nb, float* out, prcnn_stream_t stream);

#define PRCNN_NMS_ROTATED 0
#define PRCNN_NMS_NORMAL 1
/* workspace bytes prcnn_nms needs for N boxes (the suppression mask in whole blocks of 64 rows, 64 ceil(N/64) x ceil(N/64) words, + one flag byte per 64 x 64 tile of it) */
size_t prcnn_nms_workspace_bytes(int N);
/* Greedy NMS over boxes ALREADY sorted by descending score (iou3d_utils.py:64-66): box i suppresses
 * j>i iff iou(i,j) > thresh.  Entirely on the device: keep (N) i64 receives the kept positions in
 * ascending order, num_keep (1) i32 their count.  No host synchronisation.
 * max_keep: 0 = full sweep (reference semantics); > 0 = stop once that many boxes are kept -- the leading
 * max_keep entries are identical to the full result (what lib/rpn/proposal_layer.py:112 consumes). */
int prcnn_nms(const float* boxes, int N, float thresh, int kind, int max_keep, int64_t* keep, int32_t* num_keep,
              void* workspace, size_t workspace_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * Proposal stage: batched, sync-free replacements for the per-frame Python loop
 * between the RPN heads and roipool3d.  Oracle twins: prcnn_cpu_decode_bbox_target / _proposal_layer / _nms_batched.
 * ====================================================================================================== */

/* lib/utils/bbox_transform.py:24-121  decode_bbox_target(roi_box3d, pred_reg, loc_scope, loc_bin_size, num_head_bin,
 * anchor_size, get_xz_fine, get_y_by_bin, loc_y_scope, loc_y_bin_size, get_ry_fine) -- same argument meaning.
 *   roi (N, roi_cols) device: roi_cols 3 = xyz points (RPN stage, proposal_layer.py:23), 7 = RoI boxes (eval_rcnn.py:509,
 *   rotated back by roi ry).  pred_reg (N, C) device; C must equal the channel count the flags imply (the reference
 *   asserts, :106) else PRCNN_EINVAL.  anchor_size_host: 3 floats h,w,l in HOST memory (cfg.CLS_MEAN_SIZE[0]).
 *   Scalars are doubles because the reference computes them in Python floats before they meet a tensor.
 *   y_to_bottom != 0 also applies proposal_layer.py:32 (y += h/2).  out (N, 7) device [x,y,z,h,w,l,ry]. */
int prcnn_decode_bbox_target(const float* roi, int roi_cols, const float* pred_reg, long N, int C, double loc_scope,
                             double loc_bin_size, int num_head_bin, const float* anchor_size_host, int get_xz_fine,
                             int get_y_by_bin, double loc_y_scope, double loc_y_bin_size, int get_ry_fine, int y_to_bottom,
                             float* out, prcnn_stream_t stream);

/* workspace for prcnn_proposal_layer: pre_max = max(pre1, pre2), post_max = max(post1, post2) */
size_t prcnn_proposal_workspace_bytes(int B, int N, int pre_max, int post_max);
/* lib/rpn/proposal_layer.py:35-141 on decoded boxes3d (B, N, 7) and raw scores (B, N), whole batch, no host sync:
 * per frame order rows by descending score (NaN first, ties by ascending row -- torch.sort leaves tie order open),
 *   use_range != 0 (distance_based_proposal :58-117): area 1 = rows with r0 < z <= r1, area 2 = r1 < z <= r2; keep the
 *       first pre1 / pre2 of each; an empty area 2 borrows ranks [pre1, pre1+pre2) of area 1 (:91-98);
 *   use_range == 0 (score_based_proposal :119-141): one list, first pre1 rows (pre2 = post2 = 0);
 * greedy NMS (nms_kind, nms_thresh) on the BEV boxes (kitti_utils.py:134-147) of each list, first post1 / post2 survivors,
 * concatenated into out_boxes (B, post1+post2, 7) / out_scores (B, post1+post2), zero padded (:38-39).
 * out_count (B) i32, optional: rows filled per frame.  An empty area contributes nothing (the reference asserts, :90).
 * Frames of up to 16384 rows are sorted entirely in LDS; larger frames run the same bitonic network in 16384-key chunks with
 * the long strides through the workspace in HBM. */
int prcnn_proposal_layer(const float* scores, const float* boxes3d, int B, int N, int use_range, float r0, float r1, float r2,
                         int pre1, int pre2, int post1, int post2, float nms_thresh, int nms_kind, float* out_boxes,
                         float* out_scores, int32_t* out_count, void* workspace, size_t workspace_bytes, prcnn_stream_t stream);

size_t prcnn_nms_batched_workspace_bytes(int B, int M);
/* Final detection select (tools/eval_rcnn.py:600-614) for the whole batch: per frame, rows with valid[b,i] != 0
 * (valid NULL = all), ordered by descending score, greedy NMS on their BEV boxes; unlike iou3d_cuda.nms_gpu the boxes need
 * NOT be pre-sorted.  keep (B, max_keep) i32: row indices in kept order, -1 padded; num_keep (B) i32.
 * max_keep 0 = M.  PRCNN_EUNSUPPORTED when max_keep boxes do not fit the LDS kept list (~1900 rotated): use prcnn_nms. */
int prcnn_nms_batched(const float* boxes3d, const float* scores, const uint8_t* valid, int B, int M, float thresh, int kind,
                      int max_keep, int32_t* keep, int32_t* num_keep, void* workspace, size_t workspace_bytes,
                      prcnn_stream_t stream);

/* Fused RCNN input builder = lib/net/rcnn_net.py:127-154 in one pass:
 *   cat([extra0, extra1, feat]) -> roipool3d (first <= S in-box points per RoI, wrap-duplicated, boxes = pool_boxes3d,
 *   already enlarged by the caller) -> pooled xyz -= roi centre (:146-147) -> rotate_pc_along_y_torch(pooled xyz, roi ry)
 *   (kitti_utils.py:45-63), without the (B,N,2+C) and (B,M,S,5+C) tensors and without the per-frame Python loop.
 * rois (B,M,7) define the canonical frame; NULL keeps scene coordinates.  extra0 / extra1: per-point scalar channels
 * (B,N) (seg_mask, normalised depth) or NULL.  feat: (B,N,C) rows with stride ld_feat.
 * out_pts : B*M*S rows of stride ld_pts, columns [x',y',z',extra0,extra1];
 * out_feat: B*M*S rows of stride ld_out, C columns written at this pointer (point it INTO a wider buffer to place the
 *           features where the next layer wants them).  empty (B,M) i32.  An empty RoI yields zeros run through the
 *           same transform (i.e. -centre rotated), exactly what the reference's in-place ops produce.
 * distinct (B,M) i32, may be NULL: when given it receives the number of DISTINCT rows of every RoI -- min(points in the
 *           box, S), 1 for an empty RoI (all its rows are equal); rows distinct .. S-1 are wrap-copies of rows
 *           0 .. distinct-1 (roipool3d.cpp:171-177).  out_pts is still written in full (FPS and ball_query of the next
 *           level see the padded cloud), but the FEATURE rows of the copies are NOT written: hand `distinct` to the
 *           consumers as seg_cnt (prcnn_mlp_rows / prcnn_mlp_chain_rows) and valid_n (prcnn_group_compact). */
int prcnn_roipool3d_canonical(const float* xyz, const float* pool_boxes3d, const float* rois, const float* extra0,
                              const float* extra1, const float* feat, int ld_feat, int B, int N, int M, int C, int S,
                              float* out_pts, int ld_pts, float* out_feat, int ld_out, int32_t* empty, int32_t* distinct,
                              prcnn_stream_t stream);
/* ... with the scratch buffer of prcnn_roipool3d_ws (binned point selection) */
int prcnn_roipool3d_canonical_ws(const float* xyz, const float* pool_boxes3d, const float* rois, const float* extra0,
                                 const float* extra1, const float* feat, int ld_feat, int B, int N, int M, int C, int S,
                                 float* out_pts, int ld_pts, float* out_feat, int ld_out, int32_t* empty, int32_t* distinct,
                                 void* work, size_t work_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * Grid-accelerated neighbour search: the same results as prcnn_ball_query / prcnn_ball_query2 / prcnn_three_nn
 * (bit for bit), computed over a per-frame x-z grid (64 or 128 cells per axis) instead of a scan of all N points.
 * ====================================================================================================== */
/* bytes of the grid buffer for B frames of N points */
size_t prcnn_grid_bytes(int B, int N);
/* bin xyz (B,N,3) per frame: bounds -> cell size max(min_cell, extent/cells_per_axis) -> counting sort into cell-contiguous
 * float4 (x,y,z,index).  grid: 16-byte aligned device buffer of prcnn_grid_bytes(B,N).  min_cell: the largest search
 * radius that will be used (keeps a ball within 3x3 cells); 0 for three_nn.  cells_per_axis: 64 or 128 (finer cells keep
 * crowded near-sensor regions cheap for the ball query; ~1 point per cell suits the three_nn ring search). */
int prcnn_grid_build(const float* xyz, int B, int N, float min_cell, int cells_per_axis, void* grid, size_t grid_bytes,
                     prcnn_stream_t stream);
/* == prcnn_ball_query2 on the binned points (N = points per frame the grid was built with); nsample_b = 0: one radius.
 * xyz (B,N,3), the points the grid was built from, or NULL.  With xyz given, DENSE frames -- prcnn_grid_build estimates the
 * candidates a ball visits from the cell occupancy; above N/32 the grid kernel's per-candidate cost exceeds a scan's -- are
 * answered by the index-order scan of prcnn_ball_query2 instead (launched behind the grid kernel; each kernel exits at once on
 * the other's frames, so the launch sequence is static).  Results are identical either way. */
int prcnn_ball_query2_grid(const void* grid, const float* xyz, const float* new_xyz, int B, int N, int M, float radius_a,
                           int nsample_a, int32_t* idx_a, float radius_b, int nsample_b, int32_t* idx_b, prcnn_stream_t stream);
/* == prcnn_three_nn with `known` given as a grid of m points per frame */
int prcnn_three_nn_grid(const void* grid, const float* unknown, int B, int n, int m, float* dist2, int32_t* idx, float* weight,
                        prcnn_stream_t stream);

/* ======================================================================================================
 * KITTI object evaluation kernels (host side: pointrcnn_amd/kitti_eval.py).
 * Oracle twins: prcnn_cpu_rotate_iou_eval / prcnn_cpu_kitti_overlaps / prcnn_cpu_kitti_statistics.
 * ====================================================================================================== */
/* tools/kitti_object_eval_python/rotate_iou.py:287-329 rotate_iou_gpu_eval(boxes, query_boxes, criterion):
 * boxes (N,5), query (K,5) rows [cx, cy, dx, dy, angle] -> out (N,K).  criterion -1: IoU, 0: inter / area(query),
 * 1: inter / area(box), 2: intersection area (the numba kernel evaluates devRotateIoUEval(query_k, box_n), :282-284). */
int prcnn_rotate_iou_eval(const float* boxes, int N, const float* query, int K, int criterion, float* out, prcnn_stream_t stream);
/* Per-frame overlap blocks of eval.py:326-397 calculate_iou_partly for F frames in one launch: rows = first box set
 * ("dt"), columns = second ("gt").  metric 0: 2-D IoU of image boxes (.,4); 1: rotated BEV IoU, 2: 3-D IoU of camera
 * boxes (.,7) [x, y, z, l, h, w, ry] (float64 in, like the annotation arrays).  dt_off / gt_off (F+1) i32 row offsets,
 * ov_off (F+1) i64 offsets of the row-major blocks inside out (float64). */
int prcnn_kitti_overlaps(int metric, const double* dt, const int32_t* dt_off, const double* gt, const int32_t* gt_off,
                         const int64_t* ov_off, int F, double* out, prcnn_stream_t stream);
/* eval.py:155-324 compute_statistics_jit for every (frame, threshold): res (F, T, 4) = tp, fp, fn, similarity
 * (similarity -1 as in the reference when undefined).  gt_datas (G,5) [bbox, alpha], dt_datas (D,6) [bbox, alpha, score],
 * ign_gt (G) / ign_det (D) from clean_data, dc (DC,4) DontCare boxes, offsets (F+1).  compute_fp = 0 is the
 * reference's first pass (thresh ignored): matched (G) f64, optional, receives the score of the detection that made gt i
 * a true positive, NaN otherwise.  max_det_per_frame: caller-known bound (<= 1024, PRCNN_EUNSUPPORTED above). */
int prcnn_kitti_statistics(const double* overlaps, const int64_t* ov_off, const double* gt_datas, const int32_t* gt_off,
                           const double* dt_datas, const int32_t* dt_off, const int32_t* ign_gt, const int32_t* ign_det,
                           const double* dc, const int32_t* dc_off, int F, int max_det_per_frame, int metric, double min_overlap,
                           const double* thresholds, int T, int compute_fp, int compute_aos, double* res, double* matched,
                           prcnn_stream_t stream);

/* ======================================================================================================
 * Padding-free grouping (dedup.hip).  ball_query pads short groups by repeating their first hit; the rows of a group
 * beyond its cnt real hits are copies and cannot change the max-pooled result.  prcnn_group_compact splits the G = B*M
 * groups of one ball query, on the device, into
 *   sparse groups (cnt <= sparse_max): their real rows are appended to ONE flat row list -- ridx (G*sparse_max) global
 *       point index b*N + p, rnx (G*sparse_max, 3) the row's group centroid -- and the group is recorded as
 *       slist (G) group id, soff (G) first flat row, scnt (G) = cnt;
 *   dense groups (cnt > sparse_max): idxn (G, nsample) global indices of ALL nsample rows (padding included),
 *       nxn (G,3), listn (G) group id  (may be NULL when sparse_max == nsample: every group is then sparse).
 * counts (3 device i32): [0] flat rows, [1] dense groups, [2] sparse groups; list order is arbitrary.  All outputs are
 * sized for the worst case.  Run the MLP on each list as one frame (B = 1, N = B*N): the flat rows with M = G*sparse_max,
 * nsample = 1, no pooling, groups_dev = &counts[0], then prcnn_segmax_scatter; the dense list with M = G, pooling,
 * groups_dev = &counts[1], then prcnn_scatter_rows.
 * ====================================================================================================== */
int prcnn_group_compact(const int32_t* idx, const float* new_xyz, int B, int N, int M, int nsample, int sparse_max,
                        const int32_t* valid_n, int32_t* ridx, float* rnx, int32_t* slist, int32_t* soff, int32_t* scnt,
                        int32_t* idxn, float* nxn, int32_t* listn, int32_t* counts, prcnn_stream_t stream);
/* valid_n (B) i32, may be NULL: only points 0 .. valid_n[b]-1 of frame b are distinct, the rest of the frame are wrap-copies
 * of them in order (prcnn_roipool3d_canonical's `distinct`): ball_query lists ascending indices, so a hit >= valid_n[b] is a
 * copy of an earlier hit of the same group -- it ends the group's real rows like padding does, and in the dense list it is
 * replaced by the group's first hit, so that no consumer ever reads a copy's (unwritten) feature row. */
/* dst[list[j], col_off + c] = max over r < cnt[j] of src[off[j] + r, c]  for j < *count, c < C */
int prcnn_segmax_scatter(const float* src, int ld_src, const int32_t* list, const int32_t* off, const int32_t* cnt,
                         const int32_t* count, int max_groups, int C, float* dst, int ld_dst, int col_off, prcnn_stream_t stream);
/* dst[list[r], col_off : col_off + C] = src[r, 0:C] for r < *count (count: device i32; max_rows sizes the launch) */
int prcnn_scatter_rows(const float* src, int ld_src, const int32_t* list, const int32_t* count, int max_rows, int C, float* dst,
                       int ld_dst, int col_off, prcnn_stream_t stream);
/* Both scales of an MSG level (one new_xyz, no valid_n) split by ONE counter clear and ONE launch: what two prcnn_group_compact
 * calls give, as sets (list order is arbitrary).  lists_a / lists_b: host arrays of the eight list buffers in prcnn_group_compact's
 * order (ridx, rnx, slist, soff, scnt, idxn, nxn, listn); counts (6 device i32): [0..2] scale a, [3..5] scale b. */
int prcnn_group_compact_pair(const int32_t* idx_a, int ns_a, int T_a, const int32_t* idx_b, int ns_b, int T_b, const float* new_xyz,
                             int B, int N, int M, void* const* lists_a, void* const* lists_b, int32_t* counts, prcnn_stream_t stream);
/* The pooling launches of one level as ONE launch: nprob <= 4 problems into dst (ld_dst floats per row); host arrays over problems.
 * off[q] != NULL: prcnn_segmax_scatter(src[q], ld_src[q], list[q], off[q], cnt[q], count[q], max_items[q], C[q], dst, ld_dst, col_off[q]);
 * off[q] == NULL: prcnn_scatter_rows(src[q], ld_src[q], list[q], count[q], max_items[q], C[q], dst, ld_dst, col_off[q]).
 * The problems must write disjoint cells. */
int prcnn_level_pool(int nprob, const float* const* src, const int* ld_src, const int32_t* const* list, const int32_t* const* off,
                     const int32_t* const* cnt, const int32_t* const* count, const int* max_items, const int* C, const int* col_off,
                     float* dst, int ld_dst, prcnn_stream_t stream);
/* prcnn_group_compact_pair, and per flat row where its result belongs: rdst_a / rdst_b (B*M*T_a / B*M*T_b i32) hold the group id
 * for the only real row of a one-row group (its result IS the group's row of the level output) and -1 for the rows of a group
 * that has more to pool. */
int prcnn_group_compact_pair_dst(const int32_t* idx_a, int ns_a, int T_a, const int32_t* idx_b, int ns_b, int T_b, const float* new_xyz,
                                 int B, int N, int M, void* const* lists_a, void* const* lists_b, int32_t* rdst_a, int32_t* rdst_b,
                                 int32_t* counts, prcnn_stream_t stream);
/* What is left of prcnn_level_pool after prcnn_mlp_chain_group_multi_dst: every problem a flat list (off[q], cnt[q] non-NULL),
 * only groups with cnt >= 2 are pooled and stored; the cells of one-row groups are not touched. */
int prcnn_level_pool_residual(int nprob, const float* const* src, const int* ld_src, const int32_t* const* list, const int32_t* const* off,
                              const int32_t* const* cnt, const int32_t* const* count, const int* max_items, const int* C, const int* col_off,
                              float* dst, int ld_dst, prcnn_stream_t stream);

/* ======================================================================================================
 * RPN input builder (scene.hip) -- SURVEY 8(f) rank 4.  Replaces the inference branch of
 * lib/datasets/kitti_rcnn_dataset.py:246-310 (get_rpn_sample): calibration.py:51-70 lidar_to_rect + rect_to_img,
 * get_valid_flag (kitti_rcnn_dataset.py:198-219), mask compaction and the npoints sampling of :285-306, for a whole batch.
 *   raw      (total_points, 4) f32 device: the frames' velodyne scans [x y z intensity] back to back (kitti_dataset.py:40-43)
 *   offsets  (B+1) i64 device: first raw point of every frame; max_points_per_frame: host-known bound on the frame sizes
 *   calib    (B, 24) f32 device: M = V2C^T . R0^T (4x3 row-major, calibration.py:57) then P2 (3x4 row-major)
 *   img_hw   (B, 2) i32 device: image height, width (kitti_dataset.py:34-39)
 *   scope    6 doubles on the HOST [x0 x1 y0 y1 z0 z1] = cfg.PC_AREA_SCOPE, or NULL (cfg.PC_REDUCE_BY_RANGE false)
 *   out_xyz (B, npoints, 3), out_intensity (B, npoints) = intensity - 0.5, out_src (B, npoints) raw index of every row,
 *   nvalid (B) number of valid points, status (B): 0 ok; 1 = the reference raises for this frame (more than npoints
 *   far points, or fewer than npoints/2 valid ones) -- rows are still produced; 2 = no valid point (rows zero, src -1).
 * Every point at rect depth >= 40 m is kept, the rest drawn without replacement, the result shuffled; short frames are
 * topped up with a draw without replacement from themselves.  The draw uses a counter-based generator keyed by
 * (seed, frame, raw index) -- see scene.hip -- so results are reproducible and independent of launch geometry
 * (the reference uses numpy's unseeded global stream).  npoints <= 16384 (prcnn_scene_prepare_large: <= 65536).
 * ====================================================================================================== */
size_t prcnn_scene_workspace_bytes(int64_t total_points, int B);
int prcnn_scene_prepare(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                        const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                        float* out_xyz, float* out_intensity, int32_t* out_src, int32_t* nvalid, int32_t* status,
                        void* workspace, size_t workspace_bytes, prcnn_stream_t stream);
/* The same builder for npoints 1..65536; arguments, outputs and random streams as prcnn_scene_prepare.  npoints <= 16384 runs the
 * launches of prcnn_scene_prepare (same bytes, same workspace need).  16384 < npoints <= 65536: the draw writes every frame's
 * selection to a key array in the workspace, the shuffle sorts it through HBM in 16384-key chunks (3 plain launches for up to
 * 32768 points, 6 above), a last launch writes the rows -- all on `stream`, in launch order, with no host synchronisation; the
 * workspace (8-byte aligned) grows by B key arrays of npoints rounded up to a power of two, 8 bytes a key, plus 4 bytes per frame.
 * PRCNN_EINVAL for npoints outside 1..65536 (nothing launched) and for a workspace below prcnn_scene_large_workspace_bytes. */
size_t prcnn_scene_large_workspace_bytes(int64_t total_points, int B, int npoints);
int prcnn_scene_prepare_large(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                              const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                              float* out_xyz, float* out_intensity, int32_t* out_src, int32_t* nvalid, int32_t* status,
                              void* workspace, size_t workspace_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * RPN training batch (train_scene.hip).  KittiRCNNDataset.get_rpn_sample in TRAIN mode (kitti_rcnn_dataset.py:246-362, RPN.FIXED
 * false) between the GT-augmentation sampling loop (prcnn_gt_aug_sample, run before) and the label generation (prcnn_rpn_labels,
 * run after, on out_xyz / out_gt_boxes3d / out_num_gt): valid points, removal of the scene points inside the accepted objects'
 * boxes (h + 2), paste of their database points (y - y_shift), the npoints draw over the edited cloud, label boxes = training
 * labels then placed boxes, data_augmentation (rotation, scaling, flip; stage 1).  No host round trip, no (N + P) cloud.
 *   raw .. seed                as prcnn_scene_prepare
 *   gt_boxes3d (B, G, 7), gt_alpha (B, G), num_gt (B) or NULL: the frame's TRAINING labels (filtrate_objects) and their alphas
 *   acc_count (B), acc_db_id (B, K), acc_boxes3d (B, K, 7), acc_alpha (B, K), acc_y_shift (B, K) f64, acc_status (B): the outputs of
 *     prcnn_gt_aug_sample, on the device; acc_count == NULL: GT_AUG_ENABLED false.  Frames with acc_status 1 or 3 are built
 *     without paste or removal.  K <= 64, G + K <= 128.
 *   db_points (P, 3), db_intensity (P), db_offsets (D+1) i64: the packed GT database; db_max_points >= every object's point count
 *   aug_cfg  10 doubles on the HOST: rotation / scaling / flip in cfg.AUG_METHOD_LIST (0 / 1; all 0 = cfg.AUG_DATA false),
 *            AUG_METHOD_PROB[0..2], -(pi / AUG_ROT_RANGE), pi / AUG_ROT_RANGE, 0.95, 1.05
 *   out_xyz (B, npoints, 3) augmented points; out_input (B, npoints, 4) = [xyz | feature] or NULL; out_features (B, npoints) =
 *   intensity - 0.5; out_src (B, npoints): the raw index of a scene point, n_raw[b] + j for the j-th pasted point (accepted order,
 *   then database point order); nvalid (B) size of the edited cloud; status (B) as prcnn_scene_prepare;
 *   out_gt_boxes3d (B, G + K, 7) augmented label boxes, zero rows beyond out_num_gt (B);
 *   aug (B, 8) f64: aug_enable[0..2], angle, cos(angle), sin(angle), scale, flip (0 / 1) as the kernels used them; angle, cos, sin
 *   are NaN when the rotation did not run, scale when the scaling did not.
 * Random values: streams 0-2 (draw, shuffle; position = out_src's identity) and 34-36 (augmentation) of scene.hip's table.
 * ====================================================================================================== */
size_t prcnn_train_scene_workspace_bytes(int64_t total_points, int B, int K, int db_max_points);
int prcnn_train_scene_prepare(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                              const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                              const float* gt_boxes3d, const float* gt_alpha, const int32_t* num_gt, int G,
                              const int32_t* acc_count, const int32_t* acc_db_id, const float* acc_boxes3d, const float* acc_alpha,
                              const double* acc_y_shift, const int32_t* acc_status, int K, const float* db_points,
                              const float* db_intensity, const int64_t* db_offsets, int D, int db_max_points,
                              const double* aug_cfg, float* out_xyz, float* out_input, float* out_features, int32_t* out_src,
                              int32_t* nvalid, int32_t* status, float* out_gt_boxes3d, int32_t* out_num_gt, double* aug,
                              void* workspace, size_t workspace_bytes, prcnn_stream_t stream);
/* The same pass for npoints 1..65536, as prcnn_scene_prepare_large is to prcnn_scene_prepare: the one-workgroup form up to 16384
 * (same bytes, same workspace need), select -> HBM sort -> rows above it. */
size_t prcnn_train_scene_large_workspace_bytes(int64_t total_points, int B, int K, int db_max_points, int npoints);
int prcnn_train_scene_prepare_large(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                    const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                                    const float* gt_boxes3d, const float* gt_alpha, const int32_t* num_gt, int G,
                                    const int32_t* acc_count, const int32_t* acc_db_id, const float* acc_boxes3d, const float* acc_alpha,
                                    const double* acc_y_shift, const int32_t* acc_status, int K, const float* db_points,
                                    const float* db_intensity, const int64_t* db_offsets, int D, int db_max_points,
                                    const double* aug_cfg, float* out_xyz, float* out_input, float* out_features, int32_t* out_src,
                                    int32_t* nvalid, int32_t* status, float* out_gt_boxes3d, int32_t* out_num_gt, double* aug,
                                    void* workspace, size_t workspace_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * GT-augmentation database builder (gt_database.hip).  tools/generate_gt_database.py:50-84 for a batch of frames: the rect-camera
 * points of the WHOLE scan (no FOV, image or PC_AREA_SCOPE filter) that lie in each labelled object's box, in ascending raw index,
 * each with its intensity and raw index.  rect = the canonical lidar -> rect of prcnn_scene_prepare; membership = the test of
 * prcnn_pts_in_boxes3d (roipool3d.cpp:82-95, 10 m gate included).  A point inside two boxes belongs to both objects.
 *   raw, offsets, max_points_per_frame, calib   as prcnn_scene_prepare (of calib only M is read)
 *   boxes3d (B, G, 7) [x y z h w l ry], num_boxes (B) i32: the frame's kept labels; G <= 128
 * The output size depends on the data, so the caller allocates between two calls that share one workspace (its content must
 * survive from the count to the fill):
 *   prcnn_gt_database_count  -> npts (B, G) i32, zero at and beyond num_boxes[b]; per-tile hit counts go to the workspace.
 *   prcnn_gt_database_fill   <- obj_offsets (B * G + 1) i64 = the exclusive scan of npts (objects frame-major, then in label order),
 *                               total_out = obj_offsets[B * G] = the rows the three output buffers hold
 *                            -> points (total_out, 3) rect coordinates, intensity (total_out), src (total_out) i32 raw index in the frame.
 * A row's position is object offset + prefix sums of hit counts (tile, wave, lane), never the order of an atomic append: two runs
 * give identical bytes.  No row outside [0, total_out) is written, whatever obj_offsets holds.
 * PRCNN_EINVAL for G > 128, a null pointer, or a workspace smaller than prcnn_gt_database_workspace_bytes.
 * ====================================================================================================== */
size_t prcnn_gt_database_workspace_bytes(int64_t max_points_per_frame, int B, int G);
int prcnn_gt_database_count(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                            const float* calib, const float* boxes3d, const int32_t* num_boxes, int G, int32_t* npts,
                            void* workspace, size_t workspace_bytes, prcnn_stream_t stream);
int prcnn_gt_database_fill(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                           const float* calib, const float* boxes3d, const int32_t* num_boxes, int G, const int64_t* obj_offsets,
                           int64_t total_out, float* points, float* intensity, int32_t* src, void* workspace,
                           size_t workspace_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * Offline GT-augmented scenes (aug_scene.hip).  tools/generate_aug_scene.py for a batch of frames: step 1 of the reference's offline
 * RCNN recipe (the `train_aug` split that eval_rcnn.py --save_rpn_feature and train_rcnn.py --train_mode rcnn_offline then read).
 *
 * prcnn_aug_scene_sample: AugSceneGenerator.aug_one_scene's sampling loop (:157-219), one launch, no host round trip.
 *   gt_boxes3d (B, G, 7) + num_gt (B) i32 or NULL: the frame's non-DontCare labels; planes (B, 4) f64 road planes;
 *   frame_ids (B) i32: the key of the random table, the NEW sample id (epoch + 1) * 10000 + sample_id;
 *   db_boxes (D, 7), db_npts (D) i32: the database; scope: 6 doubles x0 x1 y0 y1 z0 z1 (PC_AREA_SCOPE), required;
 *   -> count (B), db_id (B, K) (-1 past count), boxes3d (B, K, 7) placed and unenlarged, y_shift (B, K) f64,
 *      stats (B, 3) i32 extra_gt_num, cnt, tries spent; status (B) i32: 0 ok, 1 the reference raises (D <= 1, or an IoU against an
 *      empty list), 2 a bound was exceeded.
 *   It is not the online loop of prcnn_gt_aug_sample: extra_gt_num = randint(10, 15) (stream 60); 50 tries and a try skipped by the range
 *   check or the "< 5 points" check is spent; the index draw randint(0, D - 1) never draws the last entry (stream 61, position = try);
 *   range check, then `cnt > extra_gt_num` break, then "< 5 points", plane move (double), cnt += 1, collision; the collision is the
 *   arithmetic of prcnn_boxes_iou3d between the moved, unenlarged box and the list (labels and accepted boxes with w + 0.5, l + 0.5),
 *   accepted iff the maximum is < 1e-8 as float32.  cnt <= 15 bounds the accepted objects.
 *   PRCNN_EINVAL for K < 15, K > 64, G + 15 > 256, a null pointer.
 *
 * prcnn_aug_scene_count / prcnn_aug_scene_fill: the augmented cloud (:240-248, :205-231).  raw, offsets, max_points_per_frame, calib,
 *   img_hw, scope as prcnn_scene_prepare; acc_* = the sampler's outputs; db_points (db_total_points, 3), db_intensity, db_offsets (D+1) i64.
 *   Per frame: lidar -> rect (canonical), the valid flag, every valid point inside an accepted box tested with h + 2 (the test of
 *   prcnn_pts_in_boxes3d) dropped, the survivors in raw order, then the accepted objects' database points in acceptance order, each
 *   object's in database order, with y - y_shift.  A frame with status 1 or count 0 comes out as its valid cloud.
 *   prcnn_aug_scene_count -> rows (B) i32: the rows of every frame (-1: more than fit the count).  The caller forms out_offsets (B+1) i64,
 *   their exclusive scan, and total_out = out_offsets[B]; the workspace's content must survive from the count to the fill.
 *   prcnn_aug_scene_fill  -> out (total_out, 4) [x y z intensity] (the raw intensity), src (total_out) i32: the raw index of a scan
 *   point, -1 - (database point row) of a pasted one.
 *   A row's position comes from prefix sums (tile, wave, lane; object sizes), never from an atomic append: two runs give identical
 *   bytes.  No row outside [0, total_out) or outside its frame's [out_offsets[b], out_offsets[b+1]) is written.
 *   PRCNN_EINVAL for K outside 1..64, a null pointer, a workspace smaller than prcnn_aug_scene_workspace_bytes, out not 16-byte aligned.
 * ====================================================================================================== */
int prcnn_aug_scene_sample(const float* gt_boxes3d, const int32_t* num_gt, const double* planes, const int32_t* frame_ids, int B, int G,
                           const float* db_boxes, const int32_t* db_npts, int D, const double* scope, int K, uint32_t seed,
                           int32_t* count, int32_t* db_id, float* boxes3d, double* y_shift, int32_t* stats, int32_t* status,
                           prcnn_stream_t stream);
size_t prcnn_aug_scene_workspace_bytes(int64_t max_points_per_frame, int B);
int prcnn_aug_scene_count(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                          const float* calib, const int32_t* img_hw, const double* scope, const int32_t* acc_count,
                          const int32_t* acc_db_id, const float* acc_boxes3d, const int32_t* acc_status, int K,
                          const int64_t* db_offsets, int D, int64_t db_total_points, int32_t* rows, void* workspace,
                          size_t workspace_bytes, prcnn_stream_t stream);
int prcnn_aug_scene_fill(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                         const float* calib, const int32_t* img_hw, const double* scope, const int32_t* acc_count,
                         const int32_t* acc_db_id, const float* acc_boxes3d, const double* acc_y_shift, const int32_t* acc_status,
                         int K, const float* db_points, const float* db_intensity, const int64_t* db_offsets, int D,
                         int64_t db_total_points, const int64_t* out_offsets, int64_t total_out, float* out, int32_t* src,
                         void* workspace, size_t workspace_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * Training-mode SharedMLP (csrc/mlp_train.h) -- BASELINE config 4, `train_rcnn.py --train_mode rpn`.
 * Replaces, for one SharedMLP layer, nn.Conv2d(1x1, bias=False) -> nn.BatchNorm2d (batch statistics, running-stat update) ->
 * ReLU and its autograd (cuDNN / ATen in the reference: lib/net/pointnet2_msg.py:20-45 via the upstream pytorch_utils.SharedMLP,
 * tools/train_rcnn.py:198-199), with F.max_pool2d(kernel=[1, nsample]) after the last layer.  All tensors are channels-last rows.
 * The layer's ONLY saved activation is its pre-normalisation output y; consumers apply relu(y * scale + shift) on load.
 *
 * prcnn_train_src_t says how the rows entering a layer's convolution are produced (mode = 0 plain rows `in`, optionally with
 * the previous layer's normalisation `pro_scale / pro_shift` (K entries zero-padded to a multiple of 32 floats) applied;
 * 1 = grouped rows [feat[idx] | xyz[idx] - new_xyz] (the weight is packed with k_rot = 3), rows = B * M * ns, K = C + 3;
 * 2 = interpolated rows [sum_j w3 known[idx3] | skip], rows = B * n, K = C2 + C1).
 * A layer's constant table cst holds 6 rows of ld_c floats: scale = gamma * invstd, shift = beta - mean * scale, mean, invstd
 * (forward), mean(dyhat), mean(dyhat * xhat) (backward).  One call runs a whole stack; the host side is C++ (no per-layer Python).
 * ====================================================================================================== */
typedef struct prcnn_train_src {
    int mode;
    int64_t rows;
    int K;
    const float* in; int ld_in; const float* pro_scale; const float* pro_shift;
    const float* xyz; const float* new_xyz; const int32_t* idx; const float* feat; int ld_feat; int B, N, M, ns, C;
    const float* known; const int32_t* idx3; const float* w3; const float* skip; int ld_known, ld_skip, n, m, C2, C1;
    /* padding-free rows (grouped source only; all NULL / 0 otherwise): the rows are the DISTINCT rows of the groups as built by
     * prcnn_train_group_rows -- B = 1, N = frames * points, M = rows = the worst case frames * npoint * nsample, ns = 1, idx = ridx,
     * new_xyz = rnx; mult (rows) row multiplicities, rows_dev the live row count on the device, norm_rows = frames * npoint *
     * nsample (what the batch statistics are normalised by), seg_off / seg_cnt (groups) first row / row count of every group,
     * row_grp (rows) the group of every row.  The pooled output has `groups` rows; arg holds the arg-max position inside the group. */
    const float* mult; const int32_t* rows_dev; int64_t norm_rows; const int32_t* seg_off; const int32_t* seg_cnt; const int32_t* row_grp;
    int groups;
} prcnn_train_src_t;

/* One layer of a stack.  The caller owns every buffer (nothing is allocated inside):
 *   W (Nout, K) conv weight in torch layout (K = the source's K for layer 0, the previous layer's Nout after that); gamma, beta,
 *   running_mean, running_var (Nout) and eps, momentum of its BatchNorm;
 *   y (rows, Nout)  the layer's saved pre-normalisation output (written by forward, read by backward);
 *   cst (6, ld_c)   constant table, ZERO-INITIALISED by the caller before forward; ld_c a multiple of 128, >= Nout;
 *   wpack           prcnn_wpack_floats(Nout, K) floats: the forward weight image (written by forward);
 *   wpack_t         prcnn_wpack_floats(Kin, Nout) floats: the dgrad weight image, Kin = K (K - 3 for a grouped layer 0, whose
 *                   xyz columns carry no gradient); NULL when the layer's input takes no gradient (layer 0 only);
 *   dW (Nout, K) in torch's channel order, dgamma, dbeta (Nout): written by backward.
 * gamma == NULL: a layer WITHOUT normalisation -- Conv (bias in `beta`, or NULL) -> ReLU, the form of the RCNN stage
 * (cfg.RCNN.USE_BN = False, lib/net/rcnn_net.py:24-60): no statistics, dbeta receives the bias gradient, dgamma / running_* unused. */
typedef struct prcnn_train_layer {
    int Nout;
    const float* W; const float* gamma; const float* beta;
    float eps, momentum;
    float* running_mean; float* running_var;
    float* y;
    float* cst; int ld_c;
    float* wpack; float* wpack_t;
    float* dW; float* dgamma; float* dbeta;
} prcnn_train_layer_t;

/* scratch both passes need (partials of the statistics, wgrad partial tiles, the inter-layer gradient ping-pong); 256-byte aligned */
size_t prcnn_train_stack_work_bytes(int64_t rows, const prcnn_train_layer_t* layers, int nl, int K0, int backward);
/* forward of the whole stack: per layer pack weights -> y = A . W^T on the MFMA pipe with per-64-row (mean, M2) partials -> batch
 * statistics in double, fixed order -> cst rows 0..3 and the running statistics ((1 - momentum) * old + momentum * new, unbiased
 * variance); then out[g, col_off + n] = max over the pool_ns rows of group g of relu(y * scale + shift), arg (groups, Nout) u8 = the
 * FIRST maximal row (torch.max / max_pool2d route the gradient there); pool_ns <= 1: plain normalise + ReLU, arg unused.
 * a_dump (rows, ld_dump): copy of the assembled first-layer rows of a gathered source (backward's wgrad reads it); NULL for plain. */
int prcnn_train_stack_fwd(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, float* a_dump, int ld_dump,
                          float* out, int ld_out, int col_off, uint8_t* arg, void* work, size_t work_bytes, prcnn_stream_t stream);
/* backward of the whole stack from gout = d loss / d out ((rows / pool_ns, N_last) rows): per layer BatchNorm reductions (dgamma,
 * dbeta), wgrad (dW), dgrad into the previous layer.  gin (rows, ld_gin), may be NULL: gradient w.r.t. the rows that entered layer 0
 * (grouped source: the C feature columns only) -- scatter it with prcnn_group_rows_grad / prcnn_interp_rows_grad. */
int prcnn_train_stack_bwd(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, const float* a_dump,
                          int ld_dump, const float* gout, int ld_gout, const uint8_t* arg, float* gin, int ld_gin, void* work,
                          size_t work_bytes, prcnn_stream_t stream);
/* The same two passes with the forward / dgrad GEMMs of the eligible layers on the split-bf16 x 6 arithmetic of the inference
 * layers (every fp32 operand cut exactly into three bf16 pieces, six v_mfma_f32_32x32x16_bf16 products, fp32 accumulation:
 * fp32-grade results, csrc/mlp_train.h).  Opt-in: prcnn_train_stack_fwd / _bwd above are unchanged.  Each takes what its twin
 * takes plus a table of nl device pointers to scratch for the split weight images, written per call; entry l NULL = layer l on
 * the fp32 pipe.
 *   wsplit[l]    prcnn_wsplit_bytes(Nout, K) bytes, 16-byte aligned.  Used when layer l reads plain rows (every layer l > 0, layer
 *                0 of a mode-0 source), K % 32 == 0 and its rows (and pro_scale / pro_shift) are 16-byte aligned;
 *   wsplit_t[l]  prcnn_wsplit_bytes(Kin, Nout) bytes (Kin as for wpack_t), 16-byte aligned.  Used when Nout % 32 == 0.
 * A layer that does not meet its condition runs the fp32 kernel it runs in the twin, whatever its entry holds; wgrad, the
 * statistics, pooling and every reduction are the twin's launches.  wpack / wpack_t are written as in the twin (the split images come
 * next to them, not instead).
 * Non-finite operands: a row whose fp32 result is +-inf or NaN in SOME column comes out non-finite (NaN) in EVERY column of its
 * 32-column blocks; rows with finite operands are unaffected by their neighbours.  Nothing is recomputed on the fp32 pipe. */
int prcnn_train_stack_fwd_split(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, float* a_dump,
                                int ld_dump, float* out, int ld_out, int col_off, uint8_t* arg, void* const* wsplit, void* work,
                                size_t work_bytes, prcnn_stream_t stream);
int prcnn_train_stack_bwd_split(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, const float* a_dump,
                                int ld_dump, const float* gout, int ld_gout, const uint8_t* arg, float* gin, int ld_gin,
                                void* const* wsplit_t, void* work, size_t work_bytes, prcnn_stream_t stream);
/* prcnn_train_stack_bwd_split with the weight gradient of the WIDE layers on the split-bf16 x 6 arithmetic as well (opt-in; the two
 * entry points above keep their launches).  A layer's wgrad runs train_wgrad_s_kernel where the twin runs the 128 x 128 LDS-staged
 * fp32 kernel: K > 64 and Nout > 64, the layer's input rows 16-byte aligned with a row stride that is a multiple of 4, and
 * PRCNN_WGRAD_DIRECT not set.  Both operands -- relu(a * scale + shift) or the raw first-layer rows, and dy rebuilt from (G, y) --
 * are cut into three bf16 pieces after the transform; partial tiles, their fixed-order reduction (deterministic) and the workspace
 * are the twin's.  Every other layer's wgrad, the reductions and the BatchNorm backward are the twin's launches; dgrad goes split
 * per layer as in prcnn_train_stack_bwd_split, and a wsplit_t table of NULL entries (the table itself must not be NULL) keeps
 * every dgrad on the fp32 pipe.
 * Non-finite operands: nothing is recomputed on the fp32 pipe.  A dW entry whose fp32 value is non-finite comes out non-finite,
 * possibly NaN where fp32 gives +-inf; entries whose operand rows are all finite are fp32-grade. */
int prcnn_train_stack_bwd_wsplit(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, const float* a_dump,
                                 int ld_dump, const float* gout, int ld_gout, const uint8_t* arg, float* gin, int ld_gin,
                                 void* const* wsplit_t, void* work, size_t work_bytes, prcnn_stream_t stream);
/* The split-bf16 x 6 arithmetic for the REST of a stack as well (opt-in; the five entry points above keep their launches and can
 * reach none of the kernels named here).  The tables are those of _fwd_split / _bwd_split, sized with prcnn_wsplit_bytes, which
 * counts whole 32-wide chunks of the reduction width: the images are zero-padded that far.  Per layer, on top of the layers the
 * two older entry points already take (those keep train_fwd_s_kernel / train_dgrad_s_kernel):
 *   forward, plain rows                 K >= 32, K % 4 == 0, 16-byte aligned rows and prologue tables; any K % 32
 *   forward, layer 0 of a mode-1 (padded or padding-free) or mode-2 source     K >= 32; any C / C2 / C1 and alignment.  a_dump
 *                                       receives exactly the bytes prcnn_train_stack_fwd writes
 *   dgrad                               Nout >= 32; fewer than 2^31 rows
 * (train_fwd_sa_kernel / train_dgrad_sa_kernel; a staged element past the width is +0 by selection and no load reaches past a
 * row's end).  K < 32 / Nout < 32 and everything else run the fp32 kernel of the twin.  ONE launch per call
 * (train_pack_split_all_kernel) writes every split image the call uses -- a grouped layer 0's with the k rotation of its fp32
 * image, its transposed one without the three xyz columns --; wpack / wpack_t are written as in the twin.
 * prcnn_train_stack_bwd_split_all: wgrad_split != 0 runs the wide layers' wgrad as prcnn_train_stack_bwd_wsplit does.
 * Non-finite operands: as for the two older entry points (no recomputation; a row with a non-finite staged value is non-finite in
 * its own row only). */
int prcnn_train_stack_fwd_split_all(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, float* a_dump,
                                    int ld_dump, float* out, int ld_out, int col_off, uint8_t* arg, void* const* wsplit, void* work,
                                    size_t work_bytes, prcnn_stream_t stream);
int prcnn_train_stack_bwd_split_all(const prcnn_train_src_t* src, const prcnn_train_layer_t* layers, int nl, int pool_ns, const float* a_dump,
                                    int ld_dump, const float* gout, int ld_gout, const uint8_t* arg, float* gin, int ld_gin,
                                    void* const* wsplit_t, void* work, size_t work_bytes, prcnn_stream_t stream, int wgrad_split);
/* Padding-free rows for a grouped stack (exact: ball_query pads a group with copies of its first hit; copies are identical rows).
 * prcnn_train_group_rows builds the distinct-row list deterministically (count -> exclusive scan -> fill, group order);
 * prcnn_flat_rows_grad scatters the first layer's row gradients back: dfeat[ridx[r], 0:C] += G[r, 0:C] for the live rows. */
int prcnn_train_group_rows(const int32_t* idx, const float* new_xyz, int B, int N, int M, int ns, int32_t* cnt, int32_t* off,
                           int32_t* rows_dev, int32_t* ridx, float* rnx, float* mult, int32_t* row_grp, prcnn_stream_t stream);
int prcnn_flat_rows_grad(const float* G, int ldG, const int32_t* ridx, const int32_t* rows_dev, int64_t max_rows, int C, float* dfeat,
                         int ld_d, prcnn_stream_t stream);
/* ... as a gather (no atomics, summed in ascending row order): frame b's rows are those of its M groups (seg_off from
 * prcnn_train_group_rows); dfeat is WRITTEN.  Scratch: >= prcnn_flat_rows_grad_work_bytes(B, N, max_rows) device bytes (0: no gather
 * form for this shape); work == NULL / too small: dfeat is cleared and prcnn_flat_rows_grad runs. */
size_t prcnn_flat_rows_grad_work_bytes(int B, int N, int64_t max_rows);
int prcnn_flat_rows_grad_ws(const float* G, int ldG, const int32_t* ridx, const int32_t* rows_dev, int64_t max_rows, int C, float* dfeat,
                            int ld_d, const int32_t* seg_off, int B, int N, int M, void* work, size_t work_bytes, prcnn_stream_t stream);
/* backward of the gathers on channels-last rows: dfeat (B, N, ld_d) += scatter of G ((B, M, ns) rows, C channels) through idx;
 * dknown (B, m, ld_d) += w3-weighted scatter of G ((B, n) rows) through idx3.  Outputs pre-zeroed by the caller. */
int prcnn_group_rows_grad(const float* G, int ldG, const int32_t* idx, int B, int M, int ns, int C, int N, float* dfeat, int ld_d,
                          prcnn_stream_t stream);
int prcnn_interp_rows_grad(const float* G, int ldG, const int32_t* idx3, const float* w3, int B, int n, int m, int C, float* dknown,
                           int ld_d, prcnn_stream_t stream);
/* The same as a gather (no atomics, summed in ascending row order: the result does not depend on scheduling) with a scratch buffer of
 * >= prcnn_interp_rows_grad_work_bytes(B, n, m) device bytes (0: this shape has no gather form).  dknown is WRITTEN, not accumulated
 * into, and need not be zeroed.  work == NULL / too small / rows not 16-byte aligned: dknown is cleared and prcnn_interp_rows_grad runs. */
size_t prcnn_interp_rows_grad_work_bytes(int B, int n, int m);
int prcnn_interp_rows_grad_ws(const float* G, int ldG, const int32_t* idx3, const float* w3, int B, int n, int m, int C, float* dknown,
                              int ld_d, void* work, size_t work_bytes, prcnn_stream_t stream);

/* ======================================================================================================
 * RCNN-stage training targets (csrc/proposal_target.hip) -- `train_rcnn.py --train_mode rcnn`.
 * prcnn_boxes_iou3d: iou3d_utils.boxes_iou3d_gpu (lib/utils/iou3d/iou3d_utils.py:20-53) as one kernel: a (Na,7), b (Nb,7)
 * [x, y(bottom), z, h, w, l, ry] -> out (Na, Nb).
 * prcnn_proposal_target_sample: ProposalTargetLayer.sample_rois_for_rcnn with sample_bg_inds, aug_roi_by_noise_torch and
 * random_aug_box3d (lib/rpn/proposal_target_layer.py:75-300) for the whole batch in one launch, no host round trip:
 *   roi_boxes3d (B, M, 7), gt_boxes3d (B, G, gt_cols >= 7) with all-zero rows padding the end (G <= 128);
 *   cfg6 (HOST pointer, six DOUBLES -- the reference's sampler does its slot arithmetic in Python doubles): RCNN.REG_FG_THRESH, CLS_FG_THRESH, CLS_BG_THRESH, CLS_BG_THRESH_LO, FG_RATIO, HARD_BG_RATIO;
 *   aug_times = RCNN.ROI_FG_AUG_TIMES; aug_method 0 = 'multiple', 1 = 'single' (RCNN.REG_AUG_METHOD);
 *   -> rois, gt_of_rois (B, R, 7), roi_iou (B, R), src (B, R) the input RoI behind every slot, max_overlaps / gt_assignment
 *   (B, M), counts (B, 4) = fg / hard-bg / easy-bg candidates and fg slots, status (B): 0 ok, 1 = neither foreground nor
 *   background candidates (the reference raises NotImplementedError), 2 = no ground-truth box.
 * The random draw is a counter-based table keyed by (seed, purpose, frame, position) -- see the kernel file; the reference's own
 * methods, answered from the same table, return the same boxes (tests/golden/ref_proposal_target.py).
 * ====================================================================================================== */
int prcnn_boxes_iou3d(const float* a, int Na, const float* b, int Nb, float* out, prcnn_stream_t stream);
/* The box trigonometry of roipool3d / iou3d / NMS / labels / RoI sampling is the reference's HOST libm arithmetic, restated bit for
 * bit (csrc/ref_trig.h: glibc 2.35 sinf / cosf / atan2f).  Element-wise evaluation for inspection / tests: fn 0 sinf(a), 1 cosf(a),
 * 2 atan2f(a, b). */
int prcnn_ref_trig(const float* a, const float* b, int n, int fn, float* out, prcnn_stream_t stream);
int prcnn_proposal_target_sample(const float* roi_boxes3d, const float* gt_boxes3d, int B, int M, int G, int gt_cols, int roi_per_image,
                                 const double* cfg6, int aug_times, int aug_method, uint32_t seed, float* rois, float* gt_of_rois,
                                 float* roi_iou, int32_t* src, float* max_overlaps, int32_t* gt_assignment, int32_t* counts,
                                 int32_t* status, prcnn_stream_t stream);

/* ======================================================================================================
 * RoI sampling for RCNN offline training (csrc/rcnn_offline.hip, per-slot arithmetic: csrc/rcnn_offline_math.h) --
 * `train_rcnn.py --train_mode rcnn_offline` with RCNN.ROI_SAMPLE_JIT False.
 * prcnn_rcnn_offline_sample: the sampling part of KittiRCNNDataset.get_rcnn_training_sample_batch
 * (lib/datasets/kitti_rcnn_dataset.py:890-957, sample_bg_inds :1024-1050, aug_roi_by_noise_batch :1052-1077, random_aug_box3d
 * :747-788) for a batch in two launches, no host round trip:
 *   roi_boxes3d (B, M, 7) with num_roi (B), gt_boxes3d (B, G, 7) with num_gt (B): both ragged and COUNTED (M <= 4096, G <= 128);
 *   frame_ids (B) or NULL: the id of every frame in the random table (NULL: its position in the batch);
 *   cfg6 (HOST pointer, six doubles) as for prcnn_proposal_target_sample; aug_times = the attempts on a foreground slot (the
 *   reference's 10; a background slot gets one), aug_method 0 = 'multiple', 1 = 'single';
 *   -> iou3d (B, M, G) kitti_utils.get_iou3d on boxes3d_to_corners3d corners (0 past the counts), rois, gt_of_rois (B, R, 7),
 *   roi_iou (B, R) the noise loop's last IoU, src (B, R) the input RoI behind every slot, max_overlaps / gt_assignment (B, M)
 *   (0 / -1 past num_roi), counts (B, 4) = foreground list length (threshold entries + the labels' best RoIs, duplicates kept) /
 *   hard / easy candidates and foreground slots, status (B): 0 ok, 1 = the reference raises (foreground but no background
 *   candidate, no candidate, no RoI), 2 = no label.  A frame with status != 0 has rois, gt_of_rois, roi_iou cleared and src -1.
 * The random draw is the counter table of csrc/counter_rand.h, streams 40, 42, 43, 50 (see the kernel file). */
int prcnn_rcnn_offline_sample(const float* roi_boxes3d, const int32_t* num_roi, const float* gt_boxes3d, const int32_t* num_gt,
                              const int32_t* frame_ids, int B, int M, int G, int roi_per_image, const double* cfg6, int aug_times,
                              int aug_method, uint32_t seed, float* iou3d, float* rois, float* gt_of_rois, float* roi_iou, int32_t* src,
                              float* max_overlaps, int32_t* gt_assignment, int32_t* counts, int32_t* status, prcnn_stream_t stream);

/* prcnn_rcnn_offline_finish: everything of that method after pooling (:976-1010) in one pass over the pooled tensor
 * (prcnn_roipool3d on the sampled RoIs, enlarged): pooled (B * R, S, ld) with xyz in columns 0:3, REWRITTEN IN PLACE -- per RoI the
 * rotation by the drawn angle, the scale, the flip (data_augmentation stage 2 with mustaug), the shift to the augmented RoI's centre
 * and the rotation by ry mod 2 pi; the other columns are not touched.  rois / gt_of_rois / roi_iou / status: the sampler's outputs;
 * pooled_empty_flag (B, R) from the pooling; cfg5 (HOST, five doubles): REG_FG_THRESH, CLS_FG_THRESH, CLS_BG_THRESH,
 * AUG_METHOD_PROB[2], AUG_ROT_RANGE; aug_methods: mask of 'rotation' 1, 'scaling' 2, 'flip' 4 in AUG_METHOD_LIST, 0 = AUG_DATA off
 * (only the canonical transform and the labels run).  -> out_rois, out_gt_of_rois (B, R, 7) the augmented boxes, gt_boxes3d_ct
 * (B, R, 7), cls_label (B, R) in {-1, 0, 1}, reg_valid_mask (B, R).  A frame with status != 0: its pooled rows (every column) and boxes cleared,
 * label -1, mask 0.  Random streams 51, 52, 53 (csrc/rcnn_offline_math.h). */
int prcnn_rcnn_offline_finish(float* pooled, int ld, int B, int R, int S, const float* rois, const float* gt_of_rois,
                              const float* roi_iou, const int32_t* pooled_empty_flag, const int32_t* status, const int32_t* frame_ids,
                              const double* cfg5, int aug_methods, uint32_t seed, float* out_rois, float* out_gt_of_rois,
                              float* gt_boxes3d_ct, int32_t* cls_label, int32_t* reg_valid_mask, prcnn_stream_t stream);

/* ======================================================================================================
 * RPN training loss and its gradient in one device pass (csrc/rpn_loss.hip, arithmetic: csrc/rpn_loss_math.h) --
 * train_functions.get_rpn_loss for LOSS_CLS = SigmoidFocalLoss with the bin-based box regression of get_reg_loss
 * (get_y_by_bin = get_ry_fine = False; LOC_XZ_FINE either way: C = (4 or 2) * nb + 1 + 2 * num_head_bin + 3 channels per row).
 * Anything else is PRCNN_EUNSUPPORTED: the caller keeps its composed path for it.
 *   rpn_cls: row r's logit at rpn_cls[r * ld_cls]; rpn_reg: row r's C predictions at rpn_reg + r * ld_reg (16-byte units when
 *   the pointer and ld_reg allow it); cls_label (npts) i32 or i64 (label_is_i64), > 0 foreground, 0 background, < 0 ignored;
 *   reg_label (npts, 7) [dx dy dz h w l ry].  A row that is not foreground never has its rpn_reg row read.
 *   prcnn_rpn_loss_counts  -> counts (4) i32 {pos, valid, fg = pos, 0} of THIS process and norm (2) f32 = {1 / max(pos, 1), 1}.
 *                             Data-parallel callers all-reduce the counts and overwrite norm with
 *                             {world / max(pos_global, 1), world * fg_local / max(fg_global, 1)}; counts stay local.
 *   prcnn_rpn_loss_forward -> terms (9) f32: loss, loss_cls, loss_reg, loss_loc, loss_angle, loss_size (3 x the mean, as the
 *                             reference), cls_pos, cls_neg, fg_sum.  Per-workgroup partial sums are doubles, added in a fixed order.
 *   prcnn_rpn_loss_backward-> dcls (npts) and dreg (npts, C) contiguous = grad_out[0] * d loss / d input, every entry written
 *                             exactly once (zeros for the rows that carry no term); grad_out is a device scalar.
 * work: >= prcnn_rpn_loss_workspace_bytes(npts) device bytes, 8-byte aligned.  Results depend on the flat row order only.
 * ====================================================================================================== */
typedef struct prcnn_rpn_loss_cfg {
    double loc_scope, loc_bin_size; /* RPN.LOC_SCOPE, LOC_BIN_SIZE: nb = int(scope / bin_size) * 2 */
    double mean_size[3];            /* CLS_MEAN_SIZE h w l */
    double gamma, alpha;            /* focal loss; has_alpha 0: alpha is None */
    double loss_weight[2];          /* RPN.LOSS_WEIGHT */
    int num_head_bin, xz_fine, y_by_bin, ry_fine;
    int loss_cls;                   /* 0 SigmoidFocalLoss, 1 DiceLoss, 2 BinaryCrossEntropy (1 and 2: the *_kind exports only) */
    int has_alpha;
} prcnn_rpn_loss_cfg_t;
size_t prcnn_rpn_loss_workspace_bytes(int64_t npts);
int prcnn_rpn_loss_counts(const void* cls_label, int label_is_i64, int64_t npts, int32_t* counts, float* norm, void* work,
                          size_t work_bytes, prcnn_stream_t stream);
int prcnn_rpn_loss_forward(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                           int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                           const int32_t* counts, const float* norm, float* terms, void* work, size_t work_bytes, prcnn_stream_t stream);
int prcnn_rpn_loss_backward(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                            int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                            const int32_t* counts, const float* norm, const float* grad_out, float* dcls, float* dreg,
                            prcnn_stream_t stream);
/* All three RPN.LOSS_CLS kinds (cfg->loss_cls 0 SigmoidFocalLoss, 1 DiceLoss, 2 BinaryCrossEntropy); the three exports above keep
 * answering PRCNN_EUNSUPPORTED for 1 and 2.  Arguments as above, and:
 *   cls_sums  DiceLoss: the two doubles {A = sum min(p, t), B = sum max(p, t)} over the valid rows that prcnn_rpn_loss_cls_sums writes
 *             (work as above; per-workgroup partials in double, added in a fixed order).  The loss is 1 - A / max(B, 1).  A
 *             data-parallel caller all-reduces the two doubles in place between that call and the next two and passes
 *             norm[0] = world: the value is the global loss, the gradient this rank's share x world.  NULL for the other kinds.
 *   fg_weight BinaryCrossEntropy: RPN.FG_WEIGHT, the weight of a foreground row (rounded to float32 once); ignored otherwise.
 *             norm[0] scales the sum of the valid rows' terms: 1 / max(valid, 1), data-parallel world / max(valid_global, 1).
 *   norm      may be NULL for DiceLoss and BinaryCrossEntropy: the single-process normalisers {1 | 1 / max(counts[1], 1), 1},
 *             read from counts on the device.  (prcnn_rpn_loss_counts writes SigmoidFocalLoss's.)
 * terms[6] and terms[7] (cls_pos, cls_neg) are 0 for DiceLoss and BinaryCrossEntropy.  For loss_cls 0 these are the launches of
 * prcnn_rpn_loss_forward / _backward. */
int prcnn_rpn_loss_cls_sums(const float* rpn_cls, int64_t ld_cls, const void* cls_label, int label_is_i64, int64_t npts, double* cls_sums,
                            void* work, size_t work_bytes, prcnn_stream_t stream);
int prcnn_rpn_loss_forward_kind(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                                int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                                const int32_t* counts, const float* norm, float* terms, void* work, size_t work_bytes,
                                const double* cls_sums, double fg_weight, prcnn_stream_t stream);
int prcnn_rpn_loss_backward_kind(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                                 int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                                 const int32_t* counts, const float* norm, const float* grad_out, float* dcls, float* dreg,
                                 const double* cls_sums, double fg_weight, prcnn_stream_t stream);

/* ======================================================================================================
 * RCNN training loss and its gradient in device passes (csrc/rcnn_loss.hip, arithmetic: csrc/rcnn_loss_math.h) --
 * train_functions.get_rcnn_loss for LOSS_CLS = BinaryCrossEntropy or SigmoidFocalLoss with get_reg_loss(get_xz_fine = True,
 * get_ry_fine = True), LOC_Y_BY_BIN and SIZE_RES_ON_ROI either way: C = 4 * nb + (2 * nby | 1) + 2 * num_head_bin + 3 channels per
 * row, any C up to 56 (no alignment of the rows is assumed), 1 <= npts <= 2^24.  Anything else is PRCNN_EUNSUPPORTED: the caller keeps
 * its composed path for it.
 *   rcnn_cls: row r's logit at rcnn_cls[r * ld_cls]; rcnn_reg: row r's C predictions at rcnn_reg + r * ld_reg; cls_label (npts) i32 or
 *   i64, > 0 positive, 0 negative, < 0 ignored (its logit is not read); reg_valid_mask (npts) i32 or i64 in {0, 1}, 1: the row is regressed --
 *   independent of the label; a row whose mask is <= 0 never has its rcnn_reg row or its targets read; roi_boxes3d (npts, 7): columns
 *   3..5 are the size anchor under size_res_on_roi (else unused, may be null); gt_of_rois (npts, 7) [dx dy dz h w l ry].
 *   prcnn_rcnn_loss_forward -> counts (4) i32 {#(label > 0), #(label >= 0), #(mask > 0), sum of mask (32-bit)} of THIS process, and the
 *                              per-workgroup unnormalised sums (doubles, fixed order) in work.  finalize != 0: also terms, with the
 *                              single-process normalisers (one launch up to 256 rows, two beyond).
 *   prcnn_rcnn_loss_finalize-> terms from work and counts; norm null: single process; else (2) f32 device
 *                              {classification scale, regression scale}: data-parallel callers run the forward with finalize = 0,
 *                              all-reduce the counts and pass {world / max(pos_global | valid_global, 1), world * fg / max(fg_global, 1)}.
 *   terms (23) f32: loss, loss_cls, loss_reg, loss_loc, loss_angle, loss_size (3 x the mean; these three carry the regression scale),
 *                   cls_pos, cls_neg (focal), the eight per-head means x_bin z_bin x_res z_res y_offset|y_bin y_res ry_bin ry_res,
 *                   unscaled loc, angle and size mean, then the four counts.
 *   prcnn_rcnn_loss_backward-> dcls (npts) and dreg (npts, C) contiguous = grad_out[0] * d loss / d input, one launch, every entry
 *                              written exactly once (zeros where no term is carried); grad_out is a device scalar; counts as the
 *                              forward wrote them, norm as given to finalize (or null).
 * work: >= prcnn_rcnn_loss_workspace_bytes(npts) device bytes, 8-byte aligned.  Results depend on the flat row order only.
 * ====================================================================================================== */
typedef struct prcnn_rcnn_loss_cfg {
    double loc_scope, loc_bin_size;     /* RCNN.LOC_SCOPE, LOC_BIN_SIZE: nb = int(scope / bin_size) * 2 */
    double loc_y_scope, loc_y_bin_size; /* RCNN.LOC_Y_SCOPE, LOC_Y_BIN_SIZE (read under y_by_bin) */
    double mean_size[3];                /* CLS_MEAN_SIZE h w l (the anchor without size_res_on_roi) */
    double gamma, alpha;                /* focal loss; has_alpha 0: alpha is None */
    int num_head_bin, y_by_bin, size_res_on_roi;
    int loss_cls;                       /* 0 SigmoidFocalLoss, 2 BinaryCrossEntropy (ops.rpn_loss_cfg's numbering) */
    int has_alpha;
} prcnn_rcnn_loss_cfg_t;
size_t prcnn_rcnn_loss_workspace_bytes(int64_t npts);
int prcnn_rcnn_loss_forward(const float* rcnn_cls, int64_t ld_cls, const float* rcnn_reg, int64_t ld_reg, const void* cls_label,
                            int label_is_i64, const void* reg_valid_mask, int mask_is_i64, const float* roi_boxes3d,
                            const float* gt_of_rois, int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, int finalize,
                            int32_t* counts, float* terms, void* work, size_t work_bytes, prcnn_stream_t stream);
int prcnn_rcnn_loss_finalize(int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, const int32_t* counts, const float* norm,
                             float* terms, const void* work, size_t work_bytes, prcnn_stream_t stream);
int prcnn_rcnn_loss_backward(const float* rcnn_cls, int64_t ld_cls, const float* rcnn_reg, int64_t ld_reg, const void* cls_label,
                             int label_is_i64, const void* reg_valid_mask, int mask_is_i64, const float* roi_boxes3d,
                             const float* gt_of_rois, int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, const int32_t* counts,
                             const float* norm, const float* grad_out, float* dcls, float* dreg, prcnn_stream_t stream);

/* ======================================================================================================
 * Evaluation statistics on the device (csrc/eval_stats.hip, per-item arithmetic: csrc/eval_stats_math.h) -- what the three loops of
 * tools/eval_rcnn.py report next to the AP: eval_one_epoch_rpn (:171-202), eval_one_epoch_rcnn (:336-364), eval_one_epoch_joint
 * (:539-573).  Two launches per batch, nothing is read on the host, both capturable in a hipGraph as a plain chain.
 * prcnn_eval_gt_max_iou: `iou3d_utils.boxes_iou3d_gpu(boxes[k], gt[k]).max(dim=0)` (:190-191, :339-349, :551-563) for every frame of S box
 * sets in one launch:
 *   boxes0, boxes1 (B, M, 7): S = 1 reads boxes0 (the RoIs), S = 2 also boxes1 (the decoded boxes); M >= 1;
 *   gt_boxes3d (B, G, gt_cols >= 7), 1 <= G <= 128, columns 0..6 [x y z h w l ry]; trailing rows whose float32 sum over all gt_cols
 *   columns, added in column order, is 0 are dropped, as prcnn_proposal_target_sample drops them; trim_mode 0 (:541-548, joint / rcnn):
 *   nothing may remain; trim_mode 1 (:183-186, rpn): the loop stops at k > 0, row 0 always stays -- an all-zero row 0 is a ground-truth
 *   box that is counted and never recalled;
 *   -> gt_max (S, B, G): the column maximum of the IoU matrix (the arithmetic of prcnn_boxes_iou3d bit for bit, every pair through the
 *   full clip), NaN when any IoU of the column is NaN (torch.max), -1 for rows >= num_gt[b]; num_gt (B) the live rows.
 * prcnn_eval_stats_accumulate: adds one batch into the caller's state -- PRCNN_EVAL_STATS_STATE_BYTES device bytes, 8-byte aligned:
 * int64 counters[16] then double sums[4]; zeroed by the caller to reset.  One workgroup in stream order is the only writer, the double
 * sums are added in the reference's order: two runs give identical bytes.
 *   counters [0..4] ground-truth boxes recalled by set 0 at float32(0.1, 0.3, 0.5, 0.7, 0.9): gt_max > thresh in float32, as torch casts
 *            the Python scalar (float32(0.1) itself is not recalled at 0.1; NaN never is); [5..9] the same for set 1; [10] live
 *            ground-truth boxes; [11] detections (det_num (B) i32 or NULL, the `num` of the NMS select); [12] frames; [13] batches.
 *   sums [0] segmentation IoU (:198-202, :568-573): seg (B, N) f32 0 / 1 and cls_label (B, N) i32 or i64, both or neither; per frame
 *            (seg_mode 0, rpn) or per batch (seg_mode 1, joint) correct = #(seg == label and label > 0), union = #(label > 0) +
 *            #(seg > 0) - correct, float32(correct) / max(float32(union), 1), widened to double.  seg_mode 1 adds the batch's ratio
 *            B times: the reference computes it inside its `for k in range(batch_size)` loop.
 *        [1], [2] RCNN classification accuracy (:355-364): pred_class (B, R) u8 0 / 1 (sigmoid(rcnn_cls) > SCORE_THRESH, formed by the
 *            caller) and gt_iou (B, R), both or neither; per frame label = gt_iou > cls_fg, valid = gt_iou >= cls_fg or gt_iou <= cls_bg,
 *            acc = sum((pred == label) * valid) / max(sum(valid), 1), acc_refined = #(pred == (gt_iou >= refine_thresh)) / max(R, 1).
 *   S = 0 or G = 0: no recall part (gt_max / num_gt may be NULL).
 * prcnn_eval_stats_workspace_bytes: bytes of gt_max (S, B, G) f32 followed by num_gt (B) i32, rounded up to 8.
 * ====================================================================================================== */
#define PRCNN_EVAL_STATS_STATE_BYTES 160
size_t prcnn_eval_stats_workspace_bytes(int S, int B, int G);
int prcnn_eval_gt_max_iou(const float* boxes0, const float* boxes1, int S, int B, int M, const float* gt_boxes3d, int G, int gt_cols,
                          int trim_mode, float* gt_max, int32_t* num_gt, prcnn_stream_t stream);
int prcnn_eval_stats_accumulate(const float* gt_max, const int32_t* num_gt, int S, int B, int G, const int32_t* det_num,
                                const float* seg, const void* cls_label, int label_is_i64, int64_t N, int seg_mode,
                                const uint8_t* pred_class, const float* gt_iou, int R, float cls_fg, float cls_bg, float refine_thresh,
                                void* state, prcnn_stream_t stream);

/* ======================================================================================================
 * adam_onecycle parameter update (csrc/optim.hip, per-element arithmetic: csrc/optim_math.h) -- gradient-norm clip, decoupled
 * weight decay and the Adam step over ALL parameter tensors in two launches (pointrcnn_amd/optim.py OneCycleAdam).
 * Both calls walk two DEVICE-resident tables the caller builds and keeps: `tensors`, one row per parameter tensor (float32,
 * contiguous; grad null: the tensor receives the decay alone, its moments are not touched and it adds nothing to the norm),
 * and `chunks`, one row per run of at most PRCNN_OPTIM_CHUNK consecutive elements of one tensor (first a multiple of
 * PRCNN_OPTIM_CHUNK, first < numel), covering every element of every tensor exactly once.  One workgroup per chunk.
 *   prcnn_optim_grad_norm -> partial (num_chunks) f64: the sum of grad^2 over each chunk, added in a fixed order; every slot
 *                            is written, no atomics: the same state gives the same bytes.
 *   prcnn_optim_step      -> coef null: every workgroup adds the partials in a fixed order, norm = float(sqrt(sum)),
 *                            coef = min(max_norm / (norm + 1e-6), 1) in float32, {norm, coef} written to state (2) f32;
 *                            coef given (a device float): it is used as it is, partial / state / max_norm are not read.
 *                            Then per element, each operation rounded to float32: g = grad * coef; param *= decay;
 *                            exp_avg += one_minus_beta1 * (g - exp_avg); exp_avg_sq = exp_avg_sq * beta2 + one_minus_beta2 * (g * g);
 *                            param += neg_step * (exp_avg / (sqrt(exp_avg_sq) / bias2_sqrt + eps)).  grad is never written.
 * The scalars are the caller's (double arithmetic rounded to float once; optim.py adam_scalars).  Nothing is read back.
 * ====================================================================================================== */
#define PRCNN_OPTIM_CHUNK 4096
typedef struct prcnn_optim_tensor {
    float* param;
    const float* grad;          /* null: decay only */
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} prcnn_optim_tensor_t;
typedef struct prcnn_optim_chunk {
    int64_t tensor, first;      /* row of `tensors`, first element of the chunk */
} prcnn_optim_chunk_t;
size_t prcnn_optim_chunk_elems(void);
int prcnn_optim_grad_norm(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks, double* partial,
                          prcnn_stream_t stream);
int prcnn_optim_step(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks, const double* partial,
                     float max_norm, const float* coef, float* state, float decay, float one_minus_beta1, float beta2,
                     float one_minus_beta2, float bias2_sqrt, float eps, float neg_step, prcnn_stream_t stream);

/* TRAIN.OPTIMIZER adam and sgd (pointrcnn_amd/optim.py ClipAdam / ClipSGD): the same tables, partial sums, coefficient and {norm, coef}
 * state as prcnn_optim_step, after the same prcnn_optim_grad_norm launch.  A tensor whose grad is null is not touched at all.
 *   prcnn_optim_step_adam  torch.optim.Adam with L2 decay: g = grad * coef; with weight_decay != 0, g = g + weight_decay * param;
 *                          exp_avg, exp_avg_sq and the parameter step as in prcnn_optim_step (no decoupled decay).
 *   prcnn_optim_step_sgd   torch.optim.SGD: g as above; exp_avg = exp_avg * momentum + g; param += neg_lr * exp_avg.  The momentum
 *                          buffer is the row's exp_avg (exp_avg_sq is not read); with momentum == 0 neither is: param += neg_lr * g.
 *                          No dampening, no Nesterov. */
int prcnn_optim_step_adam(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks,
                          const double* partial, float max_norm, const float* coef, float* state, float weight_decay,
                          float one_minus_beta1, float beta2, float one_minus_beta2, float bias2_sqrt, float eps, float neg_step,
                          prcnn_stream_t stream);
int prcnn_optim_step_sgd(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks, const double* partial,
                         float max_norm, const float* coef, float* state, float weight_decay, float momentum, float neg_lr,
                         prcnn_stream_t stream);

/* ======================================================================================================
 * Tail of a training head on channels-last rows (csrc/head_tail.hip, the mask: csrc/head_tail_math.h) -- Dropout keyed by a counter
 * and the output layer, forward and backward (pointnet2 pytorch_utils._HeadTail, switch PRCNN_HEAD_TAIL).
 *   keep(r, k) = scene_u01f(scene_rand(seed, stream_id, call, r * K + k)) >= p,  scale = 1.0f / (1.0f - p),
 *   drop(x)[r, k] = keep ? x[r, k] * scale : 0.  The dropped entry is SELECTED to zero: an Inf / NaN there contributes nothing.
 *   p == 0 keeps everything with scale 1: the tail is then the plain linear layer.
 * Domain: float32; K % 32 == 0, 32 <= K <= 256; 1 <= N <= 96; R >= 1; R * K <= 2^32; 0 <= p < 1; x (R, K) and w (N, K) contiguous
 * and 16-byte aligned.  Anything else: PRCNN_EINVAL, nothing is launched (prcnn_head_tail_work_bytes: 0).
 *   prcnn_head_tail_fwd         out (R, N) = drop(x) w^T + b (b null: no bias).  fp32 MFMA; the K order of a sum depends on (K, N)
 *                               alone: a row's output bits depend on r, its own row and the weights, not on R.
 *   prcnn_head_tail_work_bytes  bytes of the backward's workspace: one (N K + N) float tile per 512 rows.  Never cleared by anyone.
 *   prcnn_head_tail_bwd         g (R, N) with row stride ldg >= N floats (any alignment; columns past N are not read).  One pass over
 *                               x and g writes gx (R, K) = keep ? scale * (g w) : 0 -- exactly zero at every dropped entry -- and
 *                               per-workgroup partial tiles of gw (N, K) = g^T drop(x) and gb (N) = the column sums of g; a second
 *                               launch adds the partials in a fixed order.  Every output element is written exactly once, no
 *                               atomics, no memset: the same state gives the same bytes.  gx, gw, gb may each be null and its work
 *                               is skipped (all null: nothing is launched); work is needed for gw or gb, x for gw, w for gx.
 *   prcnn_dropout_rows          out (R, K) = drop(x); K % 4 == 0 suffices here.  Backward is the same call on the gradient.
 * No host synchronisation, no allocation.
 * ====================================================================================================== */
int prcnn_head_tail_fwd(const float* x, const float* w, const float* b, float* out, int64_t R, int K, int N, uint32_t seed,
                        uint32_t stream_id, uint32_t call, float p, prcnn_stream_t stream);
size_t prcnn_head_tail_work_bytes(int64_t R, int K, int N);
int prcnn_head_tail_bwd(const float* x, const float* w, const float* g, int64_t ldg, float* gx, float* gw, float* gb, void* work,
                        size_t work_bytes, int64_t R, int K, int N, uint32_t seed, uint32_t stream_id, uint32_t call, float p,
                        prcnn_stream_t stream);
int prcnn_dropout_rows(const float* x, float* out, int64_t R, int K, uint32_t seed, uint32_t stream_id, uint32_t call, float p,
                       prcnn_stream_t stream);

/* ======================================================================================================
 * KITTI result files formatted on the device (csrc/kitti_text.hip, per-box arithmetic and the "%.4f" conversion:
 * csrc/kitti_text_math.h; pointrcnn_amd/kitti_output.py DeviceResultWriter) -- tools/eval_rcnn.py:69-94 save_kitti_format for a
 * whole batch in one launch.  boxes (B,M,7) f32 [x, y, z, h, w, l, ry], scores (B,M) f32; candidate j < num[b] of frame b is box
 * keep[b,j] (keep null: box j; num null: all M); P2 (B,12) f64 the 3x4 projections row-major, img_hw (B,2) i32 [H, W];
 * class_name 1..15 bytes.  Per candidate: float32 corners (ref_trig cosf / sinf), float64 projection, min / max over the corners
 * with numpy's NaN rule, clip to the image, kept iff (x2-x1) < W*0.8 and (y2-y1) < H*0.8; alpha in float32 from ref_trig atan2f.
 *   text     (B, M * PRCNN_KITTI_LINE_MAX) u8: the kept candidates' lines "<class> -1 -1" + 13 x " %.4f" + "\n" [alpha, x1 y1 x2 y2,
 *            h w l, x y z, ry, score] in j order, packed from offset 0; text_len (B) i32 their bytes.  The digits are printf's:
 *            the exact binary value rounded to four decimals, ties to even, "-" whenever the sign bit is set.
 *   status   (B) i32: 0; 1 = a printed field of a kept box is not finite or not below 2^31 in magnitude (format the frame on the
 *            host); 2 = num[b] outside [0, M] or a keep index outside [0, M) (nothing is read through it).  status != 0 comes with
 *            text_len 0, and the frame's text bytes then mean nothing.
 *   rows     (B,M,13) f64 | null: the 13 values of candidate j; valid (B,M) u8 | null: the size test's flag.  Zeros past num.
 * One launch, one workgroup per frame, no workspace, no host synchronisation, no allocation.  B == 0 or M == 0: nothing to do.
 * ====================================================================================================== */
#define PRCNN_KITTI_LINE_MAX 256
int prcnn_kitti_result_text(const float* boxes, const float* scores, const int32_t* keep, const int32_t* num, int B, int M,
                            const double* P2, const int32_t* img_hw, const char* class_name, uint8_t* text, int32_t* text_len,
                            int32_t* status, double* rows, uint8_t* valid, prcnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PRCNN_POINTOPS_H */
