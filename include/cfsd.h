/*
 * cfsd.h — C ABI of libcfsd.so, the MI355X (gfx950) kernels of the
 * spiral-convolution mesh-VAE training step (CraniofacialSD-VAE).
 *
 * The reference has no FFI: its hot path is the Python module API of
 * model.py / swap_batch_transform.py / model_manager.py running on ATen and
 * torch-scatter.  Each entry point below names the reference interface whose
 * arithmetic it replaces (path:line in simofoti/CraniofacialSD-VAE).
 *
 * Conventions (all entry points):
 *  - every pointer is a DEVICE pointer owned by the caller; the library never
 *    allocates device memory (workspaces are passed in);
 *  - tensors are dense row-major fp32, activations [batch, vertices, channels];
 *    index tables are int32;
 *  - launches are asynchronous on `stream` (a hipStream_t, may be NULL for the
 *    default stream) with no host synchronisation, so calls can be captured
 *    into a hipGraph;
 *  - the return value is CFSD_OK (0), a negative CFSD_E* code for invalid
 *    arguments, or a positive hipError_t; cfsd_last_error_string() gives text
 *    (per calling thread).  Nothing aborts and no C++ exception crosses the ABI.
 *  - stateless and re-entrant.
 */
#ifndef CFSD_H
#define CFSD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFSD_OK 0
#define CFSD_EINVAL (-1)      /* bad shape / null pointer / unsupported size */
#define CFSD_EWORKSPACE (-2)  /* workspace too small */

#define CFSD_ACT_NONE 0
#define CFSD_ACT_ELU 1

/* Storage type of an activation / gradient operand of the mixed-precision
 * (bf16) entry points: fp32, or bfloat16 as raw uint16 (torch.bfloat16 bits). */
#define CFSD_DT_F32 0
#define CFSD_DT_BF16 1
/* Storage flag OR-ed into a *_dt argument of the mixed-precision entry points
 * (ABI 4.0): the operand is VERTEX-MAJOR.  A logical [batch, nv, c] tensor
 * then has element (b, v, k) at ((size_t)v * batch + b) * c + k, so the rows
 * of one vertex in every mesh of the batch are one contiguous block (torch:
 * an empty [nv, batch, c] tensor viewed through .permute(1, 0, 2)).  Without
 * the flag: batch-major, (b * nv + v) * c + k (the reference's [B, V, C]).
 * Each operand's layout is independent (e.g. E1 reads a vertex-major level-1
 * tensor and writes a batch-major level-2 one); results do not depend on the
 * layout.  Where one descriptor covers several operands, the entry point says
 * so. */
#define CFSD_VM 0x10
#define CFSD_DT_TYPE(dt) ((dt) & 0xf)

/* ABI version: (major << 16) | minor. */
int cfsd_version(void);
const char* cfsd_last_error_string(void);

/* ---------------------------------------------------------------- SpiralConv
 * Replaces SpiralConv.forward (model.py:27-41) + F.elu (model.py:68,84):
 *   y[b,r,o] = act( bias[o] + sum_{s,c} w[o, s*cin + c] * x[b, idx[r*seq+s], c] )
 * x [batch, vsrc, cin], idx [rows, seq] (values in [0, vsrc)), w [cout, seq*cin],
 * y [batch, rows, cout].  `rows` may be a subset of the mesh's vertices (the
 * Enblock evaluates the conv only where the 0/1 down-sample selects, which is
 * bit-identical to conv -> Pool(down) for a selection transform). */
int cfsd_spiral_conv_fwd(const float* x, const int32_t* idx, const float* w, const float* bias,
                         float* y, float* workspace, size_t workspace_bytes, int batch, int vsrc,
                         int rows, int seq, int cin, int cout, int act, void* stream);

/* Workspace (bytes) that lets cfsd_spiral_conv_fwd / _bwd_data split the
 * spiral slots of layers with few rows over more workgroups (partial sums
 * combined in a fixed order).  NULL/0 workspace is allowed for 32-channel
 * layers (no split); 64x64 layers require it. */
size_t cfsd_spiral_conv_workspace(int batch, int vsrc, int rows, int seq, int cin, int cout);

/* Replaces the autograd of model.py:34 (IndexSelectBackward = index_add_) and
 * :40 (AddmmBackward dX = dY.W), deterministically (no atomics):
 *   dx[b,u,c] = g(b,u,c) * sum_{(r,s): idx[r,s]=u} sum_o dpre[b,r,o] w[o, s*cin+c]
 * where g = elu'(elu_y[b,u,c]) computed from the ELU output when elu_y != NULL
 * (fuses the previous layer's ELU backward), else 1.
 * inv_ptr [vsrc*seq + 1] / inv_row [rows*seq]: CSR of the inverse spiral,
 * entry list of (u, s) = rows r with idx[r*seq+s] == u (r ascending);
 * inv_head [vsrc*seq][CFSD_INV_HEAD]: the first four entries of each list (-1
 * if absent, 16-B aligned rows), read up front with one load per key so the
 * gathers are issued without walking the CSR (required; inv_ptr/inv_row are
 * only read for lists longer than the head).  The spiral length must be 9
 * (all reference configs). */
#define CFSD_INV_HEAD 4
int cfsd_spiral_conv_bwd_data(const float* dpre, const int32_t* inv_ptr, const int32_t* inv_row,
                              const int32_t* inv_head, const float* w, const float* elu_y,
                              float* dx, float* workspace, size_t workspace_bytes, int batch,
                              int vsrc, int rows, int seq, int cin, int cout, void* stream);

/* Replaces AddmmBackward's dW = G^T.dY and db = sum dY (model.py:40):
 *   dw[o, s*cin+c] = sum_{b,r} dpre[b,r,o] x[b, idx[r,s], c],  db[o] = sum_{b,r} dpre[b,r,o]
 * Deterministic two-stage reduction through `workspace`
 * (cfsd_spiral_conv_bwd_weight_workspace() bytes). */
int cfsd_spiral_conv_bwd_weight(const float* x, const int32_t* idx, const float* dpre, float* dw,
                                float* db, float* workspace, size_t workspace_bytes, int batch,
                                int vsrc, int rows, int seq, int cin, int cout, void* stream);
size_t cfsd_spiral_conv_bwd_weight_workspace(int batch, int rows, int seq, int cin, int cout);

/* Deferred weight gradients.  cfsd_spiral_conv_bwd_weight / cfsd_spiral_conv_bwd
 * called with dw == db == NULL leave their per-workgroup partial sums in
 * `workspace` and skip the reduction; cfsd_dw_reduce_batch then reduces up
 * to CFSD_DW_REDUCE_MAX such layers (each with its own workspace) in ONE
 * launch, with the same fixed summation order (identical results).
 *
 * The slabs' layout is a function of (fused, batch, vsrc, rows, cin, cout)
 * alone; the library derives it in one place, for the producing launch, its
 * workspace query and both reduces.  `fused` is one of the CFSD_DW_* codes.
 * Two layouts exist.  UNIT slabs (32/64 -> 32/64 channels, fp32 kernels): per
 * slab 9*(cin/32)*(cout/32) units of 1024 floats, the db partials of all
 * slabs behind the last unit.  PLAIN slabs: per slab [cout x 9 cin | cout]
 * floats.  What a code selects:
 *   CFSD_DW_PLAIN  the fp32 weight-gradient kernels' slabs: unit slabs for
 *                  32/64 -> 32/64 channels (few-row kernel below 65536 =
 *                  batch x rows, persistent kernel from there), plain slabs
 *                  for the xyz input (cin <= 4) and output (cout <= 4) layers.
 *                  Left by cfsd_spiral_conv_bwd_weight, and by
 *                  cfsd_spiral_conv_bwd_weight_x on the xyz input layer or
 *                  on fp32 x (but see CFSD_DW_VM32).
 *   CFSD_DW_FUSED  a dx + dW call.  For a small-output layer (cout*seq <= 32,
 *                  cin 32/64) the fused kernel's own plain slabs, counted
 *                  from batch x vsrc: cfsd_spiral_conv_bwd, _bwd_x,
 *                  _bwd_out_flat.  For every other shape the same as
 *                  CFSD_DW_PLAIN: cfsd_spiral_conv_bwd, _bwd_rowsub(_x).
 *   CFSD_DW_BF16   32/64 -> 32/64 channels: the bf16 MFMA kernels' plain
 *                  slabs.  Left by cfsd_spiral_conv_bwd_weight_x on bf16 x
 *                  and by the two *_pair_bf16 calls.  Any other shape: as
 *                  CFSD_DW_FUSED.
 *   CFSD_DW_VM32   32 -> 32, batch % 16 == 0, batch x rows >= 65536: the
 *                  vertex-major fp32 kernel's unit slabs (its own count).
 *                  Left by cfsd_spiral_conv_bwd_weight_x with fp32
 *                  vertex-major x and dpre (ABI 4.3) and by
 *                  cfsd_spiral_conv_bwd_flat_pair (ABI 4.10).  Any other
 *                  shape: as CFSD_DW_FUSED.
 * cfsd_spiral_conv_bwd_weight_x is the one entry point whose code depends on
 * its operands: cfsd_spiral_conv_bwd_weight_x_slabs() below returns it. */
#define CFSD_DW_REDUCE_MAX 16
#define CFSD_DW_PLAIN 0
#define CFSD_DW_FUSED 1
#define CFSD_DW_BF16 2
#define CFSD_DW_VM32 3
typedef struct {
  const float* workspace;
  float* dw;
  float* db;
  int batch, vsrc, rows, cin, cout, fused;
} cfsd_dw_slabs;
int cfsd_dw_reduce_batch(const cfsd_dw_slabs* items, int n, void* stream);
/* cfsd_dw_reduce_batch fused with the Adam step of cfsd_adam (single-process
 * training, model_manager.py:316 after :315's backward): every item's dw/db
 * must lie inside the flat gradient `grad` [n_params]; each reduced element
 * is written to grad and updated in param / exp_avg / exp_avg_sq (and
 * param_bf16) by the thread that reduced it, every other element of the flat
 * buffers by extra workgroups of the same launch.  Same values as
 * cfsd_dw_reduce_batch followed by cfsd_adam. */
int cfsd_dw_reduce_batch_adam(const cfsd_dw_slabs* items, int n, float* param, const float* grad,
                              float* exp_avg, float* exp_avg_sq, const int32_t* step,
                              size_t n_params, float lr, float beta1, float beta2, float eps,
                              float weight_decay, uint16_t* param_bf16, void* stream);

/* Fused backward of one SpiralConv (model.py:27-41 autograd, dX and dW/db of
 * the same layer in one call): dx exactly as cfsd_spiral_conv_bwd_data
 * (skipped when dx == NULL, e.g. the first layer), dw/db exactly as
 * cfsd_spiral_conv_bwd_weight.  For small-output layers (cout*seq <= 32, the
 * xyz output conv) both come from ONE pass in source-row space: the spiral
 * transpose is folded in the 3-wide dpre space and dW is regrouped as
 * sum_{b,u} x[b,u,:] (x) t[b,u,s,:], so x is read densely, not gathered.
 * For coarse layers where cfsd_spiral_conv_bwd_paired() is 1, dx and the dW
 * slabs come from ONE launch whose workgroups interleave the two (same
 * results as the separate calls).
 * workspace: cfsd_spiral_conv_bwd_workspace() bytes (shared by both stages). */
int cfsd_spiral_conv_bwd(const float* x, const int32_t* idx, const float* dpre,
                         const int32_t* inv_ptr, const int32_t* inv_row, const int32_t* inv_head,
                         const float* w, const float* elu_y, float* dx, float* dw, float* db,
                         float* workspace, size_t workspace_bytes, int batch, int vsrc, int rows,
                         int seq, int cin, int cout, void* stream);
size_t cfsd_spiral_conv_bwd_workspace(int batch, int vsrc, int rows, int seq, int cin, int cout);
/* 1 when cfsd_spiral_conv_bwd with dx != NULL runs dx and dW as one paired
 * launch for this shape (no reference counterpart: a scheduling query). */
int cfsd_spiral_conv_bwd_paired(int batch, int vsrc, int rows, int seq, int cin, int cout);

/* Backward (dx and dW/db) of a conv evaluated on a ROW SUBSET (the Enblock
 * convs: `rows` = the kept vertices), in the reference's own two steps
 * (autograd of model.py:40 then :34): dG = dpre.W at the kept rows only
 * (MFMA, in the workspace), then dx[b,u,:] = g(b,u,:) * sum_{p in flat(u)}
 * dG[b, p, :] with flat(u) = the flattened spiral positions p = r*seq + s
 * having idx[r,s] == u, in ascending p (the sequential index_add_ order).
 * inv_flat [vsrc][flat_width] int32, -1 padded, 16-B aligned rows,
 * flat_width in {4, 8, 12, 16} (>= the largest fan-in).  dw/db exactly as
 * cfsd_spiral_conv_bwd_weight (dw == db == NULL defers: cfsd_dw_reduce_batch
 * item with fused = CFSD_DW_FUSED).  cin = 32, cout in {32, 64}.
 * workspace: cfsd_spiral_conv_bwd_rowsub_workspace() bytes (0 = unsupported). */
size_t cfsd_spiral_conv_bwd_rowsub_workspace(int batch, int vsrc, int rows, int seq, int cin,
                                             int cout);
int cfsd_spiral_conv_bwd_rowsub(const float* x, const int32_t* idx, const float* dpre,
                                const int32_t* inv_flat, int flat_width, const float* w,
                                const float* elu_y, float* dx, float* dw, float* db,
                                float* workspace, size_t workspace_bytes, int batch, int vsrc,
                                int rows, int seq, int cin, int cout, void* stream);
/* The feature swap (cfsd_swap_features_x: x = the swapped batch of bs^2
 * meshes from the resident set `data` [n_meshes][vsrc][3], in x_dt's layout)
 * and the first Enblock's xyz conv (cfsd_spiral_conv_fwd_x with cin = 3:
 * y = act(conv(x)) at the `rows` rows of idx) in ONE launch (ABI 4.9): the
 * conv gathers its inputs through the swap straight from `data`, so the two
 * are independent roles of the launch.  Same values as the two launches.
 * x fp32; y fp32 or bf16; cout 32 or 64. */
int cfsd_spiral_conv_fwd_in_swap(const float* data, const int32_t* batch_idx, const uint8_t* region_mask,
                                 const int32_t* key, int bs, int n_meshes, int n_regions, float* x, int x_dt,
                                 const int32_t* idx, const float* w, const float* bias, void* y, int y_dt,
                                 int vsrc, int rows, int cin, int cout, int act, void* stream);
/* Both gradients of a full 32 -> 32 SpiralConv (a Deblock conv, model.py:27-41
 * autograd) with EVERY operand vertex-major fp32 (x, dpre, dx, elu_y:
 * [vertex][batch][32]), batch % 16 == 0, batch x rows >= 65536, in ONE
 * launch (ABI 4.10): the flat-list data gradient of
 * cfsd_spiral_conv_bwd_data_flat (dx = elu'(elu_y) times the sum over u's
 * flat inverse list, elu_y may be NULL) and the weight-gradient slabs of
 * cfsd_spiral_conv_bwd_weight_x as interleaved workgroups, two per CU.
 * Bit-identical to those two calls.  dw == db == NULL defers
 * (cfsd_dw_reduce_batch item with fused = CFSD_DW_VM32).  inv_flat as
 * cfsd_spiral_conv_bwd_data_flat (flat_width in {8, 12, 16, 20}).
 * workspace: cfsd_spiral_conv_bwd_flat_pair_workspace() bytes (0 = unsupported). */
size_t cfsd_spiral_conv_bwd_flat_pair_workspace(int batch, int rows, int seq, int cin, int cout);
int cfsd_spiral_conv_bwd_flat_pair(const float* x, const int32_t* idx, const float* dpre, const int32_t* inv_flat,
                                   int flat_width, const float* w, const float* elu_y, float* dx, float* dw,
                                   float* db, float* workspace, size_t workspace_bytes, int batch, int vsrc,
                                   int rows, int seq, int cin, int cout, void* stream);
/* The bf16 step's Enblock backward (ABI 4.11): the flat-list dx of
 * cfsd_spiral_conv_bwd_data_rowsub (fp32 batch-major dpre at the kept rows,
 * fp32 w, fp32 products; dx / elu_y bf16 vertex-major, rounded once) and the
 * weight-gradient slabs of cfsd_spiral_conv_bwd_weight_x (x bf16
 * vertex-major) as two workgroup roles of ONE launch; always deferred
 * (cfsd_dw_reduce_batch item with fused = CFSD_DW_BF16).  32 -> 32, batch % 16 == 0,
 * flat_width in {4, 8, 12, 16}.  Same values as the two calls. */
int cfsd_spiral_conv_bwd_rowsub_pair_bf16(const void* x, const int32_t* idx, const float* dpre,
                                          const int32_t* inv_flat, int flat_width, const float* w, const void* elu_y,
                                          void* dx, float* workspace, size_t workspace_bytes, int batch, int vsrc,
                                          int rows, int seq, int cin, int cout, void* stream);
/* The same pair on the bf16 step's tensors (ABI 4.11): x, dpre, dx, elu_y
 * bf16 vertex-major, w the bf16 weight shadow; always deferred
 * (cfsd_dw_reduce_batch item with fused = CFSD_DW_BF16; workspace as
 * cfsd_spiral_conv_bwd_weight_x_workspace).  Same values as
 * cfsd_spiral_conv_bwd_data_flat + cfsd_spiral_conv_bwd_weight_x. */
int cfsd_spiral_conv_bwd_flat_pair_bf16(const void* x, const int32_t* idx, const void* dpre, const int32_t* inv_flat,
                                        int flat_width, const void* w, const void* elu_y, void* dx, float* workspace,
                                        size_t workspace_bytes, int batch, int vsrc, int rows, int seq, int cin,
                                        int cout, void* stream);

/* The same with the source level's layout (ABI 4.4): x_dt = CFSD_DT_F32
 * [| CFSD_VM] describes x, dx and elu_y (the fp32 step's E1 reads and writes
 * the vertex-major level-1 tensors); dpre stays batch-major fp32.  Few-row
 * layers only (the dW slabs of conv_dw_lat). */
int cfsd_spiral_conv_bwd_rowsub_x(const float* x, int x_dt, const int32_t* idx, const float* dpre,
                                  const int32_t* inv_flat, int flat_width, const float* w, const float* elu_y,
                                  float* dx, float* dw, float* db, float* workspace, size_t workspace_bytes,
                                  int batch, int vsrc, int rows, int seq, int cin, int cout, void* stream);

/* dx alone of the row-subset backward (as cfsd_spiral_conv_bwd_rowsub):
 * dG = dpre.W (fp32 dpre and W, fp32 MFMA) in `workspace`
 * (cfsd_spiral_conv_bwd_data_rowsub_workspace() bytes), then the ascending
 * flat-list gather-sum with elu'(elu_y); dx and elu_y stored as dx_dt
 * (CFSD_DT_F32 or CFSD_DT_BF16: one rounding of the fp32 sum).  Used by the
 * bf16 path, whose dW comes from cfsd_spiral_conv_bwd_weight_x. */
size_t cfsd_spiral_conv_bwd_data_rowsub_workspace(int batch, int rows, int seq, int cin);
int cfsd_spiral_conv_bwd_data_rowsub(const float* dpre, const int32_t* inv_flat, int flat_width,
                                     const float* w, const void* elu_y, void* dx, int dx_dt,
                                     float* workspace, size_t workspace_bytes, int batch, int vsrc,
                                     int rows, int seq, int cin, int cout, void* stream);

/* Materialising spiral gather, g[b,r,s*cin+c] = x[b, idx[r,s], c]
 * (model.py:34 index_select + view).  Used as the HBM-roofline probe. */
int cfsd_spiral_gather(const float* x, const int32_t* idx, float* g, int batch, int vsrc, int rows,
                       int seq, int cin, void* stream);

/* General-shape SpiralConv (ABI 4.19): the three products above for ANY
 * 1 <= seq <= CFSD_GEN_MAX_SEQ and 1 <= cin, cout <= CFSD_GEN_MAX_CH, fp32,
 * batch-major, on the fp32 MFMA, deterministic (fixed summation orders, no
 * atomics).  The entry points above are template instances of a few shapes
 * (spiral length 9, channels from {1, 2, 3, 16, 32, 64}) and refuse the rest;
 * cfsd_spiral_conv_has_shape says which, and these take whatever they refuse
 * (and, untuned, what they take).  Semantics and operand shapes exactly as
 * documented for cfsd_spiral_conv_fwd / _bwd_data / _bwd_weight; `rows` may be
 * a subset.  Sizes beyond the limits, and tensors or tables of 2^31 or more
 * elements, are refused with CFSD_EINVAL before any launch. */
#define CFSD_GEN_MAX_SEQ 32
#define CFSD_GEN_MAX_CH 512
int cfsd_spiral_conv_gen_fwd(const float* x, const int32_t* idx, const float* w, const float* bias,
                             float* y, int batch, int vsrc, int rows, int seq, int cin, int cout,
                             int act, void* stream);
/* dx through the (u, s)-keyed inverse CSR alone (no inv_head, no workspace):
 * the dpre rows of list (u, s) are added in list order, the sums contracted
 * with the slot's weights in ascending s.  A source vertex with no entry gets
 * exactly 0. */
int cfsd_spiral_conv_gen_bwd_data(const float* dpre, const int32_t* inv_ptr, const int32_t* inv_row,
                                  const float* w, const float* elu_y, float* dx, int batch, int vsrc,
                                  int rows, int seq, int cin, int cout, void* stream);
/* dw, db by a two-stage reduction of fixed order: the batch * rows rows are
 * cut into chunks, chunk p's sums (rows ascending) go to slab p of
 * `workspace` (cfsd_spiral_conv_gen_bwd_weight_workspace() bytes; 0 = sizes
 * outside the limits), and each element's slabs are added in a fixed order.
 * dw == db == NULL defers the second stage: the slabs stay in `workspace`
 * until cfsd_spiral_conv_gen_dw_reduce (same sizes) adds them, with the same
 * result bit for bit.  These slabs are NOT items of cfsd_dw_reduce_batch; a
 * step that ends in cfsd_dw_reduce_batch_adam reduces them into the flat
 * gradient first, and that launch's rest workgroups apply Adam to them. */
size_t cfsd_spiral_conv_gen_bwd_weight_workspace(int batch, int rows, int seq, int cin, int cout);
int cfsd_spiral_conv_gen_bwd_weight(const float* x, const int32_t* idx, const float* dpre, float* dw,
                                    float* db, float* workspace, size_t workspace_bytes, int batch,
                                    int vsrc, int rows, int seq, int cin, int cout, void* stream);
int cfsd_spiral_conv_gen_dw_reduce(const float* workspace, size_t workspace_bytes, float* dw, float* db,
                                   int batch, int rows, int seq, int cin, int cout, void* stream);
/* 1 when the fp32 batch-major entry point of `role` (cfsd_spiral_conv_fwd,
 * _bwd_data, _bwd_weight) has a kernel instance for this shape, else 0 (also
 * for an unknown role or a non-positive size).  CFSD_CONV_BWD_FUSED: the
 * shape is a small-output layer whose dx + dW cfsd_spiral_conv_bwd and
 * cfsd_spiral_conv_bwd_x run as one fused launch (32 / 64 -> 1, 2, 3), whether
 * or not _bwd_data / _bwd_weight have it on their own.  cfsd_spiral_conv_bwd
 * takes a shape when this role is 1, or _bwd_weight's is and (without dx, or)
 * _bwd_data's is. */
#define CFSD_CONV_FWD 0
#define CFSD_CONV_BWD_DATA 1
#define CFSD_CONV_BWD_WEIGHT 2
#define CFSD_CONV_BWD_FUSED 3
int cfsd_spiral_conv_has_shape(int role, int seq, int cin, int cout);

/* ---------------------------------------------------------------- Pool
 * Replaces Pool (model.py:50-55: index_select * value, torch_scatter.scatter_add)
 * and its autograd, as a row-sorted CSR SpMM whose per-row order is the COO
 * file order (so the fp32 sum order equals the reference's sequential
 * scatter_add):
 *   y[b,r,:] = g(b,r,:) * sum_{k in row r} val[k] * x[b, col[k], :]
 * with g = elu'(elu_y) when elu_y != NULL (fuses the ELU backward of the
 * tensor the transpose product returns a gradient for), else 1.
 * x [batch, n, c], y [batch, m, c]; c % 4 == 0. */
int cfsd_spmm_csr(const int32_t* row_ptr, const int32_t* col, const float* val, const float* x,
                  const float* elu_y, float* y, int batch, int m, int n, int c, void* stream);

/* cfsd_spmm_csr(_x) for matrices with long, skewed rows (the up-sampling
 * transposes): same results bit for bit; rows are visited in `order` (a
 * permutation of [0, m), rows by decreasing length: the longest sequential
 * folds start first) and each row's entry list is prefetched one chunk ahead.
 * x / elu_y / y storage types as cfsd_spmm_csr_x. */
int cfsd_spmm_csr_sched(const int32_t* row_ptr, const int32_t* col, const float* val,
                        const int32_t* order, const void* x, int x_dt, const void* elu_y, void* y,
                        int y_dt, int batch, int m, int n, int c, void* stream);

/* cfsd_spmm_csr_sched with the CSR stored in visiting order: slot i (0..m-1)
 * is output row rows_s[i] (a permutation of [0, m)) with entries
 * [ptr_s[i], ptr_s[i+1]) of col_s / val_s, each row's entries in the original
 * per-row (file) order (topology.scheduled_csr).  Same results bit for bit as
 * cfsd_spmm_csr_x; one dependent index load fewer than cfsd_spmm_csr_sched. */
int cfsd_spmm_sched_csr(const int32_t* ptr_s, const int32_t* col_s, const float* val_s,
                        const int32_t* rows_s, const void* x, int x_dt, const void* elu_y, void* y,
                        int y_dt, int batch, int m, int n, int c, void* stream);

/* cfsd_spmm_csr_x for a matrix whose rows all hold exactly k (1..4) entries,
 * row r's at [r*k, r*k + k) of col/val (the CSR arrays of the barycentric
 * up-sampling matrices, Pool(up) at model.py:84 via model.py:50-55: 3 per
 * row).  No row_ptr: one dependent load fewer per row.  Same results bit for
 * bit as cfsd_spmm_csr_x on the same CSR. */
int cfsd_spmm_uniform(int k, const int32_t* col, const float* val, const void* x, int x_dt,
                      const void* elu_y, void* y, int y_dt, int batch, int m, int n, int c,
                      void* stream);

/* ---------------------------------------------------------------- feature swap
 * Replaces SwapFeatures.__call__ / swap (swap_batch_transform.py:13-52):
 *   out[i*bs+j, v, :] = x[mesh[(i != j && mask[key*nv + v]) ? j : i], v, :]
 * x [n_meshes, nv, c] resident dataset, batch_idx [bs] device indices of the
 * base meshes, region_mask [n_regions, nv] (1 = feature vertex of the region),
 * key: device int32 scalar (region index).  Bit-exact copy.  Device values
 * are range-guarded (never fault): a key outside [0, n_regions) swaps nothing,
 * a mesh index outside [0, n_meshes) is clamped. */
int cfsd_swap_features(const float* x, const int32_t* batch_idx, const uint8_t* region_mask,
                       const int32_t* key, float* out, int bs, int nv, int c, int n_meshes,
                       int n_regions, void* stream);
/* The same with the output's layout: out_dt = CFSD_DT_F32 [| CFSD_VM] (ABI
 * 4.2; x stays batch-major [n_meshes, nv, c]). */
int cfsd_swap_features_x(const float* x, const int32_t* batch_idx, const uint8_t* region_mask,
                         const int32_t* key, float* out, int out_dt, int bs, int nv, int c,
                         int n_meshes, int n_regions, void* stream);
/* SpiralDeblock forward with the Pool(up) fused into the gather (ABI 4.4;
 * model.py:80-82: x_up = Pool(xc, up) then SpiralConv(x_up) + ELU): the input
 * row of spiral position (r, s) is sum_k comp_val[(r*9+s)*3+k] *
 * xc[b, comp_col[(r*9+s)*3+k], :] -- the composite table of a uniform
 * 3-entry up matrix (topology.up_comp), summed ((0 + x0 v0) + x1 v1) + x2 v2
 * exactly as cfsd_spmm_uniform (bit-identical up-sampled rows); idx [rows, 9]
 * with idx[r][0] == r, and y_up (optional) receives the up-sampled input
 * [batch, rows, cin] the weight gradient reads.  xc [batch, n_coarse, cin],
 * y [batch, rows, cout], batch-major fp32.  Coarse layers only:
 * cfsd_spiral_conv_fwd_up_supported() says which. */
int cfsd_spiral_conv_fwd_up_supported(int batch, int rows, int seq, int cin, int cout);
int cfsd_spiral_conv_fwd_up(const float* xc, const int32_t* comp_col, const float* comp_val, const int32_t* idx,
                            const float* w, const float* bias, float* y, float* y_up, int batch, int n_coarse,
                            int rows, int seq, int cin, int cout, int act, void* stream);
/* The un-swapped batch of a swap_features: False configuration
 * (data_loading.py:38, 81-82: MeshCollater without a feature_swapper):
 * out[b] = x[batch_idx[b]], b < bs; out_dt = CFSD_DT_F32 [| CFSD_VM] (ABI 4.4).
 * Bit-exact copy; mesh indices clamped into [0, n_meshes). */
int cfsd_gather_meshes(const float* x, const int32_t* batch_idx, float* out, int out_dt, int bs, int nv,
                       int c, int n_meshes, void* stream);

/* Spectral augmentation blend (utils.py:244-267, data_loading.py:359-364):
 * with s1 = U^T x1, s2 = U^T x2 [pairs, k, c] (U: the k smallest Laplacian
 * eigenvectors), s4[p,j,:] = s1 + values[p,j]*(s2 - s1) for j < n_blend, else
 * s1; the augmented mesh is then U s4.  values [pairs, k] (spectral_interpolation:
 * N(0.5, 0.5) draws; spectral_combination: 0/1 selector). */
int cfsd_spectral_blend(const float* s1, const float* s2, const float* values, float* s4, int pairs,
                        int k, int c, int n_blend, void* stream);

/* Dataset normalisation, (x - mean) / std with per-vertex statistics
 * (data_loading.py:259-260; mean/std [nv, c] from norm.pt): x, out
 * [n_meshes, nv, c] (may alias).  Same two IEEE roundings as torch: bit-exact. */
int cfsd_normalize(const float* x, const float* mean, const float* std, float* out, int n_meshes,
                   int nv, int c, void* stream);

/* ---------------------------------------------------------------- dense layers
 * nn.Linear of the latent bottleneck (model.py:114-124, 153-156, 167):
 *   y[i,n] = bias[n] + sum_k x[i,k] w[n,k]      x [m,k], w [n,k], y [m,n]
 * Long reductions are split across workgroups through `workspace`
 * (cfsd_linear_workspace(m,k,n) bytes; may be 0 -> NULL allowed). */
size_t cfsd_linear_workspace(int m, int k, int n);
int cfsd_linear_fwd(const float* x, const float* w, const float* bias, float* y, float* workspace,
                    size_t workspace_bytes, int m, int k, int n, void* stream);
/* Linear backward: dx = dy.w (times elu'(elu_y) when elu_y [m,k] != NULL; added
 * to dx when accumulate != 0), dw = dy^T.x, db = sum_i dy.  dx/dw/db may be NULL. */
int cfsd_linear_bwd(const float* x, const float* w, const float* dy, const float* elu_y, float* dx,
                    float* dw, float* db, float* workspace, size_t workspace_bytes, int m, int k,
                    int n, int accumulate, void* stream);

/* Linear backward with a long output (the decoder Linear, dz = dh.W with
 * W [n][k], n = 4288): dW / db as cfsd_linear_bwd and, in the SAME launch,
 * dx as cfsd_linear_bwd_split_parts(n) partial products over 64-row slices of
 * W, dx_parts [parts][m][k] (summed by cfsd_latent_bwd_parts, slice order).
 * m <= 16, k <= 128. */
int cfsd_linear_bwd_split_parts(int n);
int cfsd_linear_bwd_split(const float* x, const float* w, const float* dy, float* dx_parts,
                          float* dw, float* db, int m, int k, int n, void* stream);

/* The step's whole bottleneck backward in ONE launch (ABI 4.8; 4.12: the
 * exchange workspace, the sticky error word): the Pool(up)
 * transpose of the coarsest Deblock (model.py:172-173; CSR up_ptr/up_col/
 * up_val in plain per-row order over the fine-level gradient g [batch][n_up]
 * [cup], batch-major), the decoder Linear backward (dh.W with W = wd
 * [nd][latent], nd = coarse vertices x cup; dwd / dbd; dz as the partial
 * products of cfsd_linear_bwd_split, kept in `exchange`), the latent head
 * backward (cfsd_latent_bwd_parts: mulv, eps, dlat -> dmulv) and the encoder
 * Linear backward (cfsd_linear_bwd with x = xe [batch][ke], w = we [ne][ke],
 * dy = dmulv; dxe (x elu'(elu_y) when elu_y != NULL), dwe, dbe).  Workgroups
 * of the later stages wait on device counters for the earlier ones (only ever
 * on workgroups of lower index) and read the values they wait for from
 * `exchange` (cfsd_bottleneck_bwd_exchange_floats(batch, latent, nd, ne)
 * device floats, contents unspecified: each 128-B line is written by ONE
 * workgroup); `sync` is CFSD_BN_SYNC_INTS device int32 (19 counters and flags, one 128-B
 * line each) that must be zero before the first call and are left zero by
 * every call -- except sync[CFSD_BN_SYNC_ERR], a sticky word a wait that
 * timed out sets (the values are then wrong: the caller must check it and
 * refuse the step).  Same values bit for bit as spmm + linear_bwd_split +
 * latent_bwd_parts + linear_bwd, except that dh itself is never stored.
 * batch <= 16, latent <= 128, cup a multiple of 64, nd <= 5120, ne =
 * (is_vae ? 2 : 1) x latent <= 160. */
#define CFSD_BN_SYNC_INTS 608
#define CFSD_BN_SYNC_ERR 65
size_t cfsd_bottleneck_bwd_exchange_floats(int batch, int latent, int nd, int ne);
int cfsd_bottleneck_bwd(const int32_t* up_ptr, const int32_t* up_col, const float* up_val, const float* g,
                        int n_up, int cup, const float* z, const float* wd, float* exchange, float* dwd,
                        float* dbd, int nd, const float* mulv, const float* eps, const float* dlat,
                        float* dmulv, int train, int is_vae, int sigmoid, const float* xe, const float* we,
                        const float* elu_y, float* dxe, float* dwe, float* dbe, int ke, int ne, int accumulate,
                        int32_t* sync, int batch, int latent, void* stream);

/* ---------------------------------------------------------------- losses
 * compute_mse_loss + _compute_laplacian_regularizer (model_manager.py:333-349,
 * utils.py:153-165) fused.  Pass 1 computes, per (b,v), Lx = sum_k L[v,k] pred[b,k,:]
 * (CSR of the random-walk Laplacian, per-row order = COO order), stores the
 * unit vector Lx/|Lx| in unit_lx [batch, nv, c] and writes per-block partial
 * sums {sum (pred-gt)^2, sum |Lx|} to partials[2*nblocks] (nblocks from
 * cfsd_recon_lap_blocks).  Pass 2 writes the gradient of
 *   w_rec * mse + w_lap * sum|Lx| / (nv*batch)
 * w.r.t. pred into dpred using the transpose CSR (lt_*). */
int cfsd_recon_lap_blocks(int batch, int nv);
int cfsd_recon_lap_fwd(const float* pred, const float* gt, const int32_t* l_ptr,
                       const int32_t* l_col, const float* l_val, float* unit_lx, float* partials,
                       int batch, int nv, int c, void* stream);
int cfsd_recon_lap_bwd(const float* pred, const float* gt, const float* unit_lx,
                       const int32_t* lt_ptr, const int32_t* lt_col, const float* lt_val,
                       float* dpred, int batch, int nv, int c, float w_rec, float w_lap,
                       void* stream);
/* cfsd_recon_lap_bwd with cfsd_loss_finalize folded into its last workgroup
 * (same arguments as both; the partials were completed by the preceding
 * cfsd_recon_lap_fwd on the stream): one launch less per train step. */
int cfsd_recon_lap_bwd_finalize(const float* pred, const float* gt, const float* unit_lx,
                                const int32_t* lt_ptr, const int32_t* lt_col, const float* lt_val,
                                float* dpred, int batch, int nv, int c, float w_rec, float w_lap,
                                const float* partials, int nblocks, const float* terms, float* out,
                                float* acc, float w_kl, float w_lc, void* stream);
/* The three loss passes with pred / gt / unit_lx / dpred in one layout, dt =
 * CFSD_DT_F32 [| CFSD_VM] (ABI 4.2: the fp32 step's vertex-major level-0
 * tensors).  Same values; the loss partial sums run over the storage order,
 * so the reduced losses may differ in the last bits between layouts. */
int cfsd_recon_lap_fwd_x(const float* pred, const float* gt, const int32_t* l_ptr,
                         const int32_t* l_col, const float* l_val, float* unit_lx, float* partials,
                         int batch, int nv, int c, int dt, void* stream);
int cfsd_recon_lap_bwd_x(const float* pred, const float* gt, const float* unit_lx,
                         const int32_t* lt_ptr, const int32_t* lt_col, const float* lt_val,
                         float* dpred, int batch, int nv, int c, float w_rec, float w_lap, int dt,
                         void* stream);
int cfsd_recon_lap_bwd_finalize_x(const float* pred, const float* gt, const float* unit_lx,
                                  const int32_t* lt_ptr, const int32_t* lt_col, const float* lt_val,
                                  float* dpred, int batch, int nv, int c, float w_rec, float w_lap,
                                  const float* partials, int nblocks, const float* terms, float* out,
                                  float* acc, float w_kl, float w_lc, int dt, void* stream);

/* Latent head, forward (model.py:146-160, 184-188; model_manager.py:352-393).
 * mulv [batch, 2*latent] = [logvar | mu] when is_vae (the two encoder Linears
 * stacked, logvar = en_layers[-2], mu = en_layers[-1]), else mu [batch, latent].
 * z = mu + eps*exp(0.5*logvar) (train && is_vae), sigmoid(mu) (!is_vae && sigmoid),
 * else mu.  KL and the latent-consistency hinge for the swapped region
 * [key*region_size, +region_size) (key: device scalar; bs = sqrt(batch)).
 * Writes z [batch, latent]; terms[2] = {kl, lc}; and the head's own gradient
 * parts dlat [batch, 3*latent] = {w_lc*dLC/dz | w_kl*dKL/dmu | w_kl*dKL/dlogvar}.
 * Single workgroup holding z and the pair distances in LDS: needs
 * 4 (batch*latent + 4*npairs*bs) bytes <= 159 KB (batch 256 at latent 75:
 * 105 KB); larger shapes return CFSD_EINVAL. */
int cfsd_latent_fwd(const float* mulv, const float* eps, const int32_t* key, float* z,
                    float* dlat, float* terms, int batch, int latent, int region_size, int train,
                    int is_vae, int sigmoid, float w_kl, float w_lc, float eta1, float eta2,
                    void* stream);
/* (ABI 4.5) cfsd_latent_fwd followed by the decoder Linear (model.py:167-168)
 * y [batch, n] = z w^T + bias, w [n, latent], in ONE launch: z, dlat and y are
 * bit-identical to cfsd_latent_fwd + cfsd_linear_fwd(z, w, bias, y, batch,
 * latent, n), terms[] included.  _supported: latent <= 80 and the LDS of z,
 * the pair distances and a 32-row W slice <= 159 KB. */
int cfsd_latent_linear_fwd_supported(int batch, int latent, int n);
int cfsd_latent_linear_fwd(const float* mulv, const float* eps, const int32_t* key, float* z,
                           float* dlat, float* terms, int batch, int latent, int region_size,
                           int train, int is_vae, int sigmoid, float w_kl, float w_lc, float eta1,
                           float eta2, const float* w, const float* bias, float* y, int n,
                           void* stream);
/* Latent head, backward: dmulv (same layout as mulv) from dz_dec (gradient of
 * the decoder input) + dlat.  z is only read for the sigmoid AE variant
 * (is_vae == 0, sigmoid != 0), where a NULL z is CFSD_EINVAL. */
int cfsd_latent_bwd(const float* mulv, const float* eps, const float* z, const float* dz_dec,
                    const float* dlat, float* dmulv, int batch, int latent, int train, int is_vae,
                    int sigmoid, void* stream);
/* cfsd_latent_bwd with dz_dec given as n_parts partial products
 * [n_parts][batch][latent] (from cfsd_linear_bwd_split), summed in part order. */
int cfsd_latent_bwd_parts(const float* mulv, const float* eps, const float* z,
                          const float* dz_parts, int n_parts, const float* dlat, float* dmulv,
                          int batch, int latent, int train, int is_vae, int sigmoid, void* stream);
/* Reduce the recon partials + latent terms into out[5] = {rec, kl, lc, lap, tot}
 * (tot = rec + w_kl*kl + w_lc*lc + w_lap*lap, model_manager.py:308-312) and,
 * when acc != NULL, add them to acc[0..4] and 1 to acc[5] (per-epoch sums on
 * device: no per-step host sync, unlike the reference's 7 .item() calls). */
int cfsd_loss_finalize(const float* partials, int nblocks, const float* terms, float* out,
                       float* acc, int batch, int nv, int c, float w_kl, float w_lc, float w_lap,
                       void* stream);

/* ---------------------------------------------------------------- optimiser
 * torch.optim.Adam step (model_manager.py:69-72, 316) over one flat fp32
 * parameter buffer.  `step` is a device int32 holding the 1-based step number
 * t used for the bias corrections (advanced by cfsd_step_begin).  With
 * param_bf16 != NULL (8-B aligned) the updated parameters are also written
 * there as bf16 (the weight shadow the bf16 kernels read; may be NULL). */
int cfsd_adam(float* param, const float* grad, float* m, float* v, const int32_t* step, size_t n,
              float lr, float beta1, float beta2, float eps, float weight_decay,
              uint16_t* param_bf16, void* stream);

/* cfsd_scale(grad, n, grad_scale) then cfsd_adam in ONE launch (ABI 4.7): the
 * data-parallel step's 1/world averaging after the gradient all-reduce (SUM)
 * folded into the update (model_manager.py:316 on the averaged gradient).
 * `grad` receives the scaled gradient; same values bit for bit as the two
 * launches. */
int cfsd_adam_scaled(float* param, float* grad, float* m, float* v, const int32_t* step, size_t n,
                     float grad_scale, float lr, float beta1, float beta2, float eps,
                     float weight_decay, uint16_t* param_bf16, void* stream);

/* Per-step device bookkeeping (graph-replayable, no host input):
 * t = ++*counter; key = hash(seed, t) % n_regions (replaces random.choice,
 * swap_batch_transform.py:26); eps[n_eps] ~ N(0,1) (replaces randn_like,
 * model.py:187); the batch of MeshLoader(shuffle=True, drop_last=True)
 * (data_loading.py:40-48): with bt = (t-1) % n_batches, epoch = (t-1) / n_batches,
 *   j_q = shuffle ? P_epoch(bt*bs + q) : bt*bs + q,   batch_idx[q] = perm ? perm[j_q] : j_q
 * where P_epoch is a keyed permutation of [0, n_items) drawn from (seed, epoch)
 * (a fresh order every epoch; n_batches*bs <= n_items, the tail is dropped) and
 * perm (n_items entries, optional) maps positions to dataset rows (e.g. a
 * rank's shard); ++*adam_step (the Adam bias-correction step of this iteration).
 * Any of eps/key/batch_idx/adam_step may be NULL. */
int cfsd_step_begin(int32_t* counter, unsigned long long seed, float* eps, int n_eps,
                    int32_t* key, int n_regions, int32_t* batch_idx, int bs, int n_batches,
                    const int32_t* perm, int n_items, int shuffle, int32_t* adam_step,
                    void* stream);

/* F.elu backward written from the ELU output (model.py:68,84 autograd):
 * dx = dy * (y > 0 ? 1 : y + 1).  dx may alias dy. */
int cfsd_elu_bwd(const float* dy, const float* y, float* dx, size_t n, void* stream);

/* Element-wise y *= alpha (gradient averaging after an all-reduce). */
int cfsd_scale(float* y, size_t n, float alpha, void* stream);

/* ---------------------------------------------------------------- bf16 path
 * Mixed-precision variants (BASELINE.json configs C3/C5: bf16 activations and
 * weights, fp32 accumulation, fp32 master weights + Adam).  Each activation /
 * gradient operand carries its storage type (CFSD_DT_F32 / CFSD_DT_BF16);
 * the engine's bf16 mode keeps the level-0/1 tensors in bf16 and the coarse
 * levels + bottleneck in fp32.  Same arithmetic as the fp32 entry points
 * above (model.py:27-55 and autograd), products in bf16, sums in fp32.
 * 32/64-channel layers need x bf16 and the bf16 weight shadow `w_bf16`
 * ([cout, seq*cin], from cfsd_adam/cfsd_cast); the xyz layers use the fp32
 * `w` (input conv: x fp32 -> y bf16; output conv: x bf16 -> y fp32).
 *
 * The same entry points take the fp32 step's VERTEX-MAJOR operands (ABI 4.1,
 * the reference's fp32 arithmetic with the level-0/1 tensors stored
 * [nv][batch][c], batch % 16 == 0): a 32 -> 32/64 layer with x_dt =
 * CFSD_DT_F32 | CFSD_VM runs the fp32 vertex-major MFMA kernels with the fp32
 * `w` (y fp32, either layout; same products in the same order as
 * cfsd_spiral_conv_fwd, bit-identical outputs), and the xyz layers accept
 * fp32 operands in either layout. */
int cfsd_spiral_conv_fwd_x(const void* x, int x_dt, const int32_t* idx, const float* w,
                           const uint16_t* w_bf16, const float* bias, void* y, int y_dt, int batch,
                           int vsrc, int rows, int seq, int cin, int cout, int act, void* stream);
/* dx (bf16) of a 32/64-channel layer; dpre bf16 or fp32; elu_y bf16 or NULL.
 * dx_dt = CFSD_DT_BF16 [| CFSD_VM] (the layout of dx and elu_y). */
int cfsd_spiral_conv_bwd_data_x(const void* dpre, int dpre_dt, const int32_t* inv_ptr,
                                const int32_t* inv_row, const int32_t* inv_head,
                                const uint16_t* w_bf16, const uint16_t* elu_y, uint16_t* dx,
                                int dx_dt, int batch, int vsrc, int rows, int seq, int cin,
                                int cout, void* stream);
/* The same dx through the FLAT inverse list (topology.inverse_flat: per
 * source vertex the spiral positions p = r*seq + s naming it, ascending,
 * -1 padded to flat_width in {8, 12, 16, 20}): one MFMA per entry, exact
 * products (no bf16 rounding of per-slot row sums).  Vertex-major dpre / dx /
 * elu_y, batch % 16 == 0, 32 -> 32/64 channels (the level-0/1 Deblocks).
 * dx_dt = CFSD_DT_BF16 | CFSD_VM: `w` is the bf16 shadow, elu_y bf16, dpre
 * bf16 or fp32; dx_dt = CFSD_DT_F32 | CFSD_VM (ABI 4.1, the fp32 step): `w`,
 * elu_y and dpre fp32 -- dx[u] = elu'(elu_y[u]) * sum over the list of
 * W_s^T dpre[r] in list order (IndexSelectBackward's visiting order). */
int cfsd_spiral_conv_bwd_data_flat(const void* dpre, int dpre_dt, const int32_t* inv_flat,
                                   int flat_width, const void* w, const void* elu_y, void* dx,
                                   int dx_dt, int batch, int vsrc, int rows, int seq, int cin,
                                   int cout, void* stream);
/* dW/db (fp32): 32/64-channel layers (x bf16, dpre bf16/fp32; or x and dpre
 * fp32, each batch-major or vertex-major) and the xyz input layer (x fp32,
 * dpre bf16 or fp32).  dw == db == NULL defers the reduction: the
 * cfsd_dw_reduce_batch item's `fused` is what cfsd_spiral_conv_bwd_weight_x_slabs
 * returns for the same operands.  Workspace: cfsd_spiral_conv_bwd_weight_x_workspace
 * for a bf16 x, cfsd_spiral_conv_bwd_weight_workspace (the fp32 kernels' slab
 * set) for an fp32 x. */
size_t cfsd_spiral_conv_bwd_weight_x_workspace(int batch, int rows, int seq, int cin, int cout);
int cfsd_spiral_conv_bwd_weight_x(const void* x, int x_dt, const int32_t* idx, const void* dpre,
                                  int dpre_dt, float* dw, float* db, float* workspace,
                                  size_t workspace_bytes, int batch, int vsrc, int rows, int seq,
                                  int cin, int cout, void* stream);
/* The CFSD_DW_* code of the slabs a deferred cfsd_spiral_conv_bwd_weight_x
 * call with these operands leaves (ABI 4.20), or -1 where the entry point
 * refuses the combination of storage types and channels.  It is the entry
 * point's own routing decision; a pure function of its arguments (no device
 * call: usable during graph capture and without a GPU). */
int cfsd_spiral_conv_bwd_weight_x_slabs(int x_dt, int dpre_dt, int batch, int cin, int cout);
/* Fused dx + dW of the xyz output layer (cout*seq <= 32) with x, elu_y, dx
 * bf16 (or all three fp32, ABI 4.1) and dpre fp32 (workspace:
 * cfsd_spiral_conv_bwd_workspace; deferred items use fused = CFSD_DW_FUSED).  x_dt's
 * storage type and CFSD_VM flag are those of x, elu_y and dx; dpre_dt =
 * CFSD_DT_F32 [| CFSD_VM]. */
int cfsd_spiral_conv_bwd_x(const void* x, int x_dt, const int32_t* idx, const float* dpre,
                           int dpre_dt, const int32_t* inv_ptr, const int32_t* inv_row, const int32_t* inv_head,
                           const float* w, const void* elu_y, void* dx, float* dw, float* db,
                           float* workspace, size_t workspace_bytes, int batch, int vsrc, int rows,
                           int seq, int cin, int cout, void* stream);
/* The same fused backward of the xyz output conv (32 -> 3) for VERTEX-MAJOR
 * x / elu_y / dx (fp32 or bf16) and fp32 dpre (ABI 4.2), batch % 16 == 0:
 * per source vertex the spiral transpose is one walk of its flat inverse
 * list (topology.inverse_flat, width 8/12/16/20), dx = W^T-products of the
 * folded 3-wide dpre, dW = folded dpre (x) x.  Same workspace, slab layout
 * and deferred kind (fused = CFSD_DW_FUSED) as cfsd_spiral_conv_bwd_x. */
int cfsd_spiral_conv_bwd_out_flat(const void* x, int x_dt, const int32_t* idx, const float* dpre,
                                  int dpre_dt, const int32_t* inv_flat, int flat_width, const float* w,
                                  const void* elu_y, void* dx, float* dw, float* db, float* workspace,
                                  size_t workspace_bytes, int batch, int vsrc, int rows, int seq, int cin,
                                  int cout, void* stream);
/* cfsd_spmm_csr with per-operand storage types (elu_y has y's type). */
int cfsd_spmm_csr_x(const int32_t* row_ptr, const int32_t* col, const float* val, const void* x,
                    int x_dt, const void* elu_y, void* y, int y_dt, int batch, int m, int n, int c,
                    void* stream);
/* Storage conversion fp32 <-> bf16 (round to nearest even), n elements. */
int cfsd_cast(const void* src, int src_dt, void* dst, int dst_dt, size_t n, void* stream);

/* ---------------------------------------------------------------- evaluation
 * Replaces ModelManager.compute_vertex_errors (model_manager.py:395-400) and
 * the per-mesh reduction of Tester.reconstruction_errors (test.py:280-301):
 * out, gt [batch, nv, 3]; mean/std [nv, 3] (both NULL = no un-normalisation,
 * else u = x*std + mean as Tester._unnormalize_verts, test.py:81-84);
 *   err[b, v]  = sqrt(sum_c (u_out - u_gt)^2) * to_mm        (may be NULL)
 *   l1[b, v]   = sum_c |u_out - u_gt|  (the per-vertex L1 parity metric; may be NULL)
 *   mesh_mean[b] = mean_v err[b, v]  (fixed-order reduction; needs err; may be NULL). */
int cfsd_vertex_errors(const float* out, const float* gt, const float* mean, const float* std,
                       float* err, float* l1, float* mesh_mean, int batch, int nv, float to_mm,
                       void* stream);

/* The two device reductions of a latent traversal (Tester.latent_traversals,
 * test.py:128-229), ABI 4.17.  Plain fp32, no atomics; neither result depends
 * on the launch geometry or on the other rows of the call.
 *
 * cfsd_group_vertex_errors replaces compute_vertex_errors on (frames, frame 0
 * of each traversal expanded to its length) (test.py:157-158):
 * frames [groups * n, nv, 3] = `groups` groups of n consecutive frames;
 * mean/std [nv, 3] (both NULL = no un-normalisation, else u = x*std + mean);
 *   err[g*n + k, v] = sqrt(sum_c (u(frames[g*n + k, v, c]) - u(frames[g*n, v, c]))^2) * to_mm
 * with the operations of cfsd_vertex_errors in its order (contraction off):
 * err is bit-equal to cfsd_vertex_errors(out = frames, gt = frame 0 of every
 * group repeated n times), and err[g*n, :] is exactly 0.  Frame 0 is read in
 * place; no expanded copy exists.  groups, n, nv >= 1; groups*n*nv*3 < 2^31.
 *
 * cfsd_region_means replaces the per-region mean of a per-vertex quantity
 * (test.py:208-215: fancy indexing + torch.mean per region and row, collected
 * through pandas): values [rows, nv]; region_ptr a HOST array of
 * n_regions + 1 int32 and region_idx [region_ptr[n_regions]] int32 on the
 * device form a CSR of vertex lists (lists may overlap, need not be sorted);
 *   out[b, r] = (sum_j values[b, region_idx[j]]) / len_r,  j over list r.
 * Summation scheme: one CFSD_RM_THREADS-thread workgroup per (b, r); thread t
 * adds entries t, t + 256, t + 512, ... of the list in ascending order onto 0,
 * the 256 partials are added in a halving tree (part[t] += part[t + w], w =
 * 128, 64, ..., 1), the total is divided by len_r.  Depth (the longest chain of
 * additions one term passes through, plus one for the division):
 *   CFSD_RM_DEPTH(len) = ceil(len / 256) + 8 + 1,
 * 25 for a list of 4096 entries, 21 for the template's longest (3017).
 * CFSD_EINVAL without a launch: a null pointer, sizes < 1, n_regions >
 * CFSD_RM_MAX_REGIONS, region_ptr[0] != 0, a decreasing region_ptr, an empty
 * list.  The entries of region_idx must lie in [0, nv): they are not read on
 * the host here; the caller checks them once when it builds the CSR. */
#define CFSD_RM_MAX_REGIONS 64
#define CFSD_RM_THREADS 256
#define CFSD_RM_DEPTH(len) (((len) + CFSD_RM_THREADS - 1) / CFSD_RM_THREADS + 9)
int cfsd_group_vertex_errors(const float* frames, const float* mean, const float* std, float* err, int groups,
                             int n, int nv, float to_mm, void* stream);
int cfsd_region_means(const float* values, const int32_t* region_ptr, const int32_t* region_idx, float* out,
                      int rows, int nv, int n_regions, void* stream);

/* ---------------------------------------------------------------- latent fitting
 * The Chamfer term of Tester.fit_mesh (test.py:404-405, 427-429:
 * pytorch3d.loss.chamfer_distance between the decoded heads and an
 * unregistered scan), ABI 4.13.
 *
 * cfsd_nn_points: batched brute-force nearest neighbour.  q [bq, n, 3] queries,
 * r [br, p, 3] reference points, fp32; bq and br are each 1 or `batch` (1 =
 * the one set is shared by every batch element, read in place).  Per query
 *   dist2[b, i] = min_j |q[b,i] - r[b,j]|^2,  idx[b, i] = the arg min (int32),
 * the distance in difference form (dx*dx + dy*dy + dz*dz, d = q - r; no
 * |q|^2 + |r|^2 - 2 q.r expansion), bit-equal distances resolved to the
 * lowest j.  No atomics; the values do not depend on the launch geometry.
 * The reference points are walked in chunks of CFSD_NN_TILE; a partial last
 * chunk visits only the points that exist.  n, p >= 1.
 * workspace: cfsd_nn_points_workspace() bytes (0 = none needed, NULL allowed):
 * with few queries the reference range is cut into segments whose winners
 * are merged there. */
#define CFSD_NN_TILE 16
size_t cfsd_nn_points_workspace(int batch, int n, int p);
int cfsd_nn_points(const float* q, const float* r, float* dist2, int32_t* idx, void* workspace,
                   size_t workspace_bytes, int batch, int bq, int br, int n, int p, void* stream);

/* Gradient of the two-sided Chamfer sum with respect to the generated points
 * x [batch, n, 3] only (the target y [by, p, 3], by = 1 or batch, is constant):
 *   gx[b,i] = wx[b] 2 (x_i - y[idx_xy[b,i]]) + wy[b] sum_{j: idx_yx[b,j] = i} 2 (x_i - y_j)
 * idx_xy [batch, n] from cfsd_nn_points(x, y); the other direction's
 * idx_yx [batch, p] (cfsd_nn_points(y, x)) is passed GROUPED by generated
 * point: seg_j [batch, p] = the targets j of batch b ordered by (idx_yx[b,j], j)
 * (a stable sort), seg_ptr [batch, n + 1] = the offsets of each i's run in it.
 * Each run is summed in ascending j by one thread: deterministic, no atomics.
 * wx, wy [batch] device floats fold in the upstream gradient and the 1/n,
 * 1/p, 1/batch of the reductions.  Indices are clamped into range. */
int cfsd_chamfer_bwd(const float* x, const float* y, const int32_t* idx_xy, const int32_t* seg_ptr,
                     const int32_t* seg_j, const float* wx, const float* wy, float* gx, int batch, int by,
                     int n, int p, void* stream);

/* Exact nearest neighbour over a uniform grid, for dense point sets (ABI 4.24,
 * nn_grid.hip): the result of cfsd_nn_points BIT FOR BIT -- the same distance
 * (one shared instruction sequence, nn_dist.h) and the same index, bit-equal
 * distances resolved to the lowest original index -- at a cost that follows
 * the points near a query, not all of them.
 *
 * cfsd_nn_grid_build: r [br, p, 3] fp32, gx x gy x gz cells (each 1 ..
 * CFSD_NN_GRID_MAX) over the bounding box of EACH batch element, computed on
 * the device and never read back.  An axis whose extent is zero (planar,
 * collinear, coincident or single points) or not finite puts every point in
 * cell 0 of that axis.  `grid` is a 16-byte aligned device buffer of
 * cfsd_nn_grid_build_workspace() bytes (0 = bad sizes), laid out as
 *   records    [br, p] x 16 bytes: x, y, z and the original index (int32 bits),
 *              grouped by cell, cell id = (cz gy + cy) gx + cx ascending;
 *   header     [br, CFSD_NN_GRID_HDR] floats: lo, cell size, inverse cell
 *              size, extent, each as x y z 0;
 *   cell_start [br, gx gy gz + 1] int32 (padded to 16 bytes): the records of
 *              cell c are [cell_start[c], cell_start[c + 1]);
 *   cell_id    [br, p] int32 (padded to 16 bytes): every point's cell.
 * Two stages with the caller's sort between them (the project's usual
 * grouping, as for cfsd_chamfer_bwd):
 *   CFSD_NN_GRID_CELLS  writes header and cell_id (sorted_ids, order: NULL);
 *   CFSD_NN_GRID_GROUP  takes sorted_ids [br, p] int32, the ids of each batch
 *                       element ascending, and order [br, p] int64, the point
 *                       at each sorted position, and writes cell_start and
 *                       the records.  The order inside a cell is free: query
 *                       results do not depend on it.
 * No atomics.
 *
 * cfsd_nn_points_grid: q [bq, n, 3] against a built grid of br sets; bq and
 * br each 1 or `batch`, as for cfsd_nn_points.  One lane per query walks the
 * cells around its own in shells of growing Chebyshev radius and stops only
 * when its best distance is STRICTLY below a lower bound (shrunk by a derived
 * rounding margin, nn_grid.hip) of everything not yet visited; at most
 * max(gx, gy, gz) shells, for any input.  dist2, idx [batch, n] as
 * cfsd_nn_points.  q_perm [n] int32 or NULL: query i writes position
 * q_perm[i] of its row (queries given in a space-filling order, results in the
 * caller's).  count [batch, n] int32 or NULL: the points evaluated per query. */
#define CFSD_NN_GRID_MAX 128
#define CFSD_NN_GRID_HDR 16
#define CFSD_NN_GRID_CELLS 0
#define CFSD_NN_GRID_GROUP 1
size_t cfsd_nn_grid_build_workspace(int br, int p, int gx, int gy, int gz);
int cfsd_nn_grid_build(const float* r, void* grid, size_t grid_bytes, int stage, const int32_t* sorted_ids,
                       const int64_t* order, int br, int p, int gx, int gy, int gz, void* stream);
int cfsd_nn_points_grid(const float* q, const void* grid, size_t grid_bytes, const int32_t* q_perm, float* dist2,
                        int32_t* idx, int32_t* count, int batch, int bq, int br, int n, int p, int gx, int gy, int gz,
                        void* stream);

/* ---------------------------------------------------------------- surface fitting
 * Distance of points to a triangle mesh (Tester._point_mesh_distance,
 * test.py:522-533: pytorch3d's point_face_distance), ABI 4.14.
 *
 * cfsd_point_face: points [bp, n, 3], verts [bv, nv, 3] fp32, faces [nf, 3]
 * int32 shared by the batch; bp and bv are each 1 or `batch` (1 = shared, read
 * in place).  Per point (b, i), over the CLOSED triangles of mesh b:
 *   dist2[b, i]    = min_f |p - c_f|^2, c_f the nearest point of face f,
 *   face_idx[b, i] = the arg min (int32; equal distances: the lowest f),
 *   bary[b, i, 0:3] = the weights of c on the face's corners (sum 1).
 * The distance is the difference form, built relative to the face's first
 * corner; one instruction sequence per pair, so a pair gives the same bits
 * wherever it is evaluated.  A zero-area face counts as its segment or point;
 * finite input gives finite output.  Face indices read from memory are
 * clamped into [0, nv).
 *
 * workspace: cfsd_point_face_workspace(bv, nf) bytes, 16-byte aligned, ALWAYS
 * needed: a pre-launch writes 64 bytes per face (corners, bounding sphere)
 * and one bounding sphere per CFSD_PF_GROUP consecutive faces there.  flags:
 *   CFSD_PF_CULL      skip groups and faces whose sphere no lane of the wave
 *                     can reach (exact: bit-identical to flags without it);
 *   CFSD_PF_PREPARED  the workspace already holds THIS mesh's records (an
 *                     earlier call with the same verts / faces): no pre-launch.
 * seed_face [batch, n] int32 (may be NULL): per point one face whose distance
 * bounds the search from the start, e.g. a face at the nearest referenced
 * vertex; any face in range is valid (clamped), it only culls.
 * stats [batch * ceil(n / 64), 2] int32 (may be NULL): per wave the groups
 * entered and the faces evaluated. */
#define CFSD_PF_GROUP 16
#define CFSD_PF_CULL 1
#define CFSD_PF_PREPARED 2
size_t cfsd_point_face_workspace(int bv, int nf);
int cfsd_point_face(const float* points, const float* verts, const int32_t* faces,
                    const int32_t* seed_face, float* dist2, int32_t* face_idx, float* bary,
                    int32_t* stats, void* workspace, size_t workspace_bytes, int batch, int bp, int bv,
                    int n, int nv, int nf, int flags, void* stream);

/* Gradient of sum_{b,i} g[b,i] dist2[b,i] through fixed faces and weights:
 *   gp[b, i] = g[b,i] 2 (p - c)                    [batch, n, 3], always written
 *   gv[b, u] = - sum_{(i,k): faces[face_idx[b,i], k] = u} gp[b, i] bary[b, i, k]
 * gv [batch, nv, 3] may be NULL (points only).  The (point, corner) pairs are
 * passed GROUPED by vertex: seg_e [batch, 3 n] = the pair numbers i * 3 + k of
 * batch b ordered by (vertex, pair) (a stable sort), seg_ptr [batch, nv + 1]
 * the offsets of each vertex's run.  One thread per vertex sums its run in
 * ascending order: deterministic, no atomics; an empty run gives zero.  With
 * bp = 1 or bv = 1 the caller sums gp or gv over the batch. */
int cfsd_point_face_bwd(const float* points, const float* verts, const int32_t* faces,
                        const int32_t* face_idx, const float* bary, const float* g, float* gp,
                        const int32_t* seg_ptr, const int32_t* seg_e, float* gv, int batch, int bp,
                        int bv, int n, int nv, int nf, void* stream);

/* ---------------------------------------------------------------- rendering
 * The pictures of ModelManager.render / log_images (model_manager.py:594-658:
 * pytorch3d's MeshRasterizer with HardGouraudShader / ShadelessShader), ABI
 * 4.15.  A deterministic z-buffer rasteriser: no atomics, two calls give the
 * same bits, a mesh gives the same bits alone or in a batch.  verts
 * [batch, nv, 3] fp32, faces [nf, 3] int32 shared by the batch (indices read
 * from memory are clamped into [0, nv)).
 *
 * Convention.  cam: 14 device floats, R [3, 3] row-major, T [3], s = 1 /
 * tan(fov / 2), znear; X_view = X R + T (row vectors), x_ndc = s x_view /
 * z_view, y_ndc = s y_view / z_view.  NDC +X points left and +Y up: pixel
 * (row i, column j) of an S x S image has its centre at x = 1 - (2j + 1) / S,
 * y = 1 - (2i + 1) / S.  A pixel is covered by a face when the three edge
 * functions of the projected triangle at the pixel centre have the sign of
 * its area or are zero (inclusive edges); no back-face culling; a face of zero
 * projected area covers nothing; a face with any vertex at z_view <= znear is
 * dropped whole (no clipping).  Barycentrics are perspective-correct,
 * w_i' = (w_i / z_i) / sum_k (w_k / z_k), z = 1 / sum_k (w_k / z_k); the nearest
 * z wins, bit-equal z: the lowest face.
 *
 * cfsd_vertex_normals: normals [batch, nv, 3] = the normalised sum over the
 * faces at a vertex of cross(v1 - v0, v2 - v0) (area weighting), 0 for a
 * vertex without a face or with a zero sum.  The faces of vertex v are
 * vf_idx[vf_ptr[v] .. vf_ptr[v + 1]) (vf_ptr [nv + 1], vf_idx [3 nf], int32:
 * the face of every corner, grouped by vertex, ascending), summed in that
 * order by one thread.
 *
 * cfsd_render_vertices: ndc [batch, nv, 2] and vz [batch, nv] (view z) of
 * every vertex.  With colors [batch, nv, 3] != NULL also the Gouraud vertex
 * colour in world space, n the vertex normal, C = -T R^T the camera centre:
 *   L = normalize(light - p), V = normalize(C - p), d = max(n.L, 0),
 *   r = 2 (n.L) n - L, spec = n.L > 0 ? max(r.V, 0)^shininess : 0,
 *   colour = (ambient + diffuse d) tex + specular spec,
 * tex [bt, nv, 3] (bt = 1 or batch) or, with tex = NULL, the constant
 * tex_value.  faces, vf_ptr, vf_idx are needed only with colors.
 *
 * cfsd_rasterize: ndc, vz as written above (or any projected vertices).
 *   pix_to_face [batch, S, S] int32, -1 = background,
 *   zbuf [batch, S, S], bary [batch, S, S, 3] fp32, -1 = background,
 * and, with colors [bc, nv, 3] (bc = 1 or batch) and image both != NULL,
 *   image [batch, 3, S, S] = the bary mix of the winning face's vertex colours,
 *   background pixels exactly (bg_r, bg_g, bg_b); nothing is clamped.
 * workspace: cfsd_raster_workspace(batch, nf) bytes, 16-byte aligned: a
 * pre-launch writes a 48-byte record per face and a pixel bounding box per
 * CFSD_RN_GROUP consecutive faces there.  1 <= S <= CFSD_RN_MAX_SIZE.
 *
 * cfsd_interpolate_colors: the same image from a finished raster stage. */
#define CFSD_RN_GROUP 16
#define CFSD_RN_MAX_SIZE 4096
size_t cfsd_raster_workspace(int batch, int nf);
int cfsd_vertex_normals(const float* verts, const int32_t* faces, const int32_t* vf_ptr,
                        const int32_t* vf_idx, float* normals, int batch, int nv, int nf, void* stream);
int cfsd_render_vertices(const float* verts, const float* cam, const int32_t* faces,
                         const int32_t* vf_ptr, const int32_t* vf_idx, const float* tex, float* ndc,
                         float* vz, float* colors, int batch, int bt, int nv, int nf, float light_x,
                         float light_y, float light_z, float ambient, float diffuse, float specular,
                         float shininess, float tex_value, void* stream);
int cfsd_rasterize(const float* ndc, const float* vz, const int32_t* faces, const float* colors,
                   int32_t* pix_to_face, float* zbuf, float* bary, float* image, void* workspace,
                   size_t workspace_bytes, int batch, int bc, int nv, int nf, int image_size, float znear,
                   float bg_r, float bg_g, float bg_b, void* stream);
int cfsd_interpolate_colors(const int32_t* pix_to_face, const float* bary, const int32_t* faces,
                            const float* colors, float* image, int batch, int bc, int nv, int nf,
                            int image_size, float bg_r, float bg_g, float bg_b, void* stream);

/* ---------------------------------------------------------------- classifiers
 * The classifier stage after the VAE (ModelManager.train_and_validate_classifiers,
 * model_manager.py:428-573): LDA / QDA on the latent code and the MLP
 * classifier (model.py:191-203), ABI 4.16.  No atomics; every reduction runs
 * in an order fixed by the shapes, so two calls give the same bits.  Dependent
 * phases are separate launches enqueued by the entry point (no grid-wide
 * barrier).  In this section a workspace too small for the shapes is a bad
 * argument: CFSD_EINVAL.
 *
 * cfsd_class_stats: z [n, ld] fp32, of which the columns [col0, col0 + d) are
 * read (a window: the region classifiers read their slice of the one latent
 * buffer in place); label [n] int32.  A row whose label lies outside
 * [0, n_classes) contributes to nothing.  Two passes in fp32 (mean first):
 *   count [C] int32, mean [C, d] (0 for an empty class),
 *   scatter [C, d, d] = sum_{i: label_i = c} (z_i - mean_c)(z_i - mean_c)^T.
 * d <= CFSD_CLS_MAX_D, n_classes <= CFSD_CLS_MAX_CLASSES.  workspace: cfsd_class_stats_workspace() bytes
 * (per-slice partial sums, merged in ascending slice order).
 *
 * cfsd_discriminant_scores: z as above; mean [C, d]; whiten [Cw, d, d] with
 * Cw = n_whiten = C (one per class: QDA) or 1 (shared: LDA); offset [C].
 *   maha2 [n, C]  = |(z_i - mean_c) whiten_c|^2
 *   scores [n, C] = -0.5 maha2 + offset_c
 *   pred [n] int32 = argmax_c scores, the lowest c among equal scores
 * (each output may be NULL).
 *
 * cfsd_mlp_fwd: the whole MLPClassifier in one launch over n rows of
 * z [n, dims[0]]: n_layers <= CFSD_MLP_MAX_LAYERS Linear layers, every width <= CFSD_MLP_MAX_WIDTH, `dims`
 * a HOST array of n_layers + 1 widths, a ReLU after EVERY layer, the last
 * included (model.py:196-197), so logits >= 0.  params: one flat fp32 buffer
 * in state_dict order, W_0 [dims[1], dims[0]], b_0, W_1, ...
 *   logits [n, dims[n_layers]], pred [n] int32 (argmax, lowest index on ties;
 *   may be NULL).
 *
 * cfsd_mlp_train_steps: n_steps consecutive steps of mlp_classifier_epoch
 * (model_manager.py:428-446) over the rows [row0 + t bs, row0 + (t + 1) bs) of
 * z [n_rows, dims[0]] / label [n_rows], bs <= CFSD_MLP_MAX_BS; two launches per step:
 *  1. one workgroup: forward; loss = sum_i w[y_i] (logsumexp(o_i) - o_i[y_i]) /
 *     sum_i w[y_i] (CrossEntropyLoss(class_weight)), acc = 100 correct / bs;
 *     acc[3] += {loss, acc, 1}; *step += 1; the activation gradients (ReLU' = 0
 *     at 0), each layer's input and output gradient left in the workspace;
 *  2. one thread per parameter: its gradient (<= 16 terms, ascending row) and
 *     the cfsd_adam update in place (m, v sized like params; *step the
 *     1-based step number).  dw_out (may be NULL, sized like params) receives
 *     the last step's gradient.
 * train == 0: launch 1 without gradients (the validation epoch); params, m,
 * v, step untouched (m, v, step, workspace may be NULL).  Labels are clamped
 * into range.  workspace: cfsd_mlp_workspace(dims, n_layers, bs) bytes. */
#define CFSD_CLS_MAX_D 128
#define CFSD_CLS_MAX_CLASSES 64
#define CFSD_MLP_MAX_LAYERS 6
#define CFSD_MLP_MAX_WIDTH 1024
#define CFSD_MLP_MAX_BS 16
size_t cfsd_class_stats_workspace(int n, int d, int n_classes);
int cfsd_class_stats(const float* z, const int32_t* label, int32_t* count, float* mean, float* scatter,
                     void* workspace, size_t workspace_bytes, int n, int ld, int col0, int d,
                     int n_classes, void* stream);
int cfsd_discriminant_scores(const float* z, const float* mean, const float* whiten, const float* offset,
                             float* maha2, float* scores, int32_t* pred, int n, int ld, int col0, int d,
                             int n_classes, int n_whiten, void* stream);
int cfsd_mlp_fwd(const float* z, const float* params, float* logits, int32_t* pred, const int* dims,
                 int n_layers, int n, void* stream);
size_t cfsd_mlp_workspace(const int* dims, int n_layers, int bs);
int cfsd_mlp_train_steps(const float* z, const int32_t* label, const float* class_weight, float* params,
                         float* m, float* v, int32_t* step, float* acc, void* workspace,
                         size_t workspace_bytes, float* dw_out, const int* dims, int n_layers, int n_rows,
                         int row0, int bs, int n_steps, int train, float lr, float beta1, float beta2,
                         float eps, float weight_decay, void* stream);

/* cfsd_mlp_head_step (ABI 4.18): the MLP classifier as a head of the VAE step
 * (classifier.mlp_training_type: end2end, model_manager.py:295-318): one step
 * of cfsd_mlp_train_steps' two launches on bs <= CFSD_MLP_MAX_BS rows of the step's latent
 * codes, whose loss gradient also flows back into the latent.
 *   z: row i < bs at z + i * row_stride * ld_z (dims[0] floats).  row_stride =
 *     bs + 1 takes the diagonal of a swapped bs x bs group
 *     (model_manager.py:297), row_stride = 1 consecutive rows.
 *   label of row i: label_table[batch_idx[i]] (batch_idx [bs] int32, the step's
 *     base-mesh indices, clamped into [0, n_labels); label_table [n_labels]
 *     int32 class indices, clamped into range).
 *  1. one workgroup: forward, loss and accuracy exactly as documented for
 *     cfsd_mlp_train_steps; acc[3] += {loss, acc, 1}.  train != 0: *step += 1,
 *     the activation gradients, and one layer further dz_i = dy_0,i . W_0 (no
 *     ReLU mask: the input is z):
 *       dlat[i * row_stride * ld_dlat + c] += w_cls * dz_i[c],  c < dims[0],
 *     a plain read-modify-write by the one thread that owns the element (in
 *     stream order after cfsd_latent_fwd wrote dlat); every other element of
 *     dlat keeps its bits.
 *  2. (train != 0) one thread per parameter: w_cls times the gradient
 *     cfsd_mlp_train_steps forms (the parameters see w_cls * loss), then
 *       m, v != NULL: the cfsd_adam update in place (dw_out, may be NULL, also
 *         receives the gradient);
 *       m == v == NULL: the gradient only, into dw_out (required): the
 *         data-parallel step, where cfsd_adam_scaled runs after the all-reduce.
 * train == 0 (the validation pass, z = mu): launch 1's loss and accuracy only;
 * nothing but acc is written (m, v, step, workspace, dlat, dw_out may be NULL).
 * No atomics; two calls on the same inputs give the same bits.  workspace:
 * cfsd_mlp_workspace(dims, n_layers, bs) bytes. */
int cfsd_mlp_head_step(const float* z, int ld_z, int row_stride, const int32_t* batch_idx,
                       const int32_t* label_table, int n_labels, const float* class_weight, float* params,
                       float* m, float* v, int32_t* step, float* acc, void* workspace, size_t workspace_bytes,
                       float* dw_out, float* dlat, int ld_dlat, float w_cls, const int* dims, int n_layers,
                       int bs, int train, float lr, float beta1, float beta2, float eps, float weight_decay,
                       void* stream);

/* ---------------------------------------------------------------- t-SNE
 * The t-SNE branch of Tester.plot_embeddings (test.py:1177-1180:
 * sklearn.manifold.TSNE(n_components=2, init='random')), ABI 4.21:
 * scikit-learn 1.7.2's method='barnes_hut' at angle = 0, i.e. kNN-sparse input
 * affinities, the EXACT repulsive term, degrees_of_freedom = 1.  No atomics:
 * every sum below has one order fixed by the sizes, two calls give the same
 * bits.  Every entry point checks its arguments before any HIP call.
 *
 * cfsd_knn_rows: z [n, d] fp32 -> idx [n, k] int32, d2 [n, k] fp32: per row
 * the k nearest OTHER rows under
 *   d2(i, j) = acc_d,  acc_0 = +0,  acc_{c+1} = fma(t_c, t_c, fma(2 e_c, t_c, acc_c)),
 *   t_c = fl(z[i,c] - z[j,c]),  e_c = (z[i,c] - z[j,c]) - t_c  (exact: Knuth's TwoSum in fp32)
 * (all fp32, ascending c, nothing else fused; never |a|^2 + |b|^2 - 2ab).  The
 * sum is rounded twice per coordinate and e_c^2 is dropped: d2 is within
 * d * 2^-23 relative of the exact distance, and exact whenever every difference
 * and partial sum is representable (small integers).  Sorted ascending by
 * (d2, j): equal distances go to the lower index.  The candidates of a row
 * are walked in ascending j, CFSD_TSNE_KNN_COLS per tile and
 * CFSD_TSNE_KNN_DIMS coordinates per staged chunk, CFSD_TSNE_KNN_ROWS query
 * rows per workgroup; the selection is a sorted insertion per row and depends
 * on none of the three.  Limits (CFSD_EINVAL): 2 <= n, 1 <= k <= min(n - 1,
 * CFSD_TSNE_MAX_K), 1 <= d <= CFSD_TSNE_MAX_D, n * k < 2^31.  A NaN
 * coordinate makes its distances NaN, which sort after every number.
 * workspace: cfsd_knn_rows_workspace() bytes -- 0 in this version (a row's k
 * best live in LDS), NULL allowed.
 *
 * cfsd_tsne_affinities: _binary_search_perplexity (sklearn/manifold/_utils.pyx)
 * per row of d2 [n, k]: beta = 1 with unbounded brackets, doubled / halved
 * while unbounded and bisected after, at most 100 evaluations, stopping at
 * |H - log(perplexity)| <= 1e-5 with H = log(sum) + beta * sum_j d2_j P_j,
 * P_j = exp(-beta d2_j) / sum, and sum == 0 replaced by 1e-8 (both constants
 * are C floats there and here).  All of it in float64; a row's sums are
 * formed by one wave (lane l adds j = l, l + 64, ..., then a fixed butterfly).
 * p_cond [n, k] = P of the LAST evaluated beta and beta [n] = that beta, both
 * rounded to fp32.  Limits: those of cfsd_knn_rows on n and k; perplexity a
 * positive finite number.
 *
 * One gradient-descent step = cfsd_tsne_forces (two launches) then
 * cfsd_tsne_update (one), no host synchronisation.  y, update, gains, grad
 * [n, 2] fp32; P a symmetric CSR: row_ptr [n + 1] int32, col [nnz] int32
 * (ascending within a row, clamped into [0, n)), val [nnz] fp32.
 * With q_ij = 1 / (1 + |y_i - y_j|^2) (fp32, the hardware reciprocal):
 *   rep_i  = sum_{j != i} q_ij^2 (y_i - y_j),  zrow_i = sum_{j != i} q_ij
 *     over ALL j != i (a distinct point at the same position counts, q = 1).
 *     Workgroups of CFSD_TSNE_ROWS rows x `splits` column ranges; a range is
 *     ceil(tiles / splits) tiles of CFSD_TSNE_TILE columns.  Per row: a tile's
 *     columns are added in ascending j onto +0, the tile sums in ascending
 *     order onto the split's, the splits' in ascending order (fp32).
 *     splits = 0 means cfsd_tsne_splits(n), a function of n alone;
 *     1 <= splits <= CFSD_TSNE_MAX_SPLITS otherwise.  Different split counts
 *     group the same terms differently (fp32 rounding only).
 *   attr_i = exaggeration * sum_j val_ij q_ij (y_i - y_j) over row i.  A row of
 *     at most CFSD_TSNE_LONG_ROW entries: lane l of one wave adds the entries
 *     l, l + 64, ... in ascending order, then the butterfly.  A longer row:
 *     thread t of 1024 adds t, t + 1024, ..., each wave's butterfly, the 16
 *     wave sums in ascending order.  CFSD_TSNE_ATT_ROWS rows per workgroup.
 *   Z = max(sum_i zrow_i, DBL_EPSILON) in float64: per attraction workgroup
 *     its rows in ascending order, then thread t of 1024 adds the workgroup
 *     sums t, t + 1024, ..., then a halving tree.
 *   grad_i = 4 (attr_i - rep_i * (float)(1 / Z))
 *   _gradient_descent's rule per coordinate, fp32, nothing fused:
 *     gains = max(update * grad < 0 ? gains + 0.2 : gains * 0.8, 0.01)
 *     update = momentum * update - learning_rate * (gains * grad);  y += update
 * want_error != 0 (pass the same flag to both calls) also writes result[0..1]:
 *   result[0] = KL = a * (sum_ij p_ij log(p_ij / q_ij) + (sum p) (log a + log Z)),
 *     a = exaggeration, i.e. the divergence of a P against q / Z as
 *     _gradient_descent reports it; float64 throughout, -log q_ij evaluated
 *     as log1p(|y_i - y_j|^2).  At the extremes where scikit-learn clamps p
 *     and q / Z at float64 eps inside the logarithm: an entry p_ij <= 0
 *     contributes 0 (the limit of p log p), log1p is finite for every finite
 *     fp32 y, and Z >= DBL_EPSILON -- so KL is finite whenever y and val are.
 *   result[1] = |gains * grad|_2 over all 2n coordinates, the norm
 *     _gradient_descent compares with min_grad_norm (after its in-place
 *     grad *= gains); float64 sum, fixed order.
 *   The update then runs as ONE workgroup; y, update, gains and grad carry the
 *   same bits with and without the flag.
 * workspace: cfsd_tsne_step_workspace(n, splits) bytes (0 for invalid sizes),
 * 16-byte aligned, the same buffer and `splits` for both calls.
 * Limits: 2 <= n <= CFSD_TSNE_MAX_N, nnz >= 0, exaggeration > 0. */
#define CFSD_TSNE_MAX_K 256
#define CFSD_TSNE_MAX_D 512
#define CFSD_TSNE_MAX_N 16777216
#define CFSD_TSNE_KNN_ROWS 16
#define CFSD_TSNE_KNN_COLS 64
#define CFSD_TSNE_KNN_DIMS 64
#define CFSD_TSNE_ROWS 512
#define CFSD_TSNE_TILE 128
#define CFSD_TSNE_MAX_SPLITS 64
#define CFSD_TSNE_LONG_ROW 256
#define CFSD_TSNE_ATT_ROWS 16
size_t cfsd_knn_rows_workspace(int n, int d, int k);
int cfsd_knn_rows(const float* z, int32_t* idx, float* d2, void* workspace, size_t workspace_bytes, int n, int d,
                  int k, void* stream);
int cfsd_tsne_affinities(const float* d2, float* p_cond, float* beta, int n, int k, float perplexity,
                         void* stream);
int cfsd_tsne_splits(int n);
size_t cfsd_tsne_step_workspace(int n, int splits);
int cfsd_tsne_forces(const float* y, const int32_t* row_ptr, const int32_t* col, const float* val,
                     void* workspace, size_t workspace_bytes, int n, int nnz, int splits, float exaggeration,
                     int want_error, void* stream);
int cfsd_tsne_update(float* y, float* update, float* gains, float* grad, float* result, const void* workspace,
                     size_t workspace_bytes, int n, int splits, float exaggeration, float momentum,
                     float learning_rate, int want_error, void* stream);

/* ---------------------------------------------------------------- surgical planning
 * The arithmetic of Tester.interpolate_syndrome_to_normal (test.py:652-748)
 * and Tester.evaluate_pre_post_pair (test.py:972-1088), ABI 4.22.  One
 * CFSD_CLS_MAX_D-thread workgroup per row of work.  Operands are fp32, every
 * product and sum is float64: thread k forms component k of a whitened vector
 * (ascending j), squared norms and dot products meet in one halving tree over
 * CFSD_CLS_MAX_D slots (part[t] += part[t + w], w = 64, ..., 1; slots past the
 * width hold 0).  No atomics; a row's result depends on no other row of the
 * call and two calls give the same bits.  Every entry point checks its
 * arguments before any HIP call.
 *
 * The grid: point i of torch.linspace(s, e, steps) in fp32, nothing fused,
 *   step = (e - s) / (steps - 1),
 *   g(i) = s + step * i            for i < steps / 2,
 *          e - step * (steps-1-i)  otherwise            (so g(steps - 1) = e).
 *
 * cfsd_plan_targets: z [n, ld], of which the window [col0, col0 + d) is read,
 * d <= CFSD_CLS_MAX_D; mean [d] and whiten [d, d] of the healthy class of a
 * QDA; levels a HOST array of n_levels <= CFSD_PLAN_MAX_LEVELS positive, finite,
 * strictly descending floats (the reference: 3, 2, 1); 2 <= steps <=
 * CFSD_PLAN_MAX_STEPS (the reference: 5000).  Per row p, with s = z[p, col0 + j]
 * and e = mean[j] per column:
 *   maha[p] = |(z_p - mean) whiten|, rounded to fp32;
 *   index[p, k] (int32): along the segment the distance shrinks linearly, so
 *     i0 = ceil((steps - 1)(1 - levels[k] / maha)) clamped to [0, steps - 1]
 *     (float64, the unrounded maha); then the grid points i0 - 1, i0, i0 + 1
 *     that exist are evaluated, |(g(i) - mean) whiten|^2 <= levels[k]^2, and the
 *     lowest one inside wins (i0 + 1, clamped, if none is).  0 for a row that is
 *     already inside, and for a row equal to the mean;
 *   targets[p, k, :] = g(index[p, k]) for k < n_levels, targets[p, n_levels, :]
 *     = mean bit for bit: [n, n_levels + 1, d].
 *
 * cfsd_plan_tables: z [n, L] and targets [n, S + 1, L] of a full-width
 * cfsd_plan_targets call (L <= CFSD_CLS_MAX_D, S = n_levels); mask [P, L]
 * uint8, the columns procedure p moves (P = n_procedures >= 0; NULL allowed for
 * P = 0); 1 <= n_first <= CFSD_PLAN_MAX_FIRST (the reference: 8).  With F =
 * n_first + S:
 *   tables [n, 1 + P, F, L].  Group 0 moves every column: rows r < n_first are
 *     the grid from z to targets[:, 0] in n_first steps (n_first = 1: z), rows
 *     n_first - 1 + t are targets[:, t], t = 1..S.  Group 1 + p holds the same
 *     in the columns with mask[p] != 0 and z, bit for bit, in every other.
 *   dist [n, 1 + P, S + 1]: dist[., g, t] = mean over all L columns of
 *     (tables[., g, n_first - 1 + t, j] - targets[., S, j])^2, the reference's
 *     d3, d2, d1, dm (compute_mse_loss against the healthy mean), rounded once.
 *
 * cfsd_pair_metrics: z_pre, z_post [n, L]; windows a HOST array [W, 4] int32 of
 * (col0, d, offset into mean, offset into whiten), W <= CFSD_PLAN_MAX_WINDOWS,
 * d <= CFSD_CLS_MAX_D; mean (mean_floats floats) and whiten (whiten_floats
 * floats) the packed healthy means [d] and whitening matrices [d, d] of the
 * windows.  raw [n, W, 6], per pair and window with a = pre - mean, b = post -
 * mean, v = post - pre over the window's columns:
 *   0: |a whiten|   1: |b whiten|   2: |a|   3: |b|
 *   4: (v . -a) / (|v| |a|), the cosine between the displacement and the ideal
 *      trajectory; NaN (0 / 0) when either is the zero vector, as numpy gives
 *      the reference; no other entry becomes NaN because of it
 *   5: |v whiten|
 * CFSD_EINVAL: a null pointer, sizes < 1, a window outside [0, L) or wider
 * than CFSD_CLS_MAX_D, an offset past mean_floats / whiten_floats. */
#define CFSD_PLAN_MAX_LEVELS 8
#define CFSD_PLAN_MAX_STEPS 1048576
#define CFSD_PLAN_MAX_FIRST 64
#define CFSD_PLAN_MAX_WINDOWS 64
int cfsd_plan_targets(const float* z, const float* mean, const float* whiten, const float* levels, float* maha,
                      int32_t* index, float* targets, int n, int ld, int col0, int d, int n_levels, int steps,
                      void* stream);
int cfsd_plan_tables(const float* z, const float* targets, const uint8_t* mask, float* tables, float* dist, int n,
                     int latent, int n_levels, int n_procedures, int n_first, void* stream);
int cfsd_pair_metrics(const float* z_pre, const float* z_post, const int32_t* windows, const float* mean,
                      const float* whiten, float* raw, int n, int latent, int n_windows, int mean_floats,
                      int whiten_floats, void* stream);

/* ---------------------------------------------------------------- embedding figures
 * The pictures of Tester.plot_embeddings / plot_embeddings_per_region
 * (test.py:1161-1321), _render_embed_save_z_interpolations (test.py:750-833)
 * and _project_pre_post_pair (test.py:1090-1136), ABI 4.23: the kernel density
 * estimates seaborn's kdeplot takes from scipy's gaussian_kde, their iso-level
 * bands shaded into an image, and point / line / arrow overlays.  No atomics;
 * every sum and every blend runs in the order of its input, so the same input
 * gives the same bits.  Every entry point checks its arguments, HOST tables
 * included, before any HIP call.  The small tables (sets, panels, layers) are
 * HOST arrays that reach the kernels by value, a few rows per launch.
 *
 * cfsd_kde2d: points [n_points, 2] float64; set_ptr a HOST array [n_sets + 1]
 * int32, set s owns the points set_ptr[s] .. set_ptr[s + 1] (ascending, within
 * [0, n_points]); params a HOST array [n_sets, 8] float64 per set: L00, L10, L11
 * (the lower-triangular factor of the inverse kernel covariance), scale, lo0,
 * step0, lo1, step1 (steps > 0); 2 <= G <= CFSD_KDE_MAX_G.  density [n_sets, G,
 * G] float64:
 *   g = (lo0 + i step0, lo1 + j step1)   (each rounded once, nothing fused)
 *   u = L^T (g - x_k) = (L00 d0 + L10 d1, L11 d1)
 *   density[s, i, j] = scale * sum_k exp(-(u0^2 + u1^2) / 2),  k in point order.
 * One thread per node, the set's points staged through LDS CFSD_KDE_CHUNK at a
 * time.  An empty set gives zeros; a set's grid does not depend on the other
 * sets of the call.
 *
 * cfsd_density_shade: image [3, H, W] fp32, shaded in place; grids a device
 * array of grid_doubles float64 holding the density grids; panels a HOST array
 * [n_panels <= CFSD_SHADE_MAX_PANELS, CFSD_SHADE_PANEL_DOUBLES]: px0, py0, pw,
 * ph (the pixel rectangle, whole numbers, inside the image, panels disjoint),
 * xlo, xhi, ylo, yhi (the data window; y grows upwards, row py0 is yhi);
 * layers a HOST array [n_layers <= CFSD_SHADE_MAX_LAYERS,
 * CFSD_SHADE_LAYER_DOUBLES]:
 *   0 panel   1 offset of the grid in `grids`   2, 3 its sizes G0, G1 (node (i, j)
 *   at offset + i G1 + j)   4 lo0   5 step0   6 lo1   7 step1   8 K (1 ..
 *   CFSD_SHADE_MAX_LEVELS)   9..16 the K ascending levels   17..20 red, green,
 *   blue, alpha in [0, 1]   21 fill (0 / 1)   22 line (0 / 1)   23 unused.
 * Per pixel (x, y) of a panel, in float64 with nothing fused:
 *   tx = (x + 0.5 - px0) / pw,  dx = xlo + tx (xhi - xlo),  u = (dx - lo0) / step0
 *   ty = (y + 0.5 - py0) / ph,  dy = yhi - ty (yhi - ylo),  v = (dy - lo1) / step1
 *   d = 0 unless 0 <= u <= G0 - 1 and 0 <= v <= G1 - 1; else with i0 = min(floor
 *   u, G0 - 2), fu = u - i0 (j0, fv alike):
 *     d = (g[i0,j0] (1 - fu) + g[i0+1,j0] fu) (1 - fv) + (g[i0,j0+1] (1 - fu) + g[i0+1,j0+1] fu) fv
 *   band b = #{k : level_k <= d}.
 * Layers apply in order, in fp32 with nothing fused: with fill and b >= 1,
 * t = min(b, K - 1) / (K - 1) (1 for K = 1), shade = (1 - t) + colour t, out =
 * out (1 - alpha) + shade alpha; with line, where b differs from the band of the
 * pixel to the right or of the pixel below (those inside the panel), out = out
 * (1 - alpha) + colour alpha.  A pixel no layer touches is not written.
 *
 * cfsd_draw_primitives: images [B, 3, H, W] fp32, composited in place; prims
 * [n_prims, CFSD_PRIM_FLOATS] fp32 and prim_ptr [B + 1] int32 on the DEVICE,
 * prims_host / prim_ptr_host the same tables on the HOST (these are checked;
 * the kernel clamps what it reads from the device copies).  Image b takes the
 * primitives prim_ptr[b] .. prim_ptr[b + 1] in order.  A row: kind, x0, y0, x1,
 * y1, x2, y2, r, red, green, blue, alpha, clip x0, y0, x1, y1 (pixels; the clip
 * rectangle [x0, x1) x [y0, y1) in whole pixels inside the image).  Coverage at
 * the pixel centre p = (x + 0.5, y + 0.5):
 *   CFSD_PRIM_DISC      clamp(r + 0.5 - |p - (x0, y0)|, 0, 1)
 *   CFSD_PRIM_SEGMENT   clamp(r + 0.5 - dist(p, segment), 0, 1), r the half-width;
 *                       a zero-length segment is the disc of radius r
 *   CFSD_PRIM_TRIANGLE  clamp(0.5 - max_i e_i(p), 0, 1), e_i the signed distance
 *                       to edge i's line, positive outside for either
 *                       orientation; nothing for a zero-area triangle
 * and out = out (1 - alpha cov) + colour (alpha cov) in fp32 where cov > 0.
 * One workgroup per tile of 32 x 8 pixels walks its image's primitives in
 * rounds of CFSD_PRIM_ROUND through LDS, each culled by the bounding box of
 * where its coverage is positive (a disc's or segment's box grown by r + 0.5;
 * for a triangle the box of its three mitre points, a tip of interior angle t
 * reaching 1 / (2 sin(t / 2)) past its vertex) against the tile and the clip
 * rectangle: the result does not depend on where the tile borders fall.
 * CFSD_EINVAL: a null pointer, G < 2, K > CFSD_SHADE_MAX_LEVELS, a decreasing
 * set_ptr / prim_ptr, a rectangle outside the image, sizes outside the limits. */
#define CFSD_KDE_CHUNK 512
#define CFSD_KDE_MAX_G 4096
#define CFSD_FIG_MAX_SIZE 8192
#define CFSD_SHADE_MAX_PANELS 16
#define CFSD_SHADE_MAX_LAYERS 4096
#define CFSD_SHADE_MAX_LEVELS 8
#define CFSD_SHADE_PANEL_DOUBLES 8
#define CFSD_SHADE_LAYER_DOUBLES 24
#define CFSD_PRIM_ROUND 256
#define CFSD_PRIM_FLOATS 16
#define CFSD_PRIM_MAX 16777216
#define CFSD_PRIM_DISC 0
#define CFSD_PRIM_SEGMENT 1
#define CFSD_PRIM_TRIANGLE 2
int cfsd_kde2d(const double* points, const int32_t* set_ptr, const double* params, double* density, int n_points,
               int n_sets, int G, void* stream);
int cfsd_density_shade(float* image, const double* grids, const double* panels, const double* layers, int H, int W,
                       int n_panels, int n_layers, int grid_doubles, void* stream);
int cfsd_draw_primitives(float* images, const float* prims, const int32_t* prim_ptr, const float* prims_host,
                         const int32_t* prim_ptr_host, int B, int H, int W, int n_prims, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFSD_H */
