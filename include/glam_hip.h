/*
 * glam_hip.h — C ABI of libglam_hip.so, the MI355X (gfx950) implementation of the GLAM
 * message-passing hot path (yvquanli/GLAM src_1gp/layer.py + model.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *   - tensors are dense, row-major, fp32 ("f32") or int32/int64 as typed;
 *   - `stream` is a hipStream_t passed as void*; every entry point only enqueues work on it
 *     (no host synchronisation, no allocation), so calls are hipGraph-capturable;
 *   - return value: 0 = ok, <0 = error (GLAM_E_*); glam_last_error() returns a per-thread message.
 *     Nothing aborts; the Python mirror turns errors into RuntimeError/IndexError the way the
 *     reference raises Python exceptions (src_1gp/trainer.py:54, loss.py:56-57).
 *   - channel padding: node-feature rows are laid out [N, H, Cp] with Cp % 4 == 0 (16-byte
 *     vector loads); the host mirror zero-pads C = 15/30/45/90 to 16/32/48/92.
 *   - per-node scalar pairs are packed as [N, 8] f32: slots 0..3 = per-head "i" value,
 *     slots 4..7 = per-head "j" value (H <= 4).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).
 */
#ifndef GLAM_HIP_H
#define GLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLAM_ABI_VERSION 4   /* bumped whenever an exported signature changes or an entry point goes away */

#define GLAM_OK 0
#define GLAM_E_INVALID (-1)     /* bad argument (null pointer, negative size, misaligned) */
#define GLAM_E_UNSUPPORTED (-2) /* shape outside the compiled kernel table */
#define GLAM_E_HIP (-3)         /* HIP runtime error at launch */

int glam_abi_version(void);
const char* glam_last_error(void);

/* Which of the library's alternative routes are switched on in THIS process (the environment is read once, by the library):
 * "x3" = every dense product of the layer / GRU kernels in 3 x bf16 form on the bf16 matrix cores (GLAM_X3, default 1),
 * "wgrad_x3" = the weight-gradient products on the warp-specialised 3 x bf16 kernel (GLAM_WGRAD_X3, default 1; needs "x3").
 * The host side asks here instead of parsing the variables itself, so that both sides always agree on a route.
 * Replaces: nothing in the reference (it has one route).  Returns 1 / 0, GLAM_E_INVALID for an unknown name. */
int glam_route_enabled(const char* route);

/* Per-launch kernel timing (measurement aid of bench.py; the reference has no profiling hooks at all —
 * only wall-clock suffixes in its log lines, src_1gp/trainer.py:140-147).
 * Between glam_prof_begin(capacity) and glam_prof_end() every kernel this library launches is bound to a
 * (start, stop) event pair stamped with the dispatch's own begin / end timestamps — what a rocprofv3 kernel trace
 * reports.  Timed launches are NOT hipGraph-capturable: profile eager calls only.  glam_prof_end() returns the
 * number of launches recorded (at most `capacity`; launches beyond it go out untimed).  glam_prof_read(i, ...)
 * waits for launch i and returns its kernel name (host buffer), grid size in blocks and duration in microseconds.
 * Process-global, not thread-safe: one profiling session at a time. */
int glam_prof_begin(int capacity);
int glam_prof_end(void);
int glam_prof_read(int i, char* name_host, int name_cap, int32_t* grid_host, float* usec_host);

/* Zero-padded copies of up to 8 parameter tensors in ONE launch, and their gradients back in one.
 * Replaces: nothing in the reference (it has no padded layouts); on this side it replaces the F.pad / slice-copy pairs that
 * re-lay a GRU's gate matrices [3C, C] -> [3Cp, Cp] (src_1gp/layer.py:247) and a Linear's [M, K] -> [Mp, Kp] (src_1gp/layer.py:229)
 * once per model pass when hid_dim = 15 * hid_dim_alpha is not a multiple of four (src_1gp/glam.py:60: four of five widths).
 * Tensor t is row-major [d0, d1, d2], its padded form [d0, p1, p2]; dims = n x {d0, d1, d2, p1, p2}; src / dst are HOST arrays of n
 * device pointers.  backward = 0: dst[t] (padded) <- src[t] (plain), zeros in the pad.  backward = 1: dst[t] (plain gradient) <-
 * src[t] (padded gradient; NULL = that gradient does not exist: zeros). */
int glam_pad_group(int n, const float* const* src, float* const* dst, const int32_t* dims, int backward, void* stream);

/* 64-bit content fingerprint of up to four device buffers (bufs / nbytes: HOST arrays of n device pointers and byte counts, each
 * 4-byte aligned and a multiple of 4 bytes) into the device word out_dev, in one launch; position-sensitive, independent of the
 * launch geometry.  Replaces: nothing in the reference — its trainer collates and copies a fresh batch every iteration
 * (src_1gp/trainer.py:292-295), so a batch that comes back every epoch (the loader does not shuffle: trainer.py:37-38) can only be
 * recognised by content; glam_amd.graphs keys its staged index structures and captured hipGraphs on the fingerprint of
 * (edge_index, batch, edge_attr).  Not for use inside a stream capture by the caller that wants to read the word back. */
int glam_batch_fingerprint(int n, const void* const* bufs, const int64_t* nbytes, uint64_t* out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CSR staging of a COO edge list.
 * Replaces: the per-call index_select/scatter bookkeeping PyG's MessagePassing.propagate does for
 * `self.propagate(edge_index, ...)` (src_1gp/layer.py:40, :86) — edge_index int64 [2,E], row 0 =
 * source j, row 1 = target i.
 *   by = 0: group edges by TARGET (edge_index[1]); nbr[] holds the source of each grouped edge.
 *   by = 1: group edges by SOURCE (edge_index[0]); nbr[] holds the target (the transpose, used by
 *           the backward pass to scatter to sources without atomics).
 * Within a segment edges keep their original order (stable), so results are bit-reproducible.
 * rowptr int32[N+1], nbr int32[E], eid int32[E] (original edge id of each grouped edge).
 * err_flag int32[1]: set to 1 by the kernels if any index is outside [0,N) (such edges are
 * dropped); the caller decides when to read it back.
 * ws: scratch of at least glam_csr_workspace_bytes(N,E) bytes. */
size_t glam_csr_workspace_bytes(int64_t N, int64_t E);
int glam_csr_build(const int64_t* edge_index, int64_t N, int64_t E, int by, int32_t* rowptr, int32_t* nbr,
                   int32_t* eid, int32_t* err_flag, void* ws, size_t ws_bytes, void* stream);

/* Segment pointer of a sorted graph-id vector: ptr int32[B+1] from batch int64[N] (non-decreasing),
 * as produced by PyG collation and consumed by global_*_pool(x, batch) (src_1gp/layer.py:202). */
int glam_batch_ptr(const int64_t* batch, int64_t N, int64_t B, int32_t* ptr, int32_t* err_flag, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused neighbour gather + attention logits + per-target segment softmax + weighted scatter-add.
 * Replaces: PyG propagate -> TripletMessage.message -> aggregate (src_1gp/layer.py:40-55; softmax
 * at :51 with the +1e-16 denominator; aggr='add' at :17) when emul=1, and
 * TripletMessageLight.message -> aggregate (src_1gp/layer.py:88-97) when emul=0.
 *
 *   logit[e,h] = leaky_relu(a_ij[dst,h] + sum_k edge_attr[e,k]*M[k,h] + a_ij[src,4+h], slope)
 *   alpha      = segment softmax of logit over the incoming edges of dst
 *   emul=1: aggr[n,h,:] = sum_e alpha[e,h] * (sum_k edge_attr[e,k]*w_edge[k,h,:]) * xw[src,h,:]
 *   emul=0: aggr[n,h,:] = sum_e alpha[e,h] * xw[src,h,:]
 *
 * xw f32[N,H,Cp]; a_ij f32[N,8]; edge_attr f32[E,De] (De in {4,8}, zero padded by the host);
 * w_edge f32[De,H,Cp] (ignored when emul=0); M f32[De,4]; CSR by target (rowptr,src,eid).
 * Outputs: aggr f32[N,H,Cp]; stats f32[N,8] = per-head segment max (0..3) and exp-sum (4..7), the
 * only state the backward pass needs to recompute alpha. */
int glam_triplet_fwd(const float* xw, const float* a_ij, const float* edge_attr, const float* w_edge,
                     const float* M, const int32_t* rowptr, const int32_t* src, const int32_t* eid, int64_t N,
                     int64_t E, int H, int Cp, int De, int emul, float slope, float* aggr, float* stats,
                     void* stream);

/* Backward of glam_triplet_fwd (what torch autograd derives for src_1gp/layer.py:42-55 + PyG softmax /
 * scatter).  Two launches + one partial reduction, no atomics:
 *   B1 (by target):  alpha_e f32[E,4], dpre_e f32[E,4] (grad of the pre-activation logit),
 *                    d_a_ij[:,0:4], d_w_edge f32[De,H,Cp], d_M f32[De,4], optional d_edge_attr f32[E,De];
 *   B2 (by source, CSR transpose colptr/dst/eid_t):  d_xw f32[N,H,Cp], d_a_ij[:,4:8].
 * d_edge_attr may be NULL.  ws >= glam_triplet_bwd_workspace_bytes(...) bytes of scratch. */
size_t glam_triplet_bwd_workspace_bytes(int64_t N, int64_t E, int H, int Cp, int De);
int glam_triplet_bwd(const float* xw, const float* a_ij, const float* edge_attr, const float* w_edge,
                     const float* M, const float* aggr, const float* stats, const float* d_aggr,
                     const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int32_t* colptr,
                     const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E, int H, int Cp, int De,
                     int emul, float slope, float* d_xw, float* d_a_ij, float* d_w_edge, float* d_M,
                     float* d_edge_attr, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Graph readouts over contiguous node segments ptr int32[B+1].
 * Replaces: global_mean_pool / global_add_pool / global_max_pool / global_sort_pool(k) as called by
 * GlobalPool5.forward (src_1gp/layer.py:201-203).
 *   glam_pool5_fwd: out f32[B, (2+k)*D] = mean | add | the k rows with the largest LAST channel in
 *   descending order (ties: lower node index first; short graphs zero padded); topk_idx int32[B,k]
 *   (node index or -1) is saved for the backward pass.  k <= 8. */
int glam_pool5_fwd(const float* x, const int32_t* ptr, int64_t N, int64_t B, int D, int k, float* out,
                   int32_t* topk_idx, void* stream);
int glam_pool5_bwd(const float* d_out, const int32_t* ptr, const int32_t* topk_idx, int64_t N, int64_t B,
                   int D, int k, float* d_x, void* stream);
/* The same readout on zero-padded rows: x / d_x rows are ld floats apart and hold D channels, ld = D rounded up to a multiple
 * of four (ld <= 128; hid_dim 15 / 30 / 45 / 90 of src_1gp/glam.py:60 flow as 16 / 32 / 48 / 92), columns D..ld zero.  out / d_out
 * stay the compact [B, (2+k)*D] of the reference, the sort key is channel D - 1; d_x's pad columns are written as zeros.  ld == D
 * is glam_pool5_fwd / _bwd. */
int glam_pool5_padded_fwd(const float* x, const int32_t* ptr, int64_t N, int64_t B, int ld, int D, int k, float* out,
                          int32_t* topk_idx, void* stream);
int glam_pool5_padded_bwd(const float* d_out, const int32_t* ptr, const int32_t* topk_idx, int64_t N, int64_t B,
                          int ld, int D, int k, float* d_x, void* stream);

/* mode 0 = sum, 1 = mean, 2 = max (empty segment -> 0; argmax int32[B,D] saved for backward, may be
 * NULL for modes 0/1).  Replaces torch_scatter.scatter(x, batch, dim=0, reduce=...) behind PyG's
 * global_{add,mean,max}_pool. */
int glam_segment_pool_fwd(const float* x, const int32_t* ptr, int64_t N, int64_t B, int D, int mode, float* out,
                          int32_t* argmax, void* stream);
int glam_segment_pool_bwd(const float* d_out, const int32_t* ptr, const int32_t* argmax, int64_t N, int64_t B,
                          int D, int mode, float* d_x, void* stream);

/* Segment-softmax attention readout: out[g,:] = sum_{n in g} softmax_g(gate)[n] * v[n,:]
 * (softmax with the same +1e-16 denominator as PyG's utils.softmax).
 * Replaces: PyG GlobalAttention.forward behind GlobalLAPool (src_1gp/layer.py:206-220) and the
 * attention step of Set2Set (src_1gp/model.py:41).  gate f32[N]; v f32[N,D]; out f32[B,D];
 * stats f32[B,2] = segment max, exp-sum (saved for the backward pass). */
int glam_segment_attn_fwd(const float* gate, const float* v, const int32_t* ptr, int64_t N, int64_t B, int D,
                          float* out, float* stats, void* stream);
int glam_segment_attn_bwd(const float* gate, const float* v, const float* out, const float* stats,
                          const float* d_out, const int32_t* ptr, int64_t N, int64_t B, int D, float* d_gate,
                          float* d_v, void* stream);

/* Generic edge -> node reduction over a CSR-by-target:  out[n,:] = reduce_{e in seg(n)} msg[eid[e],:]
 * mode 0 = sum, 1 = mean, 2 = max (empty segment -> 0; argmax int32[N,D] = winning edge id, saved for
 * backward, may be NULL for modes 0/1).
 * Replaces: PyG MessagePassing.aggregate -> torch_scatter.scatter(msg, edge_index[1], dim=0, dim_size=N,
 * reduce=aggr) for message functions that stay in PyTorch, e.g. NNConv(aggr='mean')
 * (src_1gp/layer.py:119), GCNConv (src_1gp/layer.py:146). */
int glam_edge_reduce_fwd(const float* msg, const int32_t* rowptr, const int32_t* eid, int64_t N, int64_t E, int D,
                         int mode, float* out, int32_t* argmax, void* stream);
int glam_edge_reduce_bwd(const float* d_out, const int32_t* rowptr, const int32_t* eid, const int32_t* argmax,
                         int64_t N, int64_t E, int D, int mode, float* d_msg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense ends of the layer on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32).
 * Replaces: torch.matmul(x, weight_node) (src_1gp/layer.py:37), torch.matmul(aggr, weight_scale) + bias
 * (src_1gp/layer.py:58-60) and the matmuls autograd derives from them.
 *   glam_ts_gemm_make_image: lays a weight W[K, M] (logical W[k][m] = transW ? W[m*ldw+k] : W[k*ldw+m]) out as the
 *                    LDS image the GEMM blocks copy verbatim (glam_ts_gemm_image_bytes(K, M) bytes).
 *   glam_ts_gemm:    out[N, M1|M2] = [A1 | A2][N, K1+K2] @ W (+ bias on the M1 columns); all K*, M*, ld* % 4 == 0;
 *                    K1+K2 <= 192 with M <= 64, or K1+K2 <= 64 with M <= 192.
 *   glam_wgrad_gemm: out[i*stride_i + j*stride_j] = sum_n [P1 | P2 | 1][n, i] * [Q | 1][n, j]  (reduction over the
 *                    N rows; `ones` / `qones` append an all-ones column on either side, i.e. the bias gradient);
 *                    I <= 320 (five 64-column slabs), J <= 64 (ones columns included); also 64 < J (+ qones) <= 128,
 *                    computed as two column chunks in one launch. */
size_t glam_ts_gemm_image_bytes(int K, int M);
int glam_ts_gemm_make_image(const float* W, int ldw, int transW, int K, int M, float* img, void* stream);
/* The four images of a linear pair (W_a, W_b f32[M,K] as torch.nn stores them; e.g. a GRU's weight_ih / weight_hh) in one
 * launch: forward images (x @ W^T: glam_ts_gemm_image_bytes(K, M)) and input-gradient images (dy @ W: ..._bytes(M, K)). */
int glam_ts_gemm_make_image_quad(const float* Wa, const float* Wb, int K, int M, float* img_a_fwd, float* img_b_fwd,
                                 float* img_a_bwd, float* img_b_bwd, void* stream);

/* glam_ts_gemm_make_image_quad for a GRU's gate matrices w_ih, w_hh f32[3 C, C] (K = C, M = 3 C) PLUS the two gate-padded images of
 * glam_gru_fused_make_images in the same launch (fused_*: glam_gru_fused_image_bytes() each): the six re-layouts of one MessageBlock's
 * GRU (src_1gp/layer.py:246, 262) change together after every optimizer step.  C <= 64, a multiple of 4. */
int glam_gru_make_images(const float* w_ih, const float* w_hh, int C, float* img_a_fwd, float* img_b_fwd, float* img_a_bwd,
                         float* img_b_bwd, float* fused_ih, float* fused_hh, void* stream);
int glam_ts_gemm(const float* A1, int K1, int lda1, const float* A2, int K2, int lda2, const float* Wimg,
                 const float* bias, float* out1, int M1, int ldo1, float* out2, int M2, int ldo2, int64_t N,
                 void* stream);
/* glam_wgrad_gemm_pair: two independent products (same N) in one launch + one reduction: the d_W / d_b of two linears
 * that are applied side by side (the input and hidden gate linears of the GRU step, src_1gp/layer.py:262).  Workspace:
 * glam_wgrad_workspace_bytes() (sized for two products). */
int glam_wgrad_gemm_pair(const float* Pa, int Ia, int ldpa, int ones_a, const float* Qa, int Ja, int ldqa, int qones_a,
                         int qcelu_a, float* out_a, int si_a, int sj_a, const float* Pb, int Ib, int ldpb, int ones_b,
                         const float* Qb, int Jb, int ldqb, int qones_b, int qcelu_b, float* out_b, int si_b, int sj_b,
                         int64_t N, void* ws, size_t ws_bytes, void* stream);
/* [d_W | d_b] of two linears y = [x | 1] W^T (the GRU's gate linears, src_1gp/layer.py:247) in one launch + one reduction with
 * weights and biases in SEPARATE contiguous outputs: dw_x f32[I, J] = P_x^T Q_x, db_x f32[I] = column sums of P_x; optional
 * addends laid out like the outputs (gradient carry; N > 0 when one is given).  qcelu_x: Q_x is consumed as celu(Q_x). */
int glam_wgrad_gemm_pair_split(const float* Pa, int Ia, int ldpa, const float* Qa, int Ja, int ldqa, int qcelu_a, float* dw_a,
                               float* db_a, const float* Pb, int Ib, int ldpb, const float* Qb, int Jb, int ldqb, int qcelu_b,
                               float* dw_b, float* db_b, int64_t N, void* ws, size_t ws_bytes, const float* add_w_a,
                               const float* add_b_a, const float* add_w_b, const float* add_b_b, void* stream);

/* glam_wgrad_gemm (one P block, J <= 64) summed over nseg <= 3 operand sets of N rows each (+ an optional addend laid out like out): the
 * weight gradient of a tall matmul that a block applies message_steps times with shared weights — NNConv's relation product
 * [x_r | 1]^T dy, /root/reference/src_1gp/layer.py:115-122 — as ONE launch + ONE reduction.  GLAM_E_UNSUPPORTED when N is shorter than a
 * wave's row range. */
int glam_wgrad_gemm_sets(int nseg, const float* const* P, int I, int ldp, int ones, const float* const* Q, int J, int ldq, int64_t N,
                         float* out, int stride_i, int stride_j, const float* addend, void* ws, size_t ws_bytes, void* stream);

/* glam_wgrad_gemm_pair_split summed over nseg <= 3 operand sets of N rows each — Pa[s], Qa[s], Pb[s], Qb[s] with the same widths and
 * row strides — in ONE launch + ONE reduction: the weight gradients of a block applied message_steps times with shared weights
 * (/root/reference/src_1gp/model.py:53-54; the GRU's two gate matrices, src_1gp/layer.py:247) are one product over all its
 * applications instead of one per application.  N must be at least a wave's row range (GLAM_E_UNSUPPORTED otherwise: run the sets
 * one by one with the addends). */
int glam_wgrad_gemm_pair_split_seg(int nseg, const float* const* Pa, int Ia, int ldpa, const float* const* Qa, int Ja, int ldqa, int qcelu_a,
                                   float* dw_a, float* db_a, const float* const* Pb, int Ib, int ldpb, const float* const* Qb, int Jb,
                                   int ldqb, int qcelu_b, float* dw_b, float* db_b, int64_t N, void* ws, size_t ws_bytes,
                                   const float* add_w_a, const float* add_b_a, const float* add_w_b, const float* add_b_b, void* stream);

/* Both weight gradients of a GRU step (torch.nn.GRU(C, C), /root/reference/src_1gp/layer.py:247, :262) from the ONE gate-gradient
 * matrix glam_gru_bwd_ws writes when its d_gh is NULL: D[n] = [d_pr | d_pz | d_pn | d_pn r], 4C floats per row.  d_gi = D[:, 0:3C] and
 * d_gh = [D[:, 0:2C] | D[:, 3C:4C]] are column blocks of it:
 *   dw_ih[3C, C] = d_gi^T X (celu(X) with qcelu), db_ih[3C] = column sums of d_gi, dw_hh[3C, C] = d_gh^T H, db_hh[3C] = column sums of d_gh,
 * summed over nseg <= 3 operand sets (D[s], X[s], H[s]) of N rows each (X, H with row strides ldx, ldh), + optional addends laid out
 * like the outputs — glam_wgrad_gemm_pair_split_seg on the two expanded matrices, bit for bit, without their 2C duplicated columns
 * in memory.  C a multiple of 4, C + 1 <= 64.  ws >= glam_wgrad_workspace_bytes(). */
int glam_wgrad_gemm_gru_gates_seg(int nseg, const float* const* D, int C, const float* const* X, int ldx, int qcelu,
                                  const float* const* H, int ldh, float* dw_ih, float* db_ih, float* dw_hh, float* db_hh, int64_t N,
                                  void* ws, size_t ws_bytes, const float* add_w_ih, const float* add_b_ih, const float* add_w_hh,
                                  const float* add_b_hh, void* stream);

/* glam_wgrad_gemm in full ([P1 | P2 | 1]^T Q, output strides, J <= 128) summed over nseg <= 3 operand sets of N rows each (+ an
 * optional addend laid out like out): the N-deep weight gradients of the wide TripletMessage over all applications of the layer. */
int glam_wgrad_gemm_sets2(int nseg, const float* const* P1, int I1, int ldp1, const float* const* P2, int I2, int ldp2, int ones,
                          const float* const* Q, int J, int ldq, int64_t N, float* out, int stride_i, int stride_j, const float* addend,
                          void* ws, size_t ws_bytes, void* stream);
/* [d_W | d_b] of ONE linear y = [act(x) | 1] W^T with up to 127 inputs, weight and bias gradients in separate contiguous tensors with
 * optional addends (the gradient carry): dw[I, J] = P^T act(Q) (+ add_w), db[I] = column sums of P (+ add_b); act = CELU(alpha = 1)
 * when q_celu (the CELU in front of a MessageBlock's GRU, /root/reference/src_1gp/layer.py:261, folded into the gate product of a
 * wide layer).  J % 4 == 0, J + 1 <= 128, I <= 320, N >= 1. */
int glam_wgrad_gemm_linear(const float* P, int I, int ldp, const float* Q, int J, int ldq, int q_celu, float* dw, float* db,
                           const float* add_w, const float* add_b, int64_t N, void* ws, size_t ws_bytes, void* stream);
/* ... summed over nseg <= 3 operand sets of N rows each (the applications of a block that shares the linear: see
 * glam_wgrad_gemm_pair_split_seg). */
int glam_wgrad_gemm_linear_sets(int nseg, const float* const* P, int I, int ldp, const float* const* Q, int J, int ldq, int q_celu,
                                float* dw, float* db, const float* add_w, const float* add_b, int64_t N, void* ws, size_t ws_bytes,
                                void* stream);
/* glam_wgrad_gemm for ONE linear y = [x | 1] W^T with the weight and bias gradients in separate contiguous tensors:
 * dw[I, J] = P^T Q (P = dy f32[N, I], Q = x f32[N, J]), db[I] = column sums of P.  ceil4(J) + 1 <= 64, I <= 320; J need not be a
 * multiple of 4 when ldq >= ceil4(J) (a weight narrower than its zero-padded input: dw stays contiguous [I, J]). */
int glam_wgrad_gemm_split(const float* P, int I, int ldp, const float* Q, int J, int ldq, float* dw, float* db, int64_t N, void* ws,
                          size_t ws_bytes, void* stream);
/* ... of a linear whose output went through a ReLU (LinearBlock + ReLU, src_1gp/layer.py:232-237): P = dy * (Y > 0) with Y f32[N, I]
 * (row stride ldp) = the saved output — the ReLU's backward inside the product instead of an elementwise launch in front of it. */
int glam_wgrad_gemm_split_relu(const float* P, const float* Y, int I, int ldp, const float* Q, int J, int ldq, float* dw, float* db,
                               int64_t N, void* ws, size_t ws_bytes, void* stream);
/* out[N, M] = max(A[N, K] @ W + bias, 0): the Linear + ReLU of a LinearBlock (src_1gp/layer.py:232-237) whose shape runs on the
 * warp-specialised tall kernel (glam_ts_gemm_relu_supported(K, M): the input embeddings 15 -> 60 of the parity configuration and of the
 * two-tower models) — the activation in the product's epilogue instead of an elementwise launch behind it.  Wimg, alignment and
 * leading dimensions as glam_ts_gemm. */
int glam_ts_gemm_relu_supported(int K, int M);
int glam_ts_gemm_relu(const float* A, int K, int lda, const float* Wimg, const float* bias, float* out, int M, int ldo, int64_t N,
                      void* stream);
/* ... with the TRAINING-mode RReLU(rr_lower, rr_upper) of /root/reference/src_1gp/model.py:31 (the reference's default activation) in the
 * epilogue and, out_drop non-NULL, out_drop = Dropout(drop_p)(out): the twin the block behind starts with (layer.py:255-256) — from the
 * device-side Philox stream: the words glam_bias_res_act_rng_fwd draws for the same elements at the same stream position, so
 * glam_ts_gemm + glam_bias_res_act_rng_fwd and this ONE launch write the same bits, and glam_bias_res_act_rng_bwd with rng_eff is its
 * activation backward.  out, out_drop: [N, M] contiguous.  Shapes: glam_ts_gemm_rrelu_supported (K <= 64, M <= 64: the input embeddings
 * mol_lin0 / pro_lin0 of model.py:40-49). */
int glam_ts_gemm_rrelu_supported(int K, int M);
/* The input embedding in front of a TripletMessage (/root/reference/src_1gp/model.py:49, :53) with the TripletMessage's node product of
 * its rows in the same launch: out = act(A @ W + bias) — act 0: none, 1: ReLU, 4: training-mode RReLU (+ the dropped twin out_drop,
 * as glam_ts_gemm_rrelu; rng_* unused otherwise) — and xw[N, node_cols] | a_ij[N, 8] = out (out_drop when given) @ [W_node | Wa] from
 * node_pre (staged + glam_triplet_staged_node_fragments): what glam_ts_gemm writes for the same rows, bit for bit.
 * glam_triplet_layer_fwd_ell with x = NULL then starts at its aggregate launch.  Shapes: glam_ts_gemm_rrelu_supported(K, M), M = the
 * layer's Cp >= 24, 56 < node_cols = H * Cp <= 184. */
int glam_ts_gemm_act_node(const float* A, int K, int lda, const float* Wimg, const float* bias, int M, int64_t N, int act, float rr_lower,
                          float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff, float* out, float* out_drop,
                          const void* node_pre, int node_cols, float* xw, float* a_ij, void* stream);
int glam_ts_gemm_rrelu(const float* A, int K, int lda, const float* Wimg, const float* bias, int M, int64_t N, float rr_lower,
                       float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff, float* out, float* out_drop, void* stream);

/* glam_ts_gemm with the CELU(alpha=1) that MessageBlock applies in front of its GRU (src_1gp/layer.py:261) folded in:
 * a_celu = 1: out = celu(A) @ W + bias; cgrad_src non-NULL: out[r,c] *= celu'(cgrad_src[r,c]) (the chain rule of the same
 * fold on the way back); qcelu_* in glam_wgrad_gemm_pair: the weight gradient uses celu(Q). */
int glam_ts_gemm_celu(const float* A, int K, int lda, int a_celu, const float* Wimg, const float* bias, float* out, int M,
                      int ldo, const float* cgrad_src, int ld_cgrad, int64_t N, void* stream);
/* out[N, M] = A[N, K] @ W + bias + addend[N, M] (row pitch ld_add, a multiple of 4): a second gradient path into the same tensor
 * (the GRU backward's d_h = d_gh @ W_hh^T + the direct z * g term) without an add launch. */
int glam_ts_gemm_add(const float* A, int K, int lda, const float* Wimg, const float* bias, float* out, int M, int ldo,
                     const float* addend, int ld_add, int64_t N, void* stream);
/* Two products that share N and the kernel variant in ONE launch (the GRU's gate linears gi = celu(x) W_ih^T + b_ih and
 * gh = h W_hh^T + b_hh of src_1gp/layer.py:261-262, and the two input-gradient products of their backward), each with every option of
 * glam_ts_gemm_celu / glam_ts_gemm_add: out_x = act_x(A_x) @ W_x (+ bias_x) (* celu'(cgrad_x)) (+ addend_x).  Besides the dispatch it
 * saves, the second product's blocks share the CUs with the first's (two 8-wave blocks per CU for the 48 KB-image variants). */
int glam_ts_gemm_pair(const float* Aa, int Ka, int lda, int a_celu_a, const float* Wimg_a, const float* bias_a, float* out_a, int Ma,
                      int ldo_a, const float* cgrad_a, int ld_cgrad_a, const float* addend_a, int ld_add_a, const float* Ab, int Kb,
                      int ldb, int a_celu_b, const float* Wimg_b, const float* bias_b, float* out_b, int Mb, int ldo_b,
                      const float* cgrad_b, int ld_cgrad_b, const float* addend_b, int ld_add_b, int64_t N, void* stream);
size_t glam_wgrad_workspace_bytes(void);
int glam_wgrad_gemm(const float* P1, int I1, int ldp1, const float* P2, int I2, int ldp2, int ones, const float* Q,
                    int J, int ldq, int qones, int64_t N, float* out, int stride_i, int stride_j, void* ws,
                    size_t ws_bytes, void* stream);
/* glam_wgrad_gemm + addend (f32, the strides of out): out = product + addend.  The gradient carry of a weight that a block applies
 * several times per forward (src_1gp/model.py:53-54) is summed by the reduction instead of an add launch.  N > 0. */
int glam_wgrad_gemm_add(const float* P1, int I1, int ldp1, const float* P2, int I2, int ldp2, int ones, const float* Q,
                        int J, int ldq, int qones, int64_t N, float* out, int stride_i, int stride_j, const float* addend,
                        void* ws, size_t ws_bytes, void* stream);

/* The derived weights of a model pass in ONE launch (three launches of ~5 us each at the head of every training step before): the staged
 * images of a TripletMessage (exactly glam_triplet_stage_params; staged == NULL: none) and n_images <= 6 weight images of
 * glam_ts_gemm (exactly glam_ts_gemm_make_image each: dims[4 q ..] = {ldw, transW, K, M} of image q — e.g. the four images of a GRU's
 * gate matrices and the one of the input linear, /root/reference/src_1gp/model.py:40-42).  transW = 2 / 3 makes image q one matrix's
 * half of a glam_gru_ws_make_pre image instead: {ldw = C, 2: forward image | 3: backward image, K = C, M = 0: weight_ih | 1: weight_hh},
 * img[q] = that image (the two matrices' jobs name the same one). */
int glam_prestage(const float* weight_node, const float* weight_edge, const float* att, const float* weight_scale, const float* bias,
                  int C, int H, int De, int Cp, int Dp, float* staged, int n_images, const float* const* W, const int* dims,
                  float* const* img, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole TripletMessage layer (src_1gp/layer.py:36-61) as one enqueue per direction.  All node-feature
 * widths are the padded Cp (x f32[N,Cp], out f32[N,Cp]; the host mirror pads/slices when C % 4 != 0).
 *   glam_triplet_stage_params: parameters -> `staged` (glam_triplet_staged_floats floats): the four GEMM weight
 *     images ([W_node | Wa_i | Wa_j] with the separable-attention columns, W_scale, and their transposes),
 *     W_edge head-padded, M f32[Dp,4], bias padded.
 *   glam_triplet_layer_fwd:  x -> (xw, a_ij) -> aggr, stats -> out          (2 launches)
 *   glam_triplet_layer_bwd:  d_out -> d_x and `dstaged` (glam_triplet_dstaged_floats floats: d_Wcat[Cp,H*Cp+8] |
 *                            d_WsB[H*Cp+1,Cp] (last row = d_bias) | d_We_p | d_M), optional d_edge_attr
 *                            (9 launches, no atomics)
 *   glam_triplet_stage_params_bwd: chain rule from `dstaged` back to weight_node / weight_edge /
 *                            weight_triplet_att / weight_scale / bias.
 * Limits: H*Cp + 8 <= 192 and Cp <= 64 (C <= 60 at H = 3). */
size_t glam_triplet_staged_floats(int H, int Cp, int Dp);
/* offsets (floats) inside `staged` of [W_node | Wa] (K = Cp rows, H * Cp + 8 columns): as its k_ts_gemm image (what the layer's own node
 * GEMM reads), and as the pre-split operand fragments of the node product inside the GRU step (72 KB: node_pre of
 * glam_gru_ws_fwd_pre_node; (size_t)-1 where the shape has none: H * Cp + 8 <= 64) */
size_t glam_triplet_staged_node_image(int H, int Cp, int Dp);
size_t glam_triplet_staged_node_fragments(int H, int Cp, int Dp);
size_t glam_triplet_dstaged_floats(int H, int Cp, int Dp);
int glam_triplet_stage_params(const float* weight_node, const float* weight_edge, const float* att,
                              const float* weight_scale, const float* bias, int C, int H, int De, int Cp, int Dp,
                              float* staged, void* stream);
int glam_triplet_stage_params_bwd(const float* weight_node, const float* weight_edge, const float* att,
                                  const float* dstaged, int C, int H, int De, int Cp, int Dp, float* d_weight_node,
                                  float* d_weight_edge, float* d_att, float* d_weight_scale, float* d_bias,
                                  void* stream);
/* Wide layers (H*Cp + 8 > 192: hid_dim_alpha = 6 of the reference's search space, glam.py:60): the same derived
 * parameters as plain row-major matrices for library GEMMs, `plain` = Wcat f32[Cp, H*Cp+8] | Ws_p f32[H*Cp, Cp] |
 * We_p f32[Dp, H*Cp] | M f32[Dp, 4] | bias_p f32[Cp] (glam_triplet_plain_floats floats).  The host mirror sequences
 * library GEMMs, glam_triplet_fwd / _bwd and glam_wgrad_gemm around it, fills a `dstaged` buffer and calls
 * glam_triplet_stage_params_bwd (which has no width limit). */
size_t glam_triplet_plain_floats(int H, int Cp, int Dp);
int glam_triplet_stage_plain(const float* weight_node, const float* weight_edge, const float* att,
                             const float* weight_scale, const float* bias, int C, int H, int De, int Cp, int Dp,
                             float* plain, void* stream);
int glam_triplet_layer_fwd(const float* x, const float* edge_attr, const float* staged, const int32_t* rowptr,
                           const int32_t* src, const int32_t* eid, int64_t N, int64_t E, int H, int Cp, int Dp, float slope,
                           float* xw, float* a_ij, float* aggr, float* stats, float* out, void* stream);
size_t glam_triplet_layer_bwd_workspace_bytes(int64_t N, int64_t E, int H, int Cp, int Dp);
int glam_triplet_layer_bwd(const float* x, const float* edge_attr, const float* staged, const float* xw,
                           const float* a_ij, const float* aggr, const float* stats, const float* d_out,
                           const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int32_t* colptr,
                           const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E, int H, int Cp, int Dp,
                           float slope, float* d_x, float* dstaged, float* d_edge_attr, void* ws, size_t ws_bytes,
                           void* stream);

/* glam_triplet_layer_bwd with the parameter chain rule folded in: the gradients of weight_node f32[C,H*C],
 * weight_edge f32[De,H*C], weight_triplet_att f32[H,3C] (as one buffer), weight_scale f32[H*C,C] and bias f32[C]
 * come straight out of the backward pass's partial sums (what autograd derives for src_1gp/layer.py:22-61), one
 * launch instead of glam_triplet_layer_bwd's final reduction + glam_triplet_stage_params_bwd.  7 launches. */
int glam_triplet_layer_bwd_params(const float* x, const float* edge_attr, const float* staged, const float* xw,
                                  const float* a_ij, const float* aggr, const float* stats, const float* d_out,
                                  const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int32_t* colptr,
                                  const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E, int C, int H, int De,
                                  int Cp, int Dp, float slope, const float* weight_node, const float* weight_edge,
                                  const float* att, float* d_x, float* d_weight_node, float* d_weight_edge, float* d_att,
                                  float* d_weight_scale, float* d_bias, float* d_edge_attr, void* ws, size_t ws_bytes,
                                  void* stream);

/* glam_triplet_layer_bwd_params with addends for the five parameter gradients (each laid out like its output, any of them
 * NULL): out = gradient + addend.  The block is applied message_steps times with shared weights (src_1gp/model.py:53-54); the
 * gradient already accumulated by its later applications enters here instead of through a separate add launch.  N > 0.
 * ell_dst / ell_eid_t (may be NULL): ELL records BY SOURCE — glam_ell_build on (colptr, dst, eid_t); every node of a molecular graph
 * has at most 4 out-edges — select, for one-hot edge features of width 4 (edge_onehot = 1, glam_triplet_layer_ws_supported), the
 * warp-specialised B2 + d_x launch (bit-identical); ignored otherwise.  edge_onehot as in glam_triplet_fwd_ell. */
int glam_triplet_layer_bwd_params_acc(const float* x, const float* edge_attr, const float* staged, const float* xw,
                                      const float* a_ij, const float* aggr, const float* stats, const float* d_out,
                                      const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int32_t* colptr,
                                      const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E, int C, int H, int De,
                                      int Cp, int Dp, float slope, const float* weight_node, const float* weight_edge,
                                      const float* att, float* d_x, float* d_weight_node, float* d_weight_edge, float* d_att,
                                      float* d_weight_scale, float* d_bias, const float* add_weight_node,
                                      const float* add_weight_edge, const float* add_att, const float* add_weight_scale,
                                      const float* add_bias, const int32_t* ell_dst, const int32_t* ell_eid_t, int edge_onehot,
                                      float* d_edge_attr, void* ws, size_t ws_bytes, void* stream);
/* glam_triplet_layer_bwd_params_acc with the ELL records of BOTH directions: ell_src / ell_eid BY TARGET (glam_ell_build on
 * (rowptr, src, eid): what the forward used) and ell_dst / ell_eid_t BY SOURCE; either pair may be NULL.  With one-hot edge features of
 * width 4 (edge_onehot = 1, glam_triplet_layer_ws_supported) both aggregate launches of the backward run warp-specialised: B1 with the
 * d_aggr GEMM produced ahead by matrix waves (csrc/triplet_ws_b1.hip), B2 with the d_x GEMM as the consumers' product
 * (csrc/triplet_ws.hip).  d_x, d_weight_node, d_weight_scale, d_bias and every per-node / per-edge intermediate equal the general
 * route bit for bit; d_weight_edge and the edge part of d_att are the same sums in another fixed order (autograd of
 * src_1gp/layer.py:36-61). */
int glam_triplet_layer_bwd_params_ell(const float* x, const float* edge_attr, const float* staged, const float* xw,
                                      const float* a_ij, const float* aggr, const float* stats, const float* d_out,
                                      const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int32_t* colptr,
                                      const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E, int C, int H, int De,
                                      int Cp, int Dp, float slope, const float* weight_node, const float* weight_edge,
                                      const float* att, float* d_x, float* d_weight_node, float* d_weight_edge, float* d_att,
                                      float* d_weight_scale, float* d_bias, const float* add_weight_node,
                                      const float* add_weight_edge, const float* add_att, const float* add_weight_scale,
                                      const float* add_bias, const int32_t* ell_src, const int32_t* ell_eid, const int32_t* ell_dst,
                                      const int32_t* ell_eid_t, int edge_onehot, float* d_edge_attr, void* ws, size_t ws_bytes,
                                      void* stream);
/* The same with a second gradient path into the layer's input: MessageBlock keeps `identity = x` (src_1gp/layer.py:253) and adds it back
 * behind the GRU (:264), so x receives d_identity besides the layer's own input gradient.  d_x = (input gradient) + d_x_addend[N, Cp],
 * summed in the epilogue of the d_x product instead of by an add launch per block application.  Warp-specialised route only (both ELL
 * pairs given, glam_triplet_layer_ws_supported): GLAM_E_UNSUPPORTED otherwise.  d_x_addend == NULL is glam_triplet_layer_bwd_params_ell. */
int glam_triplet_layer_bwd_params_ell_add(const float* x, const float* edge_attr, const float* staged, const float* xw,
                                          const float* a_ij, const float* aggr, const float* stats, const float* d_out,
                                          const int32_t* rowptr, const int32_t* src, const int32_t* eid, const int32_t* colptr,
                                          const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E, int C, int H, int De,
                                          int Cp, int Dp, float slope, const float* weight_node, const float* weight_edge,
                                          const float* att, float* d_x, float* d_weight_node, float* d_weight_edge, float* d_att,
                                          float* d_weight_scale, float* d_bias, const float* add_weight_node,
                                          const float* add_weight_edge, const float* add_att, const float* add_weight_scale,
                                          const float* add_bias, const int32_t* ell_src, const int32_t* ell_eid, const int32_t* ell_dst,
                                          const int32_t* ell_eid_t, int edge_onehot, float* d_edge_attr, void* ws, size_t ws_bytes,
                                          const float* d_x_addend, void* stream);

/* A layer applied message_steps times with shared weights (/root/reference/src_1gp/model.py:53-54), warp-specialised route: every
 * application's backward runs its DATA half — glam_triplet_layer_bwd_data_ell: everything of glam_triplet_layer_bwd_params_ell_add
 * that produces d_x (d_x_addend may be NULL) — and leaves its operands (d_xw, d_a, the block partials of d_W_edge / d_M) in ITS
 * workspace `ws`, whose layout it reports in info (host int64[4]: byte offsets and the partial row count).  The PARAMETER half
 * runs once over the operand sets of nseg <= 3 applications: glam_triplet_layer_param_grads_sets(ws_set[s], info[4 s ..], x[s],
 * aggr[s], d_out[s]) = both weight-gradient products as ONE k_wgrad launch over all sets + ONE k_param_grads (optional addends: the
 * gradient carry).  Its own ws: >= 2 * glam_wgrad_workspace_bytes().  The workspaces of the applications must stay untouched until
 * then.  Same numbers as the per-application form up to the order of the fixed-order sums. */
int glam_triplet_layer_bwd_data_ell(const float* x, const float* edge_attr, const float* staged, const float* xw, const float* a_ij,
                                    const float* aggr, const float* stats, const float* d_out, const int32_t* rowptr, const int32_t* src,
                                    const int32_t* eid, const int32_t* colptr, const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E,
                                    int C, int H, int De, int Cp, int Dp, float slope, float* d_x, const int32_t* ell_src,
                                    const int32_t* ell_eid, const int32_t* ell_dst, const int32_t* ell_eid_t, int edge_onehot,
                                    float* d_edge_attr, void* ws, size_t ws_bytes, const float* d_x_addend, int64_t* info, void* stream);
int glam_triplet_layer_param_grads_sets(int nseg, const void* const* ws_set, const int64_t* info, const float* const* x,
                                        const float* const* aggr, const float* const* d_out, int64_t N, int C, int H, int De, int Cp, int Dp,
                                        const float* weight_node, const float* weight_edge, const float* att, float* d_weight_node,
                                        float* d_weight_edge, float* d_att, float* d_weight_scale, float* d_bias,
                                        const float* add_weight_node, const float* add_weight_edge, const float* add_att,
                                        const float* add_weight_scale, const float* add_bias, void* ws, size_t ws_bytes, void* stream);
/* ---------------------------------------------------------------------------------------------
 * MessageBlock remainder: gate math of one torch.nn.GRU(C, C) step with seq_len 1 (src_1gp/layer.py:247, :262).
 * gi = celu(x) @ W_ih^T + b_ih and gh = h @ W_hh^T + b_hh (f32[N,3C], gate order r|z|n; computed with
 * glam_ts_gemm) -> h_new f32[N,C].  The backward recomputes the gates from gi / gh. */
int glam_gru_gates_fwd(const float* gi, const float* gh, const float* h, int64_t N, int C, float* h_new, void* stream);
/* The same gate math with the rest of MessageBlock.forward folded in (src_1gp/layer.py:263-266): h_new = GRU gates
 * (the state handed to the next step), out = act(h_new + identity) with identity NULL for res=False and act in
 * {0 none, 1 ReLU, 2 LeakyReLU(slope), 3 CELU(alpha=1)}.  Backward: d_out is the gradient of `out`, d_hstate (may be
 * NULL) the gradient reaching h_new through the next step; it returns d_gi, d_gh, d_h and d_identity (if non-NULL). */
int glam_gru_tail_fwd(const float* gi, const float* gh, const float* h, const float* identity, int64_t N, int C, int act,
                      float slope, float* h_new, float* out, void* stream);
int glam_gru_tail_bwd(const float* gi, const float* gh, const float* h, const float* out, const float* d_out,
                      const float* d_hstate, int64_t N, int C, int act, float slope, float* d_gi, float* d_gh, float* d_h,
                      float* d_identity, void* stream);
int glam_gru_gates_bwd(const float* gi, const float* gh, const float* h, const float* d_hnew, int64_t N, int C,
                       float* d_gi, float* d_gh, float* d_h, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-graph normalisation over contiguous node segments ptr int32[B+1] (empty graphs are skipped).
 * Replaces: PyG PairNorm()(x, batch) behind _PairNorm (src_1gp/layer.py:179-185; mode 0, scale 1, eps 1e-5) and the
 * statistics of PyG's graph LayerNorm(x, batch) behind _LayerNorm (src_1gp/layer.py:170-176; mode 1: y = (x - mean) /
 * sqrt(var + eps) over all nodes x channels of a graph; the per-channel affine stays in the host mirror).
 * D <= 256.  The backward pass recomputes the statistics from x.  Any 4-byte-aligned pointers: the float4 kernel forms (D % 4 == 0,
 * D <= 64) are taken when every tensor sits on a 16-byte boundary, the generic kernel otherwise. */
int glam_graph_norm_fwd(const float* x, const int32_t* ptr, int64_t N, int64_t B, int D, int mode, float scale, float eps,
                        float* y, void* stream);
int glam_graph_norm_bwd(const float* x, const float* gy, const int32_t* ptr, int64_t N, int64_t B, int D, int mode,
                        float scale, float eps, float* dx, void* stream);
/* dx = glam_graph_norm_bwd's result + addend f32[N, D]: the residual path of a MessageBlock (src_1gp/layer.py:253-265: x feeds the norm
 * AND the block's skip connection) joins in the store instead of in an add launch.  Every node must belong to a graph (ptr[B] = N). */
int glam_graph_norm_bwd_add(const float* x, const float* gy, const int32_t* ptr, int64_t N, int64_t B, int D, int mode,
                            float scale, float eps, const float* addend, float* dx, void* stream);

/* The norm and the training-mode Dropout(p) a MessageBlock applies right behind it (x = norm(x); x = dropout(x),
 * /root/reference/src_1gp/layer.py:255-256; run.py's default configuration: _PairNorm + Dropout(0.2)) in ONE launch each way, on the
 * device-side Philox stream (rng_state: int64[GLAM_RNG_STATE_WORDS], advanced by the launch; rng_eff: int64[2], the stream position
 * the forward used, handed to the backward, which regenerates the mask).  y_drop = y * mask / (1 - p); y (the plain output) may be
 * NULL when nobody reads it.  Backward: dx = norm'(gy + mask / (1 - p) * gy_drop) (+ addend, may be NULL: see
 * glam_graph_norm_bwd_add); gy may be NULL.  Molecule-sized graphs only (glam_graph_norm_drop_supported: D % 4 == 0, D <= 64, fewer
 * than 64 nodes per graph on average), GLAM_E_UNSUPPORTED otherwise (run the two ops one after the other). */
int glam_graph_norm_drop_supported(int64_t N, int64_t B, int D);
int glam_graph_norm_drop_fwd(const float* x, const int32_t* ptr, int64_t N, int64_t B, int D, int mode, float scale, float eps, float drop_p,
                             int64_t* rng_state, int64_t* rng_eff, float* y, float* y_drop, void* stream);
int glam_graph_norm_drop_bwd(const float* x, const float* gy, const float* gy_drop, const int32_t* ptr, int64_t N, int64_t B, int D, int mode,
                             float scale, float eps, float drop_p, const int64_t* rng_eff, const float* addend, float* dx, void* stream);

/* Edge-weighted neighbour sums over a CSR-by-target: S[n,k,:] = (mean ? 1/deg_n : 1) * sum_{e -> n} w[eid e, k] *
 * x[src e, :]  (x f32[N,D], w f32[E,K], K in {1,4,8}, out f32[N,K,D]; K = 1 with w = the symmetric degree
 * normalisation is GCNConv's propagate, src_2gi_dti_scr/layer.py:143-149).  With one-hot edge features this is the per-relation
 * neighbour sum that evaluates NNConv(aggr='mean') (src_1gp/layer.py:115-122: per-edge [C,C] weights nn(e_ij)) as a
 * K-relation R-GCN without the [E, C*C] tensor.  The backward (w.r.t. x) walks the CSR transpose. */
int glam_edge_wsum_fwd(const float* x, const float* w, const int32_t* rowptr, const int32_t* src, const int32_t* eid,
                       int64_t N, int64_t E, int D, int K, int mean, int self_slot, float* out, void* stream);
int glam_edge_wsum_bwd(const float* d_out, const float* w, const int32_t* colptr, const int32_t* dst,
                       const int32_t* eid_t, const int32_t* rowptr, int64_t N, int64_t E, int D, int K, int mean,
                       int self_slot, float* dx, void* stream);
/* ... dx = (the same sums) + addend[N, D] (NULL: none): the gradient of a skip connection around the layer (MessageBlock,
 * src_1gp/layer.py:253-265) joins here instead of in an add launch of its own.  16-byte form only (K in {4, 8}, D % 4 == 0, aligned). */
int glam_edge_wsum_bwd_add(const float* d_out, const float* w, const int32_t* colptr, const int32_t* dst, const int32_t* eid_t,
                           const int32_t* rowptr, int64_t N, int64_t E, int D, int K, int mean, int self_slot, const float* addend,
                           float* dx, void* stream);
/* self_slot = 1 (K in {4, 8}, D % 4 == 0): out is f32[N, K+1, D] and slot K of node n is x[n] itself — NNConv's root term
 * x_i @ root (src_1gp/layer.py:119) as one more relation, so that the layer is ONE GEMM [N, (K+1) D] x [(K+1) D, out]. */

/* NNConv over continuous edge features (the protein tower of src_2gi_dti_scr/glam.py: NNConv(Cin, Cout, Linear(De, 32) -> ReLU ->
 * Linear(32, Cin*Cout), aggr in {mean, add}) with 8 contact features per residue edge) without the per-edge weight tensor [E, Cin*Cout].
 * With h_e = relu(W0 e_e + b0) (f32[E, 32]) the layer is out = [S | x] @ Wstack + bias, where [S | x] = f32[N, 34, Cin] holds
 * S[n, k, :] = (mean ? 1/deg_n : 1) * sum_{e -> n} h_e[k] x[src e] for k < 32, the same with h = 1 for k = 32, and x[n] for k = 33;
 * Wstack = f32[34*Cin, Cout] with rows k*Cin + ci = W1[ci*Cout + co, k] (k < 32), b1[ci*Cout + co] (k = 32), root[ci, co] (k = 33).
 * W0 f32[32, De], b0 f32[32], W1 f32[Cin*Cout, 32], b1 f32[Cin*Cout], root f32[Cin, Cout] are the torch layouts of nn.0 / nn.2 / root.
 * glam_nnconv_ec_supported: 1 for hidden = 32, 1 <= De <= 16, 1 <= Cin, Cout <= 96, else 0 (the entry points return
 * GLAM_E_UNSUPPORTED).  glam_nnconv_ec_stack builds Wstack (one launch); glam_nnconv_ec_unstack scatters d_Wstack back into
 * d_W1, d_b1, d_root (one launch).
 * glam_nnconv_ec_fwd: h f32[E, 32] (16-byte aligned) is written for the backward; bias may be NULL; workspace >=
 * glam_nnconv_ec_workspace_bytes(..., backward = 0) holds [S | x].
 * glam_nnconv_ec_bwd (d_out f32[N, Cout]; CSR by target and its transpose, as glam_edge_wsum_bwd): recomputes [S | x] from h,
 * writes dx f32[N, Cin] (+ addend f32[N, Cin], may be NULL: the skip connection's gradient, as glam_edge_wsum_bwd_add), d_w0, d_b0,
 * d_wstack f32[34*Cin, Cout], d_bias f32[Cout]; workspace >= glam_nnconv_ec_workspace_bytes(..., backward = 1).  No gradient
 * reaches edge_attr (edge data).  Exact fp32 MFMA products; the weight gradients are two-stage fixed-order sums (no atomics:
 * bit-identical from run to run).  No host synchronisation: hipGraph-capturable. */
int glam_nnconv_ec_supported(int De, int hidden, int Cin, int Cout);
size_t glam_nnconv_ec_workspace_bytes(int64_t N, int64_t E, int De, int Cin, int Cout, int backward);
int glam_nnconv_ec_stack(const float* w1, const float* b1, const float* root, int Cin, int Cout, float* wstack, void* stream);
int glam_nnconv_ec_unstack(const float* d_wstack, int Cin, int Cout, float* d_w1, float* d_b1, float* d_root, void* stream);
int glam_nnconv_ec_fwd(const float* x, const float* edge_attr, const int32_t* rowptr, const int32_t* src, const int32_t* eid,
                       int64_t N, int64_t E, int De, int Cin, int Cout, const float* w0, const float* b0, const float* wstack,
                       const float* bias, int mean, float* h, void* workspace, size_t workspace_bytes, float* out, void* stream);
int glam_nnconv_ec_bwd(const float* d_out, const float* x, const float* edge_attr, const int32_t* rowptr, const int32_t* src,
                       const int32_t* eid, const int32_t* colptr, const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E,
                       int De, int Cin, int Cout, const float* wstack, const float* h, int mean, const float* addend, float* dx,
                       float* d_w0, float* d_b0, float* d_wstack, float* d_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-pair fusion of the two-tower models: out f32[P,2] = [max, mean] of mol[seg_i] @ pro[seg_i]^T for every pair i
 * (segments mol_ptr / pro_ptr int32[P+1]; empty segment -> 0); argmax int32[P,2] = (ligand row, residue row) of the max;
 * sums f32[P,2,D] = the column sums of both segments, kept by the caller from the forward to the backward call.
 * Replaces: dot_and_global_pool2 (src_2gi_dti_scr/layer.py:270-283: Python loop, .item() syncs, one matmul per pair). */
size_t glam_pair_pool_workspace_bytes(int64_t P, int D);
int glam_pair_pool_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr, int64_t P,
                       int D, float* out, int32_t* argmax, float* sums, void* workspace, size_t workspace_bytes,
                       void* stream);
int glam_pair_pool_bwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                       const int32_t* argmax, const float* sums, const float* d_out, int64_t P, int D, float* d_mol,
                       float* d_pro, void* stream);
/* ... d_mol += add_mol, d_pro += add_pro (either may be NULL): the gradient of the next message step's use of the two feature
 * matrices (src_2gi_dti_scr/model.py:66-70: every step's outputs feed this fusion AND the next step), when the caller took them
 * back from this node — one add launch per tower and step less.  glam_pair_pool_add_supported(D): the widths that have it. */
int glam_pair_pool_add_supported(int D);
int glam_pair_pool_bwd_add(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr, const int32_t* argmax,
                           const float* sums, const float* d_out, int64_t P, int D, const float* add_mol, const float* add_pro,
                           float* d_mol, float* d_pro, void* stream);

/* Screening (inference): the same fusion with every protein held ONCE — pair i takes ligand rows mol_ptr[i]..mol_ptr[i+1] and the
 * residue rows of segment q = pro_of_pair[i] (int32[P], every entry in [0, Q): checked by the caller, trusted here; pro_ptr int32[Q+1]).
 * out f32[P,2] as above; the max (and argmax: row of mol, row of pro; may be NULL) is bit for bit that of glam_pair_pool_fwd on
 * physically replicated residue rows.  Forward only.  Workspace: glam_pair_pool_workspace_bytes(P, D). */
int glam_pair_pool_indexed_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                               const int32_t* pro_of_pair, int64_t P, int64_t Q, int D, float* out, int32_t* argmax,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Training against proteins held once (csrc/pairshared.hip): glam_pair_pool_indexed_fwd that ALWAYS writes argmax int32[P,2] (row of mol,
 * row of pro; -1, -1 for an empty pair) and sums f32[P,2,D] (column sum of the pair's ligand rows, column sum of its protein's residue
 * rows).  out and argmax are bit for bit those of glam_pair_pool_indexed_fwd on the same inputs. */
int glam_pair_pool_shared_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                              const int32_t* pro_of_pair, int64_t P, int64_t Q, int D, float* out, int32_t* argmax, float* sums,
                              void* workspace, size_t workspace_bytes, void* stream);
/* ... and its backward, one launch.  pair_order int32[P]: the pairs stably sorted by protein; pair_ptr int32[Q+1]: the offsets of the
 * proteins' runs in it (both built and checked by the caller, trusted here).  With gmean_i = d_out[i,1] / (n_mol n_res):
 *   d_mol, rows of pair i:  gmean_i * psum_i, + gmax_i * pro[ap_i] on row am_i (the expression of glam_pair_pool_bwd), + add_mol last.
 *   d_pro, every row b of every protein q (referenced or not):  0, + gmean_i * msum_i for the pairs i of q in pair_order order, then
 *          fmaf(gmax_i, mol[am_i], .) for the pairs of q with ap_i == b in the same order, + add_pro last.
 * Empty pairs contribute nothing.  No atomics: the order of every sum depends on pair_order alone, two runs are bit-equal.
 * add_mol / add_pro may be NULL.  D in 1..256. */
int glam_pair_pool_shared_bwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                              const int32_t* pro_of_pair, const int32_t* pair_order, const int32_t* pair_ptr, const int32_t* argmax,
                              const float* sums, const float* d_out, int64_t P, int64_t Q, int D, const float* add_mol,
                              const float* add_pro, float* d_mol, float* d_pro, void* stream);
/* d_flat f32[Q,W]: row q = the sum of the rows d_rows[i] (f32[P,W]) of q's pairs in pair_order order — the backward of gathering a
 * [Q, W] matrix by pair, without the atomics of an index_add (same bits on every run).  P == 0: nothing is written. */
int glam_pair_rows_bwd(const float* d_rows, const int32_t* pair_order, const int32_t* pair_ptr, int64_t P, int64_t Q, int W,
                       float* d_flat, void* stream);

/* Drug x drug (inference): the fusion with BOTH sides held once and both indexed — pair i takes the rows of segment a = idx1[i] of x1
 * (ptr1 int32[Q1+1]) and of segment b = idx2[i] of x2 (ptr2 int32[Q2+1]); idx1 / idx2 int32[P], every entry in [0, Q1) / [0, Q2): checked
 * by the caller, trusted here; either may be NULL = identity (needs Q1 == P / Q2 == P).  out f32[P,2] = [max, mean]; argmax int32[P,2]
 * (row of x1, row of x2; may be NULL); an empty segment on either side gives 0, 0 and -1, -1.  The max and argmax are bit for bit those of
 * glam_pair_pool_fwd on physically gathered rows; the mean is the same bits on every run.  One wave per pair, one launch, no workspace
 * (csrc/pairgather.hip): cut for segments of tens of rows.  D in 1..128, else GLAM_E_UNSUPPORTED.  Forward only.
 * glam_pair_pool_gather_load_bytes: the width of the loads a call with these matrices uses — 16 (D % 4 == 0 and both matrices 16-byte
 * aligned), 4 otherwise, 0 for a D outside the table. */
size_t glam_pair_pool_gather_load_bytes(const float* x1, const float* x2, int D);
int glam_pair_pool_gather_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* idx1,
                              const int32_t* idx2, int64_t P, int64_t Q1, int64_t Q2, int D, float* out, int32_t* argmax, void* stream);

/* Drug x drug, training on drugs held once (csrc/pairgather.hip, csrc/pairgather_bwd.hip).  glam_pair_pool_gather_train_fwd: the launch of
 * glam_pair_pool_gather_fwd that ALWAYS writes argmax int32[P,2] (-1, -1 for an empty pair) and also sums f32[P,2,D] — the column sums of
 * segment idx1[i] of x1 and of segment idx2[i] of x2, from the registers that form the mean (not written for an empty pair: nothing reads
 * them).  out and argmax are bit for bit those of glam_pair_pool_gather_fwd on the same inputs.
 * glam_pair_pool_gather_bwd: its backward, ONE launch, one wave per (side, drug), ceil((Q1 + Q2) / 4) blocks.  order1 int32[P]: the pairs
 * stably sorted by idx1; list_ptr1 int32[Q1+1]: the offsets of the drugs' runs in it; order2 / list_ptr2 the same for idx2 (with a NULL
 * index: the identity lists).  Built and checked by the caller, trusted here.  With n1, n2 the sizes of pair i's segments,
 * gmax_i = d_out[i,0], gmean_i = d_out[i,1] / (n1 n2) and (am_i, ap_i) = argmax[i]:
 *   d_x1, every row r of every segment a (referenced or not):  0, + gmean_i * sums[i,1] for the pairs i with idx1[i] == a in order1 order,
 *         then fmaf(gmax_i, x2[ap_i], .) for those of them with am_i == r in the same order, + add1[r] last;
 *   d_x2: the same with the sides exchanged (sums[i,0], x1[am_i] on row ap_i, order2, add2).
 * A pair with an empty segment on either side contributes nothing.  No atomics: the order of every sum depends on the lists alone, two
 * runs are bit-equal.  add1 / add2 (the gradients of a later use of x1 / x2) may be NULL.  16-byte loads and stores when D % 4 == 0 and
 * x1, x2, sums, add1, add2, d_x1, d_x2 are 16-byte aligned, dwords otherwise.  Both: D in 1..128, else GLAM_E_UNSUPPORTED; P == 0:
 * GLAM_OK, nothing launched or written. */
int glam_pair_pool_gather_train_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* idx1,
                                    const int32_t* idx2, int64_t P, int64_t Q1, int64_t Q2, int D, float* out, int32_t* argmax,
                                    float* sums, void* stream);
int glam_pair_pool_gather_bwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* idx1,
                              const int32_t* idx2, const int32_t* order1, const int32_t* list_ptr1, const int32_t* order2,
                              const int32_t* list_ptr2, const int32_t* argmax, const float* sums, const float* d_out, int64_t P,
                              int64_t Q1, int64_t Q2, int D, const float* add1, const float* add2, float* d_x1, float* d_x2,
                              void* stream);

/* Panel screening (inference): EVERY ligand segment l = 0..L-1 of mol (mol_ptr int32[L+1]) against every selected protein segment
 * sel[j], j = 0..Qs-1 (int32[Qs], entries in [0, Q), any order, duplicates allowed), of pro (pro_ptr int32[Q+1], each protein held once):
 * out f32[L,Qs,2] = [max, mean]; argmax int32[L,Qs,2] (row of mol, row of pro; may be NULL); an empty ligand or protein gives 0, 0 and
 * -1, -1.  The max and argmax are bit for bit those of glam_pair_pool_indexed_fwd with pro_of_pair = [sel[j]] * L; the mean is
 * <molsum[l], prosum[sel[j]]> / (n_l * n_res), one ascending fmaf chain over the D columns (molsum f32[L,D], prosum f32[Q,D]: the column
 * sums of the segments, computed by the caller).  Protein-stationary grid (csrc/pairpanel.hip): one wave per (chunk of 64 residue rows of
 * a selected protein, slab of ligands) + a finish launch.  work int32[4 * total_chunks + Qs + 1], built and checked by the caller and
 * trusted here: per chunk, in selection order, (j, first row of the chunk in pro, rows in the chunk (1..64), index of its partials in
 * the workspace), then chunk_ptr[Qs+1], the offsets of the selections' chunk runs.  slab: ligands per wave, 0 = choose (about 4 096 waves
 * where the problem has them, never fewer than 4 ligands per wave).  Workspace: glam_pair_pool_panel_workspace_bytes(total_chunks, L).
 * D in 1..128, else GLAM_E_UNSUPPORTED; glam_pair_pool_panel_supported(D) is that check alone and returns a STATUS: GLAM_OK when the
 * width has a kernel, GLAM_E_UNSUPPORTED otherwise.  L == 0 or Qs == 0: GLAM_OK, nothing launched.  Forward only. */
size_t glam_pair_pool_panel_workspace_bytes(int64_t total_chunks, int64_t L);
int glam_pair_pool_panel_supported(int D);
int glam_pair_pool_panel_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr, const int32_t* work,
                             int64_t total_chunks, const int32_t* sel, int64_t Qs, int64_t L, int64_t Q, int D, const float* molsum,
                             const float* prosum, int slab, float* out, int32_t* argmax, void* workspace, size_t workspace_bytes,
                             void* stream);
/* ... and its backward (csrc/pairpanel_bwd.hip), ONE launch: training on a ligand x protein label table.  argmax int32[L,Qs,2] and d_out
 * f32[L,Qs,2] are those of glam_pair_pool_panel_fwd (the argmax kept: not NULL here); molsum / prosum as there.  sel_order int32[Qs]: the
 * selection stably sorted by protein (a stable argsort of sel); sel_ptr int32[Q+1]: the offsets of the proteins' runs in it (both built
 * and checked by the caller, trusted here, like sel).  With g = d_out, q_j = sel[j] and w[l,j] = g[l,j,1] / ((float)n_l * (float)n_{q_j}):
 *   d_mol, every row a of every ligand l:  0, + w[l,j] * prosum[q_j] for j = 0..Qs-1 ascending, then fmaf(g[l,j,0], pro[argmax[l,j,1]], .)
 *          for the j with argmax[l,j,0] == a in the same order, + add_mol[a] last;
 *   d_pro, every row b of every protein q (selected or not):  0, + w[l,j] * molsum[l] for the pairs (l, j) with sel[j] == q in ascending
 *          l * Qs + j (the batch order of the expanded pair list), then fmaf(g[l,j,0], mol[argmax[l,j,0]], .) for those of them with
 *          argmax[l,j,1] == b in the same order, + add_pro[b] last.
 * An empty ligand or protein (argmax -1) contributes nothing; the rows of a protein no entry of sel names get exact zeros (+ add_pro);
 * duplicates in sel add up.  No atomics: the order of every sum depends on the table alone, two runs are bit-equal.  One block per
 * (segment, 16 of its rows): 32 blocks a protein, 2 a ligand, each walking its segment's list (Qs pairs for a ligand, L * (entries of
 * sel that name it) for a protein).  add_mol / add_pro (the gradients of a later use of mol / pro) may be NULL.  16-byte loads and stores
 * when D % 4 == 0 and mol, pro, molsum, prosum, add_mol, add_pro, d_mol, d_pro are 16-byte aligned, dwords otherwise.  D in 1..128, else
 * GLAM_E_UNSUPPORTED; L == 0 or Qs == 0: GLAM_OK, nothing launched or written. */
int glam_pair_pool_panel_bwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr, const int32_t* sel,
                             const int32_t* sel_order, const int32_t* sel_ptr, const int32_t* argmax, const float* d_out,
                             const float* molsum, const float* prosum, int64_t Qs, int64_t L, int64_t Q, int D, const float* add_mol,
                             const float* add_pro, float* d_mol, float* d_pro, void* stream);

/* Grid fusion (inference): EVERY selected first-side segment rows[i], i = 0..R-1 (int32[R], entries in [0, Q1), any order, duplicates
 * allowed; NULL = the identity over Q1, needs R == Q1), of x1 (ptr1 int32[Q1+1]) against every selected second-side segment cols[j],
 * j = 0..Cs-1 (int32[Cs], entries in [0, Q2), any order, duplicates allowed), of x2 (ptr2 int32[Q2+1]); each segment held once on its side:
 * out f32[R,Cs,2] = [max, mean]; argmax int32[R,Cs,2] (row of x1, row of x2; may be NULL); an empty segment on either side gives 0, 0 and
 * -1, -1.  The max and argmax are bit for bit those of glam_pair_pool_gather_fwd on the pairs (rows[i], cols[j]); the mean is
 * <sum1[rows[i]], sum2[cols[j]]> / (n1 * n2), one ascending fmaf chain over the D columns (sum1 f32[Q1,D], sum2 f32[Q2,D]: the column sums
 * of the segments, computed by the caller) — the chain of glam_pair_pool_panel_fwd.  Second-side-stationary grid with PACKED chunks
 * (csrc/pairgrid.hip): one wave per (chunk of up to 64 second-side rows — the rows of several small segments side by side —, slab of
 * first-side segments) + a finish launch.  work int32[256 * total_chunks + Cs + 1], built and checked by the caller and trusted here: per
 * chunk and lane (row of x2 the lane holds, that row inside its segment, rows of that segment, index of the partial the lane's best goes
 * to; -1 = an idle lane, which holds the row of lane 0), lanes of one partial contiguous; then part_ptr[Cs+1], the offsets of the
 * selections' partials, n_partials in all.  slab: first-side segments per wave, 0 = choose (the panel's rule, untuned: about 4 096 waves
 * where the problem has them, never fewer than 4 segments per wave).  Workspace: glam_pair_pool_grid_workspace_bytes(n_partials, R).
 * D in 1..128, else GLAM_E_UNSUPPORTED; glam_pair_pool_grid_supported(D) is that check alone and returns a STATUS: GLAM_OK when the width
 * has a kernel, GLAM_E_UNSUPPORTED otherwise.  R == 0 or Cs == 0: GLAM_OK, nothing launched, no pointer looked at.  Forward only. */
size_t glam_pair_pool_grid_workspace_bytes(int64_t n_partials, int64_t R);
int glam_pair_pool_grid_supported(int D);
int glam_pair_pool_grid_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* rows, int64_t R,
                            const int32_t* cols, int64_t Cs, const int32_t* work, int64_t total_chunks, int64_t n_partials, int64_t Q1,
                            int64_t Q2, int D, const float* sum1, const float* sum2, int slab, float* out, int32_t* argmax,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Interaction maps (inference): both marginals of the score matrix S = x1[seg a] @ x2[seg b]^T of every listed pair, S never stored
 * (csrc/pairmap.hip).  work int32[n_items,4]: per item (a, b, 2 * chunk + side, first output row of the chunk) — a wave takes the owner
 * rows 64 * chunk .. 64 * chunk + 63 of segment a of x1 (side 0; ptr1 int32[Q1+1]) or of segment b of x2 (side 1; ptr2 int32[Q2+1]) and
 * streams the whole other segment past them; built and checked by the caller (every owner row of every pair in exactly one item, output
 * rows pair-major per side), trusted here.  Per owner row, at its output row of its side's arrays: max f32 = the largest score of the
 * row, arg int32 = the row (of the OTHER matrix) of the first partner row that attains it, mean f32 = the sum of the row's scores in
 * ascending partner order over the partner's row count; an empty partner segment gives 0, -1, 0.  A score is the one ascending fmaf chain
 * of glam_pair_pool_gather_fwd: the largest max of a pair's rows, on either side, is bit for bit that call's max column and the first
 * row that holds it with its arg is that call's argmax.  ONE launch for both sides, no workspace; 16-byte loads when D % 4 == 0 and x1,
 * x2 are 16-byte aligned, dwords otherwise.  D in 1..128, else GLAM_E_UNSUPPORTED; a null pointer with n_items > 0: GLAM_E_INVALID;
 * n_items == 0: GLAM_OK, nothing launched, no pointer looked at.  Forward only. */
int glam_pair_map_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* work, int64_t n_items,
                      int D, float* max1, int32_t* arg1, float* mean1, float* max2, int32_t* arg2, float* mean2, void* stream);

/* Factored pair head (inference): the two linear layers of the pair models' head over a TABLE of R x Cs pairs, for a head without norms
 * and with an elementwise activation (csrc/pairhead.hip):
 *   out[i,j,o] = b1[o] + sum_e w1[o,e] * act(A[i,e] + B[j,e] + sum_k W0[e, 2 hid + k] * f[i,j,k])
 *   A[i,e] = b0[e] + sum_c W0[e,c] * flat_a[i,c],   B[j,e] = sum_c W0[e, hid + c] * flat_b[j,c]
 * which is lin1(act(lin0(cat[flat_a[i], flat_b[j], f[i,j]]))) without the [R*Cs, 2 hid + F] input rows and the [R*Cs, e_dim] hidden matrix.
 * flat_a f32[R,hid] (leading dimension lda >= hid), flat_b f32[Cs,hid] (ldb); f f32[R,Cs,F] contiguous (NULL with F == 0); W0
 * f32[e_dim, 2 hid + F] (leading dimension ldw), read in place; b0 f32[e_dim]; w1 f32[out_dim,e_dim] contiguous; b1 f32[out_dim]; out
 * f32[R,Cs,out_dim].  act: 0 none, 1 relu, 2 leaky (h > 0 ? h : slope * h).  Two launches on `stream`: k_pair_head_side (A and B, both from
 * the one launch, into the workspace) and k_pair_head.  Every A / B element is one ascending fmaf chain from its bias, every out element
 * one ascending chain over e from b1[o]: an entry depends on its own (flat_a[i], flat_b[j], f[i,j]) alone — the same bits whatever R, Cs
 * and the rest of the table are.  Workspace: glam_pair_head_workspace_bytes(R, Cs, e_dim) = (R + Cs) * e_dim floats, 4-byte aligned.
 * 1 <= out_dim <= 8, 0 <= F <= 16, e_dim >= 1, hid >= 1, R * Cs < 2^31 - 1, else GLAM_E_INVALID — as a null or misaligned pointer or a short
 * workspace; every check comes before any device work.  R == 0 or Cs == 0: GLAM_OK, nothing launched, no pointer looked at.  Forward only. */
size_t glam_pair_head_workspace_bytes(int64_t R, int64_t Cs, int e_dim);
int glam_pair_head_fwd(const float* flat_a, int64_t lda, const float* flat_b, int64_t ldb, const float* f, int64_t R, int64_t Cs, int hid,
                       int F, const float* W0, int64_t ldw, const float* b0, int e_dim, const float* w1, const float* b1, int out_dim,
                       int act, float slope, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* Class table (inference): the head above for ANY out_dim in 2..1024, ending in the called class and its log-softmax:
 *   x[o]  = the logit of glam_pair_head_fwd, the same chain bit for bit (acc = b1[o]; acc = fmaf(w1[o,e], h_e, acc), e ascending)
 *   cls   = argmax_o x[o]            int32[R,Cs]    (torch.argmax: a NaN is the largest, of equal values the smallest index)
 *   logp  = x[cls] - lse             f32[R,Cs]      lse = m + log(sum_o exp(x[o] - m)), kept as a running (m, sum) over o ascending
 *   sel   = x[classes[k]] - lse      f32[R,Cs,n_sel] (NULL with n_sel == 0);  classes: a HOST array of n_sel ints in [0, out_dim), n_sel <= 8,
 *                                                    duplicates allowed, order kept (read by this call and passed to the kernel by value)
 *   logits = x                       f32[R,Cs,out_dim], or NULL: not written
 * logp / sel are NaN where a logit of the pair is NaN (torch.log_softmax).  The classes are walked in tiles of 16, each with its own pass
 * over e: the registers do not depend on out_dim, and neither the hidden matrix nor (without logits) the [R,Cs,out_dim] table exists.
 * Two launches on `stream`: k_pair_head_classes_side (A, B and the transposed, tile-padded lin1 weight with its bias, into the workspace)
 * and k_pair_head_classes.  An entry depends on its own (flat_a[i], flat_b[j], f[i,j]) alone.  Workspace:
 * glam_pair_head_classes_workspace_bytes(R, Cs, e_dim, out_dim) = ((R + Cs) * e_dim + (e_dim + 1) * ceil(out_dim / 16) * 16) floats.
 * Other operands, limits and statuses as glam_pair_head_fwd; R * Cs * out_dim < 2^63.  Every check comes before any device work and before
 * any device pointer is looked at.  R == 0 or Cs == 0: GLAM_OK after the limit checks, nothing launched.  Forward only. */
size_t glam_pair_head_classes_workspace_bytes(int64_t R, int64_t Cs, int e_dim, int out_dim);
int glam_pair_head_classes_fwd(const float* flat_a, int64_t lda, const float* flat_b, int64_t ldb, const float* f, int64_t R, int64_t Cs,
                               int hid, int F, const float* W0, int64_t ldw, const float* b0, int e_dim, const float* w1, const float* b1,
                               int out_dim, int act, float slope, const int* classes, int n_sel, void* workspace, size_t workspace_bytes,
                               int* cls, float* logp, float* sel, float* logits, void* stream);

/* Screening hit lists: the best K candidates per query column, kept on the device while batches of scores stream past
 * (csrc/hits.hip).  State, owned by the caller: top_score f32[Qs,K] and top_id int32[Qs,K] — every list sorted best first, empty
 * slots (id -1, score NaN) at its end — and seen int64[1] in device memory, the number of candidates offered so far.
 * glam_hits_reset empties the lists and zeroes *seen.  glam_hits_merge offers candidate l = 0..L-1 with the score
 * score[l * ld_row + j * ld_col] (strides in elements, >= 0: one task column of an [L,Qs,out_dim] tensor is read in place) to list j,
 * j = 0..Qs-1, under the id ids[l] (int32[L], every id in [0, 2^31 - 1]; not deduplicated), or *seen + l when ids is NULL (the caller
 * keeps that below 2^31), and then adds L to *seen.  The lists are EXACT under one total order: better score first (larger if largest
 * != 0, smaller if not; -0.0 and +0.0 are equal), equal scores by ascending id, NaN scores after every number (among themselves by
 * ascending id), empty slots last; the stored scores are the candidates' original bits.  The same `largest` on every call of a list.
 * Two launches on `stream`, one after the other (grid Qs x slabs: a block filters its slab of one column against the list's K-th
 * entry and sorts the survivors in LDS; then one block per column merges the partial lists into the list), no atomics, no read-back,
 * capturable; the result does not depend on `slabs` (0 = choose; clamped to what the workspace holds) or on the order blocks run in.
 * Workspace: glam_hits_workspace_bytes(L, Qs, K), 8-byte aligned (0 for a non-positive argument).  K in 1..1024, else
 * GLAM_E_UNSUPPORTED — checked before the pointers are looked at; glam_hits_supported(K) is that check alone and returns a STATUS.
 * L == 0 or Qs == 0: GLAM_OK, nothing launched, nothing dereferenced.  L >= 2^31, a negative size or stride, a null or misaligned
 * pointer (4 bytes; seen and the workspace 8), a short workspace: GLAM_E_INVALID. */
int glam_hits_supported(int K);
size_t glam_hits_workspace_bytes(int64_t L, int64_t Qs, int K);
int glam_hits_reset(float* top_score, int32_t* top_id, int64_t* seen, int64_t Qs, int K, void* stream);
int glam_hits_merge(const float* score, int64_t ld_row, int64_t ld_col, const int32_t* ids, int64_t L, int64_t Qs, int K, int largest,
                    int slabs, float* top_score, int32_t* top_id, int64_t* seen, void* workspace, size_t workspace_bytes, void* stream);

/* Training-mode block tails of the reference's DEFAULT configuration (src_1gp/model.py:30-31, run.py:35-37: RReLU activations,
 * Dropout(0.2) in front of every conv) — the same launches as glam_gru_tail_* / glam_bias_res_act_* with two additions:
 *   act = 4: torch.nn.RReLU in training mode, out = y > 0 ? y : a * y with a ~ U(rr_lower, rr_upper) per element;
 *   out_drop (may be NULL): a second output Dropout(drop_p)(out) = out * mask / (1 - p), the next conv's input (layer.py:256).
 * Random numbers: Philox4x32-10 keyed by rng_state[0] (seed), stream position rng_state[1] (offset), both int64 in DEVICE memory
 * and ticket words at index 16 and 32 + 16 s, s < 16 (each on its own cache line): rng_state int64[GLAM_RNG_STATE_WORDS = 288], zero
 * everything but the seed once.  Every launch uses the offset it finds
 * and the last block to finish stores offset + 1 — hipGraph replays continue the sequence with no host involvement.  rng_eff
 * int64[2] receives the (seed, offset) pair the launch used; the backward entry points regenerate slopes and masks from it (no
 * mask tensors).  d_out / d_out_drop: gradients of the two outputs (either may be NULL). glam_bias_res_act_rng_fwd accepts
 * out = NULL for act = 0 (a plain Dropout). */
#define GLAM_RNG_STATE_WORDS 288
int glam_gru_tail_rng_fwd(const float* gi, const float* gh, const float* h, const float* identity, int64_t N, int C, int act,
                          float slope, float rr_lower, float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff,
                          float* h_new, float* out, float* out_drop, void* stream);
int glam_gru_tail_rng_bwd(const float* gi, const float* gh, const float* h, const float* out, const float* d_out,
                          const float* d_out_drop, const float* d_hstate, int64_t N, int C, int act, float slope, float rr_lower,
                          float rr_upper, float drop_p, const int64_t* rng_eff, float* d_gi, float* d_gh, float* d_h,
                          float* d_identity, void* stream);
int glam_bias_res_act_rng_fwd(const float* y, const float* bias, const float* identity, int64_t N, int C, int act, float slope,
                              float rr_lower, float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff, float* out,
                              float* out_drop, void* stream);
int glam_bias_res_act_rng_bwd(const float* out, const float* d_out, const float* d_out_drop, int64_t N, int C, int act,
                              float slope, float rr_lower, float rr_upper, float drop_p, const int64_t* rng_eff, float* d_y,
                              void* stream);

/* Software-pipelined forward aggregate for graphs whose in-degree never exceeds 4 (molecules): the arithmetic of
 * glam_triplet_fwd (multi-head form, emul = 1; src_1gp/layer.py:42-55 through PyG propagate / softmax / scatter-add), bit for
 * bit, with the neighbour rows staged global -> LDS by LDS-DMA and every wave prefetching the rows of its next pass and the
 * index record of the one after while it computes the current one (csrc/triplet_dma.hip).
 * glam_ell_build: index records from the by-target CSR — ell_src / ell_eid int32[N, 4] (source node and original edge id of
 * the node's incoming edges in CSR order, -1 = empty slot); *overflow_flag (int32, zero it first) is set when some node has
 * more than 4 incoming edges: such an edge list must use glam_triplet_fwd.  Built once per edge list, like the CSR.
 * glam_triplet_fwd_ell: same tensors as glam_triplet_fwd; Cp <= 64, H <= 4, De in {4, 8}; edge_onehot = 1 asserts that every
 * edge_attr row is one-hot (e_ij is then read as one W_edge row, bit-identical); grid_blocks <= 0 picks the default persistent
 * grid (two 4-wave blocks per CU). */
int glam_ell_build(const int32_t* rowptr, const int32_t* nbr, const int32_t* eid, int64_t N, int32_t* ell_src,
                   int32_t* ell_eid, int32_t* overflow_flag, void* stream);
int glam_triplet_fwd_ell_supported(int H, int Cp, int De);
int glam_triplet_fwd_ell(const float* xw, const float* a_ij, const float* edge_attr, const float* w_edge, const float* M,
                         const int32_t* ell_src, const int32_t* ell_eid, int64_t N, int64_t E, int H, int Cp, int De,
                         float slope, int edge_onehot, float* aggr, float* stats, int grid_blocks, void* stream);

/* glam_triplet_layer_fwd for molecular graphs — edge lists with an ELL form (glam_ell_build, in-degree <= 4) and one-hot edge features
 * of width 4 (src_1gp/dataset.py:82): node GEMM + the warp-specialised aggregate / update launch (csrc/triplet_ws.hip: producer waves
 * gather, consumer waves run the update GEMM out of an LDS tile ring).  Same tensors and results (bit for bit) as
 * glam_triplet_layer_fwd; the faster route at EVERY batch size.  glam_triplet_layer_ws_supported says whether a shape is inside
 * (36 <= Cp <= 64, H * Cp <= 192, Dp = 4, edge_onehot = 1); other shapes are GLAM_E_UNSUPPORTED here and belong to
 * glam_triplet_layer_fwd.
 * The INFERENCE forward (src_1gp/trainer.py:306-327: @torch.no_grad() evaluation of every split after every epoch): aggr = stats = NULL —
 * both exist only for a backward pass, and the launch then stores neither (15.3 of the 22.5 MB it writes at 1 024 molecules).  Always
 * available here; glam_triplet_layer_fwd takes NULL where glam_triplet_layer_infer_supported says so (the shapes whose update GEMM runs
 * inside the aggregate launch).  xw and a_ij are still written: the aggregate reads them.
 * x = NULL: xw and a_ij HOLD the node product already — the previous application's GRU step wrote them with the rows themselves
 * (glam_gru_ws_fwd_pre_node; /root/reference/src_1gp/model.py:53-54 applies one block message_steps times) — and the call is the
 * aggregate / update launch alone. */
int glam_triplet_layer_ws_supported(int H, int Cp, int Dp, int edge_onehot);
int glam_triplet_layer_infer_supported(int H, int Cp, int Dp);
int glam_triplet_layer_fwd_ell(const float* x, const float* edge_attr, const float* staged, const int32_t* ell_src,
                               const int32_t* ell_eid, int edge_onehot, int64_t N, int64_t E, int H, int Cp, int Dp, float slope,
                               float* xw, float* a_ij, float* aggr, float* stats, float* out, void* stream);

/* The relation-weight table of NNConv with one-hot bond features (src_1gp/layer.py:115-122: nn = Linear(De, hidden) -> ReLU ->
 * Linear(hidden, M), M = in * out): out f32[De, M] = nn(eye(De)), h f32[De, hidden] = the hidden activations (saved for the backward).
 * w1 f32[hidden, De], b1 f32[hidden], w2 f32[M, hidden], b2 f32[M] (torch.nn.Linear layouts).  De <= 8, hidden a power of two in
 * 4..64 (the reference's is 32), M <= 2^22: glam_relation_mlp_supported says whether a shape is inside.  One launch forward, two
 * backward (block partials of d_h summed in block order: bit-reproducible). */
int glam_relation_mlp_supported(int De, int hidden, int64_t M);
size_t glam_relation_mlp_workspace_bytes(int De, int hidden, int64_t M);
int glam_relation_mlp_fwd(const float* w1, const float* b1, const float* w2, const float* b2, int De, int hidden, int64_t M, float* h,
                          float* out, void* stream);
int glam_relation_mlp_bwd(const float* d_out, const float* h, const float* w2, int De, int hidden, int64_t M, float* d_w1, float* d_b1,
                          float* d_w2, float* d_b2, void* ws, size_t ws_bytes, void* stream);

/* dot_and_global_pool5 (src_1gp/layer.py:270-283): for every pair i, [max, mean, median, min, std] of
 * S_i = mol[seg_i] @ pro[seg_i]^T — the reference's Python loop of matmul + max / mean / median / min / std per pair
 * (median = torch.median of the flattened scores: the LOWER median; std unbiased).  One block per pair, the score matrix is
 * never materialised.  D % 4 == 0, D <= 128 (the host zero-pads odd widths).  out f32[P,5]; arg int32[P,6] = global row
 * indices (a, b) of the max, the median and the min element (first occurrence in flattened order), kept for the backward pass.
 * An empty pair yields zeros / -1. */
int glam_pair_pool5_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr, int64_t P,
                        int D, float* out, int32_t* arg, void* stream);
int glam_pair_pool5_bwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                        const float* out, const int32_t* arg, const float* d_out, int64_t P, int D, float* d_mol,
                        float* d_pro, void* stream);

/* Block tail of the convs without a GRU (GCNConv / GATConv blocks, src_1gp/layer.py:248 and :263-266) in one launch per
 * direction: out = act(y + bias + identity) (bias / identity may be NULL; act codes as glam_gru_tail_fwd); the backward
 * returns d_y = d_out * act'(out) (= d_identity; d_bias is its column sum). */
int glam_bias_res_act_fwd(const float* y, const float* bias, const float* identity, int64_t N, int C, int act, float slope,
                          float* out, void* stream);
int glam_bias_res_act_bwd(const float* out, const float* d_out, int64_t N, int C, int act, float slope, float* d_y,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Set2Set readout (src_1gp/model.py:41: PyG Set2Set(C, processing_steps = 3)).
 *   glam_lstm_cell_fwd/bwd: gate math of one torch.nn.LSTM cell step; gates f32[B,4C] = W_ih q* + b_ih + W_hh h + b_hh
 *     (order i|f|g|o) -> h_new, c_new f32[B,C]; the backward recomputes the gates (d_h / d_c may be NULL = zero).
 *   glam_s2s_attn_fwd/bwd: e_n = <x_n, q_g>, a = softmax over the nodes of graph g (denominator + 1e-16), r_g = sum_n a_n x_n
 *     with x f32[N,D], q f32[B,D], ptr int32[B+1] -> r f32[B,D], stats f32[B,2] (segment max, exp-sum); the backward
 *     returns d_x f32[N,D] and d_q f32[B,D].  D % 4 == 0, D <= 128. */
int glam_lstm_cell_fwd(const float* gates, const float* c_prev, int64_t B, int C, float* h_new, float* c_new, void* stream);
int glam_lstm_cell_bwd(const float* gates, const float* c_prev, const float* d_h, const float* d_c, int64_t B, int C,
                       float* d_gates, float* d_c_prev, void* stream);
int glam_s2s_attn_fwd(const float* x, const float* q, const int32_t* ptr, int64_t N, int64_t B, int D, float* r,
                      float* stats, void* stream);
int glam_s2s_attn_bwd(const float* x, const float* q, const float* r, const float* stats, const float* d_r,
                      const int32_t* ptr, int64_t N, int64_t B, int D, float* d_x, float* d_q, void* stream);

/* ---- the GRU step of a MessageBlock in one launch -------------------------------------------------------------------------
 * src_1gp/layer.py:261-266: x = celu(conv out); x, h = GRU(x, h) (one step, seq_len 1); x = act(x + identity).  Both gate linears
 * (gi = celu(x) W_ih^T + b_ih, gh = h W_hh^T + b_hh) on the fp32 matrix cores with the gate math, residual and activation in their
 * epilogue: the same results, bit for bit, as glam_ts_gemm_pair + glam_gru_tail_fwd (resp. glam_gru_tail_rng_fwd), without the round
 * trip of gi / gh between them (both are still written: the backward, glam_gru_tail_*_bwd, recomputes the gates from them).
 * C a multiple of 4, at most 64.  Images: glam_gru_fused_make_images (two buffers of glam_gru_fused_image_bytes(), rebuilt whenever
 * the weights change).  act codes / RNG arguments as glam_gru_tail_fwd / glam_gru_tail_rng_fwd. */
int glam_gru_fused_supported(int C);
size_t glam_gru_fused_image_bytes(void);
int glam_gru_fused_make_images(const float* w_ih, const float* w_hh, int C, float* img_ih, float* img_hh, void* stream);
int glam_gru_fused_fwd(const float* x, const float* h, const float* identity, const float* img_ih, const float* img_hh,
                       const float* b_ih, const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float* gi, float* gh,
                       float* h_new, float* out, void* stream);
int glam_gru_fused_rng_fwd(const float* x, const float* h, const float* identity, const float* img_ih, const float* img_hh,
                           const float* b_ih, const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float rr_lower,
                           float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff, float* gi, float* gh, float* h_new,
                           float* out, float* out_drop, void* stream);

/* The same step (src_1gp/layer.py:261-266) warp-specialised on the bf16 matrix cores in 3 x bf16 form: every fp32 operand split exactly
 * into three bf16 terms, six partial products per product, fp32 accumulation — fp32 accuracy (measured: closer to the fp64 result than
 * the fp32 matrix instructions), roundings differ from glam_gru_fused_fwd at the last bits; RReLU / Dropout use the same Philox words.
 * img_ih / img_hh are the k_ts_gemm images of W_ih^T / W_hh^T (glam_ts_gemm_make_image(w, C, 1, C, 3 C, img): the ones glam_ts_gemm_pair
 * takes).  C a multiple of 4 in 24 .. 64.
 * gh = NULL (every glam_gru_ws_*fwd* form): gi is [N, 4C] and receives THE GATES [r | z | n | gh_n] instead of the two pre-activation
 * matrices — all the backward takes from them (r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n): the values
 * the backward would recompute, bit for bit).  4C instead of 6C floats per row written here and read by glam_gru_bwd_ws* (which takes
 * this matrix when ITS gh is NULL), and no sigmoid / tanh in the backward's vector waves. */
int glam_gru_ws_supported(int C);
int glam_gru_ws_fwd(const float* x, const float* h, const float* identity, const float* img_ih, const float* img_hh,
                    const float* b_ih, const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float* gi, float* gh,
                    float* h_new, float* out, void* stream);
int glam_gru_ws_rng_fwd(const float* x, const float* h, const float* identity, const float* img_ih, const float* img_hh,
                        const float* b_ih, const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float rr_lower,
                        float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff, float* gi, float* gh, float* h_new,
                        float* out, float* out_drop, void* stream);
/* ... also writing x_celu[N, C] = celu(x), the CELU of src_1gp/layer.py:261 as the launch applies it (celu_in must be set; x_celu may be
 * NULL): the tensor to keep for the backward INSTEAD of x.  glam_gru_bwd_ws(_rng) with celu_in = 2 takes x as celu(x) and forms
 * celu'(x) = x > 0 ? 1 : celu(x) + 1 from it, and the weight gradient of W_ih reads it as Q without a CELU of its own
 * (glam_wgrad_gemm_pair_split(_seg) with qcelu_a = 0): no exponential in either (the one wave that applied the CELU to all of Q set the
 * pace of the weight-gradient launch: 35.3 -> 25.8 us for three applications at N = 20 400). */
int glam_gru_ws_fwd_xc(const float* x, const float* h, const float* identity, const float* img_ih, const float* img_hh,
                       const float* b_ih, const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float* gi, float* gh,
                       float* h_new, float* out, float* x_celu, void* stream);
int glam_gru_ws_rng_fwd_xc(const float* x, const float* h, const float* identity, const float* img_ih, const float* img_hh,
                           const float* b_ih, const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float rr_lower,
                           float rr_upper, float drop_p, int64_t* rng_state, int64_t* rng_eff, float* gi, float* gh, float* h_new,
                           float* out, float* out_drop, float* x_celu, void* stream);

/* The gate matrices as the matrix waves of the warp-specialised step hold them: every 16 x 8 operand fragment already split into its
 * three bf16 terms, stored in lane order, ONCE per weight update (one launch for both images; either may be NULL).  weight_ih / weight_hh
 * are torch.nn.GRUCell's [3C, C] (layer.py:250), contiguous.  The *_pre entry points below read these instead of the k_ts_gemm images and
 * compute bit-identical results: what they drop is the prologue in which all 256 blocks of every launch re-split the same matrices
 * (~4 k of a block's ~31 k cycles at N = 20 400: forward 18.4 -> 15.2 us, backward 21.6 -> 20.0 us per application).
 * glam_gru_ws_pre_bytes(): size of ONE image (144 KB, 16-byte aligned), any supported C. */
size_t glam_gru_ws_pre_bytes(void);
int glam_gru_ws_make_pre(const float* w_ih, const float* w_hh, int C, void* pre_fwd, void* pre_bwd, void* stream);
int glam_gru_ws_fwd_pre(const float* x, const float* h, const float* identity, const void* pre_fwd, const float* b_ih, const float* b_hh,
                        int64_t N, int C, int celu_in, int act, float slope, float* gi, float* gh, float* h_new, float* out,
                        float* x_celu, void* stream);
int glam_gru_ws_rng_fwd_pre(const float* x, const float* h, const float* identity, const void* pre_fwd, const float* b_ih,
                            const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float rr_lower, float rr_upper,
                            float drop_p, int64_t* rng_state, int64_t* rng_eff, float* gi, float* gh, float* h_new, float* out,
                            float* out_drop, float* x_celu, void* stream);
/* ... and the node product of the block's NEXT application inside the same launch.  /root/reference/src_1gp/model.py:53-54 applies ONE
 * MessageBlock message_steps times: this step's output rows (`out`; in the rng form the dropped twin `out_drop` when it is given — what
 * layer.py:255-259 hands the conv) are the next TripletMessage's input, and its first product x @ [W_node | Wa] (layer.py:37 + the
 * separable attention columns) needs nothing else.  The producer waves take every finished 16-row tile out of LDS — the consumers leave
 * it there split into bf16 terms — through the 3 x bf16 product against node_pre (that matrix as pre-split operand fragments inside the
 * layer's staged buffer: staged + glam_triplet_staged_node_fragments(H, Cp, Dp); K = C = Cp, node_cols = H * Cp with 56 < node_cols <= 184) while the
 * ring is full, and write xw[N, node_cols] and a_ij[N, 8]: the values glam_ts_gemm / glam_triplet_layer_fwd_ell write for the same
 * rows, bit for bit (same partial products in the same order).  glam_triplet_layer_fwd_ell with x = NULL then starts at its aggregate
 * launch: one launch and one re-read of the rows less per application. */
int glam_gru_ws_fwd_pre_node(const float* x, const float* h, const float* identity, const void* pre_fwd, const float* b_ih,
                             const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float* gi, float* gh, float* h_new,
                             float* out, float* x_celu, const void* node_pre, int node_cols, float* xw, float* a_ij, void* stream);
int glam_gru_ws_rng_fwd_pre_node(const float* x, const float* h, const float* identity, const void* pre_fwd, const float* b_ih,
                                 const float* b_hh, int64_t N, int C, int celu_in, int act, float slope, float rr_lower, float rr_upper,
                                 float drop_p, int64_t* rng_state, int64_t* rng_eff, float* gi, float* gh, float* h_new, float* out,
                                 float* out_drop, float* x_celu, const void* node_pre, int node_cols, float* xw, float* a_ij,
                                 void* stream);
int glam_gru_bwd_ws_pre(const float* gi, const float* gh, const float* h, const float* out, const float* d_out, const float* d_hstate,
                        const float* x, const void* pre_bwd, int64_t N, int C, int celu_in, int act, float slope, int merge_identity,
                        float* d_gi, float* d_gh, float* d_identity, float* d_x, float* d_h, void* stream);
int glam_gru_bwd_ws_rng_pre(const float* gi, const float* gh, const float* h, const float* out, const float* d_out,
                            const float* d_out_drop, const float* d_hstate, const float* x, const void* pre_bwd, int64_t N, int C,
                            int celu_in, int act, float slope, float rr_lower, float rr_upper, float drop_p, const int64_t* rng_eff,
                            int merge_identity, float* d_gi, float* d_gh, float* d_identity, float* d_x, float* d_h, void* stream);

/* Backward of the same step in ONE launch: glam_gru_tail_bwd (resp. glam_gru_tail_rng_bwd) + the two input-gradient products
 *   d_x = d_gi @ W_ih (* celu'(x) when celu_in), d_h = d_gh @ W_hh + the direct g z path,
 * warp-specialised, the products in 3 x bf16 form.  d_gi / d_gh [N, 3C] are still written (the weight-gradient launch reads them), d_h
 * comes out COMPLETE (the tail kernels' d_h is only the direct part).  img_ih_t / img_hh_t: glam_ts_gemm_make_image(w, C, 0, 3 C, C, img),
 * the images glam_ts_gemm_pair takes for these products.  x is read only with celu_in; d_identity, d_hstate, d_out_drop may be NULL
 * (d_out too in the rng form when d_out_drop is given).  merge_identity = 1: the skip connection and the GRU state are the same tensor
 * (the first application of a block, src_1gp/layer.py:254) — d_h additionally receives d_identity and d_identity is not written.
 * gh = NULL and d_gh = NULL (both or neither; every glam_gru_bwd_ws* form): gi is the gate matrix [N, 4C] of a forward called with
 * gh = NULL, and d_gi is written as [N, 4C] = [d_pr | d_pz | d_pn | d_pn r] — d_gi and d_gh differ in their last block only;
 * glam_wgrad_gemm_gru_gates_seg forms both weight gradients from it.  Same d_x, d_h, d_identity and gate gradients, bit for bit.
 * C a multiple of 4 in 24 .. 64. */
int glam_gru_bwd_ws(const float* gi, const float* gh, const float* h, const float* out, const float* d_out, const float* d_hstate,
                    const float* x, const float* img_ih_t, const float* img_hh_t, int64_t N, int C, int celu_in, int act, float slope,
                    int merge_identity, float* d_gi, float* d_gh, float* d_identity, float* d_x, float* d_h, void* stream);
int glam_gru_bwd_ws_rng(const float* gi, const float* gh, const float* h, const float* out, const float* d_out, const float* d_out_drop,
                        const float* d_hstate, const float* x, const float* img_ih_t, const float* img_hh_t, int64_t N, int C,
                        int celu_in, int act, float slope, float rr_lower, float rr_upper, float drop_p, const int64_t* rng_eff,
                        int merge_identity, float* d_gi, float* d_gh, float* d_identity, float* d_x, float* d_h, void* stream);

/* ---- narrow-output linear (the model's output head) -------------------------------------------------------------------
 * y[N, M] = x[N, K] @ w[M, K]^T + b for M <= 16, K % 4 == 0: replaces torch.nn.functional.linear / its autograd for
 * `lin_out1 = LinearBlock(e_dim, out_dim)` (reference src_1gp/model.py:47,61; layer.py:223-237), where a GEMM library spends
 * 33 us forward + 22 us backward on what is a row dot product.  b, dx, db may be NULL.  Backward: dx[N, K], dw[M, K], db[M];
 * ws >= glam_linear_narrow_bwd_workspace_bytes(K, M), 16-byte aligned.  Deterministic (fixed-order sums, no atomics). */
int glam_linear_narrow_supported(int K, int M);
int glam_linear_narrow_fwd(const float* x, const float* w, const float* b, int64_t N, int K, int M, float* y, void* stream);
size_t glam_linear_narrow_bwd_workspace_bytes(int K, int M);
int glam_linear_narrow_bwd(const float* x, const float* w, const float* dy, int64_t N, int K, int M, float* dx, float* dw, float* db,
                           void* ws, size_t ws_bytes, void* stream);
/* The head reading the hidden layer's PRE-activation: y = Linear(Dropout(drop_p)(RReLU(rr_lower, rr_upper)(x))) in TRAINING mode — the
 * RReLU of `mol_flat` (/root/reference/src_1gp/model.py:43-45, :60, default activation model.py:31) and the Dropout `lin_out1` starts
 * with (layer.py:232-236, model.py:30) applied to every element as the row dot products read it.  Neither the activated matrix nor its
 * dropped twin is written: the two elementwise launches and their two backward launches are gone.  The words are the ones
 * glam_bias_res_act_rng_fwd draws for the same elements at the same stream position (y equals the three-launch pipeline's bit for
 * bit); rng_eff receives the (seed, offset) pair.  glam_linear_narrow_act_bwd: x is the same pre-activation, dx the gradient of THAT
 * (through the Dropout and the RReLU, words regenerated from rng_eff), dw / db the head's. */
int glam_linear_narrow_act_fwd(const float* x, const float* w, const float* b, int64_t N, int K, int M, float rr_lower, float rr_upper,
                               float drop_p, int64_t* rng_state, int64_t* rng_eff, float* y, void* stream);
int glam_linear_narrow_act_bwd(const float* x, const float* w, const float* dy, int64_t N, int K, int M, float rr_lower, float rr_upper,
                               float drop_p, const int64_t* rng_eff, float* dx, float* dw, float* db, void* ws, size_t ws_bytes,
                               void* stream);

/* Column sums out[D] = sum_n x[n, 0..D) of a row-major f32[N, ld] matrix (D, ld multiples of 4): the bias gradient of a linear whose
 * matrix products stay on the GEMM library (the 300 -> 1024 readout MLP, src_1gp/model.py:44-46).  ws (>= glam_colsum_workspace_bytes)
 * is only touched for N > 2048.  Fixed summation order. */
size_t glam_colsum_workspace_bytes(int D);
int glam_colsum(const float* x, int64_t N, int D, int ld, float* out, void* ws, size_t ws_bytes, void* stream);

/* Square-ish fp32 products on the bf16 matrix cores in 3 x bf16 form (fp32 accuracy; csrc/dense_x3.hip): the readout MLP of the model
 * (`mol_flat` LinearBlock(5 * hid_dim, e_dim = 1024) and wide output heads; /root/reference/src_1gp/model.py:43-45,60-61, LinearBlock
 * src_1gp/layer.py:196-209 = norm -> dropout -> nn.Linear -> act), i.e. torch's F.linear and its autograd for matrices with ~1000 rows.
 *
 *   C[R, Cn] = act( A . B + bias ),  A(r, k) = A[r * a_rs + k * a_ks] * (gate(r, k) > 0 ? 1 : gate_slope),  B(k, c) = B[k * b_ks + c * b_cs]
 *
 * exactly one stride of each pair is 1 (any of the four layout combinations; no transposed copies are made).  gate (same strides as
 * A) and bias[Cn] may be NULL.  act: 0 none, 1 ReLU, 2 LeakyReLU(act_slope), applied after the bias.  rowsum non-NULL (needs
 * b_cs == 1): rowsum[r] = sum_k A(r, k) (a virtual all-ones column of B).  K >= 4; 16-byte accesses are used where alignment and the
 * dimensions allow (multiples of 4), scalar ones elsewhere.  Deterministic (no atomics, no split reductions). */
int glam_dense_gemm(const float* A, int64_t a_rs, int64_t a_ks, const float* gate, float gate_slope, const float* B, int64_t b_ks,
                    int64_t b_cs, const float* bias, int act, float act_slope, float* C, int64_t ldc, float* rowsum, int R, int Cn, int K,
                    void* stream);
/* y[N, M] = act(x[N, K] w[M, K]^T + b) — nn.Linear + a fused ReLU / LeakyReLU — on glam_dense_gemm's kernel (b may be NULL). */
int glam_linear_dense_fwd(const float* x, const float* w, const float* b, int64_t N, int K, int M, int act, float slope, float* y,
                          void* stream);
/* Its backward in ONE launch: with g = dy * (y_gate > 0 ? 1 : gate_slope) (y_gate = the forward's OUTPUT when an activation was
 * fused, NULL otherwise): dx[N, K] = g w, dw[M, K] = g^T x, db[M] = column sums of g.  dx may be NULL; db may be NULL; N >= 4. */
int glam_linear_dense_bwd(const float* x, const float* w, const float* dy, const float* y_gate, float gate_slope, int64_t N, int K, int M,
                          float* dx, float* dw, float* db, void* stream);
/* The same two products with a workspace (glam_dense_ws_bytes() bytes, 16-byte aligned, contents irrelevant; launches that share it must
 * be ordered on one stream) that lets a product of few tiles and a long reduction split k across blocks — dx of the reference's batch
 * of 32 (run.py:40) is 5 tiles of 32 serial chunks beside 160 one-chunk tiles of dw.  Each split writes its partial tile; a second
 * launch adds them in split order and applies bias / activation (run-to-run identical; a launch boundary, not tickets: a device-wide
 * fence between the blocks of one launch writes back and invalidates a whole L2 on this chip).  A product with more than 32 tiles or
 * fewer than 16 chunks of 32 is not split and equals the plain entry points' result bit for bit.  ws == NULL: exactly the plain entry
 * points. */
size_t glam_dense_ws_bytes(void);
int glam_linear_dense_fwd_ws(const float* x, const float* w, const float* b, int64_t N, int K, int M, int act, float slope, float* y,
                             void* ws, size_t ws_bytes, void* stream);
int glam_linear_dense_bwd_ws(const float* x, const float* w, const float* dy, const float* y_gate, float gate_slope, int64_t N, int K,
                             int M, float* dx, float* dw, float* db, void* ws, size_t ws_bytes, void* stream);

/* One Adam step over n parameter tensors in one launch per 40 tensors — the optimizer of the training loop that drives the path
 * (`Adam(self.model.parameters(), lr=args.lr)`, src_1gp/trainer.py:49-50, stepped at trainer.py:301; torch.optim.Adam semantics
 * without amsgrad / maximize; weight_decay is the L2 form).  table: HOST array [n][4] of device addresses {param, grad, exp_avg,
 * exp_avg_sq} (f32, numel[i] elements each, contiguous); step: device f32 count of the steps taken so far, advanced by the launch
 * itself (a captured launch replays correctly); ticket: device u32[GLAM_ADAM_TICKET_WORDS], zero before the first call, owned by the optimizer; lr_dev: device
 * f32 learning rate read by the launch (NULL: the host value `lr`).  In place: param, exp_avg, exp_avg_sq. */
#define GLAM_ADAM_TICKET_WORDS 544
int glam_adam_max_tensors(void);
int glam_adam_step(const uint64_t* table, const int64_t* numel, int n, float* step, unsigned* ticket, const float* lr_dev, double lr,
                   double beta1, double beta2, double eps, double weight_decay, void* stream);

/* One Ranger step (RAdam + Lookahead + gradient centralisation; reference src_1gp/ranger.py:117-205, the other optimizer of the
 * reference's search, trainer.py:45-48) over n parameter tensors in one launch per 40 tensors.  table: HOST array [n][5] of device
 * addresses {param, grad, exp_avg, exp_avg_sq, slow_buffer} (f32, numel[i] elements each, contiguous); row[i]: the row length
 * numel / size(0) of a tensor whose gradient is centralised (a mean over dimensions 1..n per index of dimension 0), 0 for one that is
 * not.  step / ticket / lr_dev as for glam_adam_step (the step count of the launch is *step + 1, read on the device, and decides the
 * rectification branch and the Lookahead sync `s % k == 0`).  gc_loc != 0 centralises the gradient before the moments and writes it
 * back to grad (as the reference leaves p.grad); gc_loc == 0 centralises the update direction instead.  In the un-rectified branch
 * the direction is exp_avg itself, so weight decay and late centralisation also land in exp_avg (as in the reference).  In place:
 * param, exp_avg, exp_avg_sq, slow_buffer, and grad when it is centralised with gc_loc != 0. */
int glam_ranger_max_tensors(void);
int glam_ranger_step(const uint64_t* table, const int64_t* numel, const int64_t* row, int n, float* step, unsigned* ticket,
                     const float* lr_dev, double lr, double beta1, double beta2, double eps, double weight_decay, double alpha, int k,
                     double n_sma_threshold, int gc_loc, void* stream);

/* The training step's loss, value and gradient in one launch (mean reduction):
 *   kind 0  squared error          — `self.criterion(output, y_true)` with nn.MSELoss, src_1gp/trainer.py:296 / loss.py:42
 *   kind 1  BCE with logits        — nn.BCEWithLogitsLoss, loss.py:48
 *   kind 2  absolute error         — nn.L1Loss ('mae'), gradient sign(d) with sign(0) = 0
 *   kind 3  smooth L1, beta = 1    — nn.SmoothL1Loss ('huber', 'smae')
 *   kind 4  BCE on probabilities   — nn.BCELoss ('bce'): logs clamped at -100, gradient (x - y) / max(x (1 - x), 1e-12)
 *   masked != 0: the mean runs over the elements with target >= 0 only — `criterion(y_score[y_true >= 0], y_true[y_true >= 0])`,
 *   trainer.py:244-245 (labels of -1 are missing, dataset.py:138), without the boolean indexing (not capturable in a hipGraph).
 * pred, target: f32[n]; loss, inv_count: f32[1] (the mean and 1 / count; count = 0 gives nan like the reference's empty mean);
 * grad: f32[n] un-normalised d loss_i / d pred_i; ws >= glam_loss_workspace_bytes(); ticket: device u32[GLAM_ADAM_TICKET_WORDS],
 * zero before the first call, re-armed by every call (n > 1024 only).  Fixed summation order.
 * glam_loss_bwd: d_pred[i] = grad[i] * g_up[0] * inv_count[0] (g_up: the f32[1] gradient arriving at the loss). */
size_t glam_loss_workspace_bytes(void);
int glam_loss_fwd(const float* pred, const float* target, int64_t n, int kind, int masked, float* loss, float* inv_count, float* grad,
                  void* ws, size_t ws_bytes, unsigned* ticket, void* stream);
int glam_loss_bwd(const float* grad, const float* inv_count, const float* g_up, int64_t n, float* d_pred, void* stream);

/* The cross-entropy family in one launch: logits x: f32[B, C] (contiguous), labels y: int64[B], weight: f32[C] or NULL.
 *   focal 0  nn.CrossEntropyLoss(weight, ignore_index): mean of w[y_i] ce_i over the rows with y_i != ignore_index, divided by the
 *            sum of their w[y_i] (nan when every row is ignored, as in torch; inv_count is then 0, torch's zero gradient)
 *   focal 1  the reference's FocalLoss(alpha, gamma) (src_1gp/loss.py:3-16): mean over all B rows of alpha (1 - pt)^gamma ce_i,
 *            pt = exp(-ce_i), ignored rows 0; gamma = 0 or gamma >= 1 only (other exponents make torch's own gradient 0 * inf on
 *            ignored rows), no weight.
 * A label outside [0, C) that is not ignore_index is never used as an index: the loss and that row's gradient are nan (torch raises
 * a device-side assert instead).  loss, inv_count, grad [B, C], ws and ticket as for glam_loss_fwd (ws / ticket are needed once
 * B exceeds one block's rows); the backward is glam_loss_bwd with n = B * C.  1 <= C <= glam_ce_loss_max_classes().  Fixed
 * summation order (per row thread-sequential, then a lane butterfly; over rows as glam_loss_fwd): bit-reproducible. */
int glam_ce_loss_max_classes(void);
int glam_ce_loss_fwd(const float* x, const int64_t* y, const float* weight, int64_t B, int C, int64_t ignore_index, int focal,
                     float alpha, float gamma, float* loss, float* inv_count, float* grad, void* ws, size_t ws_bytes, unsigned* ticket,
                     void* stream);

/* Evaluation metrics of the reference's trainers, scored on the device (reference src_1gp/metrics.py, src_2gi_ddi/utils.py; the
 * trainers call them on the validation split after every epoch, trainer.py:79-98).  Every order-based metric comes from per-sample
 * counts over the samples of the same task (O(n^2) pair steps per task, no sort); integer counts and fp64 sums in a fixed order, so a
 * call is bit-identical run to run.  Inputs are device arrays; key_dtype / dtype: 0 = f32, 1 = f64 keys (scores, targets);
 * label_dtype: 0 = f32, 1 = f64 labels and predictions.  n < GLAM_METRICS_MAX_N per task (int32 counts).  ws >=
 * glam_metrics_workspace_bytes(n, tasks, n_class) (n_class = 0 for the binary / regression forms; 0 = arguments out of range);
 * record: device buffer of GLAM_METRICS_RECORD_BYTES = int64 i[16] then f64 d[16], written by the call's last launch.  Two launches
 * per call.  The bad flag reports a label outside the allowed set or a non-finite key (the reference's ValueError).
 *
 * glam_metrics_binary — roc_auc_score / precision_recall_curve + auc / accuracy / precision / recall / f1 of binary_metrics
 * (metrics.py:16-29), binary_metrics_multi_target_nan (metrics.py:32-56; masked = 1: label -1 = missing), screening_metrics,
 * bedroc_score and enrichment_factor_single (metrics.py:102-167).  score, label, pred: [n, tasks] row-major; pred_mode 0: pred holds
 * 0/1 predictions, 1: score >= threshold, 2: score > threshold (pred unused); alpha: BEDROC's; pct_host: HOST array of n_pct <= 5
 * EF fractions.  Ties of equal scores rank in index order (the reference's unstable argsort leaves that order undefined).
 * Record: i = {kept tasks, skipped tasks (one class only), bad, P, N, tp, fp, tn, fn (task 0), EF hits [5] (task 0),
 * 2 x AUC numerator (task 0), -}, d = {sum over kept tasks of auc, acc, precision, recall (binary averaging), PR-AUC (task 0),
 * sum of exp(-alpha rank / n) over the positives (task 0)}.
 * glam_metrics_regression — cal_ci + mean_squared_error + r2_score of regression_metrics (metrics.py:59-90, and
 * src_2gi_dti_scr/utils.py:109-141).  y, f: [n].  Record: i = {pairs (y_j < y_i), of those f_j < f_i, of those f_j == f_i, bad},
 * d = {sum (y - f)^2, sum (y - mean y)^2, sum y}.
 * glam_metrics_multiclass — multi_class_metrics (src_2gi_ddi/utils.py:138-151): pred = the first argmax of score [n, n_class] (score
 * may be null when pred is given), label / pred integral in [0, n_class), n_class <= 4096.  Record: i = {correct rows, classes seen
 * (in labels or predictions), bad, n}, d = {sums over the classes seen of precision, recall, F1}. */
#define GLAM_METRICS_RECORD_BYTES 256
#define GLAM_METRICS_MAX_N 2147483647LL
size_t glam_metrics_workspace_bytes(int64_t n, int64_t tasks, int n_class);
int glam_metrics_binary(const void* score, const void* label, const void* pred, int key_dtype, int label_dtype, int64_t n, int64_t tasks,
                        int masked, int pred_mode, double threshold, double alpha, const double* pct_host, int n_pct, void* ws,
                        size_t ws_bytes, void* record, void* stream);
int glam_metrics_regression(const void* y, const void* f, int dtype, int64_t n, void* ws, size_t ws_bytes, void* record, void* stream);
int glam_metrics_multiclass(const void* score, const void* label, const void* pred, int key_dtype, int label_dtype, int64_t n,
                            int n_class, void* ws, size_t ws_bytes, void* record, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Column norms over a dense, contiguous f32[N, C] (any C >= 1, N * C < 2^31; the 16-byte path when C % 4 == 0 and the [N, C]
 * pointers are 16-byte aligned, scalar accesses otherwise).  Replaces torch.nn.BatchNorm1d behind _BatchNorm (src_1gp/layer.py:161-167)
 * and PyG's graph LayerNorm with batch = None behind _LayerNorm (src_1gp/layer.py:170-176; mol_flat and lin_out1, model.py:60-61).
 * Fixed-order sums, centred variances, no atomics: results are bit-identical from run to run.  DESIGN.md 4.12.
 *
 * form: 0 = the library's choice, 1 = one launch (BatchNorm: a block owns a column tile and walks all rows; LayerNorm: one block),
 * 2 = slab partials + apply launch (needs ws of glam_colnorm_workspace_bytes; form 1 of the LayerNorm backward needs 2 C floats of it).
 * max_blocks: cap on the grid of each launch (<= 0: the library's 1024); the grid-stride loops cover the rest (test hook).
 *
 * BatchNorm, training (N >= 2): y = (x - mean) * rstd * weight + bias with the batch statistics of each column; running_mean <-
 * (1 - momentum) running_mean + momentum mean, running_var likewise with the UNBIASED variance; save_mean / save_rstd f32[C] are what
 * the backward reads.  Eval: the same with the running statistics (save_mean = running_mean, save_rstd = 1 / sqrt(running_var + eps)).
 * Backward: d_bias = sum dy, d_weight = sum dy xhat, dx = weight rstd (dy - mean(dy) - xhat mean(dy xhat)); eval != 0: dx = dy weight rstd. */
size_t glam_colnorm_workspace_bytes(int64_t N, int C);
int glam_batch_norm_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var, int64_t N, int C,
                        float momentum, float eps, float* y, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, int form,
                        int max_blocks, void* stream);
int glam_batch_norm_eval_fwd(const float* x, const float* weight, const float* bias, const float* running_mean, const float* running_var,
                             int64_t N, int C, float eps, float* y, float* save_mean, float* save_rstd, int max_blocks, void* stream);
int glam_batch_norm_bwd(const float* x, const float* dy, const float* weight, const float* mean, const float* rstd, int64_t N, int C,
                        int eval, float* dx, float* d_weight, float* d_bias, void* ws, size_t ws_bytes, int form, int max_blocks,
                        void* stream);
/* Batch-less LayerNorm: m = mean(x), s = sqrt(mean((x - m)^2)) over ALL N * C elements, y = (x - m) / (s + eps) * weight + bias (eps is
 * added to the standard deviation); stat f32[2] = {m, s} is what the backward reads.  Backward, with g = dy weight: dx = (g - mean(g)) /
 * (s + eps) - (x - m) mean(g (x - m)) / (s (s + eps)^2), d_weight = sum_rows dy (x - m) / (s + eps), d_bias = sum_rows dy.  A constant
 * input (s = 0) has no finite gradient. */
int glam_layer_norm_flat_fwd(const float* x, const float* weight, const float* bias, int64_t N, int C, float eps, float* y, float* stat,
                             void* ws, size_t ws_bytes, int form, int max_blocks, void* stream);
int glam_layer_norm_flat_bwd(const float* x, const float* dy, const float* weight, const float* stat, int64_t N, int C, float eps, float* dx,
                             float* d_weight, float* d_bias, void* ws, size_t ws_bytes, int form, int max_blocks, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention export: the weights the fused kernels above never write (they keep only `stats`, the inference forward not even that).
 * Inference only (no backward), no atomics, every reduction in a fixed order: two runs are bit-equal.  Each entry point returns 0
 * without launching when N == 0, E == 0 or B == 0.
 *
 * glam_edge_attention: the alpha of src_1gp/layer.py:48-51 (TripletMessage) and :92-95 (TripletMessageLight), in the separable form and
 * the arithmetic of glam_triplet_fwd:
 *   logit[e,h] = leaky_relu(a_ij[dst,h] + sum_k edge_attr[e,k]*M[k,h] + a_ij[src,4+h], slope)
 *   alpha      = segment softmax of logit over the incoming edges of dst (max-shifted, denominator + 1e-16)
 * a_ij f32[N,8]; edge_attr f32[E,De] (De in {4,8}); M f32[De,4]; CSR by target (rowptr,src,eid); 1 <= H <= 4.
 * Output alpha f32[E,4] in the CALLER's edge order (row eid[e]; one 16-byte store per edge, the layout of B1's alpha_e), columns
 * H..3 written as zero.  A group of 8 lanes per target node, one edge per lane: a row of at most 8 edges (every molecular graph)
 * is one pass over memory with its logits in registers; a longer row is strided by its group (max, exp-sum, write) and recomputes
 * them — a hub's row is walked serially by its 8 lanes, which an export can afford.  In-degree 0 writes nothing. */
int glam_edge_attention(const float* a_ij, const float* edge_attr, const float* M, const int32_t* rowptr, const int32_t* src,
                        const int32_t* eid, int64_t N, int64_t E, int H, int De, float slope, float* alpha, void* stream);
/* "Attention sent": sent f32[N,4], sent[n,h] = sum of alpha[e,h] over the edges that LEAVE n (how much the neighbours listen to atom
 * n), over the CSR by source (colptr, eid_t of glam_csr_build(by = 1)) and summed in CSR order; columns H..3 are zero.  With E == 0
 * nothing is launched and sent is left as the caller passed it (glam_amd.explain passes zeros). */
int glam_edge_attention_sent(const float* alpha, const int32_t* colptr, const int32_t* eid_t, int64_t N, int64_t E, int H, float* sent,
                             void* stream);
/* Per-graph softmax weights w f32[N] over contiguous node segments ptr int32[B+1] (max-shifted, denominator + 1e-16).
 *   gate != NULL: softmax of gate f32[N] — the weights of GlobalAttention behind GlobalLAPool (src_1gp/layer.py:206-220);
 *   gate == NULL: the logits are <x_n, q_g>, formed in the kernel as in glam_s2s_attn_fwd — Set2Set's read (src_1gp/model.py:41);
 *                 x rows are ld floats apart and hold D channels, q f32[B,ld]; ld % 4 == 0, ld <= 128, 1 <= D <= ld, else
 *                 GLAM_E_UNSUPPORTED.
 * A wave per graph; empty graphs write nothing. */
int glam_segment_softmax(const float* gate, const float* x, const float* q, const int32_t* ptr, int64_t N, int64_t B, int D, int ld,
                         float* w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A batch out of a device-resident dataset, its graph index included, in ONE launch.
 * Replaces: PyG's Batch.from_data_list as the reference's DataLoader runs it for every training batch (src_1gp/trainer.py:37-41,
 * :292-295: concatenate x / edge_attr / y, offset edge_index by the running node count, build batch and ptr) and, on this side, what
 * a fresh batch costs after it: a host-to-device copy per field, glam_csr_build for both directions, glam_ell_build for both and
 * glam_batch_ptr.  A batch is a disjoint union of graphs, so all of these are segmented copies of what was built ONCE for the dataset
 * taken as one big disjoint graph (glam_csr_build by target and by source, glam_ell_build on each), with two offsets added: slot b
 * holds graph g = ids[b]; node ids move by node_off[b] - node_ptr[g], edge ids and row pointers by edge_off[b] - edge_ptr[g]; the
 * -1 of an empty ELL slot stays.  No workspace, no atomics, no flag to read back: the caller has checked the ids.
 *
 * ds_host / out_host: HOST arrays of GLAM_COLLATE_FIELDS device pointers, field by field the dataset's tensor and the batch's:
 *    0 x          rows of x_row_bytes                        ->  x [N rows]
 *    1 ei         int32 [2, Ed], graph-LOCAL node ids        ->  edge_index int64 [2, E], the batch's node ids
 *    2 ea         rows of ea_row_bytes (0: none)             ->  edge_attr [E rows]
 *    3 y          rows of y_row_bytes (0: none)              ->  y [Y rows]
 *    4 node_ptr   int32 [G + 1]                              ->  batch int64 [N]
 *    5 edge_ptr   int32 [G + 1]                              ->  ptr int64 [B + 1]
 *    6 y_ptr      int32 [G + 1]                              ->  ptr int32 [B + 1]  (the readouts' segment pointer)
 *    7..9   rowptr [Nd + 1], src [Ed], eid [Ed]   (by target) ->  rowptr int32 [N + 1] (rowptr[N] = E), src [E], eid [E]
 *   10..12  colptr [Nd + 1], dst [Ed], eid_t [Ed] (by source) ->  colptr [N + 1], dst [E], eid_t [E]
 *   13, 14  ell_src, ell_eid     int32 [Nd, 4]                ->  [N, 4], written when out_host[13] and [14] are given
 *   15, 16  ell_dst, ell_eid_t   int32 [Nd, 4]                ->  [N, 4], written when out_host[15] and [16] are given
 * Row sizes are multiples of 4 bytes; rows move as 16-byte units where they are whole units and both tensors start on one, as dwords
 * otherwise (rows of 15 or 49 floats).  ELL tensors are 16-byte aligned, int64 tensors 8-byte aligned.
 * table int32 [4, B + 1] (device): ids (B entries, one of padding), then the exclusive offsets of the slots' nodes, edges and y rows,
 * each closed by its total (N, E, Y).  glam_collate_lds_slots(): the B up to which a block keeps the table in LDS; beyond it the
 * kernel searches the table in global memory.
 * GLAM_E_INVALID for null / misaligned pointers and sizes out of range (checked before any device work), GLAM_E_UNSUPPORTED for a
 * field of 2^31 elements or more. */
#define GLAM_COLLATE_FIELDS 17
size_t glam_collate_lds_slots(void);
int glam_collate(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t N, int64_t E,
                 int64_t Y, int64_t Ed, int32_t x_row_bytes, int32_t ea_row_bytes, int32_t y_row_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * glam_collate into tensors of FIXED CAPACITY, so that the launch — grid, sizes, every pointer — is the same for every batch of B graphs
 * and can sit inside a captured hipGraph.  Replaces: nothing in the reference (its loader shuffles and its step runs eagerly); here it
 * is what lets a shuffling loop replay one captured training step.
 * The output is an ordinary batch of B + 1 graphs: the B real ones first, exactly as glam_collate writes them for the same table
 * (rows [0, N) of the node fields, [0, E) of the edge fields, [0, B * y_rows) of y, slots [0, B] of both ptr), then ONE phantom graph
 * that owns the surplus P = N_cap - N nodes and E_pad = E_cap - E edges.  N = table[1][B] and E = table[2][B] are read on the device.
 * Phantom node p (id N + p): batch = B, x row zero, a contiguous run of self-loops (N + p, N + p) of q + (p < rem) edges starting at
 * E + p * q + min(p, rem), with q = E_pad / P and rem = E_pad % P.  rowptr / colptr continue from E with those run lengths and close
 * with E_cap at [N_cap]; src = dst = N + p; eid = eid_t = the edge's own position; the ELL records (where given) hold the run in order
 * and -1 in the free slots; edge_attr rows of phantom edges are copies of the dataset's edge row 0; ptr[B] = N, ptr[B + 1] = N_cap.
 * out_host as for glam_collate with these sizes: x [N_cap rows of x_out_stride_bytes], edge_index int64 [2, E_cap], edge_attr [E_cap
 * rows], y [B * y_rows rows], batch [N_cap], ptr int64 / int32 [B + 2], rowptr / colptr [N_cap + 1], src / eid / dst / eid_t [E_cap],
 * ELL [N_cap, 4].  x_out_stride_bytes >= x_row_bytes, a multiple of 16, x output 16-byte aligned: the pad columns of EVERY row are
 * written as zero (the kernels' zero-padded row layout, written in place).  y_rows: rows of y per graph, one constant.
 * The caller guarantees: P >= 1, E_pad >= 0, 4 * P >= E_pad where an ELL pair is given (phantom degrees stay <= 4), table as for
 * glam_collate.  No workspace, no atomics, no flag.
 * GLAM_E_INVALID for null / misaligned pointers, B < 1, N_cap < 1, E_cap < 0 or E_cap > 0 over a dataset without edges, sizes
 * beyond int32, a stride that is no multiple of 16 or below x_row_bytes, y given with y_rows < 1 (all checked before any device
 * work); GLAM_E_UNSUPPORTED for a field of 2^31 elements or more. */
int glam_collate_padded(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t N_cap, int64_t E_cap,
                        int64_t y_rows, int64_t Ed, int32_t x_row_bytes, int32_t x_out_stride_bytes, int32_t ea_row_bytes,
                        int32_t y_row_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * glam_collate_padded with the surplus nodes cut into K phantom graphs, so that no phantom graph grows with the batch: the kernels
 * that give a graph to one wave or block (graph norms, readouts) then see K small graphs where glam_collate_padded hands them one of
 * P nodes.  Same kernel, same launch, capturable the same way; glam_collate_padded is K = 1.
 * The output is an ordinary batch of B + K graphs.  With s = P / K and r = P % K, phantom graph j (0 <= j < K) owns the s + (j < r)
 * consecutive nodes from N + j * s + min(j, r) on: batch[N + p] = B + (p < r (s + 1) ? p / (s + 1) : r + (p - r (s + 1)) / s),
 * ptr[B + j] = N + j * s + min(j, r) for 0 <= j <= K (ptr[B] = N, ptr[B + K] = N_cap).  Everything else — the real part, the phantom
 * nodes' self-loop runs, both CSR tails, the ELL records, edge_attr, x, y — is what glam_collate_padded writes: the runs are per node,
 * so the cut moves no edge.  out_host as for glam_collate_padded except ptr int64 / int32 [B + K + 1].  The K phantom graphs take no
 * entries of the slot table: glam_collate_lds_slots() bounds B alone.
 * The caller guarantees what glam_collate_padded asks and K <= P (no phantom graph is empty).
 * GLAM_E_INVALID as for glam_collate_padded, and for K < 1, N_cap < K or B + K beyond int32 (checked before any device work). */
int glam_collate_padded_split(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t K, int64_t N_cap,
                              int64_t E_cap, int64_t y_rows, int64_t Ed, int32_t x_row_bytes, int32_t x_out_stride_bytes,
                              int32_t ea_row_bytes, int32_t y_row_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Refillable pair lists (csrc/pairlist.hip): what glam_pair_pool_shared_fwd / _bwd, glam_pair_pool_gather_train_fwd / _bwd and
 * glam_pair_rows_bwd read of a step's pairs, written into tensors of FIXED addresses by ONE launch — grid, sizes and every pointer the
 * same for every step, so the launch can sit inside a captured hipGraph.  Replaces: nothing in the reference (its loaders collate one
 * graph per pair and side); here it is what lets an epoch of SHUFFLED pairs replay one captured forward_shared step.
 * Inputs, all on the device and trusted (the host validates before anything is enqueued): ids int32 [B], the step's pair ids, NULL =
 * identity (ids[i] = i); col_a / col_b int32 [Np], the dataset's pair columns — a segment id per pair — either NULL = that side is
 * absent; y [Np rows of y_row_bytes], the dataset's labels, or NULL.
 * Outputs per present side s, over Q_s segments, capacity P >= B, padding segment pad_s in [0, Q_s):
 *   idx_s   int32 [P]:       col_s[ids[i]] for i < B, pad_s for B <= i < P
 *   order_s int32 [P]:       the STABLE argsort of idx_s (the slots of one segment in ascending i)
 *   ptr_s   int32 [Q_s + 1]: the offsets of the segments' runs in order_s, ptr_s[Q_s] = P
 * bit for bit np.argsort(idx, kind="stable") and [0] + cumsum(bincount(idx, minlength=Q)): the lists ops.PairsByProtein builds on the
 * host, on whose order the backward kernels' run-to-run bit equality rests.  y_out [B rows] = y[ids[i]], bytewise (y_row_bytes a
 * multiple of 4, both on a 4-byte boundary).  EVERY output word is written by every launch, by exactly one lane: a second, different
 * load leaves no residue.  No workspace, no atomics, no LDS.
 * The build is O(P * Q / 64) wave rounds per side: GLAM_E_UNSUPPORTED for P > 65 536, Q > 65 536 or P * Q > 2^26 on a present side —
 * checked before the pointers are looked at; glam_pair_list_supported(P, Q) is that check alone and returns a STATUS.
 * GLAM_E_INVALID for P < 1, B outside [0, P], nothing to load (no side, no y), a present side with Q < 1, pad outside [0, Q) or a
 * null output, y without y_out (or the reverse), label rows that are no multiple of 4 bytes or misaligned. */
int glam_pair_list_supported(int64_t P, int64_t Q);
int glam_pair_list_load(const int32_t* ids, const int32_t* col_a, const int32_t* col_b, const void* y, int32_t y_row_bytes, int64_t B,
                        int64_t P, int64_t Qa, int64_t Qb, int32_t pad_a, int32_t pad_b, int32_t* idx_a, int32_t* order_a,
                        int32_t* ptr_a, int32_t* idx_b, int32_t* order_b, int32_t* ptr_b, void* y_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GCN aggregation from an edge list's own CSR (csrc/gcn.hip).  Replaces: PyG's GCNConv.propagate behind add_remaining_self_loops +
 * gcn_norm with unit edge weights (torch_geometric/nn/conv/gcn_conv.py), as a closed form over the RAW edge list — no derived edge list,
 * no per-edge norm vector — so it holds on a batch whose index a kernel rewrites in place:
 *   deg[i] = 1 + #{e -> i : src_e != i}                 dis[i] = 1 / sqrt(deg[i])
 *   out[i] = dis[i] * ( dis[i] * xw[i] + sum_{e -> i, src_e != i} dis[src_e] * xw[src_e] )
 *   d_xw[j] = dis[j] * ( dis[j] * g[j] + sum_{e : j -> i, i != j} dis[i] * g[i] )
 * Existing self-loops are skipped and every node gets one implicit loop; duplicates count as often as they occur; an isolated node
 * returns xw[i].  Summation order: the own term first, then the row's edges in CSR order (one fmaf each), then the multiply by dis.
 * glam_gcn_scale: rowptr int32 [N + 1] / src int32 [E], the CSR by target -> dis fp32 [N].
 * glam_gcn_fwd:   xw fp32 [N rows, ld floats apart, D channels], the same CSR -> out fp32 [N, D] (contiguous).
 * glam_gcn_bwd:   g fp32 [N, D], colptr int32 [N + 1] / dst int32 [E], the CSR by source -> d_xw fp32 [N, D].
 * 1 <= D <= 128 (GLAM_E_UNSUPPORTED beyond); a 16-byte path when D % 4 == 0, ld % 4 == 0 and both row bases are 16-byte aligned, a
 * scalar path otherwise.  Any degree, 0 included.  No atomics, no workspace, no read-back; every output word is written by exactly one
 * lane, so two runs agree bit for bit.  Index entries outside [0, N) are skipped.  N == 0 launches nothing.
 * GLAM_E_INVALID for N out of range, ld < D or a null pointer. */
int glam_gcn_scale(const int32_t* rowptr, const int32_t* src, int64_t N, float* dis, void* stream);
int glam_gcn_fwd(const float* xw, int64_t ld, const float* dis, const int32_t* rowptr, const int32_t* src, int64_t N, int32_t D, float* out,
                 void* stream);
int glam_gcn_bwd(const float* g, const float* dis, const int32_t* colptr, const int32_t* dst, int64_t N, int32_t D, float* d_xw,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GLAM_HIP_H */
