// Column norms over a dense f32[N, C]: torch.nn.BatchNorm1d (PyG BatchNorm behind _BatchNorm, src_1gp/layer.py:161-167) in training and
// eval mode, and PyG's graph LayerNorm with batch = None behind _LayerNorm (src_1gp/layer.py:170-176: ONE mean and ONE standard
// deviation over the whole tensor, then a per-column affine), forward and backward.  DESIGN.md §4.12.
//
// One thread layout serves every kernel: a block of 256 threads is 16 row groups x 16 column lanes (rg = tid >> 4, cl = tid & 15); a
// lane owns V consecutive columns (V = 4: one 16-byte access, taken when C % 4 == 0 and every [N, C] pointer is 16-byte aligned;
// V = 1: scalar accesses, any C, any alignment), so a block covers a column tile of 16 V columns and walks rows rg, rg + 16, ...
// Sums are reduced in a fixed order (a thread's rows in order, then the 16 row groups in order, then the row slabs in order): no
// atomics, no grid barrier, bit-identical from run to run.  Variances come from centred sums (a mean pass, then a pass over the
// deviations whose own sum corrects the mean: the corrected two-pass algorithm), never from E[x^2] - E[x]^2.
//
// Two forms of every BatchNorm pass.  Column-owner (few rows): a block owns a column tile, walks all rows, and does statistics,
// normalise + affine and the running-statistics update in ONE launch.  Row-split (many rows): launch 1 reduces slabs of kSlabRows
// rows to per-column partials in a workspace (mean, M2; the count of a slab follows from N); launch 2 combines them in every
// block (n_slabs x 16 V values) and normalises the block's slab; the blocks of slab 0 write the per-column results.
#include "common.h"

#include <initializer_list>

namespace glam {

constexpr int kSlabRows = 128;          // rows of a row-split slab: 8 per thread
constexpr int kColOwnerMaxRows = 256;   // column-owner form up to here (16 rows per thread), row-split beyond
constexpr int kLnChunk = 4096;          // flat elements of a LayerNorm statistics chunk (a multiple of 4)
constexpr int kLnOneBlock = 16384;      // N * C up to which one block runs a whole LayerNorm pass
constexpr int kNormBlocks = 1024;       // cap on the grid (4 x 256 CUs); grid-stride beyond

template <int V> __device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
    if constexpr (V == 4) { const float4 t = ld4(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
    if constexpr (V == 4) st4(p, make_float4(v[0], v[1], v[2], v[3]));
    else *p = v[0];
}

// a[k] <- sum over the 16 row groups, in row-group order, of the a[k] of the threads with this thread's column lane.
// s_part: 256 K floats.  Two barriers: every thread of the block must call it.
template <int K> __device__ __forceinline__ void colreduce(float (&a)[K], float* s_part) {
    const int tid = threadIdx.x, cl = tid & 15;
#pragma unroll
    for (int k = 0; k < K; ++k) s_part[k * 256 + tid] = a[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += s_part[k * 256 + g * 16 + cl];
        a[k] = s;
    }
    __syncthreads();
}

// sum over the block in a fixed order (DPP butterfly inside a wave, then the 4 waves in order); s_red: 4 floats; two barriers
__device__ __forceinline__ float block_sum(float v, float* s_red) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return t;
}

// Per-column mean and M2 = sum (x - mean)^2 of rows [r0, r1) for this thread's V columns from c (act: the columns exist).
template <int V>
__device__ __forceinline__ void tile_mean_m2(const float* x, int64_t r0, int64_t r1, int C, int c, bool act, float* s_part,
                                             float (&mean)[V], float (&m2)[V]) {
    const int rg = threadIdx.x >> 4;
    const float n = (float)(r1 - r0);
    float a[V], v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = 0.f;
    if (act) {
#pragma unroll 4
        for (int64_t r = r0 + rg; r < r1; r += 16) {
            ldv<V>(x + r * C + c, v);
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] += v[j];
        }
    }
    colreduce<V>(a, s_part);
#pragma unroll
    for (int j = 0; j < V; ++j) mean[j] = a[j] / n;
    float q[2 * V];
#pragma unroll
    for (int j = 0; j < 2 * V; ++j) q[j] = 0.f;
    if (act) {
#pragma unroll 4
        for (int64_t r = r0 + rg; r < r1; r += 16) {
            ldv<V>(x + r * C + c, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = v[j] - mean[j];
                q[j] += d;
                q[V + j] += d * d;
            }
        }
    }
    colreduce<2 * V>(q, s_part);
#pragma unroll
    for (int j = 0; j < V; ++j) {      // the deviations' own sum is the rounding error of the first mean: fold it back
        mean[j] += q[j] / n;
        m2[j] = fmaxf(q[V + j] - q[j] * q[j] / n, 0.f);
    }
}

// The partials of all slabs -> mean and M2 of the N rows (Chan's combination, many-way: M2 = sum M2_s + n_s (mean_s - mean)^2, with
// the same correction of the first mean as above).  ws: [n_slabs][2][C] = mean | M2 per slab.
template <int V>
__device__ __forceinline__ void combine_mean_m2(const float* ws, int64_t N, int n_slabs, int C, int c, bool act, float* s_part,
                                                float (&mean)[V], float (&m2)[V]) {
    const int rg = threadIdx.x >> 4;
    float a[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = 0.f;
    if (act)
        for (int s = rg; s < n_slabs; s += 16) {
            const float ns = (float)(min((int64_t)kSlabRows, N - (int64_t)s * kSlabRows));
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] += ns * ws[((size_t)s * 2) * C + c + j];
        }
    colreduce<V>(a, s_part);
#pragma unroll
    for (int j = 0; j < V; ++j) mean[j] = a[j] / (float)N;
    float q[2 * V];
#pragma unroll
    for (int j = 0; j < 2 * V; ++j) q[j] = 0.f;
    if (act)
        for (int s = rg; s < n_slabs; s += 16) {
            const float ns = (float)(min((int64_t)kSlabRows, N - (int64_t)s * kSlabRows));
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = ws[((size_t)s * 2) * C + c + j] - mean[j];
                q[j] += ns * d;
                q[V + j] += ws[((size_t)s * 2 + 1) * C + c + j] + ns * d * d;
            }
        }
    colreduce<2 * V>(q, s_part);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        mean[j] += q[j] / (float)N;
        m2[j] = fmaxf(q[V + j] - q[j] * q[j] / (float)N, 0.f);
    }
}

// y = (x - mean) * scale + shift over rows [r0, r1) of this thread's columns
template <int V>
__device__ __forceinline__ void tile_affine(const float* x, float* y, int64_t r0, int64_t r1, int C, int c, const float (&mean)[V],
                                            const float (&scale)[V], const float (&shift)[V]) {
    const int rg = threadIdx.x >> 4;
    float v[V];
#pragma unroll 4
    for (int64_t r = r0 + rg; r < r1; r += 16) {
        ldv<V>(x + r * C + c, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (v[j] - mean[j]) * scale[j] + shift[j];
        stv<V>(y + r * C + c, v);
    }
}

// what the owner of a column writes once the batch statistics are known (the threads of row group 0)
template <int V>
__device__ __forceinline__ void bn_write_stats(int c, int64_t N, const float (&mean)[V], const float (&m2)[V], float momentum, float eps,
                                               float* running_mean, float* running_var, float* save_mean, float* save_rstd) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        save_mean[c + j] = mean[j];
        save_rstd[c + j] = 1.f / sqrtf(m2[j] / (float)N + eps);
        running_mean[c + j] = (1.f - momentum) * running_mean[c + j] + momentum * mean[j];
        running_var[c + j] = (1.f - momentum) * running_var[c + j] + momentum * (m2[j] / (float)(N - 1));
    }
}

template <int V>
__device__ __forceinline__ void bn_scale_shift(const float* weight, const float* bias, int c, bool act, int64_t N, const float (&m2)[V],
                                               float eps, float (&scale)[V], float (&shift)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        scale[j] = act ? weight[c + j] * (1.f / sqrtf(m2[j] / (float)N + eps)) : 0.f;
        shift[j] = act ? bias[c + j] : 0.f;
    }
}

// ---- BatchNorm, training, column-owner: one launch -------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void k_bn_fwd_cols(const float* __restrict__ x, const float* __restrict__ weight,
                                                        const float* __restrict__ bias, float* running_mean, float* running_var, int64_t N,
                                                        int C, int n_ctiles, float momentum, float eps, float* __restrict__ y,
                                                        float* __restrict__ save_mean, float* __restrict__ save_rstd) {
    __shared__ float s_part[256 * 2 * V];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int ct = blockIdx.x; ct < n_ctiles; ct += gridDim.x) {
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        float mean[V], m2[V], scale[V], shift[V];
        tile_mean_m2<V>(x, 0, N, C, c, act, s_part, mean, m2);
        if (act && rg == 0) bn_write_stats<V>(c, N, mean, m2, momentum, eps, running_mean, running_var, save_mean, save_rstd);
        bn_scale_shift<V>(weight, bias, c, act, N, m2, eps, scale, shift);
        if (act) tile_affine<V>(x, y, 0, N, C, c, mean, scale, shift);
    }
}

// ---- BatchNorm, training, row-split: launch 1 (slab partials), launch 2 (combine + normalise) ------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void k_bn_fwd_partial(const float* __restrict__ x, int64_t N, int C, int n_slabs, int n_ctiles,
                                                           float* __restrict__ ws) {
    __shared__ float s_part[256 * 2 * V];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int wi = blockIdx.x; wi < n_slabs * n_ctiles; wi += gridDim.x) {
        const int slab = wi / n_ctiles, ct = wi - slab * n_ctiles;
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        const int64_t r0 = (int64_t)slab * kSlabRows, r1 = min(N, r0 + kSlabRows);
        float mean[V], m2[V];
        tile_mean_m2<V>(x, r0, r1, C, c, act, s_part, mean, m2);
        if (act && rg == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                ws[((size_t)slab * 2) * C + c + j] = mean[j];
                ws[((size_t)slab * 2 + 1) * C + c + j] = m2[j];
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_bn_fwd_apply(const float* __restrict__ x, const float* __restrict__ ws,
                                                         const float* __restrict__ weight, const float* __restrict__ bias,
                                                         float* running_mean, float* running_var, int64_t N, int C, int n_slabs, int n_ctiles,
                                                         float momentum, float eps, float* __restrict__ y, float* __restrict__ save_mean,
                                                         float* __restrict__ save_rstd) {
    __shared__ float s_part[256 * 2 * V];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int wi = blockIdx.x; wi < n_slabs * n_ctiles; wi += gridDim.x) {
        const int slab = wi / n_ctiles, ct = wi - slab * n_ctiles;
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        const int64_t r0 = (int64_t)slab * kSlabRows, r1 = min(N, r0 + kSlabRows);
        float mean[V], m2[V], scale[V], shift[V];
        combine_mean_m2<V>(ws, N, n_slabs, C, c, act, s_part, mean, m2);
        if (act && rg == 0 && slab == 0) bn_write_stats<V>(c, N, mean, m2, momentum, eps, running_mean, running_var, save_mean, save_rstd);
        bn_scale_shift<V>(weight, bias, c, act, N, m2, eps, scale, shift);
        if (act) tile_affine<V>(x, y, r0, r1, C, c, mean, scale, shift);
    }
}

// ---- BatchNorm, eval: one elementwise launch on the running statistics ------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void k_bn_eval_fwd(const float* __restrict__ x, const float* __restrict__ weight,
                                                        const float* __restrict__ bias, const float* __restrict__ running_mean,
                                                        const float* __restrict__ running_var, int64_t N, int C, int n_slabs, int n_ctiles,
                                                        float eps, float* __restrict__ y, float* __restrict__ save_mean,
                                                        float* __restrict__ save_rstd) {
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int wi = blockIdx.x; wi < n_slabs * n_ctiles; wi += gridDim.x) {
        const int slab = wi / n_ctiles, ct = wi - slab * n_ctiles;
        const int c = (ct * 16 + cl) * V;
        if (c >= C) continue;
        const int64_t r0 = (int64_t)slab * kSlabRows, r1 = min(N, r0 + kSlabRows);
        float mean[V], scale[V], shift[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float rstd = 1.f / sqrtf(running_var[c + j] + eps);
            mean[j] = running_mean[c + j];
            scale[j] = weight[c + j] * rstd;
            shift[j] = bias[c + j];
            if (slab == 0 && rg == 0) { save_mean[c + j] = mean[j]; save_rstd[c + j] = rstd; }
        }
        tile_affine<V>(x, y, r0, r1, C, c, mean, scale, shift);
    }
}

// ---- backward: column sums of dy and dy * xhat --------------------------------------------------------------------------------
// a[j] = sum dy, a[V + j] = sum dy * (x - mean) * rstd over rows [r0, r1) (LayerNorm: mean the one scalar, rstd = 1)
template <int V>
__device__ __forceinline__ void tile_dy_sums(const float* x, const float* dy, int64_t r0, int64_t r1, int C, int c, bool act,
                                             const float (&mean)[V], const float (&rstd)[V], float* s_part, float (&a)[2 * V]) {
    const int rg = threadIdx.x >> 4;
    float v[V], g[V];
#pragma unroll
    for (int j = 0; j < 2 * V; ++j) a[j] = 0.f;
    if (act) {
#pragma unroll 4
        for (int64_t r = r0 + rg; r < r1; r += 16) {
            ldv<V>(x + r * C + c, v);
            ldv<V>(dy + r * C + c, g);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                a[j] += g[j];
                a[V + j] += g[j] * ((v[j] - mean[j]) * rstd[j]);
            }
        }
    }
    colreduce<2 * V>(a, s_part);
}

// the same two sums from the slab partials ws: [n_slabs][2][C]
template <int V>
__device__ __forceinline__ void combine_dy_sums(const float* ws, int n_slabs, int C, int c, bool act, float* s_part, float (&a)[2 * V]) {
    const int rg = threadIdx.x >> 4;
#pragma unroll
    for (int j = 0; j < 2 * V; ++j) a[j] = 0.f;
    if (act)
        for (int s = rg; s < n_slabs; s += 16) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                a[j] += ws[((size_t)s * 2) * C + c + j];
                a[V + j] += ws[((size_t)s * 2 + 1) * C + c + j];
            }
        }
    colreduce<2 * V>(a, s_part);
}

template <int V>
__device__ __forceinline__ void load_cols(const float* p, int c, bool act, float fill, float (&v)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = act ? p[c + j] : fill;
}

// dx = w rstd (dy - mean(dy) - xhat mean(dy xhat))   (eval: the statistics are constants, dx = dy w rstd)
template <int V, bool EVAL>
__device__ __forceinline__ void tile_bn_dx(const float* x, const float* dy, float* dx, int64_t r0, int64_t r1, int64_t N, int C, int c,
                                           const float (&mean)[V], const float (&rstd)[V], const float (&w)[V], const float (&a)[2 * V]) {
    const int rg = threadIdx.x >> 4;
    float v[V], g[V], m_dy[V], m_dyx[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { m_dy[j] = a[j] / (float)N; m_dyx[j] = a[V + j] / (float)N; }
#pragma unroll 4
    for (int64_t r = r0 + rg; r < r1; r += 16) {
        ldv<V>(dy + r * C + c, g);
        if constexpr (EVAL) {
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] = g[j] * (w[j] * rstd[j]);
        } else {
            ldv<V>(x + r * C + c, v);
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] = (w[j] * rstd[j]) * ((g[j] - m_dy[j]) - ((v[j] - mean[j]) * rstd[j]) * m_dyx[j]);
        }
        stv<V>(dx + r * C + c, g);
    }
}

template <int V, bool EVAL>
__global__ __launch_bounds__(kBlock) void k_bn_bwd_cols(const float* __restrict__ x, const float* __restrict__ dy,
                                                        const float* __restrict__ weight, const float* __restrict__ mean_p,
                                                        const float* __restrict__ rstd_p, int64_t N, int C, int n_ctiles,
                                                        float* __restrict__ dx, float* __restrict__ d_weight, float* __restrict__ d_bias) {
    __shared__ float s_part[256 * 2 * V];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int ct = blockIdx.x; ct < n_ctiles; ct += gridDim.x) {
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        float mean[V], rstd[V], w[V], a[2 * V];
        load_cols<V>(mean_p, c, act, 0.f, mean);
        load_cols<V>(rstd_p, c, act, 0.f, rstd);
        load_cols<V>(weight, c, act, 0.f, w);
        tile_dy_sums<V>(x, dy, 0, N, C, c, act, mean, rstd, s_part, a);
        if (!act) continue;
        if (rg == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) { d_bias[c + j] = a[j]; d_weight[c + j] = a[V + j]; }
        }
        tile_bn_dx<V, EVAL>(x, dy, dx, 0, N, N, C, c, mean, rstd, w, a);
    }
}

// launch 1 of the row-split backward (BatchNorm: per-column mean / rstd; LayerNorm: stat = {mean, std} of the whole tensor)
template <int V, bool PER_COL>
__global__ __launch_bounds__(kBlock) void k_dy_partial(const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ mean_p, const float* __restrict__ rstd_p, int64_t N, int C,
                                                       int n_slabs, int n_ctiles, float* __restrict__ ws) {
    __shared__ float s_part[256 * 2 * V];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int wi = blockIdx.x; wi < n_slabs * n_ctiles; wi += gridDim.x) {
        const int slab = wi / n_ctiles, ct = wi - slab * n_ctiles;
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        const int64_t r0 = (int64_t)slab * kSlabRows, r1 = min(N, r0 + kSlabRows);
        float mean[V], rstd[V], a[2 * V];
        if constexpr (PER_COL) {
            load_cols<V>(mean_p, c, act, 0.f, mean);
            load_cols<V>(rstd_p, c, act, 0.f, rstd);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) { mean[j] = mean_p[0]; rstd[j] = 1.f; }
        }
        tile_dy_sums<V>(x, dy, r0, r1, C, c, act, mean, rstd, s_part, a);
        if (act && rg == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                ws[((size_t)slab * 2) * C + c + j] = a[j];
                ws[((size_t)slab * 2 + 1) * C + c + j] = a[V + j];
            }
        }
    }
}

template <int V, bool EVAL>
__global__ __launch_bounds__(kBlock) void k_bn_bwd_apply(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ ws, const float* __restrict__ weight,
                                                         const float* __restrict__ mean_p, const float* __restrict__ rstd_p, int64_t N, int C,
                                                         int n_slabs, int n_ctiles, float* __restrict__ dx, float* __restrict__ d_weight,
                                                         float* __restrict__ d_bias) {
    __shared__ float s_part[256 * 2 * V];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int wi = blockIdx.x; wi < n_slabs * n_ctiles; wi += gridDim.x) {
        const int slab = wi / n_ctiles, ct = wi - slab * n_ctiles;
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        const int64_t r0 = (int64_t)slab * kSlabRows, r1 = min(N, r0 + kSlabRows);
        float mean[V], rstd[V], w[V], a[2 * V];
        load_cols<V>(mean_p, c, act, 0.f, mean);
        load_cols<V>(rstd_p, c, act, 0.f, rstd);
        load_cols<V>(weight, c, act, 0.f, w);
        combine_dy_sums<V>(ws, n_slabs, C, c, act, s_part, a);
        if (!act) continue;
        if (rg == 0 && slab == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) { d_bias[c + j] = a[j]; d_weight[c + j] = a[V + j]; }
        }
        tile_bn_dx<V, EVAL>(x, dy, dx, r0, r1, N, C, c, mean, rstd, w, a);
    }
}

// ---- batch-less LayerNorm: one mean and one standard deviation over the L = N C elements ----------------------------------
// mean and M2 of the flat elements [i0, i1) (V = 4: i0 and i1 are multiples of 4)
template <int V>
__device__ __forceinline__ void flat_mean_m2(const float* x, int64_t i0, int64_t i1, float* s_red, float& mean, float& m2) {
    const float n = (float)(i1 - i0);
    float v[V], a = 0.f;
#pragma unroll 4
    for (int64_t i = i0 + (int64_t)threadIdx.x * V; i < i1; i += kBlock * V) {
        ldv<V>(x + i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) a += v[j];
    }
    mean = block_sum(a, s_red) / n;
    float q0 = 0.f, q1 = 0.f;
#pragma unroll 4
    for (int64_t i = i0 + (int64_t)threadIdx.x * V; i < i1; i += kBlock * V) {
        ldv<V>(x + i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = v[j] - mean;
            q0 += d;
            q1 += d * d;
        }
    }
    q0 = block_sum(q0, s_red);
    q1 = block_sum(q1, s_red);
    mean += q0 / n;
    m2 = fmaxf(q1 - q0 * q0 / n, 0.f);
}

// the chunk partials ws: [n_chunks][2] = mean | M2 -> mean and M2 of all L elements
__device__ __forceinline__ void flat_combine(const float* ws, int64_t L, int n_chunks, float* s_red, float& mean, float& m2) {
    float a = 0.f;
    for (int k = threadIdx.x; k < n_chunks; k += kBlock) a += (float)(min((int64_t)kLnChunk, L - (int64_t)k * kLnChunk)) * ws[2 * k];
    mean = block_sum(a, s_red) / (float)L;
    float q0 = 0.f, q1 = 0.f;
    for (int k = threadIdx.x; k < n_chunks; k += kBlock) {
        const float nk = (float)(min((int64_t)kLnChunk, L - (int64_t)k * kLnChunk)), d = ws[2 * k] - mean;
        q0 += nk * d;
        q1 += ws[2 * k + 1] + nk * d * d;
    }
    q0 = block_sum(q0, s_red);
    q1 = block_sum(q1, s_red);
    mean += q0 / (float)L;
    m2 = fmaxf(q1 - q0 * q0 / (float)L, 0.f);
}

// y = (x - m) * inv * weight[col] + bias[col] over the flat elements [i0, i1)
template <int V>
__device__ __forceinline__ void flat_ln_apply(const float* x, float* y, int64_t i0, int64_t i1, int C, float m, float inv,
                                              const float* weight, const float* bias) {
    int64_t i = i0 + (int64_t)threadIdx.x * V;
    int col = (int)(i % C);
    const int cstep = (kBlock * V) % C;
    float v[V];
    for (; i < i1; i += kBlock * V) {
        ldv<V>(x + i, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = ((v[j] - m) * inv) * weight[col + j] + bias[col + j];     // (V = 4: C % 4 == 0, one row)
        stv<V>(y + i, v);
        col += cstep;
        if (col >= C) col -= C;
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_ln_fwd_one(const float* __restrict__ x, const float* __restrict__ weight,
                                                       const float* __restrict__ bias, int64_t L, int C, float eps, float* __restrict__ y,
                                                       float* __restrict__ stat) {
    __shared__ float s_red[4];
    float m, m2;
    flat_mean_m2<V>(x, 0, L, s_red, m, m2);
    const float s = sqrtf(m2 / (float)L);
    if (threadIdx.x == 0) { stat[0] = m; stat[1] = s; }
    flat_ln_apply<V>(x, y, 0, L, C, m, 1.f / (s + eps), weight, bias);
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_ln_fwd_partial(const float* __restrict__ x, int64_t L, int n_chunks, float* __restrict__ ws) {
    __shared__ float s_red[4];
    for (int k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t i0 = (int64_t)k * kLnChunk, i1 = min(L, i0 + kLnChunk);
        float m, m2;
        flat_mean_m2<V>(x, i0, i1, s_red, m, m2);
        if (threadIdx.x == 0) { ws[2 * k] = m; ws[2 * k + 1] = m2; }
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_ln_fwd_apply(const float* __restrict__ x, const float* __restrict__ ws,
                                                         const float* __restrict__ weight, const float* __restrict__ bias, int64_t L, int C,
                                                         int n_chunks, float eps, float* __restrict__ y, float* __restrict__ stat) {
    __shared__ float s_red[4];
    float m, m2;
    flat_combine(ws, L, n_chunks, s_red, m, m2);
    const float s = sqrtf(m2 / (float)L);
    if (blockIdx.x == 0 && threadIdx.x == 0) { stat[0] = m; stat[1] = s; }
    for (int k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t i0 = (int64_t)k * kLnChunk;
        flat_ln_apply<V>(x, y, i0, min(L, i0 + kLnChunk), C, m, 1.f / (s + eps), weight, bias);
    }
}

// Backward.  With g = dy weight: dx = (g - mean(g)) / (s + eps) - (x - m) mean(g (x - m)) / (s (s + eps)^2); both means follow from
// the column sums A_c = sum_rows dy, B_c = sum_rows dy (x - m): mean(g) = sum_c w_c A_c / L, mean(g (x - m)) = sum_c w_c B_c / L;
// d_bias = A, d_weight = B / (s + eps).  ws: [n_slabs][2][C].  The block that `writes` stores d_weight and d_bias.
template <int V>
__device__ __forceinline__ void ln_bwd_apply(const float* x, const float* dy, const float* ws, const float* weight, const float* stat,
                                             int64_t L, int C, int n_slabs, float eps, int64_t i0, int64_t i1, int64_t istep, bool writes,
                                             float* dx, float* d_weight, float* d_bias, float* s_red) {
    const float m = stat[0], s = stat[1], inv = 1.f / (s + eps);
    float ga = 0.f, gb = 0.f;
    for (int c = threadIdx.x; c < C; c += kBlock) {
        float A = 0.f, B = 0.f;
        for (int sl = 0; sl < n_slabs; ++sl) {
            A += ws[((size_t)sl * 2) * C + c];
            B += ws[((size_t)sl * 2 + 1) * C + c];
        }
        ga += weight[c] * A;
        gb += weight[c] * B;
        if (writes) { d_bias[c] = A; d_weight[c] = B * inv; }
    }
    const float mg = block_sum(ga, s_red) / (float)L;
    const float k2 = (block_sum(gb, s_red) / (float)L) * inv * inv / s;
    const int cstep = (kBlock * V) % C;
    float v[V], g[V];
    for (; i0 < i1; i0 += istep) {          // the block's chunks
        const int64_t e = min(i1, i0 + kLnChunk);
        int64_t i = i0 + (int64_t)threadIdx.x * V;
        int col = (int)(i % C);
        for (; i < e; i += kBlock * V) {
            ldv<V>(x + i, v);
            ldv<V>(dy + i, g);
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] = (g[j] * weight[col + j] - mg) * inv - (v[j] - m) * k2;
            stv<V>(dx + i, g);
            col += cstep;
            if (col >= C) col -= C;
        }
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_ln_bwd_apply(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ ws, const float* __restrict__ weight,
                                                         const float* __restrict__ stat, int64_t L, int C, int n_slabs, float eps,
                                                         float* __restrict__ dx, float* __restrict__ d_weight, float* __restrict__ d_bias) {
    __shared__ float s_red[4];
    ln_bwd_apply<V>(x, dy, ws, weight, stat, L, C, n_slabs, eps, (int64_t)blockIdx.x * kLnChunk, L, (int64_t)gridDim.x * kLnChunk,
                    blockIdx.x == 0, dx, d_weight, d_bias, s_red);
}

// one block: the column sums of all rows into ws (one slab), then the same apply
template <int V>
__global__ __launch_bounds__(kBlock) void k_ln_bwd_one(const float* __restrict__ x, const float* __restrict__ dy, float* ws,
                                                       const float* __restrict__ weight, const float* __restrict__ stat, int64_t N, int C,
                                                       int n_ctiles, float eps, float* __restrict__ dx, float* __restrict__ d_weight,
                                                       float* __restrict__ d_bias) {
    __shared__ float s_part[256 * 2 * V];
    __shared__ float s_red[4];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int ct = 0; ct < n_ctiles; ++ct) {
        const int c = (ct * 16 + cl) * V;
        const bool act = c < C;
        float mean[V], rstd[V], a[2 * V];
#pragma unroll
        for (int j = 0; j < V; ++j) { mean[j] = stat[0]; rstd[j] = 1.f; }
        tile_dy_sums<V>(x, dy, 0, N, C, c, act, mean, rstd, s_part, a);
        if (act && rg == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) { ws[c + j] = a[j]; ws[C + c + j] = a[V + j]; }
        }
    }
    __syncthreads();        // the block reads back its own partials
    ln_bwd_apply<V>(x, dy, ws, weight, stat, N * C, C, 1, eps, 0, N * C, kLnChunk, true, dx, d_weight, d_bias, s_red);
}

}  // namespace glam

using namespace glam;

namespace {

struct Geom {
    int V, n_ctiles, n_slabs, n_chunks;
    int64_t L;
};

int cap_of(int max_blocks) { return max_blocks > 0 && max_blocks < kNormBlocks ? max_blocks : kNormBlocks; }

// dims shared by every entry point; `ptrs`: the [N, C] tensors whose alignment decides the 16-byte path
int colnorm_geom(const char* fn, int64_t N, int C, int form, std::initializer_list<const void*> ptrs, Geom* g) {
    if (N < 1 || C < 1) return fail(GLAM_E_INVALID, "%s: N=%lld, C=%d", fn, (long long)N, C);
    if (N * (int64_t)C >= INT32_MAX || (N + kSlabRows - 1) / kSlabRows * (int64_t)((C + 15) / 16) >= INT32_MAX)
        return fail(GLAM_E_UNSUPPORTED, "%s: N * C = %lld elements (limit 2^31 - 1)", fn, (long long)(N * (int64_t)C));
    if (form < 0 || form > 2) return fail(GLAM_E_INVALID, "%s: form=%d (0 auto, 1 one launch, 2 partials + apply)", fn, form);
    bool v4 = (C & 3) == 0;
    for (const void* p : ptrs) {
        if (!p) return fail(GLAM_E_INVALID, "%s: null pointer", fn);
        v4 = v4 && aligned16(p);
    }
    g->V = v4 ? 4 : 1;
    g->n_ctiles = (C + 16 * g->V - 1) / (16 * g->V);
    g->n_slabs = (int)((N + kSlabRows - 1) / kSlabRows);
    g->L = N * (int64_t)C;
    g->n_chunks = (int)((g->L + kLnChunk - 1) / kLnChunk);
    return GLAM_OK;
}

size_t slab_ws_bytes(int64_t N, int C) { return (size_t)((N + kSlabRows - 1) / kSlabRows) * 2 * (size_t)C * sizeof(float); }

}  // namespace

extern "C" size_t glam_colnorm_workspace_bytes(int64_t N, int C) {
    if (N < 1 || C < 1) return 0;
    const size_t chunks = (size_t)((N * (int64_t)C + kLnChunk - 1) / kLnChunk) * 2 * sizeof(float), slabs = slab_ws_bytes(N, C);
    return slabs > chunks ? slabs : chunks;
}

#define COLNORM_LAUNCH(V_, kernel, grid, ...)                                                                  \
    do {                                                                                                        \
        if ((V_) == 4) hipLaunchKernelGGL((kernel<4>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<1>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__);   \
    } while (0)
#define COLNORM_LAUNCH2(V_, B_, kernel, grid, ...)                                                              \
    do {                                                                                                        \
        if ((V_) == 4 && (B_)) hipLaunchKernelGGL((kernel<4, true>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__);        \
        else if ((V_) == 4) hipLaunchKernelGGL((kernel<4, false>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__);          \
        else if (B_) hipLaunchKernelGGL((kernel<1, true>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__);                  \
        else hipLaunchKernelGGL((kernel<1, false>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__);                         \
    } while (0)

extern "C" int glam_batch_norm_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var, int64_t N,
                                   int C, float momentum, float eps, float* y, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes,
                                   int form, int max_blocks, void* stream) {
    Geom g;
    if (int rc = colnorm_geom("glam_batch_norm_fwd", N, C, form, {x, y}, &g)) return rc;
    GLAM_REQUIRE(weight && bias && running_mean && running_var && save_mean && save_rstd, "glam_batch_norm_fwd: null pointer");
    GLAM_REQUIRE(N >= 2, "glam_batch_norm_fwd: batch statistics need more than one row (N=%lld)", (long long)N);
    if (form == 1 || (form == 0 && N <= kColOwnerMaxRows)) {
        COLNORM_LAUNCH(g.V, k_bn_fwd_cols, grid_for(g.n_ctiles, 1, cap_of(max_blocks)), x, weight, bias, running_mean, running_var, N, C, g.n_ctiles,
                       momentum, eps, y, save_mean, save_rstd);
        GLAM_LAUNCH_CHECK("glam_batch_norm_fwd");
        return GLAM_OK;
    }
    GLAM_REQUIRE(ws && ws_bytes >= slab_ws_bytes(N, C), "glam_batch_norm_fwd: workspace of %zu bytes, %zu needed", ws_bytes, slab_ws_bytes(N, C));
    const int grid = grid_for((int64_t)g.n_slabs * g.n_ctiles, 1, cap_of(max_blocks));
    COLNORM_LAUNCH(g.V, k_bn_fwd_partial, grid, x, N, C, g.n_slabs, g.n_ctiles, (float*)ws);
    GLAM_LAUNCH_CHECK("glam_batch_norm_fwd");
    COLNORM_LAUNCH(g.V, k_bn_fwd_apply, grid, x, (const float*)ws, weight, bias, running_mean, running_var, N, C, g.n_slabs, g.n_ctiles, momentum, eps,
                   y, save_mean, save_rstd);
    GLAM_LAUNCH_CHECK("glam_batch_norm_fwd");
    return GLAM_OK;
}

extern "C" int glam_batch_norm_eval_fwd(const float* x, const float* weight, const float* bias, const float* running_mean,
                                        const float* running_var, int64_t N, int C, float eps, float* y, float* save_mean, float* save_rstd,
                                        int max_blocks, void* stream) {
    Geom g;
    if (int rc = colnorm_geom("glam_batch_norm_eval_fwd", N, C, 0, {x, y}, &g)) return rc;
    GLAM_REQUIRE(weight && bias && running_mean && running_var && save_mean && save_rstd, "glam_batch_norm_eval_fwd: null pointer");
    COLNORM_LAUNCH(g.V, k_bn_eval_fwd, grid_for((int64_t)g.n_slabs * g.n_ctiles, 1, cap_of(max_blocks)), x, weight, bias, running_mean, running_var, N,
                   C, g.n_slabs, g.n_ctiles, eps, y, save_mean, save_rstd);
    GLAM_LAUNCH_CHECK("glam_batch_norm_eval_fwd");
    return GLAM_OK;
}

extern "C" int glam_batch_norm_bwd(const float* x, const float* dy, const float* weight, const float* mean, const float* rstd, int64_t N, int C,
                                   int eval, float* dx, float* d_weight, float* d_bias, void* ws, size_t ws_bytes, int form, int max_blocks,
                                   void* stream) {
    Geom g;
    if (int rc = colnorm_geom("glam_batch_norm_bwd", N, C, form, {x, dy, dx}, &g)) return rc;
    GLAM_REQUIRE(weight && mean && rstd && d_weight && d_bias, "glam_batch_norm_bwd: null pointer");
    if (form == 1 || (form == 0 && N <= kColOwnerMaxRows)) {
        COLNORM_LAUNCH2(g.V, eval != 0, k_bn_bwd_cols, grid_for(g.n_ctiles, 1, cap_of(max_blocks)), x, dy, weight, mean, rstd, N, C, g.n_ctiles, dx,
                        d_weight, d_bias);
        GLAM_LAUNCH_CHECK("glam_batch_norm_bwd");
        return GLAM_OK;
    }
    GLAM_REQUIRE(ws && ws_bytes >= slab_ws_bytes(N, C), "glam_batch_norm_bwd: workspace of %zu bytes, %zu needed", ws_bytes, slab_ws_bytes(N, C));
    const int grid = grid_for((int64_t)g.n_slabs * g.n_ctiles, 1, cap_of(max_blocks));
    COLNORM_LAUNCH2(g.V, true, k_dy_partial, grid, x, dy, mean, rstd, N, C, g.n_slabs, g.n_ctiles, (float*)ws);
    GLAM_LAUNCH_CHECK("glam_batch_norm_bwd");
    COLNORM_LAUNCH2(g.V, eval != 0, k_bn_bwd_apply, grid, x, dy, (const float*)ws, weight, mean, rstd, N, C, g.n_slabs, g.n_ctiles, dx, d_weight,
                    d_bias);
    GLAM_LAUNCH_CHECK("glam_batch_norm_bwd");
    return GLAM_OK;
}

extern "C" int glam_layer_norm_flat_fwd(const float* x, const float* weight, const float* bias, int64_t N, int C, float eps, float* y,
                                        float* stat, void* ws, size_t ws_bytes, int form, int max_blocks, void* stream) {
    Geom g;
    if (int rc = colnorm_geom("glam_layer_norm_flat_fwd", N, C, form, {x, y}, &g)) return rc;
    GLAM_REQUIRE(weight && bias && stat, "glam_layer_norm_flat_fwd: null pointer");
    if (form == 1 || (form == 0 && g.L <= kLnOneBlock)) {
        COLNORM_LAUNCH(g.V, k_ln_fwd_one, 1, x, weight, bias, g.L, C, eps, y, stat);
        GLAM_LAUNCH_CHECK("glam_layer_norm_flat_fwd");
        return GLAM_OK;
    }
    const size_t need = (size_t)g.n_chunks * 2 * sizeof(float);
    GLAM_REQUIRE(ws && ws_bytes >= need, "glam_layer_norm_flat_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int grid = grid_for(g.n_chunks, 1, cap_of(max_blocks));
    COLNORM_LAUNCH(g.V, k_ln_fwd_partial, grid, x, g.L, g.n_chunks, (float*)ws);
    GLAM_LAUNCH_CHECK("glam_layer_norm_flat_fwd");
    COLNORM_LAUNCH(g.V, k_ln_fwd_apply, grid, x, (const float*)ws, weight, bias, g.L, C, g.n_chunks, eps, y, stat);
    GLAM_LAUNCH_CHECK("glam_layer_norm_flat_fwd");
    return GLAM_OK;
}

extern "C" int glam_layer_norm_flat_bwd(const float* x, const float* dy, const float* weight, const float* stat, int64_t N, int C, float eps,
                                        float* dx, float* d_weight, float* d_bias, void* ws, size_t ws_bytes, int form, int max_blocks,
                                        void* stream) {
    Geom g;
    if (int rc = colnorm_geom("glam_layer_norm_flat_bwd", N, C, form, {x, dy, dx}, &g)) return rc;
    GLAM_REQUIRE(weight && stat && d_weight && d_bias, "glam_layer_norm_flat_bwd: null pointer");
    const bool one = form == 1 || (form == 0 && g.L <= kLnOneBlock);
    const size_t need = one ? (size_t)2 * C * sizeof(float) : slab_ws_bytes(N, C);
    GLAM_REQUIRE(ws && ws_bytes >= need, "glam_layer_norm_flat_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (one) {
        COLNORM_LAUNCH(g.V, k_ln_bwd_one, 1, x, dy, (float*)ws, weight, stat, N, C, g.n_ctiles, eps, dx, d_weight, d_bias);
        GLAM_LAUNCH_CHECK("glam_layer_norm_flat_bwd");
        return GLAM_OK;
    }
    COLNORM_LAUNCH2(g.V, false, k_dy_partial, grid_for((int64_t)g.n_slabs * g.n_ctiles, 1, cap_of(max_blocks)), x, dy, stat, stat, N, C, g.n_slabs,
                    g.n_ctiles, (float*)ws);
    GLAM_LAUNCH_CHECK("glam_layer_norm_flat_bwd");
    COLNORM_LAUNCH(g.V, k_ln_bwd_apply, grid_for(g.n_chunks, 1, cap_of(max_blocks)), x, dy, (const float*)ws, weight, stat, g.L, C, g.n_slabs, eps, dx,
                   d_weight, d_bias);
    GLAM_LAUNCH_CHECK("glam_layer_norm_flat_bwd");
    return GLAM_OK;
}
