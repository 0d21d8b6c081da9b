// The loss of the training step that drives the path, forward and gradient in one launch:
//   regression      `loss = self.criterion(output, y_true)` with nn.MSELoss            (reference src_1gp/trainer.py:296, loss.py:42)
//   classification  `self.criterion(y_score[y_true >= 0], y_true[y_true >= 0].float())` with nn.BCEWithLogitsLoss
//                   (trainer.py:244-245, loss.py:48): the mean over the labels that are present (-1 = missing, dataset.py:138)
// Through torch these are 7-10 launches of a few hundred to a few hundred thousand elements each (forward map, reduction, the
// autograd root's fill, backward maps; the masked form also needs boolean indexing, which a hipGraph cannot capture) — 25-50 us of a
// 330-830 us step.  Here: one launch writes the loss, 1 / count and the un-normalised gradient; the backward is one scale launch.
//   kind 0  l = (x - y)^2                              dl/dx = 2 (x - y)
//   kind 1  l = max(x, 0) - x y + log1p(exp(-|x|))     dl/dx = sigmoid(x) - y
//   kind 2  l = |x - y|                                dl/dx = sign(x - y), sign(0) = 0                    nn.L1Loss ('mae')
//   kind 3  l = 0.5 d^2 if |d| < 1 else |d| - 0.5      dl/dx = clamp(d, -1, 1), d = x - y                  nn.SmoothL1Loss ('huber', 'smae')
//   kind 4  l = -(y max(log x, -100) + (1 - y) max(log(1 - x), -100))
//                                                      dl/dx = (x - y) / max(x (1 - x), 1e-12)             nn.BCELoss ('bce')
//   masked  only elements with y >= 0 count (others contribute neither loss nor gradient)
// The cross-entropy family (k_ce_fwd, below) writes the same three things for logits [B, C] and int64 class labels.
// Sums run in a fixed order (thread-sequential, then a block tree, then the block partials in index order by the last block to finish):
// bit-reproducible run to run.  count = 0 gives nan, as the mean over an empty selection does in the reference.
#include "common.h"

namespace glam {

constexpr int kLossMaxBlocks = 512;
constexpr int kCeMaxClasses = 1024;

__device__ __forceinline__ void loss_elem(float x, float y, int kind, bool ok, float& l, float& g) {
    if (!ok) { l = 0.f; g = 0.f; return; }
    if (kind == 0) {
        const float d = x - y;
        l = d * d; g = 2.f * d;
    } else if (kind == 1) {
        const float e = expf(-fabsf(x));
        l = fmaxf(x, 0.f) - x * y + log1pf(e);
        const float s = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        g = s - y;
    } else if (kind == 2) {
        const float d = x - y;
        l = fabsf(d); g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else if (kind == 3) {                                       // beta = 1 (torch's default)
        const float d = x - y, a = fabsf(d);
        l = a < 1.f ? 0.5f * d * d : a - 0.5f;
        g = fminf(fmaxf(d, -1.f), 1.f);
    } else {                                                      // torch's binary_cross_entropy and its backward
        l = (y - 1.f) * fmaxf(log1pf(-x), -100.f) - y * fmaxf(logf(x), -100.f);
        g = (x - y) / fmaxf((1.f - x) * x, 1e-12f);
    }
}

// block sum of (a, b) in a fixed order: wave butterfly, then wave 0 adds the waves' results in wave order
__device__ __forceinline__ void block_sum2(float& a, float& b, float* s_a, float* s_b) {
    a = group_sum<64>(a); b = group_sum<64>(b);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { s_a[wave] = a; s_b[wave] = b; }
    __syncthreads();
    float ra = 0.f, rb = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) { ra += s_a[w]; rb += s_b[w]; }
    a = ra; b = rb;
}

// The mean of the launch: (sum, cnt) of this block -> block tree -> (nb > 1) the block partials in index order, added by the last
// block to check in.  Writes loss = sum / cnt and inv_count = 1 / cnt (zero_empty: 0 when cnt = 0, the zero gradient torch's
// nll_loss gives when every label is ignored).
__device__ __forceinline__ void finish_mean(float sum, float cnt, bool zero_empty, float* loss, float* inv_count, float* partial,
                                            unsigned* ticket, float* s_a, float* s_b, int* s_last) {
    const int tid = threadIdx.x, nb = gridDim.x;
    block_sum2(sum, cnt, s_a, s_b);
    if (nb == 1) {
        if (tid == 0) { loss[0] = sum / cnt; inv_count[0] = zero_empty && cnt == 0.f ? 0.f : 1.f / cnt; }
        return;
    }
    if (tid == 0) {
        __hip_atomic_store(partial + 2 * blockIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(partial + 2 * blockIdx.x + 1, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // two-level ticket (rng.h): the partials above are ordered before the check-in by the release of the fetch_add
        const unsigned g = gridDim.x, sidx = blockIdx.x & 15u;
        const unsigned in_sub = (g - sidx + 15u) >> 4, nsub = g < 16u ? g : 16u;
        unsigned* sub = ticket + 32 * (1 + sidx);
        int last = 0;
        if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == in_sub - 1) {
            __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nsub - 1) {
                __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
            }
        }
        *s_last = last;
    }
    __syncthreads();
    if (!*s_last) return;
    // the last block: the block partials in index order (one wave, lane-strided, then the butterfly)
    if (tid < 64) {
        float a = 0.f, b = 0.f;
        for (int q = tid; q < nb; q += 64) {
            a += __hip_atomic_load(partial + 2 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b += __hip_atomic_load(partial + 2 * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        a = group_sum<64>(a); b = group_sum<64>(b);
        if (tid == 0) { loss[0] = a / b; inv_count[0] = zero_empty && b == 0.f ? 0.f : 1.f / b; }
    }
}

__global__ void __launch_bounds__(kBlock) k_loss_fwd(const float* pred, const float* target, int n, int kind, int masked, float* loss,
                                                    float* inv_count, float* grad, float* partial, unsigned* ticket) {
    __shared__ float s_a[kBlock / 64], s_b[kBlock / 64];
    __shared__ int s_last;
    const int tid = threadIdx.x, nb = gridDim.x;
    float sum = 0.f, cnt = 0.f;
    for (int i = blockIdx.x * kBlock + tid; i < n; i += nb * kBlock) {
        const float x = pred[i], y = target[i];
        const bool ok = !masked || y >= 0.f;
        float l, g;
        loss_elem(x, y, kind, ok, l, g);
        grad[i] = g;
        sum += l; cnt += ok ? 1.f : 0.f;
    }
    finish_mean(sum, cnt, false, loss, inv_count, partial, ticket, s_a, s_b, &s_last);
}

// The cross-entropy family over logits x[B, C] and int64 class labels y[B] (as a batch's y arrives: no cast launch).  G lanes share a
// row: one lane per row for C <= 8 (a DTI head's C = 2 uses every lane), 16 lanes for C <= 128, a wave for C <= 1024; lane j of a
// group owns the classes j, j + G, ...  Per row: the max, the exp-sum in that fixed order (thread-sequential, then the group
// butterfly), ce = (m - x[y]) + log(sum), the row's loss / denominator share / gradient factor f, and grad = f (softmax - onehot(y)).
//   ce     l = w[y] ce, denominator w[y] (w = 1 without a weight), f = w[y]                        nn.CrossEntropyLoss(weight)
//   focal  l = alpha (1 - pt)^gamma ce, pt = exp(-ce), denominator 1 (every row, ignored ones included: the reference's .mean()
//          over reduction='none'), f = alpha [(1 - pt)^gamma + gamma (1 - pt)^(gamma - 1) pt ce]; gamma = 0: f = alpha, without
//          the second term (as torch's pow backward for a zero exponent: computing it is 0 * inf at pt = 1)
// A row with y == ignore_index adds 0 to the loss and has a zero gradient.  A label outside [0, C) that is not ignore_index is never
// used as an index: its row's loss and gradient are nan (torch raises a device-side assert there).
template <int G>
__device__ __forceinline__ float row_max(float v) {
    if constexpr (G >= 4) { v = fmaxf(v, dpp_move<0xB1>(v)); v = fmaxf(v, dpp_move<0x4E>(v)); }
    if constexpr (G >= 8) v = fmaxf(v, dpp_move<0x141>(v));
    if constexpr (G >= 16) v = fmaxf(v, dpp_move<0x140>(v));
    if constexpr (G == 64) { v = fmaxf(v, __shfl_xor(v, 16, 64)); v = fmaxf(v, __shfl_xor(v, 32, 64)); }
    return v;
}
template <int G>
__device__ __forceinline__ float row_sum(float v) {
    if constexpr (G == 1) return v;
    else return group_sum<G>(v);
}

template <int G>
__global__ void __launch_bounds__(kBlock) k_ce_fwd(const float* x, const int64_t* y, const float* weight, int B, int C,
                                                  int64_t ignore_index, int focal, float alpha, float gamma, float* loss,
                                                  float* inv_count, float* grad, float* partial, unsigned* ticket) {
    static_assert(G == 1 || G == 16 || G == 64, "k_ce_fwd: lanes per row");
    __shared__ float s_a[kBlock / 64], s_b[kBlock / 64];
    __shared__ int s_last;
    constexpr int kRows = kBlock / G;                              // rows of a block per pass
    const int tid = threadIdx.x, j = tid % G;
    float sum = 0.f, den = 0.f;
    // every lane of a group has the same r: a group is active or idle as a whole, so the DPP steps never read an idle lane
    for (int r = blockIdx.x * kRows + tid / G; r < B; r += gridDim.x * kRows) {
        const float* xr = x + (size_t)r * C;
        float* gr = grad + (size_t)r * C;
        float m = -INFINITY;
        for (int c = j; c < C; c += G) m = fmaxf(m, xr[c]);
        m = row_max<G>(m);
        float s = 0.f;
        for (int c = j; c < C; c += G) s += expf(xr[c] - m);
        s = row_sum<G>(s);
        const int64_t t = y[r];
        const bool ign = t == ignore_index, ok = !ign && t >= 0 && t < C;
        float l, d, f;                                             // row loss, denominator share, gradient factor
        if (ok) {
            const float ce = (m - xr[t]) + logf(s);
            if (!focal) {
                const float w = weight ? weight[t] : 1.f;
                l = w * ce; d = w; f = w;
            } else {
                const float pt = expf(-ce), omp = -expm1f(-ce);    // 1 - pt without the cancellation for small ce
                const float pg = gamma == 0.f ? 1.f : powf(omp, gamma);
                l = alpha * pg * ce; d = 1.f;
                f = gamma == 0.f ? alpha : alpha * (pg + gamma * powf(omp, gamma - 1.f) * pt * ce);
            }
        } else {
            l = ign ? 0.f : __builtin_nanf(""); d = focal ? 1.f : 0.f; f = l;
        }
        const float inv_s = 1.f / s;
        for (int c = j; c < C; c += G) {
            const float p = expf(xr[c] - m) * inv_s;
            gr[c] = ign ? 0.f : f * (c == t ? p - 1.f : p);
        }
        if (j == 0) { sum += l; den += d; }
    }
    finish_mean(sum, den, !focal, loss, inv_count, partial, ticket, s_a, s_b, &s_last);
}

// d_pred = grad * (g_up * inv_count): the gradient of the mean, scaled by whatever arrives at the loss (1 for loss.backward())
__global__ void __launch_bounds__(kBlock) k_loss_bwd(const float* grad, const float* inv_count, const float* g_up, int n, float* d_pred) {
    const float s = g_up[0] * inv_count[0];
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) d_pred[i] = grad[i] * s;
}

}  // namespace glam

using namespace glam;

extern "C" size_t glam_loss_workspace_bytes(void) { return (size_t)2 * kLossMaxBlocks * sizeof(float); }

extern "C" int glam_loss_fwd(const float* pred, const float* target, int64_t n, int kind, int masked, float* loss, float* inv_count,
                             float* grad, void* ws, size_t ws_bytes, unsigned* ticket, void* stream) {
    GLAM_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && kind >= 0 && kind <= 4, "glam_loss_fwd: bad size / kind");
    GLAM_REQUIRE(loss && inv_count && (n == 0 || (pred && target && grad)), "glam_loss_fwd: null pointer");
    int blocks = (int)((n + 4 * kBlock - 1) / (4 * kBlock));
    if (blocks < 1) blocks = 1;
    if (blocks > kLossMaxBlocks) blocks = kLossMaxBlocks;
    if (blocks > 1) GLAM_REQUIRE(ws && ws_bytes >= glam_loss_workspace_bytes() && ticket, "glam_loss_fwd: workspace / ticket missing");
    hipLaunchKernelGGL(k_loss_fwd, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, pred, target, (int)n, kind, masked, loss,
                       inv_count, grad, (float*)ws, ticket);
    GLAM_LAUNCH_CHECK("glam_loss_fwd");
    return GLAM_OK;
}

extern "C" int glam_loss_bwd(const float* grad, const float* inv_count, const float* g_up, int64_t n, float* d_pred, void* stream) {
    GLAM_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "glam_loss_bwd: bad size");
    if (n == 0) return GLAM_OK;
    GLAM_REQUIRE(grad && inv_count && g_up && d_pred, "glam_loss_bwd: null pointer");
    hipLaunchKernelGGL(k_loss_bwd, dim3(grid_for(n, kBlock, 1024)), dim3(kBlock), 0, (hipStream_t)stream, grad, inv_count, g_up, (int)n,
                       d_pred);
    GLAM_LAUNCH_CHECK("glam_loss_bwd");
    return GLAM_OK;
}

extern "C" int glam_ce_loss_max_classes(void) { return kCeMaxClasses; }

extern "C" int glam_ce_loss_fwd(const float* x, const int64_t* y, const float* weight, int64_t B, int C, int64_t ignore_index,
                                int focal, float alpha, float gamma, float* loss, float* inv_count, float* grad, void* ws,
                                size_t ws_bytes, unsigned* ticket, void* stream) {
    GLAM_REQUIRE(B >= 1 && C >= 1 && C <= kCeMaxClasses && B * C < ((int64_t)1 << 31), "glam_ce_loss_fwd: bad shape [%lld, %d]",
                 (long long)B, C);
    GLAM_REQUIRE(focal == 0 || focal == 1, "glam_ce_loss_fwd: bad mode %d", focal);
    GLAM_REQUIRE(!focal || ((gamma == 0.f || gamma >= 1.f) && !weight),
                 "glam_ce_loss_fwd: focal takes gamma = 0 or gamma >= 1 and no class weight");
    GLAM_REQUIRE(x && y && loss && inv_count && grad, "glam_ce_loss_fwd: null pointer");
    const int g = C <= 8 ? 1 : (C <= 128 ? 16 : 64);
    const int64_t rows_per_block = (int64_t)(kBlock / g) * (g == 1 ? 4 : 1);     // one lane per row: 4 rows per lane
    int blocks = (int)((B + rows_per_block - 1) / rows_per_block);
    if (blocks > kLossMaxBlocks) blocks = kLossMaxBlocks;
    if (blocks > 1) GLAM_REQUIRE(ws && ws_bytes >= glam_loss_workspace_bytes() && ticket, "glam_ce_loss_fwd: workspace / ticket missing");
    const int b = (int)B;
    if (g == 1)
        hipLaunchKernelGGL(k_ce_fwd<1>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, y, weight, b, C, ignore_index, focal,
                           alpha, gamma, loss, inv_count, grad, (float*)ws, ticket);
    else if (g == 16)
        hipLaunchKernelGGL(k_ce_fwd<16>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, y, weight, b, C, ignore_index, focal,
                           alpha, gamma, loss, inv_count, grad, (float*)ws, ticket);
    else
        hipLaunchKernelGGL(k_ce_fwd<64>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, y, weight, b, C, ignore_index, focal,
                           alpha, gamma, loss, inv_count, grad, (float*)ws, ticket);
    GLAM_LAUNCH_CHECK("glam_ce_loss_fwd");
    return GLAM_OK;
}
