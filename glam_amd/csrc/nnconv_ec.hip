// NNConv over continuous edge features (reference: src_2gi_dti_scr/glam.py's protein tower, `NNConv(C, C, Linear(De, 32) -> ReLU ->
// Linear(32, C*C), aggr)` on the 8 contact features of a residue graph) without the per-edge weight tensor nn(e_ij) [E, C*C].
//
// With h_e = relu(W0 e_e + b0) (32 values, h_e[32] = 1) and A_k[ci, co] = W1[ci*Cout + co, k] (A_32 = b1 as [Cin, Cout]):
//   out_i = sum_{k<=32} S_i[k] A_k + x_i root + bias,   S_i[k] = (1/d_i) sum_{e -> i} h_e[k] x_{s(e)}
// i.e. ONE product [S | x] @ Wstack + bias with [S | x] = f32[N, 34, Cin] (slot 33 = the node's own row) and
// Wstack = [A_0; ...; A_32; root] = f32[34 Cin, Cout].  [S | x] holds N*34*Cin floats instead of E*Cin*Cout.
//
// Forward:  k_ec_hidden (h, kept for the backward) -> k_ec_sums ([S | x]) -> k_ec_gemm (+ bias).
// Backward: k_ec_sums again (the forward keeps only h) -> k_ec_gemm split over N (d_Wstack and d_bias partials) -> k_ec_reduce;
//           k_ec_gemm d_S = G Wstack^T (into the same buffer) -> k_ec_dx (CSR transpose, root slot, addend) and
//           k_ec_dpre (d_h, relu mask, d_W0 / d_b0 per-block partials) -> k_ec_reduce.
// Every product is exact fp32 MFMA (v_mfma_f32_16x16x4_f32); every reduction is a fixed-order two-stage sum: no atomics, bit-stable.
#include "common.h"

#include <algorithm>
#include <utility>

namespace glam {

constexpr int kEcHidden = 32;          // the edge network's hidden width
constexpr int kEcSlots = kEcHidden + 2; // 32 hidden slots, the b1 slot (h = 1), the root slot (x itself)
constexpr int kEcMaxC = 96;
constexpr int kEcMaxDe = 16;
constexpr int kEcDpreBlocks = 512;     // blocks (= partial rows) of k_ec_dpre
constexpr int kEcSplitRows = 512;      // rows of N per split of the weight-gradient product

// ---- one strided exact-fp32 MFMA product: C[i, j] = sum_r X(i, r) Y(r, j) (+ bias[j]) ----------------------------------------
// X(i, r) = X[i*xi + r*xr] for i < xrows, 1 for xrows <= i < I (a row of ones: the column sums of Y ride along as row xrows);
// Y(r, j) = Y[r*yr + j*yj].  blockIdx.z takes rows [z*rchunk, (z+1)*rchunk) of the reduction and writes C + z*c_split: the
// per-split partials of a weight gradient, summed in split order by k_ec_reduce.  A 64 x 64 tile per 256-thread block, 16
// reduction rows per LDS stage, the next stage's operands fetched into registers while the MFMAs of this one run.
struct EcGemm {
    const float* X; int64_t xi, xr; int xrows;
    const float* Y; int64_t yr, yj;
    float* C; int64_t ldc, c_split;
    const float* bias;
    int I, J, R, rchunk;
};

constexpr int kGt = 64, kGr = 16;

__global__ void __launch_bounds__(kBlock) k_ec_gemm(EcGemm g) {
    __shared__ float xs[kGr][kGt + 4], ys[kGr][kGt + 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i0 = blockIdx.x * kGt, j0 = blockIdx.y * kGt;
    const int r_beg = blockIdx.z * g.rchunk, r_end = min(g.R, r_beg + g.rchunk);
    const bool x_rfast = g.xr == 1, y_jfast = g.yj == 1;      // coalesce the loads along whichever index is contiguous
    const int xi_l = x_rfast ? (t >> 4) : (t & 63), xr_l = x_rfast ? (t & 15) : (t >> 6);
    const int xi_s = x_rfast ? 16 : 0, xr_s = x_rfast ? 0 : 4;
    const int yj_l = y_jfast ? (t & 63) : (t >> 4), yr_l = y_jfast ? (t >> 6) : (t & 15);
    const int yj_s = y_jfast ? 0 : 16, yr_s = y_jfast ? 4 : 0;
    float xv[4], yv[4];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + xi_l + q * xi_s, r = r0 + xr_l + q * xr_s;
            xv[q] = (i < g.I && r < r_end) ? (i < g.xrows ? g.X[(int64_t)i * g.xi + (int64_t)r * g.xr] : 1.f) : 0.f;
            const int j = j0 + yj_l + q * yj_s, rr = r0 + yr_l + q * yr_s;
            yv[q] = (j < g.J && rr < r_end) ? g.Y[(int64_t)rr * g.yr + (int64_t)j * g.yj] : 0.f;
        }
    };
    glam_v4f acc[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[tj] = (glam_v4f){0.f, 0.f, 0.f, 0.f};
    if (r_beg < r_end) fetch(r_beg);
    for (int r0 = r_beg; r0 < r_end; r0 += kGr) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xs[xr_l + q * xr_s][xi_l + q * xi_s] = xv[q];
            ys[yr_l + q * yr_s][yj_l + q * yj_s] = yv[q];
        }
        __syncthreads();
        if (r0 + kGr < r_end) fetch(r0 + kGr);
#pragma unroll
        for (int kk = 0; kk < kGr; kk += 4) {
            const float a = xs[kk + (lane >> 4)][wave * 16 + (lane & 15)];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
                acc[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ys[kk + (lane >> 4)][tj * 16 + (lane & 15)], acc[tj], 0, 0, 0);
        }
    }
    float* C = g.C + (int64_t)blockIdx.z * g.c_split;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const int col = j0 + tj * 16 + (lane & 15);
        if (col >= g.J) continue;
        const float b = g.bias ? g.bias[col] : 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = i0 + wave * 16 + 4 * (lane >> 4) + v;
            if (row < g.I) C[(int64_t)row * g.ldc + col] = acc[tj][v] + b;
        }
    }
}

// out[o] = sum_{z < nz} part[z*stride + o] (o < n1 -> out1[o], else out2[o - n1]): ZL lanes per output take every ZL-th partial,
// then the ZL lane sums are added in lane order.  Fixed order throughout: bit-identical from run to run.
template <int ZL>
__global__ void __launch_bounds__(kBlock) k_ec_reduce(const float* part, int nz, int64_t stride, int n1, int n_out, float* out1,
                                                     float* out2) {
    constexpr int OPB = kBlock / ZL;
    __shared__ float red[ZL][OPB];
    const int ol = threadIdx.x % OPB, zl = threadIdx.x / OPB;
    const int o = blockIdx.x * OPB + ol;
    float s = 0.f;
    if (o < n_out)
        for (int z = zl; z < nz; z += ZL) s += part[(int64_t)z * stride + o];
    red[zl][ol] = s;
    __syncthreads();
    if (zl == 0 && o < n_out) {
        float tot = red[0][ol];
#pragma unroll
        for (int q = 1; q < ZL; ++q) tot += red[q][ol];
        if (o < n1) out1[o] = tot;
        else out2[o - n1] = tot;
    }
}

// h[e, k] = relu(b0[k] + sum_d W0[k, d] e[e, d])   (thread per (edge, k); W0 / b0 are 2 KiB at most: cache resident)
__global__ void __launch_bounds__(kBlock) k_ec_hidden(const float* ea, const float* w0, const float* b0, int64_t E, int De, float* h) {
    const int64_t total = E * kEcHidden;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t e = i / kEcHidden;
        const int k = (int)(i % kEcHidden);
        float a = b0[k];
        for (int d = 0; d < De; ++d) a = fmaf(w0[k * De + d], ea[e * De + d], a);
        h[i] = fmaxf(a, 0.f);
    }
}

// sx[n, k, c] = (1/d_n) sum_{e -> n} h[e, k] x[src e, c] for k < 32, the same with h = 1 for k = 32, x[n, c] for k = 33
// (thread per (node, channel), edges in CSR order, h as 8 float4 loads shared by the node's threads)
__global__ void __launch_bounds__(kBlock) k_ec_sums(const float* x, const float* h, const int* rowptr, const int* src, const int* eid,
                                                   int N, int Cin, int mean, float* sx) {
    const int64_t total = (int64_t)N * Cin;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int n = (int)(i / Cin), c = (int)(i % Cin);
        const int beg = rowptr[n], end = rowptr[n + 1];
        float acc[kEcHidden + 1];
#pragma unroll
        for (int k = 0; k <= kEcHidden; ++k) acc[k] = 0.f;
        for (int e = beg; e < end; ++e) {
            const float xv = x[(int64_t)src[e] * Cin + c];
            const float4* hp = reinterpret_cast<const float4*>(h + (int64_t)eid[e] * kEcHidden);
#pragma unroll
            for (int u = 0; u < kEcHidden / 4; ++u) {
                const float4 hv = hp[u];
                acc[4 * u + 0] = fmaf(hv.x, xv, acc[4 * u + 0]);
                acc[4 * u + 1] = fmaf(hv.y, xv, acc[4 * u + 1]);
                acc[4 * u + 2] = fmaf(hv.z, xv, acc[4 * u + 2]);
                acc[4 * u + 3] = fmaf(hv.w, xv, acc[4 * u + 3]);
            }
            acc[kEcHidden] += xv;
        }
        const float sc = mean ? 1.f / (float)max(end - beg, 1) : 1.f;
        float* o = sx + (int64_t)n * kEcSlots * Cin + c;
#pragma unroll
        for (int k = 0; k <= kEcHidden; ++k) o[(int64_t)k * Cin] = acc[k] * sc;
        o[(int64_t)(kEcSlots - 1) * Cin] = x[i];
    }
}

// dx[j, c] = dS[j, 33, c] + sum_{e: src = j} (1/d_t) (dS[t, 32, c] + sum_{k<32} h[e, k] dS[t, k, c]) (+ addend[j, c]), t = dst e
__global__ void __launch_bounds__(kBlock) k_ec_dx(const float* ds, const float* h, const int* colptr, const int* dst, const int* eid_t,
                                                 const int* rowptr, int N, int Cin, int mean, const float* addend, float* dx) {
    const int64_t total = (int64_t)N * Cin;
    const int64_t row = (int64_t)kEcSlots * Cin;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int j = (int)(i / Cin), c = (int)(i % Cin);
        float acc = ds[j * row + (int64_t)(kEcSlots - 1) * Cin + c];
        for (int e = colptr[j]; e < colptr[j + 1]; ++e) {
            const int n = dst[e];
            const float sc = mean ? 1.f / (float)max(rowptr[n + 1] - rowptr[n], 1) : 1.f;
            const float* g = ds + n * row + c;
            const float4* hp = reinterpret_cast<const float4*>(h + (int64_t)eid_t[e] * kEcHidden);
            float tv = g[(int64_t)kEcHidden * Cin];
#pragma unroll
            for (int u = 0; u < kEcHidden / 4; ++u) {
                const float4 hv = hp[u];
                tv = fmaf(hv.x, g[(int64_t)(4 * u + 0) * Cin], tv);
                tv = fmaf(hv.y, g[(int64_t)(4 * u + 1) * Cin], tv);
                tv = fmaf(hv.z, g[(int64_t)(4 * u + 2) * Cin], tv);
                tv = fmaf(hv.w, g[(int64_t)(4 * u + 3) * Cin], tv);
            }
            acc = fmaf(sc, tv, acc);
        }
        if (addend) acc += addend[i];     // the skip connection's gradient, added last (what the autograd engine's add computes)
        dx[i] = acc;
    }
}

// d_pre[e, k] = [h[e, k] > 0] (1/d_t) <x[src e], dS[t, k]>, and per block the partial sums d_W0[k, d] = sum_e d_pre[e, k] e[e, d],
// d_b0[k] = sum_e d_pre[e, k] over the nodes its waves visit (wave per target node, grid-stride; lanes k and k + 32 take the even
// and odd channels).  The block's 4 wave sums are added in wave order: part[block] = [d_W0 (32 x De) | d_b0 (32)].
__global__ void __launch_bounds__(kBlock) k_ec_dpre(const float* x, const float* ea, const float* h, const float* ds, const int* rowptr,
                                                   const int* src, const int* eid, int N, int De, int Cin, int mean, float* part) {
    __shared__ float red[4][kEcHidden * (kEcMaxDe + 1)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = lane & 31, half = lane >> 5;
    float pw[kEcMaxDe + 1];
#pragma unroll
    for (int d = 0; d <= kEcMaxDe; ++d) pw[d] = 0.f;
    const int64_t row = (int64_t)kEcSlots * Cin;
    for (int n = blockIdx.x * 4 + wave; n < N; n += gridDim.x * 4) {
        const int beg = rowptr[n], end = rowptr[n + 1];
        const float sc = mean ? 1.f / (float)max(end - beg, 1) : 1.f;
        const float* g = ds + n * row + (int64_t)k * Cin;
        for (int e = beg; e < end; ++e) {
            const float* xs = x + (int64_t)src[e] * Cin;
            const int id = eid[e];
            float d = 0.f;
            for (int c = half; c < Cin; c += 2) d = fmaf(xs[c], g[c], d);
            d += __shfl_xor(d, 32, 64);
            const float dp = h[(int64_t)id * kEcHidden + k] > 0.f ? d * sc : 0.f;
            const float* ee = ea + (int64_t)id * De;
#pragma unroll
            for (int q = 0; q < kEcMaxDe; ++q)
                if (q < De) pw[q] = fmaf(dp, ee[q], pw[q]);
            pw[kEcMaxDe] += dp;
        }
    }
    const int W = kEcHidden * (De + 1);
    if (half == 0) {
#pragma unroll
        for (int q = 0; q < kEcMaxDe; ++q)
            if (q < De) red[wave][k * De + q] = pw[q];
        red[wave][kEcHidden * De + k] = pw[kEcMaxDe];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < W; o += kBlock)
        part[(int64_t)blockIdx.x * W + o] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
}

// Wstack[k*Cin + ci, co] = W1[ci*Cout + co, k] (k < 32), b1[ci*Cout + co] (k = 32), root[ci, co] (k = 33)
__global__ void __launch_bounds__(kBlock) k_ec_stack(const float* w1, const float* b1, const float* root, int Cin, int Cout, float* ws) {
    const int total = kEcSlots * Cin * Cout;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const int co = i % Cout, ci = (i / Cout) % Cin, k = i / (Cout * Cin);
        const int m = ci * Cout + co;
        ws[i] = k < kEcHidden ? w1[m * kEcHidden + k] : (k == kEcHidden ? b1[m] : root[m]);
    }
}

// the inverse re-indexing: d_Wstack -> d_W1, d_b1, d_root
__global__ void __launch_bounds__(kBlock) k_ec_unstack(const float* dws, int Cin, int Cout, float* dw1, float* db1, float* droot) {
    const int total = kEcSlots * Cin * Cout;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
        const int co = i % Cout, ci = (i / Cout) % Cin, k = i / (Cout * Cin);
        const int m = ci * Cout + co;
        if (k < kEcHidden) dw1[m * kEcHidden + k] = dws[i];
        else if (k == kEcHidden) db1[m] = dws[i];
        else droot[m] = dws[i];
    }
}

static int ec_splits(int64_t N) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, (N + kEcSplitRows - 1) / kEcSplitRows)); }

static int launch_gemm(const EcGemm& g, int splits, hipStream_t s) {
    if (g.I <= 0 || g.J <= 0) return GLAM_OK;
    const dim3 grid((g.I + kGt - 1) / kGt, (g.J + kGt - 1) / kGt, splits);
    hipLaunchKernelGGL(k_ec_gemm, grid, dim3(kBlock), 0, s, g);
    GLAM_LAUNCH_CHECK("k_ec_gemm");
    return GLAM_OK;
}

static int ec_dims(const char* what, int64_t N, int64_t E, int De, int Cin, int Cout) {
    if (glam_nnconv_ec_supported(De, kEcHidden, Cin, Cout) != 1)
        return fail(GLAM_E_UNSUPPORTED, "%s: De=%d Cin=%d Cout=%d (hidden 32, De <= %d, Cin, Cout <= %d)", what, De, Cin, Cout, kEcMaxDe, kEcMaxC);
    if (N < 0 || E < 0 || N >= (int64_t)1 << 31 || E >= (int64_t)1 << 31 || N * kEcSlots * Cin >= (int64_t)1 << 40)
        return fail(GLAM_E_INVALID, "%s: N=%lld E=%lld out of range", what, (long long)N, (long long)E);
    return GLAM_OK;
}

}  // namespace glam

using namespace glam;

extern "C" int glam_nnconv_ec_supported(int De, int hidden, int Cin, int Cout) {
    return (hidden == kEcHidden && De >= 1 && De <= kEcMaxDe && Cin >= 1 && Cin <= kEcMaxC && Cout >= 1 && Cout <= kEcMaxC) ? 1 : 0;
}

extern "C" size_t glam_nnconv_ec_workspace_bytes(int64_t N, int64_t E, int De, int Cin, int Cout, int backward) {
    (void)E;
    if (glam_nnconv_ec_supported(De, kEcHidden, Cin, Cout) != 1 || N < 0) return 0;
    size_t floats = (size_t)N * kEcSlots * Cin;                                                       // [S | x], then d_S
    if (backward)
        floats += (size_t)ec_splits(N) * ((size_t)kEcSlots * Cin + 1) * Cout                         // d_Wstack | d_bias partials
                  + (size_t)kEcDpreBlocks * kEcHidden * (De + 1);                                     // d_W0 | d_b0 partials
    return floats * sizeof(float);
}

extern "C" int glam_nnconv_ec_stack(const float* w1, const float* b1, const float* root, int Cin, int Cout, float* wstack, void* stream) {
    if (glam_nnconv_ec_supported(1, kEcHidden, Cin, Cout) != 1) return fail(GLAM_E_UNSUPPORTED, "glam_nnconv_ec_stack: Cin=%d Cout=%d", Cin, Cout);
    GLAM_REQUIRE(w1 && b1 && root && wstack, "glam_nnconv_ec_stack: null pointer");
    hipLaunchKernelGGL(k_ec_stack, dim3(grid_for((int64_t)kEcSlots * Cin * Cout, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, w1, b1, root,
                       Cin, Cout, wstack);
    GLAM_LAUNCH_CHECK("glam_nnconv_ec_stack");
    return GLAM_OK;
}

extern "C" int glam_nnconv_ec_unstack(const float* d_wstack, int Cin, int Cout, float* d_w1, float* d_b1, float* d_root, void* stream) {
    if (glam_nnconv_ec_supported(1, kEcHidden, Cin, Cout) != 1) return fail(GLAM_E_UNSUPPORTED, "glam_nnconv_ec_unstack: Cin=%d Cout=%d", Cin, Cout);
    GLAM_REQUIRE(d_wstack && d_w1 && d_b1 && d_root, "glam_nnconv_ec_unstack: null pointer");
    hipLaunchKernelGGL(k_ec_unstack, dim3(grid_for((int64_t)kEcSlots * Cin * Cout, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, d_wstack,
                       Cin, Cout, d_w1, d_b1, d_root);
    GLAM_LAUNCH_CHECK("glam_nnconv_ec_unstack");
    return GLAM_OK;
}

extern "C" int glam_nnconv_ec_fwd(const float* x, const float* edge_attr, const int32_t* rowptr, const int32_t* src, const int32_t* eid,
                                  int64_t N, int64_t E, int De, int Cin, int Cout, const float* w0, const float* b0, const float* wstack,
                                  const float* bias, int mean, float* h, void* workspace, size_t workspace_bytes, float* out, void* stream) {
    if (int rc = ec_dims("glam_nnconv_ec_fwd", N, E, De, Cin, Cout)) return rc;
    if (N == 0) return GLAM_OK;
    GLAM_REQUIRE(x && rowptr && w0 && b0 && wstack && workspace && out && (E == 0 || (edge_attr && src && eid && h)),
                 "glam_nnconv_ec_fwd: null pointer");
    GLAM_REQUIRE(workspace_bytes >= glam_nnconv_ec_workspace_bytes(N, E, De, Cin, Cout, 0), "glam_nnconv_ec_fwd: workspace too small");
    GLAM_REQUIRE(E == 0 || aligned16(h), "glam_nnconv_ec_fwd: h must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* sx = static_cast<float*>(workspace);
    if (E > 0) {
        hipLaunchKernelGGL(k_ec_hidden, dim3(grid_for(E * kEcHidden, kBlock)), dim3(kBlock), 0, s, edge_attr, w0, b0, E, De, h);
        GLAM_LAUNCH_CHECK("k_ec_hidden");
    }
    hipLaunchKernelGGL(k_ec_sums, dim3(grid_for(N * Cin, kBlock)), dim3(kBlock), 0, s, x, h, rowptr, src, eid, (int)N, Cin, mean, sx);
    GLAM_LAUNCH_CHECK("k_ec_sums");
    const int K = kEcSlots * Cin;
    EcGemm g{sx, K, 1, (int)N, wstack, Cout, 1, out, Cout, 0, bias, (int)N, Cout, K, K};
    return launch_gemm(g, 1, s);
}

extern "C" int glam_nnconv_ec_bwd(const float* d_out, const float* x, const float* edge_attr, const int32_t* rowptr, const int32_t* src,
                                  const int32_t* eid, const int32_t* colptr, const int32_t* dst, const int32_t* eid_t, int64_t N, int64_t E,
                                  int De, int Cin, int Cout, const float* wstack, const float* h, int mean, const float* addend, float* dx,
                                  float* d_w0, float* d_b0, float* d_wstack, float* d_bias, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    if (int rc = ec_dims("glam_nnconv_ec_bwd", N, E, De, Cin, Cout)) return rc;
    GLAM_REQUIRE((N == 0 || (d_out && x)) && rowptr && colptr && wstack && workspace && dx && d_w0 && d_b0 && d_wstack && d_bias &&
                     (E == 0 || (edge_attr && src && eid && dst && eid_t && h)), "glam_nnconv_ec_bwd: null pointer");
    GLAM_REQUIRE(workspace_bytes >= glam_nnconv_ec_workspace_bytes(N, E, De, Cin, Cout, 1), "glam_nnconv_ec_bwd: workspace too small");
    GLAM_REQUIRE(E == 0 || aligned16(h), "glam_nnconv_ec_bwd: h must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int K = kEcSlots * Cin, splits = ec_splits(N);
    const int rchunk = (int)(((N + splits - 1) / splits + kGr - 1) / kGr * kGr);
    if (N == 0) {           // no rows: every gradient is zero
        for (auto [p, n] : {std::pair<float*, size_t>{d_w0, (size_t)kEcHidden * De}, {d_b0, (size_t)kEcHidden},
                            {d_wstack, (size_t)K * Cout}, {d_bias, (size_t)Cout}})
            if (hipMemsetAsync(p, 0, n * sizeof(float), s) != hipSuccess) return fail(GLAM_E_HIP, "glam_nnconv_ec_bwd: memset");
        return GLAM_OK;
    }
    float* buf = static_cast<float*>(workspace);
    float* pw = buf + (size_t)N * K;
    float* pw0 = pw + (size_t)splits * (K + 1) * Cout;
    const int64_t wsz = (int64_t)(K + 1) * Cout, w0sz = (int64_t)kEcHidden * (De + 1);
    if (N > 0) {
        hipLaunchKernelGGL(k_ec_sums, dim3(grid_for(N * Cin, kBlock)), dim3(kBlock), 0, s, x, h, rowptr, src, eid, (int)N, Cin, mean, buf);
        GLAM_LAUNCH_CHECK("k_ec_sums");
    }
    // d_Wstack = [S | x]^T G and d_bias = 1^T G (the row of ones): per-split partials, then the split-order sum
    EcGemm gw{buf, 1, K, K, d_out, Cout, 1, pw, Cout, wsz, nullptr, K + 1, Cout, (int)N, rchunk};
    if (int rc = launch_gemm(gw, splits, s)) return rc;
    hipLaunchKernelGGL(k_ec_reduce<4>, dim3((unsigned)((wsz + kBlock / 4 - 1) / (kBlock / 4))), dim3(kBlock), 0, s, pw, splits, wsz,
                       K * Cout, (int)wsz, d_wstack, d_bias);
    GLAM_LAUNCH_CHECK("k_ec_reduce(d_wstack)");
    if (N > 0) {
        // d_S = G Wstack^T into the buffer [S | x] held (stream order: the product above has read it)
        EcGemm gs{d_out, Cout, 1, (int)N, wstack, 1, Cout, buf, K, 0, nullptr, (int)N, K, Cout, Cout};
        if (int rc = launch_gemm(gs, 1, s)) return rc;
        hipLaunchKernelGGL(k_ec_dx, dim3(grid_for(N * Cin, kBlock)), dim3(kBlock), 0, s, buf, h, colptr, dst, eid_t, rowptr, (int)N, Cin, mean,
                           addend, dx);
        GLAM_LAUNCH_CHECK("k_ec_dx");
    }
    hipLaunchKernelGGL(k_ec_dpre, dim3(kEcDpreBlocks), dim3(kBlock), 0, s, x, edge_attr, h, buf, rowptr, src, eid, (int)N, De, Cin, mean, pw0);
    GLAM_LAUNCH_CHECK("k_ec_dpre");
    hipLaunchKernelGGL(k_ec_reduce<16>, dim3((unsigned)((w0sz + kBlock / 16 - 1) / (kBlock / 16))), dim3(kBlock), 0, s, pw0, kEcDpreBlocks,
                       w0sz, kEcHidden * De, (int)w0sz, d_w0, d_b0);
    GLAM_LAUNCH_CHECK("k_ec_reduce(d_w0)");
    return GLAM_OK;
}
