// Attention export (inference only, no backward): the weights the fused kernels never write.
//   k_edge_attention       alpha[e,h] of a TripletMessage / TripletMessageLight / GATConv step (src_1gp/layer.py:48-51, :92-95)
//   k_edge_attention_sent  sent[n,h] = sum of alpha over the edges that LEAVE n
//   k_segment_softmax      per-node weights of GlobalAttention (src_1gp/layer.py:206-220) and of Set2Set's read (src_1gp/model.py:41)
// No atomics; every reduction runs in a fixed order (lane-local in row order, then a fixed butterfly), so two runs are bit-equal.
#include <math.h>

#include "common.h"

namespace glam {

constexpr int kAttnG = 8;                    // lanes per target node: molecular in-degrees are <= 4 (5 with GATConv's self loop)
constexpr int kWavesPerBlockAE = kBlock / 64;

template <int G>
__device__ __forceinline__ float group_max(float v) {
    static_assert(G == 8, "group_max: lanes per node");
    v = fmaxf(v, dpp_move<0xB1>(v));         // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp_move<0x4E>(v));         // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp_move<0x141>(v));        // row_half_mirror
    return v;
}

__device__ __forceinline__ float leaky_ae(float v, float slope) { return v > 0.f ? v : v * slope; }

// the four head logits of CSR slot e (the arithmetic of k_triplet_fwd: a_i + <edge_attr, M> + a_j, fma chain over k, then leaky)
template <int DE>
__device__ __forceinline__ float4 edge_logits(const float* a_ij, const float* edge_attr, const float (&Mr)[DE][4], const int* src,
                                              const int* eid, float4 ai, int e, float slope, int* id_out) {
    const int s = src[e], id = eid[e];
    float ea[DE];
#pragma unroll
    for (int u = 0; u < DE / 4; ++u) {
        const float4 v = ld4(edge_attr + (size_t)id * DE + 4 * u);
        ea[4 * u] = v.x; ea[4 * u + 1] = v.y; ea[4 * u + 2] = v.z; ea[4 * u + 3] = v.w;
    }
    const float4 aj = ld4(a_ij + (size_t)s * 8 + 4);
    float l[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        float ee = 0.f;
#pragma unroll
        for (int k = 0; k < DE; ++k) ee = fmaf(ea[k], Mr[k][h], ee);
        l[h] = leaky_ae(f4get(ai, h) + ee + f4get(aj, h), slope);
    }
    *id_out = id;
    return make_float4(l[0], l[1], l[2], l[3]);
}

__device__ __forceinline__ float4 max4(float4 a, float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}
__device__ __forceinline__ float4 exp4(float4 l, float4 m) {
    return make_float4(softmax_exp(l.x - m.x), softmax_exp(l.y - m.y), softmax_exp(l.z - m.z), softmax_exp(l.w - m.w));
}
__device__ __forceinline__ float4 head_mask(float4 v, int H) {
    return make_float4(v.x, H > 1 ? v.y : 0.f, H > 2 ? v.z : 0.f, H > 3 ? v.w : 0.f);
}

// G lanes per target node, one incoming edge per lane, the heads as a float4.  A row of at most G edges keeps its logits in registers
// (one pass over memory); a longer row is strided by its group three times (max, exp-sum, write) and recomputes the logits.
template <int DE>
__global__ void __launch_bounds__(kBlock) k_edge_attention(const float* a_ij, const float* edge_attr, const float* M, const int* rowptr,
                                                          const int* src, const int* eid, int N, int H, float slope, float* alpha) {
    constexpr int G = kAttnG, GPB = kBlock / G;
    const int tid = threadIdx.x, lg = tid % G;
    float Mr[DE][4];
#pragma unroll
    for (int k = 0; k < DE; ++k)
#pragma unroll
        for (int h = 0; h < 4; ++h) Mr[k][h] = M[k * 4 + h];
    const float4 ninf = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int base = blockIdx.x * GPB; base < N; base += gridDim.x * GPB) {
        const int n = base + tid / G;
        if (n >= N) continue;                                   // (uniform per lane group)
        const int beg = rowptr[n], end = rowptr[n + 1];
        if (end <= beg) continue;
        const float4 ai = ld4(a_ij + (size_t)n * 8);
        if (end - beg <= G) {
            const bool ok = beg + lg < end;
            int id = 0;
            float4 l = ninf;
            if (ok) l = edge_logits<DE>(a_ij, edge_attr, Mr, src, eid, ai, beg + lg, slope, &id);
            const float4 m = make_float4(group_max<G>(l.x), group_max<G>(l.y), group_max<G>(l.z), group_max<G>(l.w));
            const float4 p = ok ? exp4(l, m) : f4zero();
            const float4 s = make_float4(group_sum<G>(p.x), group_sum<G>(p.y), group_sum<G>(p.z), group_sum<G>(p.w));
            if (ok) {
                const float4 inv = make_float4(1.f / (s.x + 1e-16f), 1.f / (s.y + 1e-16f), 1.f / (s.z + 1e-16f), 1.f / (s.w + 1e-16f));
                st4(alpha + (size_t)id * 4, head_mask(inv * p, H));
            }
            continue;
        }
        int id;
        float4 m = ninf;
        for (int e = beg + lg; e < end; e += G) m = max4(m, edge_logits<DE>(a_ij, edge_attr, Mr, src, eid, ai, e, slope, &id));
        m = make_float4(group_max<G>(m.x), group_max<G>(m.y), group_max<G>(m.z), group_max<G>(m.w));
        float4 s = f4zero();
        for (int e = beg + lg; e < end; e += G) {
            const float4 p = exp4(edge_logits<DE>(a_ij, edge_attr, Mr, src, eid, ai, e, slope, &id), m);
            s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
        }
        s = make_float4(group_sum<G>(s.x), group_sum<G>(s.y), group_sum<G>(s.z), group_sum<G>(s.w));
        const float4 inv = make_float4(1.f / (s.x + 1e-16f), 1.f / (s.y + 1e-16f), 1.f / (s.z + 1e-16f), 1.f / (s.w + 1e-16f));
        for (int e = beg + lg; e < end; e += G) {
            const float4 p = exp4(edge_logits<DE>(a_ij, edge_attr, Mr, src, eid, ai, e, slope, &id), m);
            st4(alpha + (size_t)id * 4, head_mask(inv * p, H));
        }
    }
}

// A lane per source node; its outgoing edges in CSR order, four alpha rows in flight.
__global__ void __launch_bounds__(kBlock) k_edge_attention_sent(const float* alpha, const int* colptr, const int* eid_t, int N, int H,
                                                               float* sent) {
    for (int n = blockIdx.x * kBlock + threadIdx.x; n < N; n += gridDim.x * kBlock) {
        const int beg = colptr[n], end = colptr[n + 1];
        float4 acc = f4zero();
        for (int e0 = beg; e0 < end; e0 += 4) {
            float4 r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = e0 + k < end ? ld4(alpha + (size_t)eid_t[e0 + k] * 4) : f4zero();
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc.x += r[k].x; acc.y += r[k].y; acc.z += r[k].z; acc.w += r[k].w; }
        }
        st4(sent + (size_t)n * 4, head_mask(acc, H));
    }
}

// Wave per graph.  LPR = 1: the logits are gate[n], a lane per node.  LPR = 16 / 32: the logits are <x_n, q_g> formed by LPR lanes per
// row (lane = (row group, float4 chunk), the dot product of k_s2s_attn_fwd).  A graph of at most (64 / LPR) * 8 nodes keeps its logits
// in registers; a longer one is read three times.
template <int LPR>
__global__ void __launch_bounds__(kBlock) k_segment_softmax(const float* gate, const float* x, const float* q, const int* ptr, int B, int D,
                                                           int ld, float* w) {
    constexpr int RG = 64 / LPR, R = 8;
    const int lane = threadIdx.x & 63, c4 = lane % LPR, rg = lane / LPR;
    const int wave = blockIdx.x * kWavesPerBlockAE + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlockAE;
    const bool act = LPR > 1 && 4 * c4 < D;
    for (int g = wave; g < B; g += nwaves) {
        const int beg = ptr[g], end = ptr[g + 1];
        float4 qv = f4zero();
        if (act) {                                             // (channels D..ld of a padded row do not enter the logit)
            qv = ld4(q + (size_t)g * ld + 4 * c4);
            if (4 * c4 + 1 >= D) qv.y = 0.f;
            if (4 * c4 + 2 >= D) qv.z = 0.f;
            if (4 * c4 + 3 >= D) qv.w = 0.f;
        }
        const bool small = end - beg <= RG * R;
        float e[R];
        auto logits = [&](int b0) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int n = b0 + rg + RG * u;
                const bool okr = n < end;
                if constexpr (LPR == 1) {
                    e[u] = okr ? gate[n] : -INFINITY;
                } else {
                    const float4 row = (act && okr) ? ld4(x + (size_t)n * ld + 4 * c4) : f4zero();
                    const float d = group_sum<LPR>(dot4(row, qv));
                    e[u] = okr ? d : -INFINITY;
                }
            }
        };
        float m = -INFINITY;
        for (int b0 = beg; b0 < end; b0 += RG * R) {
            logits(b0);
#pragma unroll
            for (int u = 0; u < R; ++u) m = fmaxf(m, e[u]);
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
        float ssum = 0.f;
        for (int b0 = beg; b0 < end; b0 += RG * R) {
            if (!small) logits(b0);
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (b0 + rg + RG * u < end) ssum += expf(e[u] - m);
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) ssum += __shfl_xor(ssum, off);
        const float inv = 1.f / (ssum + 1e-16f);
        for (int b0 = beg; b0 < end; b0 += RG * R) {
            if (!small) logits(b0);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int n = b0 + rg + RG * u;
                if (n < end && c4 == 0) w[n] = expf(e[u] - m) * inv;
            }
        }
    }
}

}  // namespace glam

using namespace glam;

extern "C" int glam_edge_attention(const float* a_ij, const float* edge_attr, const float* M, const int32_t* rowptr, const int32_t* src,
                                   const int32_t* eid, int64_t N, int64_t E, int H, int De, float slope, float* alpha, void* stream) {
    if (N < 0 || E < 0 || N > INT32_MAX || E > INT32_MAX) return fail(GLAM_E_INVALID, "glam_edge_attention: N/E out of range");
    if (De != 4 && De != 8) return fail(GLAM_E_UNSUPPORTED, "glam_edge_attention: De=%d (host must zero-pad edge features to 4 or 8)", De);
    if (H < 1 || H > 4) return fail(GLAM_E_UNSUPPORTED, "glam_edge_attention: heads=%d not in 1..4", H);
    if (N == 0 || E == 0) return GLAM_OK;
    GLAM_REQUIRE(a_ij && edge_attr && M && rowptr && src && eid && alpha, "glam_edge_attention: null pointer");
    GLAM_REQUIRE(aligned16(a_ij) && aligned16(edge_attr) && aligned16(alpha), "glam_edge_attention: pointers must be 16-byte aligned");
    const dim3 grid(grid_for(N, kBlock / kAttnG)), block(kBlock);
    if (De == 4)
        hipLaunchKernelGGL(k_edge_attention<4>, grid, block, 0, (hipStream_t)stream, a_ij, edge_attr, M, rowptr, src, eid, (int)N, H, slope, alpha);
    else
        hipLaunchKernelGGL(k_edge_attention<8>, grid, block, 0, (hipStream_t)stream, a_ij, edge_attr, M, rowptr, src, eid, (int)N, H, slope, alpha);
    GLAM_LAUNCH_CHECK("glam_edge_attention");
    return GLAM_OK;
}

extern "C" int glam_edge_attention_sent(const float* alpha, const int32_t* colptr, const int32_t* eid_t, int64_t N, int64_t E, int H,
                                        float* sent, void* stream) {
    if (N < 0 || E < 0 || N > INT32_MAX || E > INT32_MAX) return fail(GLAM_E_INVALID, "glam_edge_attention_sent: N/E out of range");
    if (H < 1 || H > 4) return fail(GLAM_E_UNSUPPORTED, "glam_edge_attention_sent: heads=%d not in 1..4", H);
    if (N == 0 || E == 0) return GLAM_OK;                      // (no edge leaves any node: the caller's zero-filled sent stands)
    GLAM_REQUIRE(alpha && colptr && eid_t && sent, "glam_edge_attention_sent: null pointer");
    GLAM_REQUIRE(aligned16(alpha) && aligned16(sent), "glam_edge_attention_sent: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(k_edge_attention_sent, dim3(grid_for(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, alpha, colptr, eid_t, (int)N, H, sent);
    GLAM_LAUNCH_CHECK("glam_edge_attention_sent");
    return GLAM_OK;
}

extern "C" int glam_segment_softmax(const float* gate, const float* x, const float* q, const int32_t* ptr, int64_t N, int64_t B, int D, int ld,
                                    float* w, void* stream) {
    if (N < 0 || B < 0 || N > INT32_MAX || B > INT32_MAX) return fail(GLAM_E_INVALID, "glam_segment_softmax: N/B out of range");
    if (N == 0 || B == 0) return GLAM_OK;                      // (an empty gate tensor has no address either: before the form is chosen)
    if (!gate && ((ld & 3) || ld > 128 || D < 1 || D > ld))
        return fail(GLAM_E_UNSUPPORTED, "glam_segment_softmax: D=%d ld=%d (1 <= D <= ld, ld a multiple of 4, <= 128)", D, ld);
    GLAM_REQUIRE(ptr && w && (gate || (x && q)), "glam_segment_softmax: null pointer");
    GLAM_REQUIRE(gate || (aligned16(x) && aligned16(q)), "glam_segment_softmax: x and q must be 16-byte aligned");
    const dim3 grid(grid_for(B, kWavesPerBlockAE)), block(kBlock);
    const int Bi = (int)B;
    if (gate) hipLaunchKernelGGL(k_segment_softmax<1>, grid, block, 0, (hipStream_t)stream, gate, x, q, ptr, Bi, D, ld, w);
    else if (ld <= 64) hipLaunchKernelGGL(k_segment_softmax<16>, grid, block, 0, (hipStream_t)stream, gate, x, q, ptr, Bi, D, ld, w);
    else hipLaunchKernelGGL(k_segment_softmax<32>, grid, block, 0, (hipStream_t)stream, gate, x, q, ptr, Bi, D, ld, w);
    GLAM_LAUNCH_CHECK("glam_segment_softmax");
    return GLAM_OK;
}
