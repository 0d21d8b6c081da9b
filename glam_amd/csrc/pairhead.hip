// Factored pair head (inference): the two-layer head of the pair models over a TABLE of R x Cs pairs, without the [pairs, 2 hid + F] input
// rows and without the [pairs, e_dim] hidden matrix.  Over a table the first linear layer separates:
//   lin_out0(cat[a_i, b_j, f_ij]) = (W0[:, :hid] a_i + b0) + W0[:, hid:2 hid] b_j + W0[:, 2 hid:] f_ij = A[i, :] + B[j, :] + Wf f_ij
// so only the F fusion columns are per pair, and with no norm in the head and an elementwise activation
//   out[i, j, o] = b1[o] + sum_e w1[o, e] * act(A[i, e] + B[j, e] + sum_k Wf[e, k] * f[i, j, k])
//
// k_pair_head_side — the two small products.  One thread per output element and ONE fmaf chain per element:
//   A[r, e] = fmaf(W0[e, col0 + K-1], x[r, K-1], ... fmaf(W0[e, col0], x[r, 0], b0[e] or 0.f))          c ascending
// The chain of an element depends on nothing but its own row of x and its own row of W0: not on n, not on the launch shape, not on whether
// the result is stored as [n, e_dim] or transposed as [e_dim, n].  (A library GEMM picks its tiling — and with it its roundings — by the row
// count; these two products are what makes a table entry independent of the selection it is computed in.)  A thread takes one index of
// the axis the lanes run along (the contiguous axis of the output: e, or with the transposed output the row) and four consecutive indices
// of the other axis, so that one of its two operands is loaded once for four chains.  W0 is read in place (col0, leading dimension).
//
// k_pair_head — the table.  The lanes of a wave run along one axis of the table (64 entries), the wave takes kHeadRows consecutive entries of
// the other axis, and the loop over e is the serial loop:
//   the LANE side's matrix comes TRANSPOSED, Lt[e, l]: one coalesced 256-byte load per e, used by every entry of the other axis the wave holds;
//   the UNIFORM side's matrix U[u, e], Wf[e, :] and w1[:, e] are wave-uniform and are read through the constant address space (scalar loads:
//       the scalar unit fetches them once per wave and every multiply-add takes them as its scalar operand).  No launch of this kernel writes
//       them: U was written by the side launch before it;
//   f[i, j, :] (F numbers) and the kHeadRows x out_dim accumulators sit in registers.
// No LDS, no barrier, no atomics, no cross-lane step.  A pair's result is ONE chain, whatever the shape of the table around it:
//   h = A[i, e] + B[j, e];  h = fmaf(Wf[e, k], f[i, j, k], h) for k ascending;  h = act(h);  acc[o] = fmaf(w1[o, e], h, acc[o]),  e ascending from
//   acc[o] = b1[o].
// Which axis the lanes take is the host's choice (the axis that fills its 64-lane chunks better; the columns on a tie): the sum A + B
// commutes bit for bit, so the choice does not show in the result.  A 1 024 x 15 panel puts its rows on the lanes (fill 100 %), a 32 x 15
// one too (fill 50 %).
#include <algorithm>
#include <utility>

#include "common.h"

namespace glam {

constexpr int kHeadRows = 4;                   // entries of the uniform axis per wave
constexpr int kHeadWaves = kBlock / 64;
constexpr int kHeadMaxOut = 8;
constexpr int kHeadMaxF = 16;
constexpr int kSideQuad = 4;                   // chains per thread of the side kernel

struct HeadSide {          // one of the two products: out = x[n, K] (ldx) @ W[e_dim, K]^T (ldw, already offset by col0) (+ b0)
    const float* x;
    const float* W;
    const float* b0;       // may be null
    float* out;            // [n, e_dim], or with trans [e_dim, n]
    int64_t ldx, ldw;
    int n, K, trans;
    int blocks;            // blocks of the launch that belong to this product
};

// kTrans = false: lanes along e, four consecutive rows per thread (W0[e, c] loaded once for the four);  true: lanes along the row, four
// consecutive e per thread (x[r, c] loaded once for the four).  Either way element (r, e) is the chain in the header of this file.
template <bool kTrans>
__device__ __forceinline__ void head_side(const HeadSide& s, int e_dim, int64_t t) {
    const int na = kTrans ? s.n : e_dim, nb = kTrans ? e_dim : s.n;
    const int64_t groups = (nb + kSideQuad - 1) / kSideQuad;
    if (t >= (int64_t)na * groups) return;
    const int a = (int)(t % na), g0 = (int)(t / na) * kSideQuad;
    int b[kSideQuad];
    float acc[kSideQuad];
#pragma unroll
    for (int q = 0; q < kSideQuad; ++q) {
        b[q] = min(g0 + q, nb - 1);                            // (past the end: the last one again, not stored)
        acc[q] = s.b0 ? s.b0[kTrans ? b[q] : a] : 0.f;
    }
    if constexpr (kTrans) {
        const float* xr = s.x + (size_t)a * s.ldx;
        for (int c = 0; c < s.K; ++c) {
            const float xv = xr[c];
#pragma unroll
            for (int q = 0; q < kSideQuad; ++q) acc[q] = fmaf(s.W[(size_t)b[q] * s.ldw + c], xv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < kSideQuad; ++q)
            if (g0 + q < nb) s.out[(size_t)b[q] * s.n + a] = acc[q];
    } else {
        const float* wr = s.W + (size_t)a * s.ldw;
        for (int c = 0; c < s.K; ++c) {
            const float wv = wr[c];
#pragma unroll
            for (int q = 0; q < kSideQuad; ++q) acc[q] = fmaf(wv, s.x[(size_t)b[q] * s.ldx + c], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < kSideQuad; ++q)
            if (g0 + q < nb) s.out[(size_t)b[q] * e_dim + a] = acc[q];
    }
}

// Both products from one launch: blocks [0, s0.blocks) take the first, the rest the second.
__global__ void __launch_bounds__(kBlock) k_pair_head_side(HeadSide s0, HeadSide s1, int e_dim) {
    const bool first = (int)blockIdx.x < s0.blocks;
    const HeadSide& s = first ? s0 : s1;
    const int64_t t = (int64_t)(first ? blockIdx.x : blockIdx.x - s0.blocks) * kBlock + threadIdx.x;
    if (s.trans) head_side<true>(s, e_dim, t);
    else head_side<false>(s, e_dim, t);
}

// The serial loop of one wave.  kRelu: act = max-with-zero that keeps a NaN; otherwise h > 0 ? h : slope * h (slope = 1: no activation,
// the product with 1.f is exact).
template <int OUT, int F, bool kRelu>
__device__ __forceinline__ void head_loop(glam_cf1* const (&ur)[kHeadRows], const float* lt, int nl, glam_cf1* wf, int ldw, glam_cf1* w1,
                                          int e_dim, float slope, const float (&fr)[kHeadRows][F > 0 ? F : 1], float (&acc)[kHeadRows][OUT]) {
    // (not unrolled: an iteration holds 4 + F + OUT scalar operands, and two iterations of the wide instantiations spill them; the lane side's
    //  value of the NEXT e is loaded one iteration ahead instead — the last iteration loads its own again)
    float ahead = ld1g(lt);
#pragma unroll 1
    for (int e = 0; e < e_dim; ++e) {
        const float bt = ahead;
        ahead = ld1g(lt + (size_t)min(e + 1, e_dim - 1) * nl);
        glam_cf1* wfe = wf + (size_t)e * ldw;
        float h[kHeadRows];
#pragma unroll
        for (int r = 0; r < kHeadRows; ++r) {
            h[r] = ur[r][e] + bt;
#pragma unroll
            for (int k = 0; k < F; ++k) h[r] = fmaf(wfe[k], fr[r][k], h[r]);
            if constexpr (kRelu) h[r] = h[r] < 0.f ? 0.f : h[r];
            else h[r] = h[r] > 0.f ? h[r] : h[r] * slope;
        }
#pragma unroll
        for (int o = 0; o < OUT; ++o) {
            const float w = w1[(size_t)o * e_dim + e];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) acc[r][o] = fmaf(w, h[r], acc[r][o]);
        }
    }
}

// U [nu, e_dim]: the uniform side;  Lt [e_dim, nl]: the lane side, transposed;  pair (u, l) is entry u * su + l * sl of the table (f and out
// are indexed by it: su = Cs, sl = 1 with the columns on the lanes, su = 1, sl = Cs with the rows on them).  Wf = W0 + 2 hid.
// grid: ceil(nl / 64) * ceil(nu / (kHeadWaves * kHeadRows)) blocks, the lane chunk fastest; the four waves of a block take four consecutive
// groups of the uniform axis against the same lane chunk (its Lt loads are the same lines).
template <int OUT, int F>
__global__ void __launch_bounds__(kBlock) k_pair_head(const float* __restrict__ U, const float* __restrict__ Lt, const float* __restrict__ f,
                                                     const float* __restrict__ Wf, int ldw, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, int e_dim, int nu, int nl, int lane_chunks, int64_t su,
                                                     int64_t sl, int act, float slope, float* __restrict__ out) {
    static_assert(OUT >= 1 && OUT <= kHeadMaxOut && F >= 0 && F <= kHeadMaxF, "k_pair_head: out_dim / F");
    const int lane = threadIdx.x & 63;
    const int lc = blockIdx.x % lane_chunks, ug = blockIdx.x / lane_chunks;
    const int u0 = (ug * kHeadWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * kHeadRows;
    if (u0 >= nu) return;                                  // a wave without an entry (no barrier below: the others go on)
    const int l = lc * 64 + lane;
    const bool valid = l < nl;
    const int lr = valid ? l : nl - 1;                     // (an idle lane computes the last entry again and does not store)
    glam_cf1* ur[kHeadRows];
    size_t pair[kHeadRows];
    float fr[kHeadRows][F > 0 ? F : 1];
    float acc[kHeadRows][OUT];
    glam_cf1* b1u = uniform_cf1(b1);
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) {
        const int u = min(u0 + r, nu - 1);                 // (past the end: the last one again, not stored)
        ur[r] = uniform_cf1(U + (size_t)u * e_dim);
        pair[r] = (size_t)u * su + (size_t)lr * sl;
#pragma unroll
        for (int k = 0; k < F; ++k) fr[r][k] = ld1g(f + pair[r] * F + k);
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[r][o] = b1u[o];
    }
    if (act == 1) head_loop<OUT, F, true>(ur, Lt + lr, nl, uniform_cf1(Wf), ldw, uniform_cf1(w1), e_dim, slope, fr, acc);
    else head_loop<OUT, F, false>(ur, Lt + lr, nl, uniform_cf1(Wf), ldw, uniform_cf1(w1), e_dim, slope, fr, acc);
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) {
        if (valid && u0 + r < nu) {
#pragma unroll
            for (int o = 0; o < OUT; ++o) st1g(out + pair[r] * OUT + o, acc[r][o]);
        }
    }
}

typedef void (*head_kernel)(const float*, const float*, const float*, const float*, int, const float*, const float*, int, int, int, int, int64_t,
                            int64_t, int, float, float*);

// [(OUT - 1) * (kHeadMaxF + 1) + F] -> the instantiation of (OUT, F)
template <int... I>
static const head_kernel* head_table(std::integer_sequence<int, I...>) {
    static const head_kernel t[] = {k_pair_head<I / (kHeadMaxF + 1) + 1, I % (kHeadMaxF + 1)>...};
    return t;
}

// share of the lanes of ceil(n / 64) chunks that hold an entry, as a comparable integer pair: fill(a) > fill(b)
static inline bool fills_better(int64_t a, int64_t b) { return a * ((b + 63) / 64) > b * ((a + 63) / 64); }

}  // namespace glam

using namespace glam;

extern "C" size_t glam_pair_head_workspace_bytes(int64_t R, int64_t Cs, int e_dim) {
    if (R <= 0 || Cs <= 0 || e_dim <= 0) return 0;
    return ((size_t)R + (size_t)Cs) * (size_t)e_dim * sizeof(float);
}

extern "C" int glam_pair_head_fwd(const float* flat_a, int64_t lda, const float* flat_b, int64_t ldb, const float* f, int64_t R, int64_t Cs,
                                  int hid, int F, const float* W0, int64_t ldw, const float* b0, int e_dim, const float* w1, const float* b1,
                                  int out_dim, int act, float slope, void* workspace, size_t workspace_bytes, float* out, void* stream) {
    GLAM_REQUIRE(out_dim >= 1 && out_dim <= kHeadMaxOut, "glam_pair_head_fwd: out_dim=%d not in 1..%d", out_dim, kHeadMaxOut);
    GLAM_REQUIRE(F >= 0 && F <= kHeadMaxF, "glam_pair_head_fwd: F=%d fusion columns not in 0..%d", F, kHeadMaxF);
    GLAM_REQUIRE(e_dim >= 1 && hid >= 1, "glam_pair_head_fwd: e_dim=%d and hid=%d must be at least 1", e_dim, hid);
    GLAM_REQUIRE(act >= 0 && act <= 2, "glam_pair_head_fwd: act=%d is not 0 (none), 1 (relu) or 2 (leaky)", act);
    GLAM_REQUIRE(R >= 0 && R < INT32_MAX && Cs >= 0 && Cs < INT32_MAX, "glam_pair_head_fwd: R / Cs out of range");
    GLAM_REQUIRE(R * Cs < INT32_MAX, "glam_pair_head_fwd: R * Cs out of range");
    GLAM_REQUIRE(lda >= hid && ldb >= hid && ldw >= 2 * (int64_t)hid + F && ldw < INT32_MAX,
                 "glam_pair_head_fwd: a leading dimension is shorter than its row (flat: hid, W0: 2 hid + F)");
    if (R == 0 || Cs == 0) return GLAM_OK;
    GLAM_REQUIRE((R + Cs) * (int64_t)e_dim < INT32_MAX * (int64_t)kBlock, "glam_pair_head_fwd: (R + Cs) * e_dim out of range");
    GLAM_REQUIRE(flat_a && flat_b && W0 && b0 && w1 && b1 && out && (f || F == 0), "glam_pair_head_fwd: null pointer");
    GLAM_REQUIRE((((uintptr_t)flat_a | (uintptr_t)flat_b | (uintptr_t)f | (uintptr_t)W0 | (uintptr_t)b0 | (uintptr_t)w1 | (uintptr_t)b1 |
                   (uintptr_t)out) & 3u) == 0, "glam_pair_head_fwd: operands must be 4-byte aligned");
    const size_t need = glam_pair_head_workspace_bytes(R, Cs, e_dim);
    GLAM_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3u) == 0,
                 "glam_pair_head_fwd: workspace too small or misaligned (glam_pair_head_workspace_bytes)");
    // the lanes take the axis that fills its 64-lane chunks better (the columns on a tie); the other side is the uniform one
    const bool rows_on_lanes = fills_better(R, Cs);
    float* A = (float*)workspace;                          // [R, e_dim], or with the rows on the lanes At [e_dim, R]
    float* B = A + (size_t)R * e_dim;                      // Bt [e_dim, Cs], or with the rows on the lanes B [Cs, e_dim]
    const auto side_blocks = [&](int64_t n, bool trans) {
        const int64_t na = trans ? n : e_dim, nb = trans ? e_dim : n;
        return (int)((na * ((nb + kSideQuad - 1) / kSideQuad) + kBlock - 1) / kBlock);
    };
    const HeadSide sa{flat_a, W0, b0, A, lda, ldw, (int)R, hid, rows_on_lanes, side_blocks(R, rows_on_lanes)};
    const HeadSide sb{flat_b, W0 + hid, nullptr, B, ldb, ldw, (int)Cs, hid, !rows_on_lanes, side_blocks(Cs, !rows_on_lanes)};
    hipLaunchKernelGGL(k_pair_head_side, dim3((unsigned)(sa.blocks + sb.blocks)), dim3(kBlock), 0, (hipStream_t)stream, sa, sb, e_dim);
    GLAM_LAUNCH_CHECK("glam_pair_head_fwd (side)");
    const int64_t nu = rows_on_lanes ? Cs : R, nl = rows_on_lanes ? R : Cs;
    const int64_t lane_chunks = (nl + 63) / 64, groups = (nu + kHeadWaves * kHeadRows - 1) / (kHeadWaves * kHeadRows);
    GLAM_REQUIRE(lane_chunks * groups < INT32_MAX, "glam_pair_head_fwd: grid out of range");
    const head_kernel k = head_table(std::make_integer_sequence<int, kHeadMaxOut * (kHeadMaxF + 1)>())[(out_dim - 1) * (kHeadMaxF + 1) + F];
    GLAM_PROF_LABEL("k_pair_head");
    hipLaunchKernelGGL(k, dim3((unsigned)(lane_chunks * groups)), dim3(kBlock), 0, (hipStream_t)stream, rows_on_lanes ? B : A,
                       rows_on_lanes ? A : B, f, W0 + 2 * (size_t)hid, (int)ldw, w1, b1, e_dim, (int)nu, (int)nl, (int)lane_chunks,
                       rows_on_lanes ? (int64_t)1 : Cs, rows_on_lanes ? Cs : (int64_t)1, act, act == 0 ? 1.f : slope, out);
    GLAM_LAUNCH_CHECK("glam_pair_head_fwd");
    return GLAM_OK;
}
