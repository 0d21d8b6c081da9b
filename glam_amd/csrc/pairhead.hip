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
//
// k_pair_head_classes — the same table read as a classifier, for any out_dim: called class, its log-softmax and selected log-softmaxes,
// the classes walked in tiles (described where it stands, below k_pair_head).
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

// ---------------------------------------------------------------------------------------------------------------------------------
// The class table: the same head for ANY out_dim, ending in the called class and its log-softmax instead of the logits.
//
// k_pair_head_classes keeps the layout of k_pair_head (lanes along one axis, kHeadRows entries of the other per wave, the lane side
// transposed, everything wave-uniform through the constant address space; no LDS, no barrier, no atomics, no cross-lane step) and walks the
// classes in TILES of kClassTile: each tile runs its own serial loop over e, recomputes h (3 + F operations per e against kClassTile
// multiply-adds per entry) and holds kHeadRows x kClassTile accumulators — the registers do not grow with out_dim and out_dim is a runtime
// argument.  The lin_out1 weights come from a transposed, tile-padded copy w1t[e_dim + 1, tpad] (tpad = out_dim rounded up to the tile;
// row e_dim is b1; padded columns are 0 and are never reduced over), written by the SIDE launch: a tile's weights at one e are contiguous
// dwords.  Logit o is k_pair_head's chain bit for bit: acc = b1[o]; acc = fmaf(w1[o, e], h_e, acc), e ascending.
// Per pair, over the classes in ascending order (whatever tile they fall in), from m = logit 0, cls = 0, s = 1:
//   up = x > m || (x is NaN && m is not);  t = expf(-|x - m|);  s = up ? s * t + 1 : s + t;  if (up) m = x, cls = o
// and after the last class lse = m + logf(s), logp = m - lse, sel[k] = logit[classes[k]] - lse.  A NaN logit is the largest (the first
// one wins, as in torch.argmax) and makes s, lse, logp and sel NaN (as torch.log_softmax); of equal logits the smallest index wins.
// Nothing of the table's shape, the lane axis or the selection enters the sequence.
constexpr int kClassTile = 16;                 // classes per pass over e: kHeadRows x kClassTile accumulators in registers
constexpr int kHeadMaxClasses = 1024;
constexpr int kMaxSel = 8;

struct HeadSel { int c[kMaxSel]; };            // the selected classes, by value in the kernel arguments; -1: no class

// k_pair_head_side's two products (the same head_side chains) and, from the blocks after them, w1t: one thread per element of
// [e_dim + 1, tpad].
__global__ void __launch_bounds__(kBlock) k_pair_head_classes_side(HeadSide s0, HeadSide s1, int e_dim, const float* __restrict__ w1,
                                                                  const float* __restrict__ b1, float* __restrict__ w1t, int out_dim,
                                                                  int tpad) {
    const int blk = (int)blockIdx.x;
    if (blk >= s0.blocks + s1.blocks) {
        const int64_t t = (int64_t)(blk - s0.blocks - s1.blocks) * kBlock + threadIdx.x;
        if (t >= (int64_t)(e_dim + 1) * tpad) return;
        const int e = (int)(t / tpad), c = (int)(t % tpad);
        w1t[t] = c >= out_dim ? 0.f : e < e_dim ? w1[(size_t)c * e_dim + e] : b1[c];
        return;
    }
    const bool first = blk < s0.blocks;
    const HeadSide& s = first ? s0 : s1;
    const int64_t t = (int64_t)(first ? blk : blk - s0.blocks) * kBlock + threadIdx.x;
    if (s.trans) head_side<true>(s, e_dim, t);
    else head_side<false>(s, e_dim, t);
}

// One tile's serial loop: head_loop with the weights of classes [c0, c0 + kClassTile) read from row e of w1t.
template <int F, bool kRelu>
__device__ __forceinline__ void class_tile_loop(glam_cf1* const (&ur)[kHeadRows], const float* lt, int nl, glam_cf1* wf, int ldw, glam_cf1* wt,
                                                int tpad, int e_dim, float slope, const float (&fr)[kHeadRows][F > 0 ? F : 1],
                                                float (&acc)[kHeadRows][kClassTile]) {
    float ahead = ld1g(lt);
#pragma unroll 1
    for (int e = 0; e < e_dim; ++e) {
        const float bt = ahead;
        ahead = ld1g(lt + (size_t)min(e + 1, e_dim - 1) * nl);
        glam_cf1* wfe = wf + (size_t)e * ldw;
        glam_cf1* we = wt + (size_t)e * tpad;
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
        for (int o = 0; o < kClassTile; ++o) {
            const float w = we[o];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) acc[r][o] = fmaf(w, h[r], acc[r][o]);
        }
    }
}

// The arguments of k_pair_head with w1t / tpad in place of w1 / b1 and out_dim at run time; the grid is k_pair_head's.
// cls int32 [R, Cs], logp f32 [R, Cs]; sel f32 [R, Cs, n_sel] (unused with n_sel = 0); logits f32 [R, Cs, out_dim] or null.
template <int F, bool kRelu>
__global__ void __launch_bounds__(kBlock) k_pair_head_classes(const float* __restrict__ U, const float* __restrict__ Lt,
                                                             const float* __restrict__ f, const float* __restrict__ Wf, int ldw,
                                                             const float* __restrict__ w1t, int tpad, int e_dim, int out_dim, int nu, int nl,
                                                             int lane_chunks, int64_t su, int64_t sl, float slope, HeadSel sel, int n_sel,
                                                             int* __restrict__ cls, float* __restrict__ logp, float* __restrict__ selo,
                                                             float* __restrict__ logits) {
    static_assert(F >= 0 && F <= kHeadMaxF, "k_pair_head_classes: F");
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
    float m[kHeadRows], s[kHeadRows], sv[kHeadRows][kMaxSel];
    int best[kHeadRows];
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) {
        const int u = min(u0 + r, nu - 1);                 // (past the end: the last one again, not stored)
        ur[r] = uniform_cf1(U + (size_t)u * e_dim);
        pair[r] = (size_t)u * su + (size_t)lr * sl;
#pragma unroll
        for (int k = 0; k < F; ++k) fr[r][k] = ld1g(f + pair[r] * F + k);
#pragma unroll
        for (int k = 0; k < kMaxSel; ++k) sv[r][k] = 0.f;
        m[r] = 0.f, s[r] = 1.f, best[r] = 0;
    }
    glam_cf1* wfu = uniform_cf1(Wf);
    glam_cf1* wt = uniform_cf1(w1t);
#pragma unroll 1
    for (int c0 = 0; c0 < out_dim; c0 += kClassTile) {
        float acc[kHeadRows][kClassTile];
        glam_cf1* bt = wt + (size_t)e_dim * tpad + c0;     // b1, padded
#pragma unroll
        for (int o = 0; o < kClassTile; ++o) {
            const float b = bt[o];
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) acc[r][o] = b;
        }
        class_tile_loop<F, kRelu>(ur, Lt + lr, nl, wfu, ldw, wt + c0, tpad, e_dim, slope, fr, acc);
        // the tile's classes, in order, into the running maximum / first index / sum (all conditions on c0 are wave-uniform)
#pragma unroll
        for (int o = 0; o < kClassTile; ++o) {
            if (c0 + o >= out_dim) break;
            if (c0 + o == 0) {
#pragma unroll
                for (int r = 0; r < kHeadRows; ++r) m[r] = acc[r][0];
                continue;
            }
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) {
                const float x = acc[r][o];
                const bool up = x > m[r] || (x != x && m[r] == m[r]);
                const float t = expf(-fabsf(x - m[r]));
                s[r] = up ? s[r] * t + 1.f : s[r] + t;
                m[r] = up ? x : m[r];
                best[r] = up ? c0 + o : best[r];
            }
        }
#pragma unroll
        for (int k = 0; k < kMaxSel; ++k) {
            const int d = sel.c[k] - c0;
            if ((unsigned)d < (unsigned)kClassTile) {
#pragma unroll
                for (int o = 0; o < kClassTile; ++o)
                    if (d == o) {
#pragma unroll
                        for (int r = 0; r < kHeadRows; ++r) sv[r][k] = acc[r][o];
                    }
            }
        }
        if (logits) {
#pragma unroll
            for (int r = 0; r < kHeadRows; ++r) {
                if (valid && u0 + r < nu) {
#pragma unroll
                    for (int o = 0; o < kClassTile; ++o)
                        if (c0 + o < out_dim) st1g(logits + pair[r] * (size_t)out_dim + c0 + o, acc[r][o]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r) {
        if (valid && u0 + r < nu) {
            const float lse = m[r] + logf(s[r]);
            cls[pair[r]] = best[r];
            st1g(logp + pair[r], m[r] - lse);
#pragma unroll
            for (int k = 0; k < kMaxSel; ++k)
                if (k < n_sel) st1g(selo + pair[r] * (size_t)n_sel + k, sv[r][k] - lse);
        }
    }
}

typedef void (*class_kernel)(const float*, const float*, const float*, const float*, int, const float*, int, int, int, int, int, int, int64_t,
                             int64_t, float, HeadSel, int, int*, float*, float*, float*);

// [2 * F + relu] -> the instantiation of (F, relu)
template <int... I>
static const class_kernel* class_table(std::integer_sequence<int, I...>) {
    static const class_kernel t[] = {k_pair_head_classes<I / 2, (I % 2) != 0>...};
    return t;
}

static inline int64_t class_tpad(int out_dim) { return ((int64_t)out_dim + kClassTile - 1) / kClassTile * kClassTile; }

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

extern "C" size_t glam_pair_head_classes_workspace_bytes(int64_t R, int64_t Cs, int e_dim, int out_dim) {
    if (R <= 0 || Cs <= 0 || e_dim <= 0 || out_dim <= 0) return 0;
    return (((size_t)R + (size_t)Cs) * (size_t)e_dim + ((size_t)e_dim + 1) * (size_t)class_tpad(out_dim)) * sizeof(float);
}

extern "C" int glam_pair_head_classes_fwd(const float* flat_a, int64_t lda, const float* flat_b, int64_t ldb, const float* f, int64_t R,
                                          int64_t Cs, int hid, int F, const float* W0, int64_t ldw, const float* b0, int e_dim,
                                          const float* w1, const float* b1, int out_dim, int act, float slope, const int* classes, int n_sel,
                                          void* workspace, size_t workspace_bytes, int* cls, float* logp, float* sel, float* logits,
                                          void* stream) {
    const char* const me = "glam_pair_head_classes_fwd";
    GLAM_REQUIRE(out_dim >= 2 && out_dim <= kHeadMaxClasses, "%s: out_dim=%d not in 2..%d", me, out_dim, kHeadMaxClasses);
    GLAM_REQUIRE(F >= 0 && F <= kHeadMaxF, "%s: F=%d fusion columns not in 0..%d", me, F, kHeadMaxF);
    GLAM_REQUIRE(e_dim >= 1 && hid >= 1, "%s: e_dim=%d and hid=%d must be at least 1", me, e_dim, hid);
    GLAM_REQUIRE(act >= 0 && act <= 2, "%s: act=%d is not 0 (none), 1 (relu) or 2 (leaky)", me, act);
    GLAM_REQUIRE(n_sel >= 0 && n_sel <= kMaxSel, "%s: n_sel=%d selected classes not in 0..%d", me, n_sel, kMaxSel);
    GLAM_REQUIRE(n_sel == 0 || classes, "%s: n_sel=%d without the classes", me, n_sel);
    HeadSel hs;
    for (int k = 0; k < kMaxSel; ++k) hs.c[k] = -1;
    for (int k = 0; k < n_sel; ++k) {                      // (a HOST array: read here, passed on by value)
        GLAM_REQUIRE(classes[k] >= 0 && classes[k] < out_dim, "%s: classes[%d]=%d not in [0, %d)", me, k, classes[k], out_dim);
        hs.c[k] = classes[k];
    }
    GLAM_REQUIRE(R >= 0 && R < INT32_MAX && Cs >= 0 && Cs < INT32_MAX, "%s: R / Cs out of range", me);
    GLAM_REQUIRE(R * Cs < INT32_MAX, "%s: R * Cs out of range", me);
    GLAM_REQUIRE(lda >= hid && ldb >= hid && ldw >= 2 * (int64_t)hid + F && ldw < INT32_MAX,
                 "%s: a leading dimension is shorter than its row (flat: hid, W0: 2 hid + F)", me);
    if (R == 0 || Cs == 0) return GLAM_OK;
    GLAM_REQUIRE((R + Cs) * (int64_t)e_dim < INT32_MAX * (int64_t)kBlock, "%s: (R + Cs) * e_dim out of range", me);
    GLAM_REQUIRE(flat_a && flat_b && W0 && b0 && w1 && b1 && cls && logp && (f || F == 0) && (sel || n_sel == 0), "%s: null pointer", me);
    GLAM_REQUIRE((((uintptr_t)flat_a | (uintptr_t)flat_b | (uintptr_t)f | (uintptr_t)W0 | (uintptr_t)b0 | (uintptr_t)w1 | (uintptr_t)b1 |
                   (uintptr_t)cls | (uintptr_t)logp | (uintptr_t)sel | (uintptr_t)logits) & 3u) == 0, "%s: operands must be 4-byte aligned", me);
    const size_t need = glam_pair_head_classes_workspace_bytes(R, Cs, e_dim, out_dim);
    GLAM_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3u) == 0,
                 "%s: workspace too small or misaligned (glam_pair_head_classes_workspace_bytes)", me);
    // the lane axis and the two products: as in glam_pair_head_fwd
    const bool rows_on_lanes = fills_better(R, Cs);
    float* A = (float*)workspace;
    float* B = A + (size_t)R * e_dim;
    float* w1t = B + (size_t)Cs * e_dim;                   // [e_dim + 1, tpad]: lin_out1's weight transposed, then its bias
    const int tpad = (int)class_tpad(out_dim);
    const auto side_blocks = [&](int64_t n, bool trans) {
        const int64_t na = trans ? n : e_dim, nb = trans ? e_dim : n;
        return (int)((na * ((nb + kSideQuad - 1) / kSideQuad) + kBlock - 1) / kBlock);
    };
    const HeadSide sa{flat_a, W0, b0, A, lda, ldw, (int)R, hid, rows_on_lanes, side_blocks(R, rows_on_lanes)};
    const HeadSide sb{flat_b, W0 + hid, nullptr, B, ldb, ldw, (int)Cs, hid, !rows_on_lanes, side_blocks(Cs, !rows_on_lanes)};
    const int64_t wt_blocks = (((int64_t)e_dim + 1) * tpad + kBlock - 1) / kBlock;
    GLAM_REQUIRE(sa.blocks + (int64_t)sb.blocks + wt_blocks < INT32_MAX, "%s: grid out of range", me);
    hipLaunchKernelGGL(k_pair_head_classes_side, dim3((unsigned)(sa.blocks + sb.blocks + wt_blocks)), dim3(kBlock), 0, (hipStream_t)stream, sa,
                       sb, e_dim, w1, b1, w1t, out_dim, tpad);
    GLAM_LAUNCH_CHECK("glam_pair_head_classes_fwd (side)");
    const int64_t nu = rows_on_lanes ? Cs : R, nl = rows_on_lanes ? R : Cs;
    const int64_t lane_chunks = (nl + 63) / 64, groups = (nu + kHeadWaves * kHeadRows - 1) / (kHeadWaves * kHeadRows);
    GLAM_REQUIRE(lane_chunks * groups < INT32_MAX, "%s: grid out of range", me);
    const class_kernel k = class_table(std::make_integer_sequence<int, 2 * (kHeadMaxF + 1)>())[2 * F + (act == 1)];
    GLAM_PROF_LABEL("k_pair_head_classes");
    hipLaunchKernelGGL(k, dim3((unsigned)(lane_chunks * groups)), dim3(kBlock), 0, (hipStream_t)stream, rows_on_lanes ? B : A,
                       rows_on_lanes ? A : B, f, W0 + 2 * (size_t)hid, (int)ldw, w1t, tpad, e_dim, out_dim, (int)nu, (int)nl, (int)lane_chunks,
                       rows_on_lanes ? (int64_t)1 : Cs, rows_on_lanes ? Cs : (int64_t)1, act == 0 ? 1.f : act == 1 ? 0.f : slope, hs, n_sel,
                       cls, logp, sel, logits);
    GLAM_LAUNCH_CHECK("glam_pair_head_classes_fwd");
    return GLAM_OK;
}
