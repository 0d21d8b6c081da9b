// The core of the streamed-row pair kernels: k_pair_gather (pairgather.hip), k_pair_panel (pairpanel.hip), k_pair_grid (pairgrid.hip) and
// k_pair_map (pairmap.hip).  In each of them one wave holds up to 64 OWNER rows, one per lane, in registers, and the PARTNER rows are
// streamed past the lanes two at a time through wave-uniform loads (why these and not an LDS slice: pairgather.hip).  What the four must
// do ALIKE is here, once: the row load, the score, the partial and its finish kernel, the width table, the slab rule.  The order on
// (value, index) is pair_better of common.h.  What differs stays in the kernels: the loop nest around the score, what is kept of it
// (best and index, or best, row and running sum), and the reduction across lanes.
#pragma once
#include <algorithm>
#include <utility>

#include "common.h"

namespace glam {

constexpr int kStreamChunk = 64;               // owner rows per chunk: one per lane (= PANEL_CHUNK, GRID_CHUNK, MAP_CHUNK of ops_pair.py)
constexpr int kStreamWaves = kBlock / 64;      // waves per block, each with a unit of work of its own: they never meet
constexpr int kStreamMaxD = 128;               // widest row with a kernel
constexpr int kStreamTargetWaves = 4096;       // automatic slab: 256 CUs x 4 SIMDs x 4 waves
constexpr int kStreamMinSlab = 4;

// ---- the lane's owner row: D registers ----
// kVec: D % 4 == 0 and the matrix 16-byte aligned (16-byte loads); otherwise dword loads.
template <int D, bool kVec>
__device__ __forceinline__ void stream_owner_row(const float* prow, float (&pr)[D]) {
    static_assert(D >= 1 && D <= kStreamMaxD && (!kVec || D % 4 == 0), "pair stream: width");
    if constexpr (kVec) {
#pragma unroll
        for (int u = 0; u < D / 4; ++u) {
            const float4 v = ld4g(prow + 4 * u);
            pr[4 * u] = v.x; pr[4 * u + 1] = v.y; pr[4 * u + 2] = v.z; pr[4 * u + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < D; ++c) pr[c] = ld1g(prow + c);
    }
}

// ---- the scores of two streamed rows against the owner row ----
// THE CHAIN.  Every score of the pair fusion family is ONE fmaf chain over channels 0 .. D-1 in ascending order from 0.f (the chain of
// k_pair_max_partial and k_pair_pool_fwd, pairpool_kernels.h; -ffp-contract=off, and the chain is written out), in the 16-byte form as in
// the dword form.  With the total order of pair_better that makes a maximum and its argmax the same bits in every kernel of the family,
// whatever the order of its reduction; and fmaf(a, b, c) = fmaf(b, a, c), so either side of a pair may be the owner.
// row: the first of the two rows, the same in every lane; nothing the launch writes (it is read through the constant address space: the
// scalar unit fetches it once per wave and every multiply-add takes it as its scalar operand).  two == false: d1 is d0 again (an odd
// last row is scored twice; the caller counts it once).
struct StreamScores {
    float d0, d1;
};
template <int D, bool kVec>
__device__ __forceinline__ StreamScores stream_score2(const float* row, bool two, const float (&pr)[D]) {
    glam_cf1* q0 = uniform_cf1(row);
    glam_cf1* q1 = q0 + (two ? D : 0);
    float d0 = 0.f, d1 = 0.f;
    if constexpr (kVec) {
#pragma unroll
        for (int u = 0; u < D / 4; ++u) {
            const glam_v4f v0 = ((glam_cv4*)q0)[u], v1 = ((glam_cv4*)q1)[u];
            d0 = fmaf(v0.x, pr[4 * u], d0); d0 = fmaf(v0.y, pr[4 * u + 1], d0); d0 = fmaf(v0.z, pr[4 * u + 2], d0); d0 = fmaf(v0.w, pr[4 * u + 3], d0);
            d1 = fmaf(v1.x, pr[4 * u], d1); d1 = fmaf(v1.y, pr[4 * u + 1], d1); d1 = fmaf(v1.z, pr[4 * u + 2], d1); d1 = fmaf(v1.w, pr[4 * u + 3], d1);
        }
    } else {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            d0 = fmaf(q0[c], pr[c], d0);
            d1 = fmaf(q1[c], pr[c], d1);
        }
    }
    return {d0, d1};
}

// ---- the width table ----
// A kernel file names its kernel by a tag,  struct K { template <int D, bool kVec> static constexpr auto get() { return &k<D, kVec>; } };
// (a function template cannot be a template argument), and stream_kernel<K>(D, a, b) is the instantiation for a call with matrices a, b.
static inline bool stream_vec(int D, const void* a, const void* b) { return (D & 3) == 0 && aligned16(a) && aligned16(b); }

template <class K>
using stream_fn = decltype(K::template get<1, false>());

// [D - 1] -> the dword instantiation of width D;  [D / 4 - 1] -> the 16-byte one
template <class K, int... I>
static stream_fn<K> stream_dword_table(int D, std::integer_sequence<int, I...>) {
    static const stream_fn<K> t[] = {K::template get<I + 1, false>()...};
    return t[D - 1];
}
template <class K, int... I>
static stream_fn<K> stream_vec_table(int D, std::integer_sequence<int, I...>) {
    static const stream_fn<K> t[] = {K::template get<4 * (I + 1), true>()...};
    return t[D / 4 - 1];
}
template <class K>
static stream_fn<K> stream_kernel(int D, const void* a, const void* b) {      // D in 1 .. kStreamMaxD: the caller's check
    return stream_vec(D, a, b) ? stream_vec_table<K>(D, std::make_integer_sequence<int, kStreamMaxD / 4>())
                               : stream_dword_table<K>(D, std::make_integer_sequence<int, kStreamMaxD>());
}

// ---- slabs (panel, grid): a wave keeps its owner rows for `slab` of the n streamed segments ----
// slab == 0, the automatic one: about kStreamTargetWaves waves where the problem has them, never fewer than kStreamMinSlab segments per wave
static inline int64_t stream_slab(int slab, int64_t n, int64_t total_chunks) {
    const int64_t sl = slab > 0 ? slab : std::max<int64_t>(kStreamMinSlab, (n * total_chunks + kStreamTargetWaves - 1) / kStreamTargetWaves);
    return std::min<int64_t>(sl, n);
}

// ---- partials and their finish (panel, grid) ----
struct PairPartial {       // the best (value, flattened index) of one (streamed segment, run of lanes): written by one vector store
    float v;
    int ix;
};
static_assert(sizeof(PairPartial) == 8, "PairPartial: one 8-byte store");

// One thread per (i, j), i fastest (the partials of a run are read side by side): streamed segment a = rows[i] (kRows; rows == NULL: i)
// or i, owner segment q = cols[j], whose partials are part_ptr[j] .. part_ptr[j + 1] of ws [partial][R], combined in ascending order.
// Mean: <sum1[a], sum2[q]> / (n1 n2), one ascending fmaf chain over the D columns.  (kRows is a template parameter and not the NULL
// alone: the panel, which has no row selection, keeps the registers its own finish kernel had.)
template <bool kRows>
__global__ void __launch_bounds__(kBlock) k_pair_stream_finish(const PairPartial* __restrict__ ws, const int* __restrict__ part_ptr,
                                                              const int* __restrict__ rows, const int* __restrict__ cols,
                                                              const int* __restrict__ ptr1, const int* __restrict__ ptr2,
                                                              const float* __restrict__ sum1, const float* __restrict__ sum2, int R, int Cs,
                                                              int D, float* __restrict__ out, int* __restrict__ arg) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)R * Cs) return;
    const int j = (int)(t / R), i = (int)(t % R);
    const int a = kRows && rows ? rows[i] : i, q = cols[j];
    const int m0 = ptr1[a], n1 = ptr1[a + 1] - m0;
    const int p0 = ptr2[q], n2 = ptr2[q + 1] - p0;
    const size_t o = 2 * ((size_t)i * Cs + j);
    if (n1 <= 0 || n2 <= 0) {
        out[o] = 0.f; out[o + 1] = 0.f;
        if (arg) { arg[o] = -1; arg[o + 1] = -1; }
        return;
    }
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = part_ptr[j]; c < part_ptr[j + 1]; ++c) {
        const PairPartial p = ws[(size_t)c * R + i];
        if (pair_better(p.v, p.ix, best, bidx)) { best = p.v; bidx = p.ix; }
    }
    const float* u = sum1 + (size_t)a * D;
    const float* v = sum2 + (size_t)q * D;
    float tot = 0.f;
    for (int c = 0; c < D; ++c) tot = fmaf(u[c], v[c], tot);
    out[o] = best;
    out[o + 1] = tot / ((float)n1 * (float)n2);
    if (arg) { arg[o] = m0 + bidx / n2; arg[o + 1] = p0 + bidx % n2; }
}

}  // namespace glam
