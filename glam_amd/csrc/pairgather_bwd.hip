// Backward of the doubly indexed fusion of pairgather.hip (drug x drug, BOTH sides held once): DDI training on shared drugs.
//   forward   glam_pair_pool_gather_train_fwd (pairgather.hip): k_pair_gather, which there also stores the two column sums its wave holds.
//   backward  glam_pair_pool_gather_bwd, ONE launch: one wave owns one (side, drug) — waves 0 .. Q1-1 the drugs of x1, waves Q1 .. Q1+Q2-1
//             those of x2, four waves per block.  The sides write disjoint outputs and read only forward results: nothing orders them.
//             For drug q of a side the host hands q's pairs in batch order (order / list_ptr: PairIndex.by_protein of that side's index):
//               S        = 0, + gmean_i * colsum_i(partner segment) for the pairs i of q, in list order      (the same for every row of q)
//               d_x[r]   = S, then fmaf(gmax_i, partner[ap_i], .) for the pairs of q whose maximum sits on row r, in list order, + add[r] last
//             No atomics; the order depends on the lists alone, never on the grid or on timing.  A drug no pair references gets S = 0.
// The waves of a block own different drugs and differ in trip count: there is no block-wide barrier and no shared memory in this file.
// A pair list is walked in tiles of 64 held in REGISTERS: lane k loads what is wave-uniform about pair k of the tile (its number, gmean,
// gmax, both argmax rows; -1 for an empty pair), the wave reads those values as broadcasts (v_readlane).  The [tile, D] addends are loaded
// kGbRound pairs a round, every load independent of the others; only the add chain is serial.  The fmaf terms of a row group go four a
// round the same way.  Nothing here is read through the constant address space but what the compiler proves uniform among the read-only
// operands (segment offsets, list offsets); add1 / add2 (written by the launch before this one) and the outputs are never marked read-only
// and are addressed per lane: vector loads and plain vector stores.
#include "common.h"

namespace glam {

constexpr int kGbWaves = kBlock / 64;      // (side, drug) waves per block
constexpr int kGbMaxD = 128;
constexpr int kGbTile = 64;                // pairs per staged tile: one per lane
constexpr int kGbRound = 8;                // addends of the common term in flight per lane
constexpr int kGbHits = 4;                 // fmaf addends in flight per lane

// what lane k holds of pair k of the staged tile
struct GbMeta {
    int i;          // pair number, -1: an empty pair or no pair (contributes nothing)
    float gmean;    // d_out[i, 1] / (n1 * n2)
    float gmax;     // d_out[i, 0]
    int own;        // row of the maximum in this side's matrix (-1 with i)
    int oth;        // ... in the partner's matrix (a row that exists, also for an empty pair: it is only loaded then)
};

__device__ __forceinline__ float gb_bcast(float v, int k) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k)); }
__device__ __forceinline__ int gb_bcast(int v, int k) { return __builtin_amdgcn_readlane(v, k); }

// A lane's NV values of a row: 16-byte form — columns 4 cg .. 4 cg + 3; dword form — columns cg and cg + 64.  A column past D is read
// from column 0 (in bounds) and never stored.
template <bool kVec>
__device__ __forceinline__ void gb_load(const float* row, int cg, int D, float* t) {
    if constexpr (kVec) {
        const float4 v = ld4g(row + (4 * cg < D ? 4 * cg : 0));
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    } else {
        t[0] = ld1g(row + (cg < D ? cg : 0));
        t[1] = ld1g(row + (cg + 64 < D ? cg + 64 : 0));
    }
}

template <bool kVec>
__device__ __forceinline__ void gb_store(float* row, int cg, int D, const float* v) {
    if constexpr (kVec) {
        if (4 * cg < D) st4g(row + 4 * cg, make_float4(v[0], v[1], v[2], v[3]));
    } else {
        if (cg < D) st1g(row + cg, v[0]);
        if (cg + 64 < D) st1g(row + cg + 64, v[1]);
    }
}

// G lanes per row (kVec: 16 for D <= 64, 32 above; dword form: all 64), 64 / G rows of the drug per sweep
template <int G, bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_gather_bwd(
    const float* __restrict__ x1, const float* __restrict__ x2, const int* __restrict__ ptr1, const int* __restrict__ ptr2,
    const int* __restrict__ idx1, const int* __restrict__ idx2, const int* __restrict__ order1, const int* __restrict__ lptr1,
    const int* __restrict__ order2, const int* __restrict__ lptr2, const int* __restrict__ arg, const float* __restrict__ sums,
    const float* __restrict__ d_out, int Q1, int Q2, int D, const float* add1, const float* add2, float* d_x1, float* d_x2) {
    static_assert(kVec ? (G == 16 || G == 32) : G == 64, "k_pair_gather_bwd: lanes per row");
    constexpr int NV = kVec ? 4 : 2, R = 64 / G;
    const int lane = threadIdx.x & 63, cg = lane & (G - 1), rg = lane / G;
    const int w = blockIdx.x * kGbWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= Q1 + Q2) return;                              // a wave without a drug (no barrier below: the others go on)
    const bool second = w >= Q1;
    const int q = second ? w - Q1 : w;
    const int so = second ? 0 : 1;                         // the partner's half of sums[i] and its column of arg[i]
    const float* xt = second ? x1 : x2;                    // the partner's rows
    const int* optr = second ? ptr1 : ptr2;
    const int* oidx = second ? idx1 : idx2;
    const int* sptr = second ? ptr2 : ptr1;
    const int* order = second ? order2 : order1;
    const int* lptr = second ? lptr2 : lptr1;
    const float* add = second ? add2 : add1;
    float* dx = second ? d_x2 : d_x1;
    const int r0 = __builtin_amdgcn_readfirstlane(sptr[q]), r1 = __builtin_amdgcn_readfirstlane(sptr[q + 1]), ns = r1 - r0;
    if (ns <= 0) return;                                   // no row to write
    const int k0 = __builtin_amdgcn_readfirstlane(lptr[q]), k1 = __builtin_amdgcn_readfirstlane(lptr[q + 1]);

    GbMeta m;
    auto stage = [&](int t0) {
        const int k = t0 + lane;
        const bool in = k < k1;
        const int i = in ? order[k] : order[k1 - 1];       // (a lane past the list reads the last pair and drops it)
        const int b = oidx ? oidx[i] : i;
        const int no = optr[b + 1] - optr[b];
        const bool empty = !in || no <= 0;
        const float nn = second ? (float)no * (float)ns : (float)ns * (float)no;       // (float)n1 * (float)n2, the forward's product
        m.i = empty ? -1 : i;
        m.gmean = empty ? 0.f : d_out[2 * (size_t)i + 1] / nn;
        m.gmax = d_out[2 * (size_t)i];
        m.own = empty ? -1 : arg[2 * (size_t)i + 1 - so];
        m.oth = empty ? 0 : arg[2 * (size_t)i + so];
    };
    const bool one = k1 - k0 <= kGbTile;                   // the usual case: staged once for both walks
    m.i = -1; m.gmean = 0.f; m.gmax = 0.f; m.own = -1; m.oth = 0;
    if (one && k1 > k0) stage(k0);

    // ---- the common term: gmean_i * (column sums of the partner segment of pair i), pairs in list order ----
    float S[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) S[j] = 0.f;
    for (int t0 = k0; t0 < k1; t0 += kGbTile) {
        if (!one) stage(t0);
        const int tn = min(kGbTile, k1 - t0);
        for (int kb = 0; kb < tn; kb += kGbRound) {
            float t[kGbRound][NV], gm[kGbRound];
            bool ok[kGbRound];
#pragma unroll
            for (int u = 0; u < kGbRound; ++u) {
                const int kk = min(kb + u, tn - 1);
                const int i = gb_bcast(m.i, kk);
                ok[u] = kb + u < tn && i >= 0;
                gm[u] = gb_bcast(m.gmean, kk);
                gb_load<kVec>(sums + ((size_t)max(i, 0) * 2 + so) * D, cg, D, t[u]);
            }
#pragma unroll
            for (int u = 0; u < kGbRound; ++u)
#pragma unroll
                for (int j = 0; j < NV; ++j) S[j] = ok[u] ? S[j] + gm[u] * t[u][j] : S[j];
        }
    }

    // ---- rows: S, then the fmaf terms of the pairs whose maximum sits on the row, in list order, then add ----
    for (int rb = r0; rb < r1; rb += R) {
        const int r = rb + rg;
        float v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = S[j];
        for (int t0 = k0; t0 < k1; t0 += kGbTile) {
            if (!one) stage(t0);
            unsigned long long left = __ballot(m.own >= rb && m.own < rb + R);
            while (left) {
                float t[kGbHits][NV], g[kGbHits];
                bool mine[kGbHits];
                const int first = __builtin_ctzll(left);
#pragma unroll
                for (int u = 0; u < kGbHits; ++u) {
                    const bool has = left != 0;
                    const int kk = has ? __builtin_ctzll(left) : first;
                    left &= left - 1;                      // (0 stays 0)
                    mine[u] = has && gb_bcast(m.own, kk) == r;
                    g[u] = gb_bcast(m.gmax, kk);
                    gb_load<kVec>(xt + (size_t)gb_bcast(m.oth, kk) * D, cg, D, t[u]);
                }
#pragma unroll
                for (int u = 0; u < kGbHits; ++u)
#pragma unroll
                    for (int j = 0; j < NV; ++j) v[j] = mine[u] ? fmaf(g[u], t[u][j], v[j]) : v[j];
            }
        }
        if (r < r1) {
            if (add) {
                float t[NV];
                gb_load<kVec>(add + (size_t)r * D, cg, D, t);
#pragma unroll
                for (int j = 0; j < NV; ++j) v[j] += t[j];
            }
            gb_store<kVec>(dx + (size_t)r * D, cg, D, v);
        }
    }
}

}  // namespace glam

using namespace glam;

// order1 / list_ptr1: the pairs stably sorted by idx1 and the Q1 + 1 offsets of the drugs' runs (PairIndex.by_protein of that side; with
// idx1 == NULL the identity lists); order2 / list_ptr2 the same for side 2.  Built and checked by the host, trusted here, like idx1 / idx2.
extern "C" int glam_pair_pool_gather_bwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* idx1,
                                         const int32_t* idx2, const int32_t* order1, const int32_t* list_ptr1, const int32_t* order2,
                                         const int32_t* list_ptr2, const int32_t* argmax, const float* sums, const float* d_out, int64_t P,
                                         int64_t Q1, int64_t Q2, int D, const float* add1, const float* add2, float* d_x1, float* d_x2,
                                         void* stream) {
    GLAM_REQUIRE(P >= 0 && P < INT32_MAX, "glam_pair_pool_gather_bwd: P out of range");
    GLAM_REQUIRE(Q1 >= 0 && Q2 >= 0 && Q1 + Q2 < INT32_MAX, "glam_pair_pool_gather_bwd: Q1 / Q2 out of range");
    if (D <= 0 || D > kGbMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_gather_bwd: D=%d not in 1..%d", D, kGbMaxD);
    if (P == 0) return GLAM_OK;                 // (nothing is written: the caller's zeros stand)
    GLAM_REQUIRE(Q1 > 0 && Q2 > 0, "glam_pair_pool_gather_bwd: pairs but no segment on one side");
    GLAM_REQUIRE(idx1 || Q1 == P, "glam_pair_pool_gather_bwd: idx1 = NULL pairs i with segment i of x1: needs Q1 == P");
    GLAM_REQUIRE(idx2 || Q2 == P, "glam_pair_pool_gather_bwd: idx2 = NULL pairs i with segment i of x2: needs Q2 == P");
    GLAM_REQUIRE(x1 && x2 && ptr1 && ptr2 && order1 && list_ptr1 && order2 && list_ptr2 && argmax && sums && d_out && d_x1 && d_x2,
                 "glam_pair_pool_gather_bwd: null pointer");
    const void* f32s[] = {x1, x2, sums, d_out, add1, add2, d_x1, d_x2};
    bool vec = (D & 3) == 0;
    for (const void* p : f32s) {
        GLAM_REQUIRE(((uintptr_t)p & 3u) == 0, "glam_pair_pool_gather_bwd: rows must be 4-byte aligned");
        vec = vec && (p == d_out || aligned16(p));
    }
    const dim3 grid((unsigned)((Q1 + Q2 + kGbWaves - 1) / kGbWaves));
#define GLAM_GB_LAUNCH(G, V)                                                                                                              \
    hipLaunchKernelGGL((k_pair_gather_bwd<G, V>), grid, dim3(kBlock), 0, (hipStream_t)stream, x1, x2, ptr1, ptr2, idx1, idx2, order1,     \
                       list_ptr1, order2, list_ptr2, argmax, sums, d_out, (int)Q1, (int)Q2, D, add1, add2, d_x1, d_x2)
    GLAM_PROF_LABEL("k_pair_gather_bwd");
    if (!vec) GLAM_GB_LAUNCH(64, false);
    else if (D <= 64) GLAM_GB_LAUNCH(16, true);
    else GLAM_GB_LAUNCH(32, true);
#undef GLAM_GB_LAUNCH
    GLAM_LAUNCH_CHECK("glam_pair_pool_gather_bwd");
    return GLAM_OK;
}
