// Interaction maps: the two MARGINALS of the score matrix of the fusion, S = x1[seg a] @ x2[seg b]^T, for every pair and both sides —
//   side 1, per row r1 of segment a:  max1 = max_r2 S,  arg1 = row of x2 of the smallest r2 that attains it,  mean1 = sum_r2 S / n2
//   side 2, per row r2 of segment b:  max2 = max_r1 S,  arg2 = row of x1 of the smallest r1 that attains it,  mean2 = sum_r1 S / n1
// — without S ever being stored.  The outputs are ragged and pair-major: the rows of pair i on side k are out_ptr_k[i] .. out_ptr_k[i + 1]
// (ops.map_plan).  An empty partner segment gives max = 0, mean = 0, arg = -1 (the fusion's own rule for an empty pair).
//
// Shape.  A work item is (pair, side, chunk of up to 64 OWNER rows); one wave runs one item, kBlock / 64 items per block, as in
// pairgather.hip: no block-wide barrier, no shared memory, no workspace, no atomics, ONE launch for both sides.
//   owner rows:   a lane holds its row in registers;
//   partner rows: the whole partner segment is streamed past the lanes in ascending row order, two rows at a time, through WAVE-UNIFORM
//       loads (the constant address space: the scalar unit fetches a row once per wave — see pairgather.hip for why not LDS), which needs
//       the width as a compile-time constant: the kernel is instantiated per width (D = 1..128), 16-byte and dword forms.
// The side is a wave-uniform swap of the two base pointers, not a second kernel: s(r1, r2) is the chain of stream_score2 (pairstream.h), and
// fmaf(a, b, c) = fmaf(b, a, c), so either side may own.
// Maximum: a strict > in ascending stream order keeps the first row that attains it: no index compare.  max over a pair's max1 rows (or
// max2 rows) is therefore bit for bit the max column of the fusion kernels, and the first such row with its arg1 is their argmax.
// Mean: the lane adds every score to a running sum in stream order — a fixed order, the same bits on every run.
#include "pairstream.h"

namespace glam {

// work: int32[n_items, 4] = (a, b, 2 * chunk + side, first output row of the chunk); side 0: segment a of x1 owns, 1: segment b of x2.
// kVec: D % 4 == 0 and both matrices 16-byte aligned (16-byte loads); otherwise dword loads.  The table is trusted.
template <int D, bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_map(const float* __restrict__ x1, const float* __restrict__ x2,
                                                    const int* __restrict__ ptr1, const int* __restrict__ ptr2,
                                                    const int* __restrict__ work, int n_items,
                                                    float* __restrict__ max1, int* __restrict__ arg1, float* __restrict__ mean1,
                                                    float* __restrict__ max2, int* __restrict__ arg2, float* __restrict__ mean2) {
    const int lane = threadIdx.x & 63;
    const int it = blockIdx.x * kStreamWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (it >= n_items) return;                            // a wave without an item (no barrier below: the others go on)
    const int a = __builtin_amdgcn_readfirstlane(work[4 * (size_t)it]), b = __builtin_amdgcn_readfirstlane(work[4 * (size_t)it + 1]);
    const int sc = __builtin_amdgcn_readfirstlane(work[4 * (size_t)it + 2]), o0 = __builtin_amdgcn_readfirstlane(work[4 * (size_t)it + 3]);
    const int m0 = __builtin_amdgcn_readfirstlane(ptr1[a]), n1 = __builtin_amdgcn_readfirstlane(ptr1[a + 1]) - m0;
    const int p0 = __builtin_amdgcn_readfirstlane(ptr2[b]), n2 = __builtin_amdgcn_readfirstlane(ptr2[b + 1]) - p0;
    // ---- the side: which matrix owns (a row per lane) and which is streamed ----
    const bool second = (sc & 1) != 0;
    const float* xo = second ? x2 : x1;
    const float* xp = second ? x1 : x2;
    const int ob = second ? p0 : m0, on = second ? n2 : n1;          // owner segment: first row, rows
    const int pb = second ? m0 : p0, pn = second ? n1 : n2;          // partner segment
    float* omax = second ? max2 : max1;
    int* oarg = second ? arg2 : arg1;
    float* omean = second ? mean2 : mean1;
    const int c0 = (sc >> 1) * kStreamChunk;                          // first owner row of the chunk, inside its segment (< on)
    const bool valid = c0 + lane < on;
    const size_t o = (size_t)o0 + lane;
    if (pn <= 0) {                                                    // empty partner: the fill
        if (valid) { omax[o] = 0.f; omean[o] = 0.f; oarg[o] = -1; }
        return;
    }
    const float* prow = xo + (size_t)(ob + c0 + (valid ? lane : 0)) * D;      // (a lane past the end reads the chunk's first row and stores nothing)
    float pr[D];
    stream_owner_row<D, kVec>(prow, pr);
    float best = -INFINITY, sum = 0.f;
    int brow = 0;
    for (int r = 0; r < pn; r += 2) {
        const bool two = r + 1 < pn;                       // (an odd last row is scored twice and counted once)
        const auto [d0, d1] = stream_score2<D, kVec>(xp + (size_t)(pb + r) * D, two, pr);
        // (strict >, ascending r: a later row that only ties never takes the place of an earlier one)
        if (d0 > best) { best = d0; brow = r; }
        sum += d0;
        if (two) {                                         // (wave-uniform: the row loads above stay so)
            if (d1 > best) { best = d1; brow = r + 1; }
            sum += d1;
        }
    }
    if (valid) {
        omax[o] = best;
        oarg[o] = pb + brow;
        omean[o] = sum / (float)pn;
    }
}

struct MapKernel { template <int D, bool kVec> static constexpr auto get() { return &k_pair_map<D, kVec>; } };

}  // namespace glam

using namespace glam;

extern "C" int glam_pair_map_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* work,
                                 int64_t n_items, int D, float* max1, int32_t* arg1, float* mean1, float* max2, int32_t* arg2,
                                 float* mean2, void* stream) {
    const char* who = "glam_pair_map_fwd";
    GLAM_REQUIRE(n_items >= 0 && n_items < INT32_MAX,"%s: n_items out of range", who);
    if (D <= 0 || D > kStreamMaxD) return fail(GLAM_E_UNSUPPORTED, "%s: D=%d not in 1..%d", who, D, kStreamMaxD);
    if (n_items == 0) return GLAM_OK;
    GLAM_REQUIRE(x1 && x2 && ptr1 && ptr2 && work && max1 && arg1 && mean1 && max2 && arg2 && mean2, "%s: null pointer", who);
    GLAM_REQUIRE(((uintptr_t)x1 & 3u) == 0 && ((uintptr_t)x2 & 3u) == 0, "%s: rows must be 4-byte aligned", who);
    const auto k = stream_kernel<MapKernel>(D, x1, x2);
    GLAM_PROF_LABEL("k_pair_map");
    hipLaunchKernelGGL(k, dim3((unsigned)((n_items + kStreamWaves - 1) / kStreamWaves)), dim3(kBlock), 0, (hipStream_t)stream, x1, x2, ptr1,
                       ptr2, work, (int)n_items, max1, arg1, mean1, max2, arg2, mean2);
    GLAM_LAUNCH_CHECK(who);
    return GLAM_OK;
}
