// Doubly indexed fusion of two SMALL segments (drug x drug): for pair i with a = idx1[i], b = idx2[i],
//   S = x1[ptr1[a]:ptr1[a+1]] @ x2[ptr2[b]:ptr2[b+1]]^T,  out[i] = [max S, mean S],  arg[i] = (row of x1, row of x2) of the maximum.
// Both matrices hold every drug ONCE (ArchitectureDDI.encode_drugs); a pair is two indices, no rows are gathered or collated.
//
// Shape.  The fusion kernels of pairpool.hip are cut for proteins: 16 blocks of 64 residue lanes per pair plus a finish launch.  Two
// molecules of 20-40 atoms fill ONE wave's 64 lanes once, so here a pair is one wave: four pairs per 256-thread block, ceil(P / 4)
// blocks, no workspace, no second launch, no atomics.  The four waves of a block own different pairs and never meet: there is no
// block-wide barrier and no shared memory in this file.
//   second segment: a lane owns one of its rows in registers, 64 rows per chunk (a longer segment loops over chunks);
//   first segment:  its rows are streamed past the lanes two at a time through WAVE-UNIFORM loads (the constant address space: the
//       scalar unit fetches the row once per wave and every multiply-add takes it as its scalar operand).  The alternative, a per-wave
//       LDS slice, costs a ds_read_b128 per four multiply-adds in each of the four waves of a CU — the one LDS pipe would be the
//       limit — plus a write -> read ordering inside the wave to argue about; the scalar route has neither, and a drug that many
//       pairs reference stays in the scalar cache.  Its price is that the row width must be a compile-time constant, or the loads would
//       sit behind per-chunk guards and each would expose its latency: the kernel is instantiated per width (D = 1..128).
// Maximum: the chain of stream_score2 (pairstream.h) and the total order of pair_better (common.h): the max column and the argmax are
// bit for bit those of glam_pair_pool_fwd on physically gathered rows whatever the order of the reduction.
// Mean: sum(S) = <sum of rows of segment 1, sum of rows of segment 2>; lane c keeps columns c and c + 64 of both sums (rows added in
// ascending order), the products are summed by the fixed butterfly of group_sum<64>: the same bits on every run.
// Training (glam_pair_pool_gather_train_fwd): the same kernel also stores those two column sums (sums[i] = [s1 | s2]) for the backward of
// pairgather_bwd.hip — a runtime pointer, NULL in the inference call, not a second template axis.
#include "pairstream.h"

namespace glam {

// column c of the sums of rows [m0, m0 + n1) of x1 and [p0, p0 + n2) of x2, rows in ascending order.  Both segments go eight rows a
// round, sixteen loads in flight; a row past the end of a segment is read from the segment's last row (in bounds) and adds 0.  (On
// 20-atom molecules this measured the same as one segment after the other, four loads in flight: 11.6 against 11.5 us per launch; it
// is here for long segments — 130 rows are 17 dependent rounds instead of 66 — which were not timed.)
template <int D>
__device__ __forceinline__ void gather_colsums(const float* x1, int m0, int n1, const float* x2, int p0, int n2, int c, float& s1, float& s2) {
    const float* a = x1 + (size_t)m0 * D + c;
    const float* b = x2 + (size_t)p0 * D + c;
    s1 = 0.f;
    s2 = 0.f;
    for (int r = 0; r < max(n1, n2); r += 8) {
        float v[8], w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = ld1g(a + (size_t)min(r + k, n1 - 1) * D);
            w[k] = ld1g(b + (size_t)min(r + k, n2 - 1) * D);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s1 += r + k < n1 ? v[k] : 0.f;
            s2 += r + k < n2 ? w[k] : 0.f;
        }
    }
}

// kVec: D % 4 == 0 and both matrices 16-byte aligned (16-byte loads); otherwise dword loads.  The indices are trusted.
template <int D, bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_gather(const float* __restrict__ x1, const float* __restrict__ x2,
                                                       const int* __restrict__ ptr1, const int* __restrict__ ptr2,
                                                       const int* __restrict__ idx1, const int* __restrict__ idx2, int P,
                                                       float* __restrict__ out, int* __restrict__ arg, float* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kStreamWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= P) return;                                   // a wave without a pair (no barrier below: the others go on)
    const int a = idx1 ? idx1[i] : i, b = idx2 ? idx2[i] : i;
    const int m0 = __builtin_amdgcn_readfirstlane(ptr1[a]), n1 = __builtin_amdgcn_readfirstlane(ptr1[a + 1]) - m0;
    const int p0 = __builtin_amdgcn_readfirstlane(ptr2[b]), n2 = __builtin_amdgcn_readfirstlane(ptr2[b + 1]) - p0;
    if (n1 <= 0 || n2 <= 0) {
        if (lane == 0) {
            out[2 * (size_t)i] = 0.f; out[2 * (size_t)i + 1] = 0.f;
            if (arg) { arg[2 * (size_t)i] = -1; arg[2 * (size_t)i + 1] = -1; }
        }
        return;
    }
    // ---- mean: <column sums of segment 1, column sums of segment 2> ----
    // (sums, f32[P,2,D] or NULL: the training forward keeps the two column sums for the backward's common term)
    float t = 0.f, s1, s2;
    if (lane < D) {
        gather_colsums<D>(x1, m0, n1, x2, p0, n2, lane, s1, s2);
        t = s1 * s2;
        if (sums) { sums[(size_t)i * 2 * D + lane] = s1; sums[(size_t)i * 2 * D + D + lane] = s2; }
    }
    if (D > 64 && lane + 64 < D) {
        gather_colsums<D>(x1, m0, n1, x2, p0, n2, lane + 64, s1, s2);
        t = fmaf(s1, s2, t);
        if (sums) { sums[(size_t)i * 2 * D + lane + 64] = s1; sums[(size_t)i * 2 * D + D + lane + 64] = s2; }
    }
    const float tot = group_sum<64>(t);
    // ---- maximum ----
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c0 = 0; c0 < n2; c0 += 64) {
        const int r2 = c0 + lane;
        const bool valid = r2 < n2;
        const float* prow = x2 + (size_t)(p0 + (valid ? r2 : 0)) * D;      // (a lane past the end reads row 0 and drops its scores)
        float pr[D];
        stream_owner_row<D, kVec>(prow, pr);
        for (int r1 = 0; r1 < n1; r1 += 2) {
            const bool two = r1 + 1 < n1;                  // (an odd last row is scored twice and counted once)
            const auto [d0, d1] = stream_score2<D, kVec>(x1 + (size_t)(m0 + r1) * D, two, pr);
            // (selects, not a branch on `valid`: under a divergent branch the row loads above would stop being wave-uniform)
            const float s0 = valid ? d0 : -INFINITY, s1 = valid && two ? d1 : -INFINITY;
            const int i0 = valid ? r1 * n2 + r2 : 0x7fffffff, i1 = valid && two ? i0 + n2 : 0x7fffffff;
            if (pair_better(s0, i0, best, bidx)) { best = s0; bidx = i0; }
            if (pair_better(s1, i1, best, bidx)) { best = s1; bidx = i1; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(best, o, 64);
        const int ix = __shfl_xor(bidx, o, 64);
        if (pair_better(v, ix, best, bidx)) { best = v; bidx = ix; }
    }
    if (lane == 0) {
        out[2 * (size_t)i] = best;
        out[2 * (size_t)i + 1] = tot / ((float)n1 * (float)n2);
        if (arg) { arg[2 * (size_t)i] = m0 + bidx / n2; arg[2 * (size_t)i + 1] = p0 + bidx % n2; }
    }
}

struct GatherKernel { template <int D, bool kVec> static constexpr auto get() { return &k_pair_gather<D, kVec>; } };

}  // namespace glam

using namespace glam;

// bytes per load of a call with these matrices: 16 (D % 4 == 0 and both 16-byte aligned), 4 otherwise, 0: D outside the kernel table
extern "C" size_t glam_pair_pool_gather_load_bytes(const float* x1, const float* x2, int D) {
    if (D <= 0 || D > kStreamMaxD) return 0;
    return stream_vec(D, x1, x2) ? 16 : 4;
}

// the two entry points: sums == NULL is the inference call (the bits of the kernel before it took the pointer), sums != NULL training
static int gather_launch(const char* who, const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* idx1,
                         const int32_t* idx2, int64_t P, int64_t Q1, int64_t Q2, int D, float* out, int32_t* argmax, float* sums,
                         bool training, void* stream) {
    GLAM_REQUIRE(P >= 0 && P < INT32_MAX, "%s: P out of range", who);
    GLAM_REQUIRE(Q1 >= 0 && Q1 < INT32_MAX && Q2 >= 0 && Q2 < INT32_MAX, "%s: Q1 / Q2 out of range", who);
    if (D <= 0 || D > kStreamMaxD) return fail(GLAM_E_UNSUPPORTED, "%s: D=%d not in 1..%d", who, D, kStreamMaxD);
    if (P == 0) return GLAM_OK;
    GLAM_REQUIRE(Q1 > 0 && Q2 > 0, "%s: pairs but no segment on one side", who);
    GLAM_REQUIRE(idx1 || Q1 == P, "%s: idx1 = NULL pairs i with segment i of x1: needs Q1 == P", who);
    GLAM_REQUIRE(idx2 || Q2 == P, "%s: idx2 = NULL pairs i with segment i of x2: needs Q2 == P", who);
    GLAM_REQUIRE(x1 && x2 && ptr1 && ptr2 && out && (!training || (argmax && sums)), "%s: null pointer", who);
    GLAM_REQUIRE(((uintptr_t)x1 & 3u) == 0 && ((uintptr_t)x2 & 3u) == 0 && ((uintptr_t)sums & 3u) == 0, "%s: rows must be 4-byte aligned", who);
    const auto k = stream_kernel<GatherKernel>(D, x1, x2);
    GLAM_PROF_LABEL("k_pair_gather");
    hipLaunchKernelGGL(k, dim3((unsigned)((P + kStreamWaves - 1) / kStreamWaves)), dim3(kBlock), 0, (hipStream_t)stream, x1, x2, ptr1,
                       ptr2, idx1, idx2, (int)P, out, argmax, sums);
    GLAM_LAUNCH_CHECK(who);
    return GLAM_OK;
}

extern "C" int glam_pair_pool_gather_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2,
                                         const int32_t* idx1, const int32_t* idx2, int64_t P, int64_t Q1, int64_t Q2, int D,
                                         float* out, int32_t* argmax, void* stream) {
    return gather_launch("glam_pair_pool_gather_fwd", x1, x2, ptr1, ptr2, idx1, idx2, P, Q1, Q2, D, out, argmax, nullptr, false, stream);
}

// ... for training (csrc/pairgather_bwd.hip): argmax and sums f32[P,2,D] are always written (sums not for an empty pair: nothing reads it)
extern "C" int glam_pair_pool_gather_train_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2,
                                               const int32_t* idx1, const int32_t* idx2, int64_t P, int64_t Q1, int64_t Q2, int D,
                                               float* out, int32_t* argmax, float* sums, void* stream) {
    return gather_launch("glam_pair_pool_gather_train_fwd", x1, x2, ptr1, ptr2, idx1, idx2, P, Q1, Q2, D, out, argmax, sums, true, stream);
}
