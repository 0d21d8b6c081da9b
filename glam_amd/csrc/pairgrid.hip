// Grid fusion: every SELECTED first-side segment a = rows[i], i = 0..R-1, of x1 against every SELECTED second-side segment q = cols[j],
// j = 0..Cs-1, of x2 (each segment held once on its side, as in a DrugEncoding):
//   S = x1[ptr1[a]:ptr1[a+1]] @ x2[ptr2[q]:ptr2[q+1]]^T,  out[i, j] = [max S, mean S],  arg[i, j] = (row of x1, row of x2) of the maximum.
//
// Shape.  The loop nest of k_pair_panel (pairpanel.hip) with PACKED chunks.  The panel gives a wave one chunk of 64 rows of ONE
// second-side segment: a 15-30-row drug fills a quarter to a half of its lanes and the idle lanes' multiply-adds are issued anyway.  Here
//   unit of work: one wave for (chunk of up to 64 second-side rows, slab of first-side segments).  A lane loads ONE row of x2 into
//       registers, once, and keeps it for the whole slab;
//   a chunk holds the rows of SEVERAL small segments, laid out by the host plan (ops.grid_plan) in selection order, greedily:
//       consecutive whole segments share a chunk while their rows fit in the 64 lanes; a segment of more than 64 rows closes the running
//       chunk and takes ceil(n / 64) slices of its own (its last slice is not shared); an empty segment takes no lane;
//   the slab's first-side segments are streamed past, their rows two a round through WAVE-UNIFORM loads (the constant address space,
//       the route of stream_score2, pairstream.h);
//   the four waves of a block take four CONSECUTIVE chunks against the same slab.  The waves never meet: no LDS, no block barrier, no
//       atomics.
// So the segment a lane belongs to, its row inside that segment (b), the segment's size (n2) and the partial its best goes to are PER
// LANE, read from the plan's table; only the first-side quantities are wave-uniform.
//
// The table (work, int32, built and checked on the host and trusted here): [total_chunks][64 lanes][4] =
//       (row of x2 the lane holds,  b: that row inside its segment,  n2: rows of that segment,  partial: where the lane's best goes)
//   with partial = part_ptr[j] + slice for a lane of selection j, and -1 for an IDLE lane (past the rows of the chunk), which holds the
//   row of lane 0 (every chunk has one) and drops its scores by a select; then part_ptr int32[Cs + 1], the offsets of the selections'
//   partials (one per whole segment, ceil(n / 64) for a sliced one, none for an empty one).  Lanes of one partial are contiguous.
// Per first-side segment the lanes' best (value, flattened index r1 * n2 + b OF THE LANE'S OWN SEGMENT) is reduced WITHIN each run of
// lanes that share a partial — six __shfl_down steps, each combining only with a partner of the same partial — and the first lane of a
// run stores ONE 8-byte partial to the workspace [partial][R].  k_pair_stream_finish (pairstream.h) — one thread per (i, j) — combines a
// selection's partials in ascending order and forms the mean.
// Maximum: the chain of stream_score2 and the total order of pair_better: the max column and the argmax are bit for bit those of
// glam_pair_pool_gather_fwd on the pair (rows[i], cols[j]) whatever the packing, the slab and the order of the reduction.
// Mean: <sum1[a], sum2[q]> / (n1 n2), the panel's.
#include "pairstream.h"

namespace glam {

constexpr int kGridLane = 4;                   // int32 per lane of the table: row, b, n2, partial

// kVec: D % 4 == 0 and both matrices 16-byte aligned (16-byte loads); otherwise dword loads.  work and rows are trusted.
// grid: ceil(total_chunks / 4) * n_slabs blocks, the chunk block fastest.
template <int D, bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_grid(const float* __restrict__ x1, const float* __restrict__ x2,
                                                     const int* __restrict__ ptr1, const int* __restrict__ rows, int R,
                                                     const int* __restrict__ work, int total_chunks, int chunk_blocks, int slab,
                                                     PairPartial* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const int cb = blockIdx.x % chunk_blocks, s = blockIdx.x / chunk_blocks;
    const int w = cb * kStreamWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= total_chunks) return;                        // a wave without a chunk (no barrier below: the others go on)
    // ---- this lane's entry of the table: PER LANE, not per wave ----
    const int* e = work + ((size_t)w * kStreamChunk + lane) * kGridLane;
    const int row = e[0], b = e[1], n2 = e[2], pid = e[3];
    const bool valid = pid >= 0;                          // (an idle lane holds the row of lane 0 and drops its scores)
    const int before = __shfl_up(pid, 1, 64);
    const bool head = valid && (lane == 0 || before != pid);       // the first lane of a run of one partial: it stores the run's best
    // ---- the lane's second-side row, for the whole slab ----
    const float* prow = x2 + (size_t)row * D;
    float pr[D];
    stream_owner_row<D, kVec>(prow, pr);
    const int i1 = (int)min((int64_t)R, (int64_t)(s + 1) * slab);
    for (int i = s * slab; i < i1; ++i) {
        const int a = rows ? __builtin_amdgcn_readfirstlane(rows[i]) : i;
        const int m0 = __builtin_amdgcn_readfirstlane(ptr1[a]), n1 = __builtin_amdgcn_readfirstlane(ptr1[a + 1]) - m0;
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        // The first-side rows are read through the constant address space: NOTHING in this launch writes x1 (the launch writes ws only).
        for (int r1 = 0; r1 < n1; r1 += 2) {
            const bool two = r1 + 1 < n1;                  // (an odd last row is scored twice and counted once)
            const auto [d0, d1] = stream_score2<D, kVec>(x1 + (size_t)(m0 + r1) * D, two, pr);
            // (selects, not a branch on `valid`: under a divergent branch the row loads above would stop being wave-uniform)
            const float s0 = valid ? d0 : -INFINITY, s1 = valid && two ? d1 : -INFINITY;
            const int i0 = valid ? r1 * n2 + b : 0x7fffffff, ix1 = valid && two ? i0 + n2 : 0x7fffffff;     // the lane's OWN segment
            if (pair_better(s0, i0, best, bidx)) { best = s0; bidx = i0; }
            if (pair_better(s1, ix1, best, bidx)) { best = s1; bidx = ix1; }
        }
        // segmented reduction: after the step of offset o a lane holds the best of lanes [lane, lane + 2 o) of its own run (runs are
        // contiguous: a partner of the same partial means every lane in between is of it too); a run's first lane ends with the run's
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float v = __shfl_down(best, o, 64);
            const int ix = __shfl_down(bidx, o, 64);
            const int other = __shfl_down(pid, o, 64);
            // (past lane 63 there is no partner: __shfl_down hands the lane its OWN pair back, and pair_better() of a pair over itself is false —
            //  a test of the lane number here cost two registers, and at D = 60 a wave per SIMD)
            if (other == pid && pair_better(v, ix, best, bidx)) { best = v; bidx = ix; }
        }
        // (the address is formed from pid here: no pointer is kept per lane across the slab)
        if (head) ws[(size_t)pid * R + i] = PairPartial{best, bidx};        // (an empty first-side segment: -inf, 0x7fffffff)
    }
}

struct GridKernel { template <int D, bool kVec> static constexpr auto get() { return &k_pair_grid<D, kVec>; } };

}  // namespace glam

using namespace glam;

extern "C" size_t glam_pair_pool_grid_workspace_bytes(int64_t n_partials, int64_t R) {
    if (n_partials <= 0 || R <= 0) return 0;
    return (size_t)n_partials * (size_t)R * sizeof(PairPartial);
}

// a STATUS, as every int of this ABI that is not listed as a value: GLAM_OK when width D has a kernel
extern "C" int glam_pair_pool_grid_supported(int D) {
    if (D < 1 || D > kStreamMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_grid: D=%d not in 1..%d", D, kStreamMaxD);
    return GLAM_OK;
}

extern "C" int glam_pair_pool_grid_fwd(const float* x1, const float* x2, const int32_t* ptr1, const int32_t* ptr2, const int32_t* rows,
                                       int64_t R, const int32_t* cols, int64_t Cs, const int32_t* work, int64_t total_chunks,
                                       int64_t n_partials, int64_t Q1, int64_t Q2, int D, const float* sum1, const float* sum2, int slab,
                                       float* out, int32_t* argmax, void* workspace, size_t workspace_bytes, void* stream) {
    GLAM_REQUIRE(R >= 0 && R < INT32_MAX && Cs >= 0 && Cs < INT32_MAX, "glam_pair_pool_grid_fwd: R / Cs out of range");
    GLAM_REQUIRE(Q1 >= 0 && Q1 < INT32_MAX && Q2 >= 0 && Q2 < INT32_MAX, "glam_pair_pool_grid_fwd: Q1 / Q2 out of range");
    GLAM_REQUIRE(total_chunks >= 0 && total_chunks < INT32_MAX / (kStreamChunk * kGridLane), "glam_pair_pool_grid_fwd: total_chunks out of range");
    GLAM_REQUIRE(n_partials >= 0 && n_partials < INT32_MAX, "glam_pair_pool_grid_fwd: n_partials out of range");
    GLAM_REQUIRE(slab >= 0, "glam_pair_pool_grid_fwd: slab must be 0 (choose) or the first-side segments per wave");
    if (const int rc = glam_pair_pool_grid_supported(D)) return rc;
    if (R == 0 || Cs == 0) return GLAM_OK;
    GLAM_REQUIRE(Q1 > 0 && Q2 > 0, "glam_pair_pool_grid_fwd: a selection but no segment on one side");
    GLAM_REQUIRE(rows || R == Q1, "glam_pair_pool_grid_fwd: rows = NULL is the identity over Q1 and needs R == Q1");
    GLAM_REQUIRE(R * Cs < INT32_MAX, "glam_pair_pool_grid_fwd: R * Cs out of range");
    GLAM_REQUIRE(n_partials >= total_chunks, "glam_pair_pool_grid_fwd: fewer partials than chunks (every chunk holds the head of one)");
    GLAM_REQUIRE(x1 && x2 && ptr1 && ptr2 && cols && work && sum1 && sum2 && out, "glam_pair_pool_grid_fwd: null pointer");
    GLAM_REQUIRE(((uintptr_t)x1 & 3u) == 0 && ((uintptr_t)x2 & 3u) == 0, "glam_pair_pool_grid_fwd: rows must be 4-byte aligned");
    const size_t need = glam_pair_pool_grid_workspace_bytes(n_partials, R);
    GLAM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7u) == 0),
                 "glam_pair_pool_grid_fwd: workspace too small or misaligned (glam_pair_pool_grid_workspace_bytes)");
    PairPartial* ws = (PairPartial*)workspace;
    GLAM_PROF_LABEL("k_pair_grid");
    if (total_chunks > 0) {
        const int64_t sl = stream_slab(slab, R, total_chunks);      // (the panel's rule, taken over as it is: not tuned for packed chunks)
        const int64_t n_slabs = (R + sl - 1) / sl, chunk_blocks = (total_chunks + kStreamWaves - 1) / kStreamWaves;
        GLAM_REQUIRE(chunk_blocks * n_slabs < INT32_MAX, "glam_pair_pool_grid_fwd: grid out of range");
        const auto k = stream_kernel<GridKernel>(D, x1, x2);
        hipLaunchKernelGGL(k, dim3((unsigned)(chunk_blocks * n_slabs)), dim3(kBlock), 0, (hipStream_t)stream, x1, x2, ptr1, rows, (int)R, work,
                           (int)total_chunks, (int)chunk_blocks, (int)sl, ws);
        GLAM_LAUNCH_CHECK("glam_pair_pool_grid_fwd");
    }
    GLAM_PROF_LABEL("k_pair_grid_finish");
    hipLaunchKernelGGL(k_pair_stream_finish<true>, dim3((unsigned)((R * Cs + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, ws,
                       work + (size_t)total_chunks * kStreamChunk * kGridLane, rows, cols, ptr1, ptr2, sum1, sum2, (int)R, (int)Cs, D, out,
                       argmax);
    GLAM_LAUNCH_CHECK("glam_pair_pool_grid_fwd (finish)");
    return GLAM_OK;
}
