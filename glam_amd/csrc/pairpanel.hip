// Panel fusion: every ligand segment l = 0..L-1 of mol against every SELECTED protein segment sel[j], j = 0..Qs-1, of pro (each protein
// held once, as in a ProteinEncoding):
//   S = mol[mol_ptr[l]:mol_ptr[l+1]] @ pro[pro_ptr[q]:pro_ptr[q+1]]^T with q = sel[j],  out[l, j] = [max S, mean S],
//   arg[l, j] = (row of mol, row of pro) of the maximum.
//
// Shape.  The indexed fusion of pairpool.hip is cut for pairs that each own a protein: 16 blocks per pair, every block loading its 64
// residue rows for the ~20 rows of ONE ligand.  Here the proteins are few and every ligand meets all of them, so the grid is
// PROTEIN-STATIONARY — the loop nest of k_pair_gather (pairgather.hip) turned inside out:
//   unit of work: one wave for (chunk of 64 residue rows of a selected protein, slab of ligands).  A lane loads ONE residue row of the
//       chunk into registers, once, and keeps it for the whole slab;
//   the slab's ligands are streamed past it one after the other, their rows two a round through WAVE-UNIFORM loads (the constant
//       address space: the scalar unit fetches a row once per wave, every multiply-add takes it as its scalar operand; the width is a
//       template parameter for the reason given in pairgather.hip);
//   the four waves of a block take four CONSECUTIVE chunks of the work table against the same slab: the ligand rows a block streams
//       are fetched once into the scalar cache of its CU and read by all four.  The waves never meet: no LDS, no block barrier.
// Per (ligand, chunk) the lanes' best (value, flattened index a * n_res + b) is reduced across the wave with pair_better() and lane 0
// stores ONE 8-byte partial to the workspace [chunk of the selection][L]; k_pair_stream_finish (pairstream.h) — one thread per (l, j) —
// combines a protein's chunk partials in ascending chunk order and forms the mean.
// Maximum: the chain of stream_score2 and the total order of pair_better: the max column and the argmax are bit for bit those of
// glam_pair_pool_indexed_fwd with pro_of_pair = [sel[j]] * L whatever the order of the reduction (lanes, chunks, slabs).
// Mean: sum(S) = <molsum[l], prosum[q]>, both column sums inputs (the ligands' made once per call, the proteins' once per encoding).
#include "pairstream.h"

namespace glam {

constexpr int kPanelWork = 4;                  // int32 per chunk of the work table: j, first residue row, rows, offset of its partials

// kVec: D % 4 == 0 and both matrices 16-byte aligned (16-byte loads); otherwise dword loads.  work and sel are trusted.
// grid: ceil(total_chunks / 4) * n_slabs blocks, the chunk block fastest.
template <int D, bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_panel(const float* __restrict__ mol, const float* __restrict__ pro,
                                                      const int* __restrict__ mol_ptr, const int* __restrict__ pro_ptr,
                                                      const int* __restrict__ work, int total_chunks, int chunk_blocks,
                                                      const int* __restrict__ sel, int L, int slab, PairPartial* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const int cb = blockIdx.x % chunk_blocks, s = blockIdx.x / chunk_blocks;
    const int w = cb * kStreamWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= total_chunks) return;                        // a wave without a chunk (no barrier below: the others go on)
    const int* e = work + (size_t)w * kPanelWork;
    const int q = __builtin_amdgcn_readfirstlane(sel[e[0]]);
    const int first = __builtin_amdgcn_readfirstlane(e[1]), rows = __builtin_amdgcn_readfirstlane(e[2]);
    const int off = __builtin_amdgcn_readfirstlane(e[3]);
    const int p0 = __builtin_amdgcn_readfirstlane(pro_ptr[q]), n_res = __builtin_amdgcn_readfirstlane(pro_ptr[q + 1]) - p0;
    const bool valid = lane < rows;
    const int b = first - p0 + lane;                      // this lane's residue row inside its protein
    // ---- the lane's residue row, for the whole slab (a lane past the end of the chunk reads its first row and drops its scores) ----
    const float* prow = pro + (size_t)(first + (valid ? lane : 0)) * D;
    float pr[D];
    stream_owner_row<D, kVec>(prow, pr);
    PairPartial* const part = ws + (size_t)off * L;
    const int l1 = (int)min((int64_t)L, (int64_t)(s + 1) * slab);
    for (int l = s * slab; l < l1; ++l) {
        const int m0 = __builtin_amdgcn_readfirstlane(mol_ptr[l]), n1 = __builtin_amdgcn_readfirstlane(mol_ptr[l + 1]) - m0;
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        // The ligand rows are read through the constant address space: NOTHING in this launch writes mol (the launch writes ws only).
        for (int r1 = 0; r1 < n1; r1 += 2) {
            const bool two = r1 + 1 < n1;                  // (an odd last row is scored twice and counted once)
            const auto [d0, d1] = stream_score2<D, kVec>(mol + (size_t)(m0 + r1) * D, two, pr);
            // (selects, not a branch on `valid`: under a divergent branch the row loads above would stop being wave-uniform)
            const float s0 = valid ? d0 : -INFINITY, s1 = valid && two ? d1 : -INFINITY;
            const int i0 = valid ? r1 * n_res + b : 0x7fffffff, i1 = valid && two ? i0 + n_res : 0x7fffffff;
            if (pair_better(s0, i0, best, bidx)) { best = s0; bidx = i0; }
            if (pair_better(s1, i1, best, bidx)) { best = s1; bidx = i1; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v = __shfl_xor(best, o, 64);
            const int ix = __shfl_xor(bidx, o, 64);
            if (pair_better(v, ix, best, bidx)) { best = v; bidx = ix; }
        }
        if (lane == 0) part[l] = PairPartial{best, bidx};          // (an empty ligand: -inf, 0x7fffffff)
    }
}

struct PanelKernel { template <int D, bool kVec> static constexpr auto get() { return &k_pair_panel<D, kVec>; } };

}  // namespace glam

using namespace glam;

extern "C" size_t glam_pair_pool_panel_workspace_bytes(int64_t total_chunks, int64_t L) {
    if (total_chunks <= 0 || L <= 0) return 0;
    return (size_t)total_chunks * (size_t)L * sizeof(PairPartial);
}

// a STATUS, as every int of this ABI that is not listed as a value: GLAM_OK when width D has a kernel
extern "C" int glam_pair_pool_panel_supported(int D) {
    if (D < 1 || D > kStreamMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_panel: D=%d not in 1..%d", D, kStreamMaxD);
    return GLAM_OK;
}

extern "C" int glam_pair_pool_panel_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                                        const int32_t* work, int64_t total_chunks, const int32_t* sel, int64_t Qs, int64_t L, int64_t Q,
                                        int D, const float* molsum, const float* prosum, int slab, float* out, int32_t* argmax,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    GLAM_REQUIRE(L >= 0 && L < INT32_MAX, "glam_pair_pool_panel_fwd: L out of range");
    GLAM_REQUIRE(Q >= 0 && Q < INT32_MAX && Qs >= 0 && Qs < INT32_MAX, "glam_pair_pool_panel_fwd: Q / Qs out of range");
    GLAM_REQUIRE(total_chunks >= 0 && total_chunks < INT32_MAX, "glam_pair_pool_panel_fwd: total_chunks out of range");
    GLAM_REQUIRE(slab >= 0, "glam_pair_pool_panel_fwd: slab must be 0 (choose) or the ligands per wave");
    if (const int rc = glam_pair_pool_panel_supported(D)) return rc;
    if (L == 0 || Qs == 0) return GLAM_OK;
    GLAM_REQUIRE(Q > 0, "glam_pair_pool_panel_fwd: a selection but no protein segment");
    GLAM_REQUIRE(L * Qs < INT32_MAX, "glam_pair_pool_panel_fwd: L * Qs out of range");
    GLAM_REQUIRE(mol && pro && mol_ptr && pro_ptr && work && sel && molsum && prosum && out, "glam_pair_pool_panel_fwd: null pointer");
    GLAM_REQUIRE(((uintptr_t)mol & 3u) == 0 && ((uintptr_t)pro & 3u) == 0, "glam_pair_pool_panel_fwd: rows must be 4-byte aligned");
    const size_t need = glam_pair_pool_panel_workspace_bytes(total_chunks, L);
    GLAM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7u) == 0),
                 "glam_pair_pool_panel_fwd: workspace too small or misaligned (glam_pair_pool_panel_workspace_bytes)");
    PairPartial* ws = (PairPartial*)workspace;
    GLAM_PROF_LABEL("k_pair_panel");
    if (total_chunks > 0) {
        const int64_t sl = stream_slab(slab, L, total_chunks);
        const int64_t n_slabs = (L + sl - 1) / sl, chunk_blocks = (total_chunks + kStreamWaves - 1) / kStreamWaves;
        GLAM_REQUIRE(chunk_blocks * n_slabs < INT32_MAX, "glam_pair_pool_panel_fwd: grid out of range");
        const auto k = stream_kernel<PanelKernel>(D, mol, pro);
        hipLaunchKernelGGL(k, dim3((unsigned)(chunk_blocks * n_slabs)), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr,
                           work, (int)total_chunks, (int)chunk_blocks, sel, (int)L, (int)sl, ws);
        GLAM_LAUNCH_CHECK("glam_pair_pool_panel_fwd");
    }
    GLAM_PROF_LABEL("k_pair_panel_finish");
    hipLaunchKernelGGL(k_pair_stream_finish<false>, dim3((unsigned)((L * Qs + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, ws,
                       work + (size_t)total_chunks * kPanelWork, nullptr, sel, mol_ptr, pro_ptr, molsum, prosum, (int)L, (int)Qs, D, out,
                       argmax);
    GLAM_LAUNCH_CHECK("glam_pair_pool_panel_fwd (finish)");
    return GLAM_OK;
}
