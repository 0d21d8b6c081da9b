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
// Per (ligand, chunk) the lanes' best (value, flattened index a * n_res + b) is reduced across the wave with better() and lane 0
// stores ONE 8-byte partial to the workspace [chunk of the selection][L]; k_pair_panel_finish — one thread per (l, j) — combines a
// protein's chunk partials in ascending chunk order and forms the mean.
// Maximum: every score is ONE fmaf chain over channels 0 .. D-1 in ascending order from 0.f — the chain of k_pair_max_partial,
// k_pair_pool_fwd and k_pair_gather — and ties go to the smallest flattened index, which makes (value, index) a total order: the max
// column and the argmax are bit for bit those of glam_pair_pool_indexed_fwd with pro_of_pair = [sel[j]] * L whatever the order of the
// reduction (lanes, chunks, slabs).  Mean: sum(S) = <molsum[l], prosum[q]>, both column sums inputs (the ligands' made once per call,
// the proteins' once per encoding), one ascending fmaf chain over the D columns in the finish thread.
#include <algorithm>
#include <utility>

#include "common.h"

namespace glam {

constexpr int kPanelWaves = kBlock / 64;       // chunks (waves) per block
constexpr int kPanelChunk = 64;                // residue rows per chunk: one per lane
constexpr int kPanelMaxD = 128;
constexpr int kPanelWork = 4;                  // int32 per chunk of the work table: j, first residue row, rows, offset of its partials
constexpr int kPanelTargetWaves = 4096;        // automatic slab: 256 CUs x 4 SIMDs x 4 waves
constexpr int kPanelMinSlab = 4;

typedef __attribute__((address_space(4))) const float panel_cf1;         // wave-uniform reads of data no launch of this file writes
typedef __attribute__((address_space(4))) const glam_v4f panel_cv4;

struct PanelPartial {      // one (ligand, chunk): 8 bytes, written by one vector store
    float v;
    int ix;
};

// p, which every lane of the wave holds alike, said so to the compiler (its loads then go to the scalar unit whatever the analysis finds)
__device__ __forceinline__ const float* panel_uniform(const float* p) {
    const uintptr_t v = (uintptr_t)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const float*)(((uintptr_t)hi << 32) | lo);
}

__device__ __forceinline__ bool panel_better(float v, int ix, float best, int bidx) { return v > best || (v == best && ix < bidx); }

// kVec: D % 4 == 0 and both matrices 16-byte aligned (16-byte loads); otherwise dword loads.  work and sel are trusted.
// grid: ceil(total_chunks / 4) * n_slabs blocks, the chunk block fastest.
template <int D, bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_panel(const float* __restrict__ mol, const float* __restrict__ pro,
                                                      const int* __restrict__ mol_ptr, const int* __restrict__ pro_ptr,
                                                      const int* __restrict__ work, int total_chunks, int chunk_blocks,
                                                      const int* __restrict__ sel, int L, int slab, PanelPartial* __restrict__ ws) {
    static_assert(D >= 1 && D <= kPanelMaxD && (!kVec || D % 4 == 0), "k_pair_panel: width");
    static_assert(kPanelChunk == 64, "k_pair_panel: one residue row of a chunk per lane of the wave");
    const int lane = threadIdx.x & 63;
    const int cb = blockIdx.x % chunk_blocks, s = blockIdx.x / chunk_blocks;
    const int w = cb * kPanelWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
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
    PanelPartial* const part = ws + (size_t)off * L;
    const int l1 = (int)min((int64_t)L, (int64_t)(s + 1) * slab);
    for (int l = s * slab; l < l1; ++l) {
        const int m0 = __builtin_amdgcn_readfirstlane(mol_ptr[l]), n1 = __builtin_amdgcn_readfirstlane(mol_ptr[l + 1]) - m0;
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        // The ligand rows are read through the constant address space: NOTHING in this launch writes mol (the launch writes ws only).
        for (int r1 = 0; r1 < n1; r1 += 2) {
            const bool two = r1 + 1 < n1;                  // (an odd last row is scored twice and counted once)
            const float* q0 = panel_uniform(mol + (size_t)(m0 + r1) * D);
            const float* q1 = q0 + (two ? D : 0);
            float d0 = 0.f, d1 = 0.f;
            if constexpr (kVec) {
#pragma unroll
                for (int u = 0; u < D / 4; ++u) {
                    const glam_v4f v0 = ((panel_cv4*)q0)[u], v1 = ((panel_cv4*)q1)[u];
                    d0 = fmaf(v0.x, pr[4 * u], d0); d0 = fmaf(v0.y, pr[4 * u + 1], d0); d0 = fmaf(v0.z, pr[4 * u + 2], d0); d0 = fmaf(v0.w, pr[4 * u + 3], d0);
                    d1 = fmaf(v1.x, pr[4 * u], d1); d1 = fmaf(v1.y, pr[4 * u + 1], d1); d1 = fmaf(v1.z, pr[4 * u + 2], d1); d1 = fmaf(v1.w, pr[4 * u + 3], d1);
                }
            } else {
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    d0 = fmaf(((panel_cf1*)q0)[c], pr[c], d0);
                    d1 = fmaf(((panel_cf1*)q1)[c], pr[c], d1);
                }
            }
            // (selects, not a branch on `valid`: under a divergent branch the row loads above would stop being wave-uniform)
            const float s0 = valid ? d0 : -INFINITY, s1 = valid && two ? d1 : -INFINITY;
            const int i0 = valid ? r1 * n_res + b : 0x7fffffff, i1 = valid && two ? i0 + n_res : 0x7fffffff;
            if (panel_better(s0, i0, best, bidx)) { best = s0; bidx = i0; }
            if (panel_better(s1, i1, best, bidx)) { best = s1; bidx = i1; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v = __shfl_xor(best, o, 64);
            const int ix = __shfl_xor(bidx, o, 64);
            if (panel_better(v, ix, best, bidx)) { best = v; bidx = ix; }
        }
        if (lane == 0) part[l] = PanelPartial{best, bidx};          // (an empty ligand: -inf, 0x7fffffff)
    }
}

// One thread per (l, j), l fastest (the partials of a chunk are read side by side).  chunk_ptr int32[Qs + 1]: the chunks of selection j.
__global__ void __launch_bounds__(kBlock) k_pair_panel_finish(const PanelPartial* __restrict__ ws, const int* __restrict__ chunk_ptr,
                                                             const int* __restrict__ sel, const int* __restrict__ mol_ptr,
                                                             const int* __restrict__ pro_ptr, const float* __restrict__ molsum,
                                                             const float* __restrict__ prosum, int L, int Qs, int D,
                                                             float* __restrict__ out, int* __restrict__ arg) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)L * Qs) return;
    const int j = (int)(t / L), l = (int)(t % L);
    const int q = sel[j];
    const int m0 = mol_ptr[l], n1 = mol_ptr[l + 1] - m0;
    const int p0 = pro_ptr[q], n_res = pro_ptr[q + 1] - p0;
    const size_t o = 2 * ((size_t)l * Qs + j);
    if (n1 <= 0 || n_res <= 0) {
        out[o] = 0.f; out[o + 1] = 0.f;
        if (arg) { arg[o] = -1; arg[o + 1] = -1; }
        return;
    }
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = chunk_ptr[j]; c < chunk_ptr[j + 1]; ++c) {
        const PanelPartial p = ws[(size_t)c * L + l];
        if (panel_better(p.v, p.ix, best, bidx)) { best = p.v; bidx = p.ix; }
    }
    const float* a = molsum + (size_t)l * D;
    const float* b = prosum + (size_t)q * D;
    float tot = 0.f;
    for (int c = 0; c < D; ++c) tot = fmaf(a[c], b[c], tot);
    out[o] = best;
    out[o + 1] = tot / ((float)n1 * (float)n_res);
    if (arg) { arg[o] = m0 + bidx / n_res; arg[o + 1] = p0 + bidx % n_res; }
}

typedef void (*panel_kernel)(const float*, const float*, const int*, const int*, const int*, int, int, const int*, int, int, PanelPartial*);

// [D - 1] -> the dword instantiation of width D;  [D / 4 - 1] -> the 16-byte one
template <int... I>
static const panel_kernel* panel_dword_table(std::integer_sequence<int, I...>) {
    static const panel_kernel t[] = {k_pair_panel<I + 1, false>...};
    return t;
}
template <int... I>
static const panel_kernel* panel_vec_table(std::integer_sequence<int, I...>) {
    static const panel_kernel t[] = {k_pair_panel<4 * (I + 1), true>...};
    return t;
}

}  // namespace glam

using namespace glam;

extern "C" size_t glam_pair_pool_panel_workspace_bytes(int64_t total_chunks, int64_t L) {
    if (total_chunks <= 0 || L <= 0) return 0;
    return (size_t)total_chunks * (size_t)L * sizeof(PanelPartial);
}

// a STATUS, as every int of this ABI that is not listed as a value: GLAM_OK when width D has a kernel
extern "C" int glam_pair_pool_panel_supported(int D) {
    if (D < 1 || D > kPanelMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_panel: D=%d not in 1..%d", D, kPanelMaxD);
    return GLAM_OK;
}

extern "C" int glam_pair_pool_panel_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                                        const int32_t* work, int64_t total_chunks, const int32_t* sel, int64_t Qs, int64_t L, int64_t Q,
                                        int D, const float* molsum, const float* prosum, int slab, float* out, int32_t* argmax,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(sizeof(PanelPartial) == 8, "PanelPartial: one 8-byte store");
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
    PanelPartial* ws = (PanelPartial*)workspace;
    GLAM_PROF_LABEL("k_pair_panel");
    if (total_chunks > 0) {
        // automatic slab: about kPanelTargetWaves waves where the problem has them, never fewer than kPanelMinSlab ligands per wave
        int64_t sl = slab > 0 ? slab : std::max<int64_t>(kPanelMinSlab, (L * total_chunks + kPanelTargetWaves - 1) / kPanelTargetWaves);
        sl = std::min<int64_t>(sl, L);
        const int64_t n_slabs = (L + sl - 1) / sl, chunk_blocks = (total_chunks + kPanelWaves - 1) / kPanelWaves;
        GLAM_REQUIRE(chunk_blocks * n_slabs < INT32_MAX, "glam_pair_pool_panel_fwd: grid out of range");
        const panel_kernel k = (D & 3) == 0 && aligned16(mol) && aligned16(pro)
                                   ? panel_vec_table(std::make_integer_sequence<int, kPanelMaxD / 4>())[D / 4 - 1]
                                   : panel_dword_table(std::make_integer_sequence<int, kPanelMaxD>())[D - 1];
        hipLaunchKernelGGL(k, dim3((unsigned)(chunk_blocks * n_slabs)), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr,
                           work, (int)total_chunks, (int)chunk_blocks, sel, (int)L, (int)sl, ws);
        GLAM_LAUNCH_CHECK("glam_pair_pool_panel_fwd");
    }
    GLAM_PROF_LABEL("k_pair_panel_finish");
    hipLaunchKernelGGL(k_pair_panel_finish, dim3((unsigned)((L * Qs + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, ws,
                       work + (size_t)total_chunks * kPanelWork, sel, mol_ptr, pro_ptr, molsum, prosum, (int)L, (int)Qs, D, out, argmax);
    GLAM_LAUNCH_CHECK("glam_pair_pool_panel_fwd (finish)");
    return GLAM_OK;
}
