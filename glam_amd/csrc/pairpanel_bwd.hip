// Backward of the panel fusion of pairpanel.hip (every ligand l against every selected protein sel[j], each protein held once): DTI
// training on a ligand x protein label table.
//   forward   glam_pair_pool_panel_fwd with the argmax kept (pairpanel.hip; nothing is added to it).
//   backward  glam_pair_pool_panel_bwd, ONE launch with two block roles — k_pair_shared_bwd (pairshared.hip) with a list on BOTH sides.
//             The roles write disjoint outputs and read only forward results: nothing orders them.
//             A segment (a ligand, or a protein) is owned kPbRows = 16 rows a sweep by the blocks (segment, s), s < split, block s taking the
//             rows s * 16 + k * split * 16 + r; every block walks its segment's LIST of pairs:
//               ligand l    the pairs (l, j), j = 0 .. Qs-1 ascending                                           (length Qs)
//               protein q   the pairs (l, j) with sel[j] == q in ascending l * Qs + j — the batch order of the expanded pair list: l
//                           ascending, and within an l the entries order[ptr[q] .. ptr[q+1]) of the selection grouped by protein, a
//                           STABLE argsort of sel                                                              (length L * dups)
//             and with w = d_out[l, j, 1] / ((float)n_l * (float)n_q):
//               S       = 0, + w * (column sums of the partner segment) for the pairs of the list, in list order   (the same for every row)
//               d_x[r]  = S, then fmaf(d_out[l, j, 0], partner[arg of the partner side], .) for the pairs of the list whose maximum sits
//                         on row r, in list order, + add[r] last
//             No atomics; the order depends on the table alone, never on the grid or on timing.  A protein no entry of sel names has an
//             empty list: S = 0 and no hit, its rows get exact zeros (+ add).
// The list is walked in tiles staged in LDS: what is block-uniform about a pair (its partner's sum row and w; its two argmax rows and
// d_out[., 0]) is loaded once per tile by one thread each and then broadcast, the [tile, D] addends of S are loaded by the whole block
// with every load independent of the others, a ballot marks the pairs of a tile whose maximum sits in the block's 16 rows, their
// partner rows are loaded kPbHits a round (by every thread: the loads do not wait for a row test), and only the add chains themselves
// are serial.
// A thread holds kPbNV = 8 columns of one of the 16 rows: 16-byte form — columns 4 cg .. 4 cg + 3 and 64 + 4 cg .. 64 + 4 cg + 3;
// dword form — columns cg + 16 u, u < 8 (cg = tid & 15, row tid >> 4).
#include "common.h"

namespace glam {

constexpr int kPbMaxD = 128;
constexpr int kPbRows = 16;         // rows a block owns per sweep
constexpr int kPbMolSplit = 2;      // blocks per ligand: a sweep of 32 rows
constexpr int kPbProSplit = 32;     // blocks per protein: a sweep of 512 rows
constexpr int kPbTileFloats = 8192; // the staged tile of addends: 32 KB, min(256, 8192 / ceil4(D)) pairs of it a round (D = 60: 136, 128: 64)
constexpr int kPbHits = 8;          // fmaf addends in flight per thread
constexpr int kPbNV = 8;            // columns a thread holds

static_assert(kPbRows * 16 == kBlock, "pairpanel_bwd: 16 threads per row, 16 rows per block");

// A thread's kPbNV values of a row.  A column past D is never loaded (the value stays 0) and never stored.
template <bool kVec>
__device__ __forceinline__ void pb_load(const float* row, int cg, int D, float* t) {
    if constexpr (kVec) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float4 v = f4zero();
            if (64 * u + 4 * cg < D) v = ld4(row + 64 * u + 4 * cg);
            t[4 * u] = v.x; t[4 * u + 1] = v.y; t[4 * u + 2] = v.z; t[4 * u + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < kPbNV; ++u) t[u] = cg + 16 * u < D ? row[cg + 16 * u] : 0.f;
    }
}

template <bool kVec>
__device__ __forceinline__ void pb_store(float* row, int cg, int D, const float* v) {
    if constexpr (kVec) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (64 * u + 4 * cg < D) st4(row + 64 * u + 4 * cg, make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]));
    } else {
#pragma unroll
        for (int u = 0; u < kPbNV; ++u)
            if (cg + 16 * u < D) row[cg + 16 * u] = v[u];
    }
}

// grid: Q * kPbProSplit protein blocks, then L * kPbMolSplit ligand blocks
template <bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_panel_bwd(const float* mol, const float* pro, const int* mptr, const int* pptr,
                                                          const int* sel, const int* order, const int* qptr, const int* arg,
                                                          const float* d_out, const float* molsum, const float* prosum, int Qs, int L, int Q,
                                                          int D, const float* add_mol, const float* add_pro, float* d_mol, float* d_pro) {
    __shared__ __attribute__((aligned(16))) float s_tile[kPbTileFloats];
    __shared__ __attribute__((aligned(16))) float s_S[kPbMaxD];
    __shared__ int s_own[kBlock], s_oth[kBlock];                             // walk of S: s_own = row of the partner's sum matrix, -1: an empty pair
    __shared__ float s_g[kBlock];                                            // walk of S: w
    __shared__ unsigned long long s_mask[kBlock / 64];
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    const int pro_blocks = Q * kPbProSplit;
    const bool ligand = (int)blockIdx.x >= pro_blocks;                      // (block-uniform)
    const int bid = ligand ? blockIdx.x - pro_blocks : blockIdx.x;
    const int split = ligand ? kPbMolSplit : kPbProSplit;
    const int seg = bid / split, sp = bid % split;
    const int* optr_own = ligand ? mptr : pptr;
    const int r0 = optr_own[seg], r1 = optr_own[seg + 1], n_own = r1 - r0;
    if (sp * kPbRows >= n_own) return;                                      // no row to write (block-uniform, before the first barrier)
    // the list: ligand — j = t; protein — l = t / dups, j = order[k0 + t % dups]
    const int k0 = ligand ? 0 : qptr[seg], dups = ligand ? 1 : qptr[seg + 1] - k0;
    const int len = ligand ? Qs : L * dups;
    const float* osum = ligand ? prosum : molsum;                           // the partner's column sums ...
    const float* oth_x = ligand ? pro : mol;                                // ... and rows
    const int own_col = ligand ? 0 : 1;                                     // this side's column of arg[l, j]
    const float* add = ligand ? add_mol : add_pro;
    float* dx = ligand ? d_mol : d_pro;

    // item t of the list -> its pair number l * Qs + j, the partner segment and its row count
    auto item = [&](int t, int& partner, int& n_oth) {
        int l, j;
        if (ligand) {
            l = seg; j = t;
            partner = sel[j];
            n_oth = pptr[partner + 1] - pptr[partner];
        } else {
            l = t / dups; j = order[k0 + t - l * dups];
            partner = l;
            n_oth = mptr[l + 1] - mptr[l];
        }
        return l * Qs + j;
    };

    // ---- S: w * (column sums of the partner), pairs in list order ----
    const int per = kVec ? D >> 2 : D;                                      // loads per pair of a tile
    const int stride = (D + 3) & ~3, tile = min(kBlock, kPbTileFloats / stride);        // floats per pair in s_tile, pairs per round
    float S = 0.f;                                                          // of column tid (tid < D)
    for (int t0 = 0; t0 < len; t0 += tile) {
        const int tn = min(tile, len - t0);
        __syncthreads();
        if (tid < tn) {
            int partner, n_oth;
            const int i = item(t0 + tid, partner, n_oth);
            const bool empty = n_oth <= 0;                                  // (n_own > 0 here: the block owns rows)
            const float nn = ligand ? (float)n_own * (float)n_oth : (float)n_oth * (float)n_own;     // (float)n_l * (float)n_q
            s_own[tid] = empty ? -1 : partner;
            s_g[tid] = empty ? 0.f : d_out[2 * (size_t)i + 1] / nn;
        }
        __syncthreads();
        for (int e = tid; e < tn * per; e += kBlock) {
            const int k = e / per, c = e - k * per;
            const int src = s_own[k];
            if constexpr (kVec) st4(s_tile + k * stride + 4 * c, src < 0 ? f4zero() : s_g[k] * ld4(osum + (size_t)src * D + 4 * c));
            else s_tile[k * stride + c] = src < 0 ? 0.f : s_g[k] * osum[(size_t)src * D + c];
        }
        __syncthreads();
        if (tid < D)
            for (int k = 0; k < tn; ++k) S += s_tile[k * stride + tid];
    }
    if (tid < kPbMaxD) s_S[tid] = tid < D ? S : 0.f;
    __syncthreads();
    float Sv[kPbNV];
    pb_load<kVec>(s_S, cg, D, Sv);

    // ---- rows: S, then the fmaf terms of the pairs whose maximum sits on the row, in list order, then add ----
    for (int b0 = r0 + sp * kPbRows; b0 < r1; b0 += split * kPbRows) {
        float v[kPbNV];
#pragma unroll
        for (int u = 0; u < kPbNV; ++u) v[u] = Sv[u];
        for (int t0 = 0; t0 < len; t0 += kBlock) {
            bool hit = false;
            __syncthreads();
            if (t0 + tid < len) {
                int partner, n_oth;
                const int i = item(t0 + tid, partner, n_oth);
                const int own = n_oth <= 0 ? -1 : arg[2 * (size_t)i + own_col];
                hit = own >= b0 && own < b0 + kPbRows;
                s_own[tid] = own;
                s_oth[tid] = arg[2 * (size_t)i + 1 - own_col];
                s_g[tid] = d_out[2 * (size_t)i];
            }
            const unsigned long long m = __ballot(hit);
            if ((tid & 63) == 0) s_mask[tid >> 6] = m;
            __syncthreads();
            for (int w = 0; w < kBlock / 64; ++w) {
                unsigned long long left = s_mask[w];
                while (left) {                                              // (block-uniform) kPbHits hits a round: their loads side by side
                    float t[kPbHits][kPbNV], g[kPbHits];
                    bool mine[kPbHits];
                    const int first = __builtin_ctzll(left);
#pragma unroll
                    for (int h = 0; h < kPbHits; ++h) {
                        const bool has = left != 0;
                        const int kk = w * 64 + (has ? __builtin_ctzll(left) : first);
                        left &= left - 1;                                   // (0 stays 0)
                        mine[h] = has && s_own[kk] == b0 + rg;
                        g[h] = s_g[kk];
                        pb_load<kVec>(oth_x + (size_t)s_oth[kk] * D, cg, D, t[h]);      // (a hit: its partner row exists)
                    }
#pragma unroll
                    for (int h = 0; h < kPbHits; ++h)
#pragma unroll
                        for (int u = 0; u < kPbNV; ++u) v[u] = mine[h] ? fmaf(g[h], t[h][u], v[u]) : v[u];
                }
            }
        }
        const int b = b0 + rg;
        if (b < r1) {
            if (add) {
                float t[kPbNV];
                pb_load<kVec>(add + (size_t)b * D, cg, D, t);
#pragma unroll
                for (int u = 0; u < kPbNV; ++u) v[u] += t[u];
            }
            pb_store<kVec>(dx + (size_t)b * D, cg, D, v);
        }
    }
}

}  // namespace glam

using namespace glam;

// sel_order / sel_ptr: the selection stably sorted by protein and the Q + 1 offsets of the proteins' runs (PanelPlan.by_protein: built
// and checked by the host, trusted here, like sel).  add_mol / add_pro may be NULL.
extern "C" int glam_pair_pool_panel_bwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                                        const int32_t* sel, const int32_t* sel_order, const int32_t* sel_ptr, const int32_t* argmax,
                                        const float* d_out, const float* molsum, const float* prosum, int64_t Qs, int64_t L, int64_t Q, int D,
                                        const float* add_mol, const float* add_pro, float* d_mol, float* d_pro, void* stream) {
    GLAM_REQUIRE(L >= 0 && L < INT32_MAX, "glam_pair_pool_panel_bwd: L out of range");
    GLAM_REQUIRE(Q >= 0 && Q < INT32_MAX && Qs >= 0 && Qs < INT32_MAX, "glam_pair_pool_panel_bwd: Q / Qs out of range");
    if (D <= 0 || D > kPbMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_panel_bwd: D=%d not in 1..%d", D, kPbMaxD);
    if (L == 0 || Qs == 0) return GLAM_OK;      // (nothing is written: the caller's zeros stand)
    GLAM_REQUIRE(Q > 0, "glam_pair_pool_panel_bwd: a selection but no protein segment");
    GLAM_REQUIRE(L * Qs < INT32_MAX, "glam_pair_pool_panel_bwd: L * Qs out of range");
    const int64_t grid = Q * kPbProSplit + L * kPbMolSplit;
    GLAM_REQUIRE(grid < INT32_MAX, "glam_pair_pool_panel_bwd: grid out of range");
    GLAM_REQUIRE(mol && pro && mol_ptr && pro_ptr && sel && sel_order && sel_ptr && argmax && d_out && molsum && prosum && d_mol && d_pro,
                 "glam_pair_pool_panel_bwd: null pointer");
    const void* f32s[] = {mol, pro, d_out, molsum, prosum, add_mol, add_pro, d_mol, d_pro};
    bool vec = (D & 3) == 0;
    for (const void* p : f32s) {
        GLAM_REQUIRE(((uintptr_t)p & 3u) == 0, "glam_pair_pool_panel_bwd: rows must be 4-byte aligned");
        vec = vec && (p == d_out || aligned16(p));
    }
    GLAM_PROF_LABEL("k_pair_panel_bwd");
    if (vec)
        hipLaunchKernelGGL(k_pair_panel_bwd<true>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr, sel,
                           sel_order, sel_ptr, argmax, d_out, molsum, prosum, (int)Qs, (int)L, (int)Q, D, add_mol, add_pro, d_mol, d_pro);
    else
        hipLaunchKernelGGL(k_pair_panel_bwd<false>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr, sel,
                           sel_order, sel_ptr, argmax, d_out, molsum, prosum, (int)Qs, (int)L, (int)Q, D, add_mol, add_pro, d_mol, d_pro);
    GLAM_LAUNCH_CHECK("glam_pair_pool_panel_bwd");
    return GLAM_OK;
}
