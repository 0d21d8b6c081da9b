// Training the two-tower model against proteins that are held ONCE (a LIT-PCBA step: 32 ligands, one target): the indexed fusion
// of pairpool.hip with a backward pass.
//   forward   glam_pair_pool_shared_fwd: the kernels of glam_pair_pool_indexed_fwd (pairpool_kernels.h, kIndexed = true), which here
//             always keep the argmax and, per pair, the column sums of its ligand rows and of its protein's residue rows.
//   backward  glam_pair_pool_shared_bwd, ONE launch with two block roles (the roles share no data, so nothing orders them):
//             d_mol  one block per pair — the expression of k_pair_pool_bwd_split / k_pair_pool_bwd, the protein read through the index;
//             d_pro  the gradient of a residue row is a sum over every pair that points at its protein.  The host hands the pairs
//                    sorted by protein (pair_order / pair_ptr, a stable sort), block (q, s) owns the residue rows s*16 + k*32*16 + r of
//                    protein q and walks q's pair list for them:
//                      S_q = sum_i gmean_i * msum_i                (the same for every row: once per block, pairs in list order)
//                      d_pro[b] = S_q, then fmaf(gmax_i, mol[am_i], .) for the pairs whose maximum sits on row b, in list order
//                    No atomics; the order depends on the list alone, never on the grid or on timing.
//   glam_pair_rows_bwd: d_flat[q] = sum of d_rows[i] over q's pairs in list order (the backward of gathering a [Q, W] matrix by pair).
// The pair list is walked in tiles staged in LDS: what is block-uniform (a pair's index, gradient scale, argmax) is loaded once per
// tile by one lane each and then broadcast, the [tile, D] addends are loaded by the whole block with every load independent of the
// others, and only the add chain itself is serial.
#include "pairpool_kernels.h"

namespace glam {

constexpr int kProSplit = 32;     // blocks per protein in the d_pro role
constexpr int kProRows = 16;      // residue rows a block owns per sweep
constexpr int kSumTile = 64;      // pairs per staged tile of addends (vector form: [64, 64] floats)

// (empty pair: no contribution — the flag is the index -1)
__device__ __forceinline__ void shared_meta(const int* mptr, const int* order, const float* d_out, int np, int k, int* s_i, float* s_gm) {
    const int i = order[k];
    const int nm = mptr[i + 1] - mptr[i];
    const bool empty = nm <= 0 || np <= 0;
    s_i[threadIdx.x] = empty ? -1 : i;
    s_gm[threadIdx.x] = empty ? 0.f : d_out[2 * i + 1] / ((float)nm * (float)np);
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock) k_pair_shared_bwd(const float* mol, const float* pro, const int* mptr, const int* pptr,
                                                           const int* pidx, const int* order, const int* qptr, const int* arg,
                                                           const float* sums, const float* d_out, int Q, int D, const float* add_mol,
                                                           const float* add_pro, float* d_mol, float* d_pro) {
    const int tid = threadIdx.x;
    const int pro_blocks = Q * kProSplit;
    if ((int)blockIdx.x >= pro_blocks) {
        // ---- d_mol of pair i ----
        const int i = blockIdx.x - pro_blocks;
        const int j = pidx[i];
        const int m0 = mptr[i], m1 = mptr[i + 1], nm = m1 - m0, np = pptr[j + 1] - pptr[j];
        const bool empty = nm <= 0 || np <= 0;
        const float gmax = empty ? 0.f : d_out[2 * i], gmean = empty ? 0.f : d_out[2 * i + 1] / ((float)nm * (float)np);
        const int am = empty ? -1 : arg[2 * i], ap = empty ? -1 : arg[2 * i + 1];
        if constexpr (kVec) {
            const int c4 = tid & 15, rg = tid >> 4;
            if (4 * c4 >= D) return;
            const float4 psum = empty ? f4zero() : gmean * ld4(sums + (size_t)i * 2 * D + D + 4 * c4);
            for (int a = m0 + rg; a < m1; a += 16) {
                float4 v = psum;
                if (a == am) {
                    const float4 t = ld4(pro + (size_t)ap * D + 4 * c4);
                    v.x = fmaf(gmax, t.x, v.x); v.y = fmaf(gmax, t.y, v.y); v.z = fmaf(gmax, t.z, v.z); v.w = fmaf(gmax, t.w, v.w);
                }
                if (add_mol) { const float4 t = ld4(add_mol + (size_t)a * D + 4 * c4); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
                st4(d_mol + (size_t)a * D + 4 * c4, v);
            }
        } else {
            for (int k = tid; k < max(nm, 0) * D; k += kBlock) {
                const int a = m0 + k / D, c = k % D;
                float v = 0.f;
                if (!empty) v = gmean * sums[(size_t)i * 2 * D + D + c] + (a == am ? gmax * pro[(size_t)ap * D + c] : 0.f);
                if (add_mol) v += add_mol[(size_t)a * D + c];
                d_mol[(size_t)a * D + c] = v;
            }
        }
        return;
    }
    // ---- d_pro of the rows of protein q this block owns ----
    __shared__ int s_i[kBlock];
    __shared__ float s_gm[kBlock];
    __shared__ int s_ap[kBlock], s_am[kBlock];
    __shared__ float s_g[kBlock];
    __shared__ unsigned long long s_mask[kBlock / 64];
    const int q = blockIdx.x / kProSplit, sp = blockIdx.x % kProSplit;
    const int p0 = pptr[q], p1 = pptr[q + 1], np = p1 - p0;
    const int k0 = qptr[q], k1 = qptr[q + 1];
    if (sp * kProRows >= np) return;          // (block-uniform, before the first barrier)
    // S_q, pairs in list order
    float S = 0.f;                            // vector form: of column tid (tid < D); general form: the same
    if constexpr (kVec) {
        __shared__ __attribute__((aligned(16))) float s_tile[kSumTile * 64];
        for (int t0 = k0; t0 < k1; t0 += kSumTile) {
            const int tn = min(kSumTile, k1 - t0);
            __syncthreads();
            if (tid < tn) shared_meta(mptr, order, d_out, np, t0 + tid, s_i, s_gm);
            __syncthreads();
            for (int e = tid; e < tn * 16; e += kBlock) {
                const int k = e >> 4, c4 = e & 15;
                if (4 * c4 < D) {
                    const int i = s_i[k];
                    st4(s_tile + k * 64 + 4 * c4, i < 0 ? f4zero() : s_gm[k] * ld4(sums + (size_t)i * 2 * D + 4 * c4));
                }
            }
            __syncthreads();
            if (tid < D)
                for (int k = 0; k < tn; ++k) S += s_tile[k * 64 + tid];
        }
    } else {
        for (int t0 = k0; t0 < k1; t0 += kBlock) {
            const int tn = min(kBlock, k1 - t0);
            __syncthreads();
            if (tid < tn) shared_meta(mptr, order, d_out, np, t0 + tid, s_i, s_gm);
            __syncthreads();
            if (tid < D)
                for (int k = 0; k < tn; ++k) {
                    const int i = s_i[k];
                    if (i >= 0) S += s_gm[k] * sums[(size_t)i * 2 * D + tid];
                }
        }
    }
    __shared__ __attribute__((aligned(16))) float s_S[kMaxD];
    __shared__ float s_acc[kVec ? 1 : kProRows * kMaxD];
    __syncthreads();
    if (tid < D) s_S[tid] = S;
    __syncthreads();
    const int c4 = tid & 15, rg = tid >> 4;
    for (int b0 = p0 + sp * kProRows; b0 < p1; b0 += kProSplit * kProRows) {
        float4 v = f4zero();
        if constexpr (kVec) {
            if (4 * c4 < D) v = ld4(s_S + 4 * c4);
        } else {
            if (tid < D)
                for (int r = 0; r < kProRows; ++r) s_acc[r * kMaxD + tid] = S;     // (a thread touches its own column only: no barrier)
        }
        // the pairs whose maximum sits on one of the rows b0 .. b0 + 15, in list order
        for (int t0 = k0; t0 < k1; t0 += kBlock) {
            const int k = t0 + tid;
            bool hit = false;
            __syncthreads();
            if (k < k1) {
                const int i = order[k];
                const int nm = mptr[i + 1] - mptr[i];
                const int ap = nm <= 0 ? -1 : arg[2 * i + 1];          // (np > 0 here: the block owns rows)
                hit = ap >= b0 && ap < b0 + kProRows;
                s_ap[tid] = ap;
                s_am[tid] = arg[2 * i];
                s_g[tid] = d_out[2 * i];
            }
            const unsigned long long m = __ballot(hit);
            if ((tid & 63) == 0) s_mask[tid >> 6] = m;
            __syncthreads();
            for (int w = 0; w < kBlock / 64; ++w) {
                unsigned long long left = s_mask[w];
                while (left) {
                    const int kk = w * 64 + __builtin_ctzll(left);
                    left &= left - 1;
                    const int ap = s_ap[kk], am = s_am[kk];
                    const float g = s_g[kk];
                    if constexpr (kVec) {
                        if (ap == b0 + rg && 4 * c4 < D) {
                            const float4 t = ld4(mol + (size_t)am * D + 4 * c4);
                            v.x = fmaf(g, t.x, v.x); v.y = fmaf(g, t.y, v.y); v.z = fmaf(g, t.z, v.z); v.w = fmaf(g, t.w, v.w);
                        }
                    } else {
                        if (tid < D) {
                            float* acc = s_acc + (ap - b0) * kMaxD + tid;
                            *acc = fmaf(g, mol[(size_t)am * D + tid], *acc);
                        }
                    }
                }
            }
        }
        if constexpr (kVec) {
            const int b = b0 + rg;
            if (b < p1 && 4 * c4 < D) {
                if (add_pro) { const float4 t = ld4(add_pro + (size_t)b * D + 4 * c4); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
                st4(d_pro + (size_t)b * D + 4 * c4, v);
            }
        } else {
            if (tid < D)
                for (int r = 0; r < kProRows && b0 + r < p1; ++r) {
                    float x = s_acc[r * kMaxD + tid];
                    if (add_pro) x += add_pro[(size_t)(b0 + r) * D + tid];
                    d_pro[(size_t)(b0 + r) * D + tid] = x;
                }
        }
    }
}

// d_flat[q, c] = sum over q's pairs (list order) of d_rows[i, c].  Block (q, 64-column chunk): a tile of 64 rows is loaded by the four
// waves side by side (wave w the rows w, w + 4, ...), then wave 0 adds them in list order.
__global__ void __launch_bounds__(kBlock) k_pair_rows_bwd(const float* d_rows, const int* order, const int* qptr, int W, int chunks,
                                                         float* d_flat) {
    __shared__ int s_i[kSumTile];
    __shared__ float s_tile[kSumTile * 64];
    const int q = blockIdx.x / chunks, c = (blockIdx.x % chunks) * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6, tid = threadIdx.x;
    const int k0 = qptr[q], k1 = qptr[q + 1];
    float acc = 0.f;
    for (int t0 = k0; t0 < k1; t0 += kSumTile) {
        const int tn = min(kSumTile, k1 - t0);
        __syncthreads();
        if (tid < tn) s_i[tid] = order[t0 + tid];
        __syncthreads();
        if (c < W)
            for (int k = w; k < tn; k += kBlock / 64) s_tile[k * 64 + (tid & 63)] = d_rows[(size_t)s_i[k] * W + c];
        __syncthreads();
        if (w == 0 && c < W)
            for (int k = 0; k < tn; ++k) acc += s_tile[k * 64 + tid];
    }
    if (w == 0 && c < W) d_flat[(size_t)q * W + c] = acc;
}

}  // namespace glam

using namespace glam;

static bool pair_split(int D) { return (D & 3) == 0 && D <= 64; }

extern "C" int glam_pair_pool_shared_fwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                                         const int32_t* pro_of_pair, int64_t P, int64_t Q, int D, float* out, int32_t* argmax,
                                         float* sums, void* ws, size_t ws_bytes, void* stream) {
    GLAM_REQUIRE(P >= 0 && P < INT32_MAX / kPairSplit, "glam_pair_pool_shared_fwd: P out of range");
    GLAM_REQUIRE(Q >= 0 && Q < INT32_MAX, "glam_pair_pool_shared_fwd: Q out of range");
    if (D <= 0 || D > kMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_shared_fwd: D=%d not in 1..%d", D, kMaxD);
    if (P == 0) return GLAM_OK;
    GLAM_REQUIRE(Q > 0, "glam_pair_pool_shared_fwd: pairs but no protein segment");
    GLAM_REQUIRE(mol && pro && mol_ptr && pro_ptr && pro_of_pair && out && argmax && sums, "glam_pair_pool_shared_fwd: null pointer");
    if (pair_split(D)) {
        GLAM_REQUIRE(aligned16(mol) && aligned16(pro), "glam_pair_pool_shared_fwd: rows must be 16-byte aligned");
        GLAM_REQUIRE(ws && ws_bytes >= glam_pair_pool_workspace_bytes(P, D), "glam_pair_pool_shared_fwd: workspace too small");
        hipLaunchKernelGGL(k_pair_max_partial<true>, dim3((int)P * kPairSplit), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr,
                           pro_ptr, pro_of_pair, D, (float*)ws);
        hipLaunchKernelGGL(k_pair_finish<true>, dim3((int)P), dim3(64), 0, (hipStream_t)stream, mol, mol_ptr, pro_ptr, pro_of_pair,
                           (const float*)ws, D, out, argmax, sums);
    } else {
        hipLaunchKernelGGL(k_pair_pool_fwd<true>, dim3((int)P), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr,
                           pro_of_pair, D, out, argmax, sums);
    }
    GLAM_LAUNCH_CHECK("glam_pair_pool_shared_fwd");
    return GLAM_OK;
}

// pair_order / pair_ptr: the pairs stably sorted by protein and the Q + 1 offsets of the proteins' runs (built and checked by the
// host, trusted here, like pro_of_pair).  add_mol / add_pro may be NULL.
extern "C" int glam_pair_pool_shared_bwd(const float* mol, const float* pro, const int32_t* mol_ptr, const int32_t* pro_ptr,
                                         const int32_t* pro_of_pair, const int32_t* pair_order, const int32_t* pair_ptr,
                                         const int32_t* argmax, const float* sums, const float* d_out, int64_t P, int64_t Q, int D,
                                         const float* add_mol, const float* add_pro, float* d_mol, float* d_pro, void* stream) {
    GLAM_REQUIRE(P >= 0 && P < INT32_MAX / kPairSplit, "glam_pair_pool_shared_bwd: P out of range");
    GLAM_REQUIRE(Q >= 0 && Q < INT32_MAX / (2 * kProSplit), "glam_pair_pool_shared_bwd: Q out of range");
    if (D <= 0 || D > kMaxD) return fail(GLAM_E_UNSUPPORTED, "glam_pair_pool_shared_bwd: D=%d not in 1..%d", D, kMaxD);
    if (P == 0) return GLAM_OK;
    GLAM_REQUIRE(Q > 0, "glam_pair_pool_shared_bwd: pairs but no protein segment");
    GLAM_REQUIRE(mol && pro && mol_ptr && pro_ptr && pro_of_pair && pair_order && pair_ptr && argmax && sums && d_out && d_mol && d_pro,
                 "glam_pair_pool_shared_bwd: null pointer");
    const int grid = (int)Q * kProSplit + (int)P;
    if (pair_split(D)) {
        GLAM_REQUIRE(aligned16(mol) && aligned16(pro) && aligned16(sums) && aligned16(d_mol) && aligned16(d_pro) && aligned16(add_mol) &&
                         aligned16(add_pro), "glam_pair_pool_shared_bwd: rows must be 16-byte aligned");
        hipLaunchKernelGGL(k_pair_shared_bwd<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr, pro_of_pair,
                           pair_order, pair_ptr, argmax, sums, d_out, (int)Q, D, add_mol, add_pro, d_mol, d_pro);
    } else {
        hipLaunchKernelGGL(k_pair_shared_bwd<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, mol, pro, mol_ptr, pro_ptr, pro_of_pair,
                           pair_order, pair_ptr, argmax, sums, d_out, (int)Q, D, add_mol, add_pro, d_mol, d_pro);
    }
    GLAM_LAUNCH_CHECK("glam_pair_pool_shared_bwd");
    return GLAM_OK;
}

extern "C" int glam_pair_rows_bwd(const float* d_rows, const int32_t* pair_order, const int32_t* pair_ptr, int64_t P, int64_t Q, int W,
                                  float* d_flat, void* stream) {
    GLAM_REQUIRE(P >= 0 && P < INT32_MAX, "glam_pair_rows_bwd: P out of range");
    GLAM_REQUIRE(Q >= 0 && Q < INT32_MAX && W > 0, "glam_pair_rows_bwd: Q / W out of range");
    if (P == 0) return GLAM_OK;                 // (nothing is written: the caller's zeros stand)
    GLAM_REQUIRE(Q > 0, "glam_pair_rows_bwd: pairs but no row to sum them into");
    const int64_t chunks = ((int64_t)W + 63) / 64;
    GLAM_REQUIRE(Q * chunks < INT32_MAX, "glam_pair_rows_bwd: Q x W out of range");
    GLAM_REQUIRE(d_rows && pair_order && pair_ptr && d_flat, "glam_pair_rows_bwd: null pointer");
    hipLaunchKernelGGL(k_pair_rows_bwd, dim3((int)(Q * chunks)), dim3(kBlock), 0, (hipStream_t)stream, d_rows, pair_order, pair_ptr, W,
                       (int)chunks, d_flat);
    GLAM_LAUNCH_CHECK("glam_pair_rows_bwd");
    return GLAM_OK;
}
