// The forward kernels of the per-pair fusion that more than one translation unit launches: pairpool.hip (one protein graph per pair;
// screening against proteins held once) and pairshared.hip (training against proteins held once: the same indexed kernels, which then
// also keep the argmax and the two column sums for the backward pass).  See pairpool.hip for the scheme.
#pragma once
#include "common.h"

namespace glam {

constexpr int kMolTile = 32;      // ligand rows staged per LDS pass
constexpr int kMaxD = 256;
constexpr int kPairSplit = 16;    // residue chunks (blocks) per pair in the split path
constexpr int kResChunk = 64;     // residues per chunk pass: one per lane
constexpr int kPartStride = 68;   // floats per (pair, split) partial: val, idx, pad, pad, colsum[64]

// Split path (D % 4 == 0, D <= 64).  Block (i, s): residues s*64 + k*16*64 + lane of pair i; wave q takes the ligand rows
// a = q (mod 4), two at a time (independent dot-product chains; each dot keeps the channel order of the scalar path, so
// values and argmax are those of the one-block kernel).
template <bool kIndexed>
__global__ void __launch_bounds__(kBlock) k_pair_max_partial(const float* mol, const float* pro, const int* mptr,
                                                            const int* pptr, const int* pidx, int D, float* part) {
    __shared__ __attribute__((aligned(16))) float s_mol[kMolTile * 64];
    __shared__ float s_val[kBlock];
    __shared__ int s_idx[kBlock];
    const int i = blockIdx.x / kPairSplit, sp = blockIdx.x % kPairSplit, tid = threadIdx.x;
    const int lane = tid & 63, q = tid >> 6;
    const int j = kIndexed ? pidx[i] : i;      // the pair's protein segment
    const int m0 = mptr[i], m1 = mptr[i + 1], p0 = pptr[j], p1 = pptr[j + 1];
    const int nm = m1 - m0, np = p1 - p0;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    float4 cs[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) cs[u] = f4zero();
    for (int b0 = sp * kResChunk; b0 < np; b0 += kPairSplit * kResChunk) {
        const int b = b0 + lane;
        const bool valid = b < np;
        const float* prow = pro + (size_t)(p0 + (valid ? b : 0)) * D;
        float4 pr[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            pr[u] = (valid && 4 * u < D) ? ld4(prow + 4 * u) : f4zero();
            cs[u].x += pr[u].x; cs[u].y += pr[u].y; cs[u].z += pr[u].z; cs[u].w += pr[u].w;
        }
        for (int t0 = 0; t0 < nm; t0 += kMolTile) {
            const int tn = min(kMolTile, nm - t0);
            __syncthreads();
            for (int k = tid; k < tn * D; k += kBlock) s_mol[k] = mol[(size_t)(m0 + t0) * D + k];
            __syncthreads();
            for (int a = q; a < tn; a += 8) {
                const bool two = a + 4 < tn;
                const float* r0 = s_mol + a * D;
                const float* r1 = s_mol + (two ? a + 4 : a) * D;
                float d0 = 0.f, d1 = 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    if (4 * u < D) {
                        const float4 v0 = ld4(r0 + 4 * u), v1 = ld4(r1 + 4 * u);
                        d0 = fmaf(v0.x, pr[u].x, d0); d0 = fmaf(v0.y, pr[u].y, d0); d0 = fmaf(v0.z, pr[u].z, d0); d0 = fmaf(v0.w, pr[u].w, d0);
                        d1 = fmaf(v1.x, pr[u].x, d1); d1 = fmaf(v1.y, pr[u].y, d1); d1 = fmaf(v1.z, pr[u].z, d1); d1 = fmaf(v1.w, pr[u].w, d1);
                    }
                }
                if (valid) {
                    const int i0 = (t0 + a) * np + b, i1 = (t0 + a + 4) * np + b;
                    if (pair_better(d0, i0, best, bidx)) { best = d0; bidx = i0; }
                    if (two && pair_better(d1, i1, best, bidx)) { best = d1; bidx = i1; }
                }
            }
        }
    }
    s_val[tid] = best;
    s_idx[tid] = bidx;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o && pair_better(s_val[tid + o], s_idx[tid + o], s_val[tid], s_idx[tid])) { s_val[tid] = s_val[tid + o]; s_idx[tid] = s_idx[tid + o]; }
        __syncthreads();
    }
    float* dst = part + (size_t)blockIdx.x * kPartStride;
    if (tid == 0) { dst[0] = s_val[0]; reinterpret_cast<int*>(dst)[1] = s_idx[0]; }
    if (q == 0) {                    // column sums of this block's residues (every wave loaded the same rows)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float x = group_sum<64>(cs[u].x), y = group_sum<64>(cs[u].y), z = group_sum<64>(cs[u].z), w = group_sum<64>(cs[u].w);
            if (lane == 0) st4(dst + 4 + 4 * u, make_float4(x, y, z, w));
        }
    }
}

template <bool kIndexed>
__global__ void __launch_bounds__(64) k_pair_finish(const float* mol, const int* mptr, const int* pptr, const int* pidx,
                                                   const float* part, int D, float* out, int* arg, float* sums) {
    const int i = blockIdx.x, c = threadIdx.x;
    const int j = kIndexed ? pidx[i] : i;
    const int m0 = mptr[i], m1 = mptr[i + 1], p0 = pptr[j], np = pptr[j + 1] - p0, nm = m1 - m0;
    const float* pp = part + (size_t)i * kPairSplit * kPartStride;
    float ps = 0.f, ms = 0.f;
    if (c < D) {
        for (int s = 0; s < kPairSplit; ++s) ps += pp[s * kPartStride + 4 + c];
        int a = m0;
        for (; a + 3 < m1; a += 4) {
            const float v0 = mol[(size_t)a * D + c], v1 = mol[(size_t)(a + 1) * D + c], v2 = mol[(size_t)(a + 2) * D + c],
                        v3 = mol[(size_t)(a + 3) * D + c];
            ms += v0; ms += v1; ms += v2; ms += v3;
        }
        for (; a < m1; ++a) ms += mol[(size_t)a * D + c];
        if (sums) {                  // (indexed: only the training call keeps them — the sum of the pair's OWN protein's rows)
            sums[(size_t)i * 2 * D + c] = ms;
            sums[(size_t)i * 2 * D + D + c] = ps;
        }
    }
    const float tot = group_sum<64>(ms * ps);
    if (c == 0) {
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        for (int s = 0; s < kPairSplit; ++s) {
            const float v = pp[s * kPartStride];
            const int ix = reinterpret_cast<const int*>(pp + s * kPartStride)[1];
            if (pair_better(v, ix, best, bidx)) { best = v; bidx = ix; }
        }
        const bool empty = nm <= 0 || np <= 0;
        out[2 * i] = empty ? 0.f : best;
        out[2 * i + 1] = empty ? 0.f : tot / ((float)nm * (float)np);
        if (!kIndexed || arg) {
            arg[2 * i] = empty ? -1 : m0 + bidx / np;
            arg[2 * i + 1] = empty ? -1 : p0 + bidx % np;
        }
    }
}

template <bool kIndexed>
__global__ void __launch_bounds__(kBlock) k_pair_pool_fwd(const float* mol, const float* pro, const int* mptr,
                                                         const int* pptr, const int* pidx, int D, float* out, int* arg, float* sums) {
    __shared__ __attribute__((aligned(16))) float s_mol[kMolTile * kMaxD];
    __shared__ float s_val[kBlock];
    __shared__ int s_idx[kBlock];
    __shared__ float s_sum[2 * kMaxD];
    __shared__ __attribute__((aligned(16))) float s_part[16 * 16 * 4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int j = kIndexed ? pidx[i] : i;
    const int m0 = mptr[i], m1 = mptr[i + 1], p0 = pptr[j], p1 = pptr[j + 1];
    const int nm = m1 - m0, np = p1 - p0;
    // column sums of both segments (mean)
    block_colsum(mol, m0, m1, D, s_part, s_sum);
    block_colsum(pro, p0, p1, D, s_part, s_sum + D);
    if (sums)                        // (the training call against shared proteins: its backward reads them instead of summing again)
        for (int c = tid; c < 2 * D; c += kBlock) sums[(size_t)i * 2 * D + c] = s_sum[c];
    float best = -INFINITY;
    int bidx = 0x7fffffff;          // flattened (a * np + b): first occurrence wins ties, like a flattened argmax
    const bool vec = (D & 3) == 0 && D <= 64;
    for (int t0 = 0; t0 < nm; t0 += kMolTile) {
        const int tn = min(kMolTile, nm - t0);
        __syncthreads();
        for (int k = tid; k < tn * D; k += kBlock) s_mol[k] = mol[(size_t)(m0 + t0) * D + k];
        __syncthreads();
        for (int b = tid; b < np; b += kBlock) {
            const float* prow = pro + (size_t)(p0 + b) * D;
            if (vec) {
                // the residue row lives in registers (one set of loads per residue instead of one per ligand row); the ligand
                // rows are LDS broadcasts.  Same c order as the scalar path: identical dot products and argmax.
                float4 pr[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) pr[u] = 4 * u < D ? ld4(prow + 4 * u) : f4zero();
                for (int a = 0; a < tn; ++a) {
                    float d = 0.f;
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        if (4 * u < D) {
                            const float4 mv = ld4(s_mol + a * D + 4 * u);
                            d = fmaf(mv.x, pr[u].x, d); d = fmaf(mv.y, pr[u].y, d); d = fmaf(mv.z, pr[u].z, d); d = fmaf(mv.w, pr[u].w, d);
                        }
                    }
                    const int idx = (t0 + a) * np + b;
                    if (d > best || (d == best && idx < bidx)) { best = d; bidx = idx; }
                }
            } else {
                for (int a = 0; a < tn; ++a) {
                    float d = 0.f;
                    for (int c = 0; c < D; ++c) d = fmaf(s_mol[a * D + c], prow[c], d);
                    const int idx = (t0 + a) * np + b;
                    if (d > best || (d == best && idx < bidx)) { best = d; bidx = idx; }
                }
            }
        }
    }
    s_val[tid] = best;
    s_idx[tid] = bidx;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const float v = s_val[tid + o];
            const int ix = s_idx[tid + o];
            if (v > s_val[tid] || (v == s_val[tid] && ix < s_idx[tid])) { s_val[tid] = v; s_idx[tid] = ix; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        float tot = 0.f;
        for (int c = 0; c < D; ++c) tot = fmaf(s_sum[c], s_sum[D + c], tot);
        const bool empty = nm <= 0 || np <= 0;
        out[2 * i] = empty ? 0.f : s_val[0];
        out[2 * i + 1] = empty ? 0.f : tot / ((float)nm * (float)np);
        if (!kIndexed || arg) {
            arg[2 * i] = empty ? -1 : m0 + s_idx[0] / np;
            arg[2 * i + 1] = empty ? -1 : p0 + s_idx[0] % np;
        }
    }
}

}  // namespace glam
