// GCN aggregation read from a batch's OWN CSR: PyG's add_remaining_self_loops + gcn_norm with unit edge weights as a
// closed form over the raw edge list — no derived edge list, no per-edge norm vector, nothing cached on the host, so it stays true on a
// batch that a kernel rewrites in place (glam_amd.data.ResidentDTIRefillBatch).
//
//   deg[i] = 1 + #{e -> i : src_e != i}                      dis[i] = 1 / sqrt(deg[i])
//   out[i] = dis[i] * ( dis[i] * x[i] + sum_{e -> i, src_e != i} dis[src_e] * x[src_e] )
//
// Existing self-loops are skipped, every node gets exactly one implicit loop, duplicate edges count as often as they occur, an isolated
// node returns x[i].  The backward is the same sum over the CSR by source with g in place of x, so forward and backward are one body.
//
// Summation order (fixed): the OWN term first — acc = dis[i] * x[i] — then the row's edges in CSR order, one fmaf(dis[s], x[s], acc) per
// kept edge, then one multiply by dis[i].  Every output word is written by exactly one lane, no atomics, no workspace: two runs agree bit
// for bit.
//
// Lane layout.  G consecutive lanes own one node (G = 16 for D <= 64, 32 for D <= 128), each lane four channels: on the 16-byte path
// (D % 4 == 0, aligned rows) the float4 at 4 * lane, so a group reads a source row as one contiguous run of up to 512 bytes; on the scalar
// path the channels lane + G * r, r < 4, again contiguous across the group.  The row's index entries are read G at a time, one per lane
// (coalesced), together with dis[src]; the group then walks them by broadcast (ds_bpermute inside the group), four rows in flight.  A round
// whose G entries are all self-loops is skipped on one ballot: a phantom node of a padded batch carries a run of thousands of self-loops,
// which costs it E_run / G index reads and no row traffic.  Residue graphs have 10 - 30 contacts per residue: one or two rounds.  A thread
// per (node, float4) as in k_edge_wsum1_fwd_v4 would walk such a run entry by entry on a dependent compare.
#include "common.h"

namespace glam {

template <int G>
__device__ __forceinline__ unsigned group_bits(unsigned long long m, int gbase) {
    return (unsigned)(m >> gbase) & (G == 32 ? 0xffffffffu : ((1u << G) - 1u));
}

// dis[i] from the CSR by target: 16 lanes per node, a popcount per round
__global__ void __launch_bounds__(kBlock) k_gcn_scale(const int* __restrict__ rowptr, const int* __restrict__ src, int N, float* __restrict__ dis) {
    constexpr int G = 16;
    const int lane = threadIdx.x & 63, l = lane & (G - 1), gbase = lane & ~(G - 1);
    const int groups = (int)gridDim.x * (kBlock / G);
    for (int i = (int)blockIdx.x * (kBlock / G) + (int)(threadIdx.x / G); i < N; i += groups) {
        const int beg = rowptr[i], end = rowptr[i + 1];
        int deg = 1;
        for (int base = beg; base < end; base += G) {
            const int e = base + l;
            const bool kept = e < end && src[e] != i;
            deg += __popc(group_bits<G>(__ballot(kept), gbase));
        }
        if (l == 0) dis[i] = 1.0f / sqrtf((float)deg);
    }
}

template <int G, bool V4>
__device__ __forceinline__ void gcn_load(const float* __restrict__ row, int l, int D, float (&v)[4]) {
    if constexpr (V4) {
        if (4 * l < D) {
            const float4 t = ld4(row + 4 * l);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (l + G * r < D) v[r] = row[l + G * r];
    }
}

template <int G, bool V4>
__device__ __forceinline__ void gcn_body(const float* __restrict__ x, int ld, const float* __restrict__ dis, const int* __restrict__ ptr,
                                         const int* __restrict__ nbr, int N, int D, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, l = lane & (G - 1), gbase = lane & ~(G - 1);
    const int groups = (int)gridDim.x * (kBlock / G);
    for (int i = (int)blockIdx.x * (kBlock / G) + (int)(threadIdx.x / G); i < N; i += groups) {
        const int beg = ptr[i], end = ptr[i + 1];
        const float di = dis[i];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        gcn_load<G, V4>(x + (size_t)i * ld, l, D, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = di * acc[r];                       // the own term first
        for (int base = beg; base < end; base += G) {
            const int e = base + l;
            int s = i;                                                           // (a lane past the row's end: skipped like a self-loop)
            if (e < end) s = nbr[e];
            const bool kept = s != i && (unsigned)s < (unsigned)N;
            const float w = kept ? dis[s] : 0.f;
            if (!kept) s = i;
            if (group_bits<G>(__ballot(kept), gbase) == 0u) continue;           // a round of self-loops: no row is read
            const int cnt = min(G, end - base);
            for (int k = 0; k < cnt; k += 4) {
                int sk[4];
                float wk[4], v[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {                                    // (k + u < G; lanes k + u >= cnt hold s = i: skipped)
                    sk[u] = __shfl(s, gbase + k + u, 64);
                    wk[u] = __shfl(w, gbase + k + u, 64);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[u][r] = 0.f;
                    if (sk[u] != i) gcn_load<G, V4>(x + (size_t)sk[u] * ld, l, D, v[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (sk[u] != i) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[r] = fmaf(wk[u], v[u][r], acc[r]);
                    }
            }
        }
        float* __restrict__ o = out + (size_t)i * D;
        if constexpr (V4) {
            if (4 * l < D) st4(o + 4 * l, make_float4(di * acc[0], di * acc[1], di * acc[2], di * acc[3]));
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (l + G * r < D) o[l + G * r] = di * acc[r];
        }
    }
}

// two names for the one body: the kernel timer (glam_prof_*) tells the forward launch from the backward one
template <int G, bool V4>
__global__ void __launch_bounds__(kBlock) k_gcn_fwd(const float* x, int ld, const float* dis, const int* rowptr, const int* src, int N, int D,
                                                    float* out) {
    gcn_body<G, V4>(x, ld, dis, rowptr, src, N, D, out);
}
template <int G, bool V4>
__global__ void __launch_bounds__(kBlock) k_gcn_bwd(const float* g, int ld, const float* dis, const int* colptr, const int* dst, int N, int D,
                                                    float* d_x) {
    gcn_body<G, V4>(g, ld, dis, colptr, dst, N, D, d_x);
}

constexpr int kGcnMaxD = 128;

static int gcn_check(const char* fn, const void* x, int64_t ld, const void* dis, const void* ptr, const void* nbr, int64_t N, int D,
                     const void* out) {
    if (N < 0 || N >= INT32_MAX) return fail(GLAM_E_INVALID, "%s: N=%lld out of range", fn, (long long)N);
    if (D < 1 || D > kGcnMaxD) return fail(GLAM_E_UNSUPPORTED, "%s: D=%d not in 1..%d", fn, D, kGcnMaxD);
    if (ld < D || ld >= INT32_MAX) return fail(GLAM_E_INVALID, "%s: row stride %lld below D=%d", fn, (long long)ld, D);
    if (N > 0 && !(x && dis && ptr && out)) return fail(GLAM_E_INVALID, "%s: null pointer", fn);
    (void)nbr;                                           // (may be NULL for an edge list without edges)
    return GLAM_OK;
}

template <bool BWD>
static void gcn_launch(const float* x, int ld, const float* dis, const int* ptr, const int* nbr, int N, int D, float* out, hipStream_t s) {
    const bool v4 = (D & 3) == 0 && (ld & 3) == 0 && aligned16(x) && aligned16(out);
    const int G = D <= 64 ? 16 : 32;
    const dim3 grid(grid_for(N, kBlock / G)), block(kBlock);
#define GLAM_GCN_GO(GG, VV)                                                                                  \
    do {                                                                                                     \
        if (BWD) hipLaunchKernelGGL((k_gcn_bwd<GG, VV>), grid, block, 0, s, x, ld, dis, ptr, nbr, N, D, out); \
        else hipLaunchKernelGGL((k_gcn_fwd<GG, VV>), grid, block, 0, s, x, ld, dis, ptr, nbr, N, D, out);     \
    } while (0)
    GLAM_PROF_LABEL(BWD ? "k_gcn_bwd" : "k_gcn_fwd");
    if (G == 16 && v4) GLAM_GCN_GO(16, true);
    else if (G == 16) GLAM_GCN_GO(16, false);
    else if (v4) GLAM_GCN_GO(32, true);
    else GLAM_GCN_GO(32, false);
#undef GLAM_GCN_GO
}

}  // namespace glam

using namespace glam;

extern "C" int glam_gcn_scale(const int32_t* rowptr, const int32_t* src, int64_t N, float* dis, void* stream) {
    if (N < 0 || N >= INT32_MAX) return fail(GLAM_E_INVALID, "glam_gcn_scale: N=%lld out of range", (long long)N);
    if (N == 0) return GLAM_OK;
    GLAM_REQUIRE(rowptr && dis, "glam_gcn_scale: null pointer");
    hipLaunchKernelGGL(k_gcn_scale, dim3(grid_for(N, kBlock / 16)), dim3(kBlock), 0, (hipStream_t)stream, rowptr, src, (int)N, dis);
    GLAM_LAUNCH_CHECK("glam_gcn_scale");
    return GLAM_OK;
}

extern "C" int glam_gcn_fwd(const float* xw, int64_t ld, const float* dis, const int32_t* rowptr, const int32_t* src, int64_t N, int32_t D,
                            float* out, void* stream) {
    if (const int rc = gcn_check("glam_gcn_fwd", xw, ld, dis, rowptr, src, N, D, out)) return rc;
    if (N == 0) return GLAM_OK;
    gcn_launch<false>(xw, (int)ld, dis, rowptr, src, (int)N, D, out, (hipStream_t)stream);
    GLAM_LAUNCH_CHECK("glam_gcn_fwd");
    return GLAM_OK;
}

extern "C" int glam_gcn_bwd(const float* g, const float* dis, const int32_t* colptr, const int32_t* dst, int64_t N, int32_t D, float* d_xw,
                            void* stream) {
    if (const int rc = gcn_check("glam_gcn_bwd", g, D, dis, colptr, dst, N, D, d_xw)) return rc;
    if (N == 0) return GLAM_OK;
    gcn_launch<true>(g, D, dis, colptr, dst, (int)N, D, d_xw, (hipStream_t)stream);
    GLAM_LAUNCH_CHECK("glam_gcn_bwd");
    return GLAM_OK;
}
