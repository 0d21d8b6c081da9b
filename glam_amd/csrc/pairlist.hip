// Refillable pair lists: what ops.pair_pool_shared / pair_pool_gather_shared / pair_rows read of a step's pairs — the pair -> segment index,
// the pairs grouped by segment (order, ptr) — and the step's labels, written into tensors of FIXED addresses by ONE launch, so that a
// captured training step holds the launch and a replay follows whatever pair ids the host has put on the device since.
//
// Per present side s (Q segments, capacity P >= B, padding segment pad):
//   key(i)  = col[ids ? ids[i] : i] for i < B,  pad for B <= i < P
//   idx[i]  = key(i)
//   order   = the STABLE argsort of the keys: the slots of one segment in ascending i        (np.argsort(idx, kind="stable"))
//   ptr[q]  = the number of keys < q, ptr[Q] = P                                             ([0] + cumsum(bincount(idx, minlength=Q)))
// and y_out[i] = y[ids ? ids[i] : i] for i < B, bytewise (rows of a multiple of 4 bytes, copied as dwords).
//
// Shape.  One wave per (side, segment q); the waves never meet: no LDS, no barrier, no atomics, no workspace.  A wave walks the P keys 64
// a round (coalesced loads of ids, a gather of col) twice: the first pass counts the keys < q with __ballot / __popcll — that IS ptr[q]
// — the second writes slot i of every key == q to order[ptr[q] + rank], rank = matches in earlier rounds + matches in lower lanes of this
// round: ascending i by construction.  Every slot has exactly one key, so the waves of a side write disjoint parts of order and cover it;
// the wave of q = Q - 1 also writes ptr[Q].  The blocks behind the segment blocks write idx and y_out, grid-strided.  So every output
// word is written by every launch, by exactly one lane: no residue of the load before, nothing that depends on an order of execution.
// Work: 2 * P * Q / 64 wave rounds per side — negligible for the lists of a training step (P, Q up to a few thousand), quadratic beyond:
// the entry point refuses P or Q above kPairListMaxDim and P * Q above kPairListMaxWork (glam_pair_list_supported).
#include "common.h"

namespace glam {

constexpr int64_t kPairListMaxDim = 65536;           // P and Q each
constexpr int64_t kPairListMaxWork = 1ll << 26;      // P * Q per side: 2^21 wave rounds over 1 024 SIMDs, about 2 000 short rounds each
constexpr int kPairListWaves = kBlock / 64;
constexpr int kPairListCopyBlocks = 64;              // cap on the blocks that write idx / y_out (grid-strided beyond)

struct PairListArgs {
    const int* ids;
    const int* col[2];
    int* idx[2];
    int* order[2];
    int* ptr[2];
    int Q[2], pad[2];
    int seg_blocks[2];                               // blocks of segment waves per side (0: side absent)
    const int* y;
    int* y_out;
    int y_words;                                     // dwords per label row
    int B, P;
};

__device__ __forceinline__ int pair_list_key(const int* __restrict__ ids, const int* __restrict__ col, int i, int B, int pad) {
    return i < B ? col[ids ? ids[i] : i] : pad;
}

__global__ void __launch_bounds__(kBlock) k_pair_list_load(PairListArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int block = blockIdx.x;
    for (int s = 0; s < 2; ++s) {
        if (block >= a.seg_blocks[s]) { block -= a.seg_blocks[s]; continue; }
        // ---- one wave per segment of side s ----
        const int q = block * kPairListWaves + wave, Q = a.Q[s];
        if (q >= Q) return;
        const int* __restrict__ col = a.col[s];
        const int pad = a.pad[s];
        int before = 0;                              // keys < q: the run of q starts there
        for (int base = 0; base < a.P; base += 64) {
            const int i = base + lane;
            const int k = i < a.P ? pair_list_key(a.ids, col, i, a.B, pad) : 0x7fffffff;
            before += __popcll(__ballot(k < q));
        }
        if (lane == 0) {
            a.ptr[s][q] = before;
            if (q == Q - 1) a.ptr[s][Q] = a.P;
        }
        int* __restrict__ order = a.order[s];
        int run = 0;                                 // matches in the rounds before
        for (int base = 0; base < a.P; base += 64) {
            const int i = base + lane;
            const int k = i < a.P ? pair_list_key(a.ids, col, i, a.B, pad) : 0x7fffffff;
            const unsigned long long m = __ballot(k == q);
            if (k == q) order[before + run + __popcll(m & ((1ull << lane) - 1ull))] = i;
            run += __popcll(m);
        }
        return;
    }
    // ---- the blocks behind: idx of both sides and the labels ----
    const int stride = (int)(gridDim.x - a.seg_blocks[0] - a.seg_blocks[1]) * kBlock;
    const int t0 = block * kBlock + (int)threadIdx.x;
    for (int s = 0; s < 2; ++s) {
        if (!a.seg_blocks[s]) continue;
        for (int i = t0; i < a.P; i += stride) a.idx[s][i] = pair_list_key(a.ids, a.col[s], i, a.B, a.pad[s]);
    }
    if (a.y_out) {
        const int W = a.y_words;
        const int64_t total = (int64_t)a.B * W;      // (below 2^31: checked on the host)
        for (int64_t w = t0; w < total; w += stride) {
            const int i = (int)(w / W), c = (int)(w - (int64_t)i * W);
            a.y_out[w] = a.y[(size_t)(a.ids ? a.ids[i] : i) * W + c];
        }
    }
}

}  // namespace glam

using namespace glam;

// a STATUS, as every int of this ABI that is not listed as a value: GLAM_OK when a side of capacity P over Q segments has the kernel
extern "C" int glam_pair_list_supported(int64_t P, int64_t Q) {
    if (P > kPairListMaxDim || Q > kPairListMaxDim || (P > 0 && Q > 0 && P * Q > kPairListMaxWork))
        return fail(GLAM_E_UNSUPPORTED, "glam_pair_list: P=%lld over Q=%lld is beyond P, Q <= %lld and P * Q <= %lld (the build is O(P * Q))",
                    (long long)P, (long long)Q, (long long)kPairListMaxDim, (long long)kPairListMaxWork);
    return GLAM_OK;
}

extern "C" int glam_pair_list_load(const int32_t* ids, const int32_t* col_a, const int32_t* col_b, const void* y, int32_t y_row_bytes,
                                   int64_t B, int64_t P, int64_t Qa, int64_t Qb, int32_t pad_a, int32_t pad_b, int32_t* idx_a,
                                   int32_t* order_a, int32_t* ptr_a, int32_t* idx_b, int32_t* order_b, int32_t* ptr_b, void* y_out,
                                   void* stream) {
    GLAM_REQUIRE(P >= 1 && B >= 0 && B <= P, "glam_pair_list_load: needs 0 <= B <= P and P >= 1, got B=%lld P=%lld", (long long)B, (long long)P);
    GLAM_REQUIRE(Qa >= 0 && Qb >= 0, "glam_pair_list_load: Q out of range");
    // (before the pointers' outputs are looked at; an absent side counts with Q = 0: P alone)
    if (const int rc = glam_pair_list_supported(P, col_a ? Qa : 0)) return rc;
    if (const int rc = glam_pair_list_supported(P, col_b ? Qb : 0)) return rc;
    GLAM_REQUIRE(col_a || col_b || y, "glam_pair_list_load: no side and no labels: nothing to load");
    GLAM_REQUIRE(!col_a || (Qa >= 1 && pad_a >= 0 && pad_a < Qa && idx_a && order_a && ptr_a),
                 "glam_pair_list_load: side a needs Q >= 1, pad in [0, Q) and its three outputs");
    GLAM_REQUIRE(!col_b || (Qb >= 1 && pad_b >= 0 && pad_b < Qb && idx_b && order_b && ptr_b),
                 "glam_pair_list_load: side b needs Q >= 1, pad in [0, Q) and its three outputs");
    GLAM_REQUIRE((y != nullptr) == (y_out != nullptr), "glam_pair_list_load: y and y_out go together");
    GLAM_REQUIRE(!y || (y_row_bytes >= 4 && y_row_bytes % 4 == 0 && (((uintptr_t)y | (uintptr_t)y_out) & 3u) == 0),
                 "glam_pair_list_load: label rows must be a multiple of 4 bytes on a 4-byte boundary");
    GLAM_REQUIRE(!y || B * (int64_t)(y_row_bytes / 4) < INT32_MAX, "glam_pair_list_load: B label rows do not fit int32");
    PairListArgs a{};
    a.ids = ids;
    a.col[0] = col_a; a.col[1] = col_b;
    a.idx[0] = idx_a; a.idx[1] = idx_b;
    a.order[0] = order_a; a.order[1] = order_b;
    a.ptr[0] = ptr_a; a.ptr[1] = ptr_b;
    a.Q[0] = (int)Qa; a.Q[1] = (int)Qb;
    a.pad[0] = pad_a; a.pad[1] = pad_b;
    a.seg_blocks[0] = col_a ? (int)((Qa + kPairListWaves - 1) / kPairListWaves) : 0;
    a.seg_blocks[1] = col_b ? (int)((Qb + kPairListWaves - 1) / kPairListWaves) : 0;
    a.y = (const int*)y;
    a.y_out = (int*)y_out;
    a.y_words = y ? y_row_bytes / 4 : 0;
    a.B = (int)B;
    a.P = (int)P;
    const int64_t items = P > B * (int64_t)a.y_words ? P : B * (int64_t)a.y_words;
    const int copy_blocks = grid_for(items, kBlock, kPairListCopyBlocks);
    hipLaunchKernelGGL(k_pair_list_load, dim3((unsigned)(a.seg_blocks[0] + a.seg_blocks[1] + copy_blocks)), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    GLAM_LAUNCH_CHECK("glam_pair_list_load");
    return GLAM_OK;
}
