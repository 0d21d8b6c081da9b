// Screening hit lists: the best K candidates per query column, kept on the device while score batches stream past.
//   state (the caller's): top_score f32[Qs, K], top_id int32[Qs, K] — every list sorted best first, empty slots (id -1, score NaN) last —
//       and seen int64[1], the number of candidates offered so far (the default id of candidate l of a call is *seen + l);
//   one call merges score[l * ld_row + j * ld_col], l < L, j < Qs, into list j.
//
// Order.  ONE total order, and the lists are exact under it: better score first (larger if `largest`, smaller if not; -0.0 == +0.0),
// equal scores by ascending id, NaN after every number (among themselves by ascending id), empty slots last.  A 64-bit key turns it into
// an unsigned descending sort: high word = the monotone uint32 image of the score (zeros canonicalised, negated for largest = 0; 0 for a
// NaN — the image of -inf is 0x007fffff, so nothing real gets there), low word = 0xffffffff - id (>= 0x80000000 for an id <= 2^31 - 1);
// the whole key is 0 for an empty slot, below every candidate's.  The key loses the sign of a zero and the payload of a NaN and the
// lists store the ORIGINAL bits, so an entry is (key, bits) — 12 bytes — and the sort compares (key, bits): among entries of one key
// (only a caller's repeated id with an equal score) the larger bit pattern goes first, which keeps the result a function of the
// candidates alone whatever the grid.
//
// Shape.  k_hits_slab, grid Qs x S: a block takes one column and one slab of the L candidates, 256 a round, one per thread.  A candidate
// survives when its key reaches the threshold — the key of the column's last slot (lists are sorted: that is the K-th; 0 while the list
// has room) and, once the block holds K of its own, its own K-th.  With warm lists almost nothing passes.  Survivors are
// ballot-compacted (wave ballots + the four waves' counts through LDS: positions are those of the candidates, no atomics) behind the
// block's sorted partial list in ONE LDS array of 2 048 entries; when the next round might not fit, and at the end, the array is
// bitonic-sorted and cut to K.  The block writes its partial (keys, bits, count) to the workspace.  k_hits_finish, one block per
// column: the old list and the S partials go through the same append-and-sort into the new list; thread 0 of block 0 then adds L to
// *seen, which nothing else in that launch touches (k_hits_slab only reads it, a launch earlier on the stream).
// No float atomics, no atomics at all; the result does not depend on S, on the grid or on the order blocks run in.  Static LDS:
// 2 048 x 12 bytes and a few counters, 24 616 bytes.  Two launches per call, one after the other on the caller's stream: capturable, no branches.
#include <algorithm>

#include "common.h"

namespace glam {

constexpr int kHitsMaxK = 1024;
constexpr int kHitsCap = 2048;               // entries of the LDS array: a full list + at least 1 024 staged survivors
constexpr int kHitsMinSlab = 64;             // candidates per slab at the least (also bounds S for the workspace)
constexpr int kHitsMaxSlabs = 64;
constexpr int kHitsAutoSlab = 1024;          // automatic S: slabs of about this many candidates ...
constexpr int kHitsAutoBlocks = 512;         // ... while the grid stays within about this many blocks
constexpr unsigned kHitsNaNBits = 0x7fc00000u;

__device__ __forceinline__ unsigned long long hits_key(unsigned bits, int id, int largest) {
    unsigned hi = 0;                                                          // NaN
    if ((bits & 0x7fffffffu) <= 0x7f800000u) {
        unsigned b = (bits << 1) == 0 ? 0u : (largest ? bits : bits ^ 0x80000000u);
        hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((unsigned long long)hi << 32) | (0xffffffffu - (unsigned)id);
}

__device__ __forceinline__ bool hits_before(unsigned long long ka, unsigned va, unsigned long long kb, unsigned vb) {
    return ka > kb || (ka == kb && va > vb);
}

// Entries [0, m) of (key, val) -> sorted, best first (bitonic over the next power of two, padded with empty keys).  Whole block; ends
// with a barrier.  m <= kHitsCap.
__device__ void hits_sort(unsigned long long* key, unsigned* val, int m) {
    const int tid = threadIdx.x;
    int n = 2;
    while (n < m) n <<= 1;
    for (int i = m + tid; i < n; i += kBlock) { key[i] = 0ull; val[i] = 0u; }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += kBlock) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const unsigned long long ka = key[a], kb = key[b];
                const unsigned va = val[a], vb = val[b];
                const bool down = (a & k) == 0;                               // this run is sorted best first
                if (down ? hits_before(kb, vb, ka, va) : hits_before(ka, va, kb, vb)) {
                    key[a] = kb; key[b] = ka; val[a] = vb; val[b] = va;
                }
            }
            __syncthreads();
        }
    }
}

struct HitsLds {
    unsigned long long key[kHitsCap];
    unsigned val[kHitsCap];
    int wave_count[2][kBlock / 64];
    int have;
};

// The sorted prefix [0, have) and the cnt entries staged behind it -> the sorted best min(have + cnt, K).  Returns the new `have`.
__device__ __forceinline__ int hits_flush(HitsLds& s, int have, int cnt, int K) {
    if (cnt > 0) hits_sort(s.key, s.val, have + cnt);                         // (nothing staged: the prefix is sorted as it is)
    return min(have + cnt, K);
}

// grid: Qs * S blocks, the slab fastest.  ws_key / ws_val [Qs * S][K], ws_count [Qs * S].
__global__ void __launch_bounds__(kBlock) k_hits_slab(const float* __restrict__ score, long long ld_row, long long ld_col,
                                                     const int* __restrict__ ids, const long long* __restrict__ seen, int L, int K, int S,
                                                     int largest, const float* __restrict__ top_score, const int* __restrict__ top_id,
                                                     unsigned long long* __restrict__ ws_key, unsigned* __restrict__ ws_val,
                                                     int* __restrict__ ws_count) {
    __shared__ HitsLds s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x / S, sl = blockIdx.x % S;
    const int per = (int)(((long long)L + S - 1) / S);
    const int l0 = min((long long)L, (long long)sl * per), l1 = (int)min((long long)L, (long long)l0 + per);
    const size_t last = (size_t)j * K + (K - 1);
    const int last_id = top_id[last];
    unsigned long long thr = last_id < 0 ? 0ull : hits_key(__float_as_uint(top_score[last]), last_id, largest);
    const long long id0 = ids ? 0 : *seen;
    const float* col = score + (size_t)j * ld_col;
    int have = 0, cnt = 0;
    int round = 0;
    for (long long base = l0; base < l1; base += kBlock, ++round) {                // (64-bit: L may sit just below 2^31)
        const long long l = base + tid;
        unsigned bits = 0;
        unsigned long long key = 0;
        bool pass = false;
        if (l < l1) {
            bits = __float_as_uint(ld1g(col + (size_t)l * ld_row));
            key = hits_key(bits, ids ? ids[l] : (int)(id0 + l), largest);
            pass = key >= thr;
        }
        const unsigned long long m = __ballot(pass);
        if (lane == 0) s.wave_count[round & 1][wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            const int c = s.wave_count[round & 1][w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (have + cnt + total > kHitsCap) {                                  // (block-uniform) make room: at most K stay
            have = hits_flush(s, have, cnt, K);
            cnt = 0;
            if (have == K) thr = max(thr, s.key[K - 1]);                      // (the staging below writes at have = K and beyond)
        }
        if (pass) {
            const int at = have + cnt + before + __popcll(m & ((1ull << lane) - 1ull));
            s.key[at] = key;
            s.val[at] = bits;
        }
        cnt += total;
    }
    __syncthreads();
    have = hits_flush(s, have, cnt, K);
    const size_t o = (size_t)blockIdx.x * K;
    for (int i = tid; i < have; i += kBlock) { ws_key[o + i] = s.key[i]; ws_val[o + i] = s.val[i]; }
    if (tid == 0) ws_count[blockIdx.x] = have;
}

// grid: Qs blocks.
__global__ void __launch_bounds__(kBlock) k_hits_finish(const unsigned long long* __restrict__ ws_key, const unsigned* __restrict__ ws_val,
                                                       const int* __restrict__ ws_count, int L, int K, int S, int largest,
                                                       float* __restrict__ top_score, int* __restrict__ top_id,
                                                       long long* __restrict__ seen) {
    __shared__ HitsLds s;
    const int tid = threadIdx.x, j = blockIdx.x;
    float* const ts = top_score + (size_t)j * K;
    int* const ti = top_id + (size_t)j * K;
    if (tid == 0) s.have = 0;
    __syncthreads();
    for (int i = tid; i < K; i += kBlock) {                                   // the old list: sorted, its empty slots last
        const int id = ti[i];
        if (id >= 0) {
            const unsigned bits = __float_as_uint(ts[i]);
            s.key[i] = hits_key(bits, id, largest);
            s.val[i] = bits;
            if (i == K - 1 || ti[i + 1] < 0) s.have = i + 1;
        }
    }
    __syncthreads();
    int have = s.have, cnt = 0;
    for (int p = 0; p < S; ++p) {
        const int c = ws_count[j * S + p];                                    // <= K
        if (have + cnt + c > kHitsCap) {
            __syncthreads();
            have = hits_flush(s, have, cnt, K);
            cnt = 0;
        }
        const size_t o = ((size_t)j * S + p) * K;
        for (int i = tid; i < c; i += kBlock) { s.key[have + cnt + i] = ws_key[o + i]; s.val[have + cnt + i] = ws_val[o + i]; }
        cnt += c;
    }
    __syncthreads();
    have = hits_flush(s, have, cnt, K);
    for (int i = tid; i < K; i += kBlock) {
        const bool full = i < have;
        st1g(ts + i, __uint_as_float(full ? s.val[i] : kHitsNaNBits));
        ti[i] = full ? (int)(0xffffffffu - (unsigned)s.key[i]) : -1;
    }
    if (j == 0 && tid == 0) *seen = *seen + L;                                // the only access to *seen in this launch
}

__global__ void __launch_bounds__(kBlock) k_hits_reset(float* __restrict__ top_score, int* __restrict__ top_id, long long n,
                                                      long long* __restrict__ seen) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        st1g(top_score + i, __uint_as_float(kHitsNaNBits));
        top_id[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *seen = 0;
}

// the most slabs a call over L candidates may use: what the workspace is sized for
static inline int64_t hits_max_slabs(int64_t L) { return std::max<int64_t>(1, std::min<int64_t>(kHitsMaxSlabs, L / kHitsMinSlab)); }

static inline size_t hits_align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace glam

using namespace glam;

// a STATUS, as every int of this ABI that is not listed as a value: GLAM_OK when a list of K entries has a kernel
extern "C" int glam_hits_supported(int K) {
    if (K < 1 || K > kHitsMaxK) return fail(GLAM_E_UNSUPPORTED, "glam_hits: K=%d not in 1..%d", K, kHitsMaxK);
    return GLAM_OK;
}

extern "C" size_t glam_hits_workspace_bytes(int64_t L, int64_t Qs, int K) {
    if (L <= 0 || Qs <= 0 || K <= 0) return 0;
    const size_t lists = (size_t)Qs * (size_t)hits_max_slabs(L);
    return lists * (size_t)K * 8 + hits_align8(lists * (size_t)K * 4) + hits_align8(lists * 4);
}

extern "C" int glam_hits_reset(float* top_score, int32_t* top_id, int64_t* seen, int64_t Qs, int K, void* stream) {
    GLAM_REQUIRE(Qs >= 0 && Qs < INT32_MAX, "glam_hits_reset: Qs out of range");
    if (const int rc = glam_hits_supported(K)) return rc;
    GLAM_REQUIRE(seen && ((uintptr_t)seen & 7u) == 0, "glam_hits_reset: seen is null or not 8-byte aligned");
    GLAM_REQUIRE(Qs == 0 || (top_score && top_id && ((uintptr_t)top_score & 3u) == 0 && ((uintptr_t)top_id & 3u) == 0),
                 "glam_hits_reset: the lists are null or not 4-byte aligned");
    const int64_t n = Qs * K;
    hipLaunchKernelGGL(k_hits_reset, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, top_score, top_id, (long long)n,
                       (long long*)seen);
    GLAM_LAUNCH_CHECK("glam_hits_reset");
    return GLAM_OK;
}

extern "C" int glam_hits_merge(const float* score, int64_t ld_row, int64_t ld_col, const int32_t* ids, int64_t L, int64_t Qs, int K,
                               int largest, int slabs, float* top_score, int32_t* top_id, int64_t* seen, void* workspace,
                               size_t workspace_bytes, void* stream) {
    GLAM_REQUIRE(L >= 0 && L <= INT32_MAX, "glam_hits_merge: L out of range (at most 2^31 - 1 candidates a call)");
    GLAM_REQUIRE(Qs >= 0 && Qs < INT32_MAX, "glam_hits_merge: Qs out of range");
    GLAM_REQUIRE(slabs >= 0, "glam_hits_merge: slabs must be 0 (choose) or the slabs per column");
    if (const int rc = glam_hits_supported(K)) return rc;
    if (L == 0 || Qs == 0) return GLAM_OK;
    GLAM_REQUIRE(ld_row >= 0 && ld_col >= 0, "glam_hits_merge: negative stride");
    GLAM_REQUIRE(ld_row <= INT64_MAX / 8 / L && ld_col <= INT64_MAX / 8 / Qs, "glam_hits_merge: the strides reach beyond the address space");
    GLAM_REQUIRE(score && top_score && top_id && seen, "glam_hits_merge: null pointer");
    GLAM_REQUIRE(((uintptr_t)score & 3u) == 0 && ((uintptr_t)ids & 3u) == 0 && ((uintptr_t)top_score & 3u) == 0 &&
                     ((uintptr_t)top_id & 3u) == 0 && ((uintptr_t)seen & 7u) == 0,
                 "glam_hits_merge: scores, ids and lists must be 4-byte aligned, seen 8-byte aligned");
    GLAM_REQUIRE(workspace && workspace_bytes >= glam_hits_workspace_bytes(L, Qs, K) && ((uintptr_t)workspace & 7u) == 0,
                 "glam_hits_merge: workspace too small or misaligned (glam_hits_workspace_bytes)");
    // automatic S: slabs of about kHitsAutoSlab candidates while the grid stays within about kHitsAutoBlocks blocks
    int64_t S = slabs > 0 ? slabs : std::min<int64_t>((L + kHitsAutoSlab - 1) / kHitsAutoSlab, std::max<int64_t>(1, kHitsAutoBlocks / Qs));
    S = std::max<int64_t>(1, std::min<int64_t>(S, hits_max_slabs(L)));
    GLAM_REQUIRE(Qs * S < INT32_MAX, "glam_hits_merge: grid out of range");
    const size_t lists = (size_t)Qs * (size_t)S;
    unsigned long long* ws_key = (unsigned long long*)workspace;
    unsigned* ws_val = (unsigned*)(ws_key + lists * K);
    int* ws_count = (int*)((char*)ws_val + hits_align8(lists * K * 4));
    hipLaunchKernelGGL(k_hits_slab, dim3((unsigned)(Qs * S)), dim3(kBlock), 0, (hipStream_t)stream, score, (long long)ld_row,
                       (long long)ld_col, ids, (const long long*)seen, (int)L, K, (int)S, largest != 0, (const float*)top_score,
                       (const int*)top_id, ws_key, ws_val, ws_count);
    GLAM_LAUNCH_CHECK("glam_hits_merge");
    hipLaunchKernelGGL(k_hits_finish, dim3((unsigned)Qs), dim3(kBlock), 0, (hipStream_t)stream, (const unsigned long long*)ws_key,
                       (const unsigned*)ws_val, (const int*)ws_count, (int)L, K, (int)S, largest != 0, top_score, top_id,
                       (long long*)seen);
    GLAM_LAUNCH_CHECK("glam_hits_merge (finish)");
    return GLAM_OK;
}
