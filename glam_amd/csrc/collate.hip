// Collation of a batch out of a device-resident dataset, its graph index included, in one launch (glam_collate in include/glam_hip.h).
// Reference semantics replaced: PyG's Batch.from_data_list as the reference's DataLoader runs it for every training batch
// (src_1gp/trainer.py:37-41, :292-295) and, on this side, what the host path does for a fresh batch after it: one host-to-device copy per
// field, the CSR builds of both directions, the two ELL builds and the segment pointer (csr.hip, triplet_pipe.hip).
//
// A batch is a disjoint union of graphs, so everything above is a SEGMENTED COPY of what was built once for the whole dataset: slot b of
// the batch holds graph g = ids[b]; its nodes are the dataset's nodes node_ptr[g] .. node_ptr[g+1] moved to node_off[b] .., its edges the
// dataset's edges edge_ptr[g] .. moved to edge_off[b] ..  — in the caller's order AND in both CSR orders, because a stable grouping by
// global target (source) of a disjoint union is the concatenation of the per-graph groupings.  Node ids are re-based by
// node_off[b] - node_ptr[g], edge ids and row pointers by edge_off[b] - edge_ptr[g]; the -1 of an empty ELL slot stays.
//
// Work is cut into items of kCollateItem consecutive OUTPUT elements of one of six streams (x, edge_attr and y rows; nodes; edges; slots);
// blocks stride over the items, a thread finds the slot of its element by binary search in the offset table — held in LDS up to
// kCollateSlots slots, in global memory beyond.  No workspace, no atomics, no flag: the host has checked the ids.
#include "common.h"

namespace glam {

constexpr int kCollateSlots = 1024;   // slots whose offset table a block keeps in LDS (6 x 4 KiB)
constexpr int kCollateItem = 1024;    // output elements of one work item: 4 per thread, each a coalesced wave access
constexpr int kCollateBlocks = 512;   // grid cap: every block reads the table once, so few blocks with several items each

struct CollateArgs {
    // the dataset (device): rows as dwords, local edge list int32 [2, Ed], prefix sums, both CSRs, both ELL pairs (may be null)
    const uint32_t *x, *ea, *y;
    const int* ei;
    const int *node_ptr, *edge_ptr, *y_ptr;
    const int *rowptr, *src, *eid, *colptr, *dst, *eid_t;
    const int4 *ell_src, *ell_eid, *ell_dst, *ell_eid_t;
    // the slot table (device): ids[B], then three exclusive offset rows of B + 1 entries
    const int *ids, *node_off, *edge_off, *y_off;
    // the batch
    uint32_t *ox, *oea, *oy;
    int64_t *oei, *obatch, *optr64;
    int *optr32, *orowptr, *osrc, *oeid, *ocolptr, *odst, *oeid_t;
    int4 *oell_src, *oell_eid, *oell_dst, *oell_eid_t;
    int B, N, E, Y, Ed;
    int xw, eaw, yw;            // units per row of x / edge_attr / y ...
    int xvec, eavec, yvec;      // ... a unit being 16 bytes (1) or a dword (0)
    int first[7];               // first item of each stream (x, edge_attr, y, nodes, edges, slots) and the item count
};

// largest b in [0, B) with off[b] <= v, for 0 <= v < off[B]: the slot that holds element v (empty slots share their offset with the next
// one and are stepped over)
__device__ __forceinline__ int find_slot(const int* off, int B, int v) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// where a thread finds offsets and dataset starts of the slots: the block's LDS copy, or the table and the dataset's prefix sums
template <bool LDS>
struct SlotTable {
    const int *off, *start, *ids;
    __device__ __forceinline__ int first_of(int b) const { return LDS ? start[b] : start[ids[b]]; }
};

// element idx of a row stream: unit c of output row r = unit c of dataset row r - off[b] + start(b)
template <bool LDS, typename V>
__device__ __forceinline__ void copy_unit(const SlotTable<LDS>& t, int B, const V* in, V* out, int idx, int w) {
    const int r = idx / w, c = idx - r * w;
    const int b = find_slot(t.off, B, r);
    const int64_t sr = (int64_t)(r - t.off[b]) + t.first_of(b);
    out[idx] = in[sr * w + c];
}

__device__ __forceinline__ int4 rebase4(int4 v, int d) {      // (-1 = empty ELL slot)
    return make_int4(v.x < 0 ? v.x : v.x + d, v.y < 0 ? v.y : v.y + d, v.z < 0 ? v.z : v.z + d, v.w < 0 ? v.w : v.w + d);
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) k_collate(const CollateArgs a) {
    constexpr int kRow = kCollateSlots + 1;
    __shared__ int s_tab[LDS ? 6 * kRow : 1];
    SlotTable<LDS> tn, te, ty;
    const int B = a.B;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i <= B; i += kBlock) {
            s_tab[i] = a.node_off[i];
            s_tab[kRow + i] = a.edge_off[i];
            s_tab[2 * kRow + i] = a.y_off[i];
            if (i < B) {
                const int g = a.ids[i];
                s_tab[3 * kRow + i] = a.node_ptr[g];
                s_tab[4 * kRow + i] = a.edge_ptr[g];
                s_tab[5 * kRow + i] = a.y_ptr[g];
            }
        }
        __syncthreads();
        tn = {s_tab, s_tab + 3 * kRow, nullptr};
        te = {s_tab + kRow, s_tab + 4 * kRow, nullptr};
        ty = {s_tab + 2 * kRow, s_tab + 5 * kRow, nullptr};
    } else {
        tn = {a.node_off, a.node_ptr, a.ids};
        te = {a.edge_off, a.edge_ptr, a.ids};
        ty = {a.y_off, a.y_ptr, a.ids};
    }
    for (int item = blockIdx.x; item < a.first[6]; item += gridDim.x) {
        int s = 0;
        while (item >= a.first[s + 1]) ++s;                  // (block-uniform)
        const int base = (item - a.first[s]) * kCollateItem + threadIdx.x;
#pragma unroll
        for (int k = 0; k < kCollateItem / kBlock; ++k) {
            const int idx = base + k * kBlock;
            if (s == 0) {
                if (idx >= a.N * a.xw) break;
                if (a.xvec) copy_unit(tn, B, reinterpret_cast<const uint4*>(a.x), reinterpret_cast<uint4*>(a.ox), idx, a.xw);
                else copy_unit(tn, B, a.x, a.ox, idx, a.xw);
            } else if (s == 1) {
                if (idx >= a.E * a.eaw) break;
                if (a.eavec) copy_unit(te, B, reinterpret_cast<const uint4*>(a.ea), reinterpret_cast<uint4*>(a.oea), idx, a.eaw);
                else copy_unit(te, B, a.ea, a.oea, idx, a.eaw);
            } else if (s == 2) {
                if (idx >= a.Y * a.yw) break;
                if (a.yvec) copy_unit(ty, B, reinterpret_cast<const uint4*>(a.y), reinterpret_cast<uint4*>(a.oy), idx, a.yw);
                else copy_unit(ty, B, a.y, a.oy, idx, a.yw);
            } else if (s == 3) {                             // nodes: batch, both row pointers (and their closing entry), the ELL records
                if (idx > a.N) break;
                if (idx == a.N) { a.orowptr[idx] = a.E; a.ocolptr[idx] = a.E; break; }
                const int b = find_slot(tn.off, B, idx);
                const int dn = tn.off[b] - tn.first_of(b), de = te.off[b] - te.first_of(b);
                const int sn = idx - dn;
                a.obatch[idx] = b;
                a.orowptr[idx] = a.rowptr[sn] + de;
                a.ocolptr[idx] = a.colptr[sn] + de;
                if (a.oell_src) {
                    a.oell_src[idx] = rebase4(a.ell_src[sn], dn);
                    a.oell_eid[idx] = rebase4(a.ell_eid[sn], de);
                }
                if (a.oell_dst) {
                    a.oell_dst[idx] = rebase4(a.ell_dst[sn], dn);
                    a.oell_eid_t[idx] = rebase4(a.ell_eid_t[sn], de);
                }
            } else if (s == 4) {                             // edges: the caller's order (int64, global ids) and both CSR orders
                if (idx >= a.E) break;
                const int b = find_slot(te.off, B, idx);
                const int dn = tn.off[b] - tn.first_of(b), de = te.off[b] - te.first_of(b);
                const int se = idx - de;
                a.oei[idx] = (int64_t)(a.ei[se] + tn.off[b]);
                a.oei[(int64_t)a.E + idx] = (int64_t)(a.ei[(int64_t)a.Ed + se] + tn.off[b]);
                a.osrc[idx] = a.src[se] + dn;
                a.oeid[idx] = a.eid[se] + de;
                a.odst[idx] = a.dst[se] + dn;
                a.oeid_t[idx] = a.eid_t[se] + de;
            } else {                                         // slots: ptr as int64 (the batch's field) and int32 (the readouts' segments)
                if (idx > B) break;
                const int v = a.node_off[idx];
                a.optr64[idx] = v;
                a.optr32[idx] = v;
            }
        }
    }
}

// ---- fixed-capacity batches (glam_collate_padded) ---------------------------------------------------------------------------------
// The same segmented copy into tensors whose sizes do not depend on the ids: B real graphs, then ONE phantom graph that owns the
// surplus P = N_cap - N nodes and E_pad = E_cap - E edges.  N and E are read from the table on the device, so grid, sizes and pointers
// are those of the bucket and the launch can sit in a captured graph.  Phantom node p = N + p carries a contiguous run of self-loops,
// q + (p < rem) of them from E + p * q + min(p, rem) on (q = E_pad / P, rem = E_pad % P): both CSR orders of the padded edge list are
// then the real ones followed by the runs, an edge's id its own position.  Phantom x rows are zero, phantom edge_attr rows copies of
// the dataset's edge row 0 (it carries whatever one-hot mark the dataset has), so every phantom activation is finite.
// glam_collate_padded_split cuts the phantom nodes into K phantom graphs by the same divmod: graph j owns s + (j < r) consecutive nodes
// from N + j * s + min(j, r) on (s = P / K, r = P % K), so batch and ptr are closed forms of p and j and the edge runs, which are per
// node, do not move.  K = 1 is the single phantom graph: owner 0 for every p, ptr[B + 1] = N + P.
struct CollatePadArgs {
    CollateArgs c;              // (c.N / c.E / c.Y are not read: the totals come from the table)
    int N_cap, E_cap;
    int K;                      // phantom graphs (>= 1; the caller guarantees K <= P, so none is empty)
    int xwo;                    // units per OUTPUT row of x (>= c.xw; the pad units are written as zero)
};

// phantom node (0-based) that owns phantom edge j, for runs of q + (p < rem) edges — and, over nodes, the phantom graph that owns phantom
// node j for graphs of q + (g < rem) nodes
__device__ __forceinline__ int phantom_owner(int j, int q, int rem) {
    const int head = rem * (q + 1);
    return j < head ? j / (q + 1) : rem + (j - head) / q;      // (j >= head only where q >= 1: j < E_pad = head + (P - rem) * q)
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) k_collate_padded(const CollatePadArgs pa) {
    constexpr int kRow = kCollateSlots + 1;
    __shared__ int s_tab[LDS ? 6 * kRow : 1];
    const CollateArgs& a = pa.c;
    SlotTable<LDS> tn, te, ty;
    const int B = a.B;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i <= B; i += kBlock) {
            s_tab[i] = a.node_off[i];
            s_tab[kRow + i] = a.edge_off[i];
            s_tab[2 * kRow + i] = a.y_off[i];
            if (i < B) {
                const int g = a.ids[i];
                s_tab[3 * kRow + i] = a.node_ptr[g];
                s_tab[4 * kRow + i] = a.edge_ptr[g];
                s_tab[5 * kRow + i] = a.y_ptr[g];
            }
        }
        __syncthreads();
        tn = {s_tab, s_tab + 3 * kRow, nullptr};
        te = {s_tab + kRow, s_tab + 4 * kRow, nullptr};
        ty = {s_tab + 2 * kRow, s_tab + 5 * kRow, nullptr};
    } else {
        tn = {a.node_off, a.node_ptr, a.ids};
        te = {a.edge_off, a.edge_ptr, a.ids};
        ty = {a.y_off, a.y_ptr, a.ids};
    }
    const int N = tn.off[B], E = te.off[B], Y = ty.off[B];
    const int P = pa.N_cap - N, E_pad = pa.E_cap - E;            // (the caller guarantees P >= 1, E_pad >= 0)
    const int q = P > 0 ? E_pad / P : 0, rem = P > 0 ? E_pad % P : 0;
    const int gs = P > 0 ? P / pa.K : 0, gr = P > 0 ? P % pa.K : 0;  // (phantom graph j: gs + (j < gr) nodes; gs >= 1 as K <= P)
    for (int item = blockIdx.x; item < a.first[6]; item += gridDim.x) {
        int s = 0;
        while (item >= a.first[s + 1]) ++s;                  // (block-uniform)
        const int base = (item - a.first[s]) * kCollateItem + threadIdx.x;
#pragma unroll
        for (int k = 0; k < kCollateItem / kBlock; ++k) {
            const int idx = base + k * kBlock;
            if (s == 0) {                                    // x: real rows, zero pad units, zero phantom rows
                if (idx >= pa.N_cap * pa.xwo) break;
                const int r = idx / pa.xwo, c = idx - r * pa.xwo;
                const bool real = r < N && c < a.xw;
                int64_t from = 0;
                if (real) {
                    const int b = find_slot(tn.off, B, r);
                    from = ((int64_t)(r - tn.off[b]) + tn.first_of(b)) * a.xw + c;
                }
                if (a.xvec) reinterpret_cast<uint4*>(a.ox)[idx] = real ? reinterpret_cast<const uint4*>(a.x)[from] : make_uint4(0, 0, 0, 0);
                else a.ox[idx] = real ? a.x[from] : 0u;
            } else if (s == 1) {                             // edge_attr: real rows, then copies of the dataset's row 0
                if (idx >= pa.E_cap * a.eaw) break;
                const int r = idx / a.eaw, c = idx - r * a.eaw;
                int64_t from = c;
                if (r < E) {
                    const int b = find_slot(te.off, B, r);
                    from = ((int64_t)(r - te.off[b]) + te.first_of(b)) * a.eaw + c;
                }
                if (a.eavec) reinterpret_cast<uint4*>(a.oea)[idx] = reinterpret_cast<const uint4*>(a.ea)[from];
                else a.oea[idx] = a.ea[from];
            } else if (s == 2) {                             // y: the real graphs' rows (the phantom graph has none)
                if (idx >= Y * a.yw) break;
                if (a.yvec) copy_unit(ty, B, reinterpret_cast<const uint4*>(a.y), reinterpret_cast<uint4*>(a.oy), idx, a.yw);
                else copy_unit(ty, B, a.y, a.oy, idx, a.yw);
            } else if (s == 3) {                             // nodes
                if (idx > pa.N_cap) break;
                if (idx == pa.N_cap) { a.orowptr[idx] = pa.E_cap; a.ocolptr[idx] = pa.E_cap; break; }
                if (idx < N) {
                    const int b = find_slot(tn.off, B, idx);
                    const int dn = tn.off[b] - tn.first_of(b), de = te.off[b] - te.first_of(b);
                    const int sn = idx - dn;
                    a.obatch[idx] = b;
                    a.orowptr[idx] = a.rowptr[sn] + de;
                    a.ocolptr[idx] = a.colptr[sn] + de;
                    if (a.oell_src) {
                        a.oell_src[idx] = rebase4(a.ell_src[sn], dn);
                        a.oell_eid[idx] = rebase4(a.ell_eid[sn], de);
                    }
                    if (a.oell_dst) {
                        a.oell_dst[idx] = rebase4(a.ell_dst[sn], dn);
                        a.oell_eid_t[idx] = rebase4(a.ell_eid_t[sn], de);
                    }
                } else {                                     // phantom node: its run of self-loops, the same by target and by source
                    const int p = idx - N;
                    const int start = E + p * q + min(p, rem), len = q + (p < rem);
                    a.obatch[idx] = B + phantom_owner(p, gs, gr);
                    a.orowptr[idx] = start;
                    a.ocolptr[idx] = start;
                    const int4 nodes = make_int4(len > 0 ? idx : -1, len > 1 ? idx : -1, len > 2 ? idx : -1, len > 3 ? idx : -1);
                    const int4 edges = make_int4(len > 0 ? start : -1, len > 1 ? start + 1 : -1, len > 2 ? start + 2 : -1, len > 3 ? start + 3 : -1);
                    if (a.oell_src) { a.oell_src[idx] = nodes; a.oell_eid[idx] = edges; }
                    if (a.oell_dst) { a.oell_dst[idx] = nodes; a.oell_eid_t[idx] = edges; }
                }
            } else if (s == 4) {                             // edges
                if (idx >= pa.E_cap) break;
                if (idx < E) {
                    const int b = find_slot(te.off, B, idx);
                    const int dn = tn.off[b] - tn.first_of(b), de = te.off[b] - te.first_of(b);
                    const int se = idx - de;
                    a.oei[idx] = (int64_t)(a.ei[se] + tn.off[b]);
                    a.oei[(int64_t)pa.E_cap + idx] = (int64_t)(a.ei[(int64_t)a.Ed + se] + tn.off[b]);
                    a.osrc[idx] = a.src[se] + dn;
                    a.oeid[idx] = a.eid[se] + de;
                    a.odst[idx] = a.dst[se] + dn;
                    a.oeid_t[idx] = a.eid_t[se] + de;
                } else {                                     // phantom edge: a self-loop of its owner, at its own position in both orders
                    const int node = N + phantom_owner(idx - E, q, rem);
                    a.oei[idx] = node;
                    a.oei[(int64_t)pa.E_cap + idx] = node;
                    a.osrc[idx] = node;
                    a.oeid[idx] = idx;
                    a.odst[idx] = node;
                    a.oeid_t[idx] = idx;
                }
            } else {                                         // slots: the B real graphs, then the K phantom graphs that cut [N, N_cap)
                if (idx > B + pa.K) break;
                const int j = idx - B;
                const int v = j <= 0 ? a.node_off[idx] : N + j * gs + min(j, gr);
                a.optr64[idx] = v;
                a.optr32[idx] = v;
            }
        }
    }
}

}  // namespace glam

using namespace glam;

extern "C" size_t glam_collate_lds_slots(void) { return kCollateSlots; }

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int glam_collate(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t N, int64_t E,
                            int64_t Y, int64_t Ed, int32_t x_row_bytes, int32_t ea_row_bytes, int32_t y_row_bytes, void* stream) {
    GLAM_REQUIRE(ds_host && out_host && table, "glam_collate: null pointer (ds_host / out_host / table)");
    GLAM_REQUIRE(B >= 0 && N >= 0 && E >= 0 && Y >= 0 && Ed >= 0 && B < INT32_MAX && N < INT32_MAX && E < INT32_MAX && Ed < INT32_MAX && Y < INT32_MAX,
                 "glam_collate: B / N / E / Y / Ed negative or beyond int32");
    GLAM_REQUIRE(x_row_bytes >= 0 && ea_row_bytes >= 0 && y_row_bytes >= 0 && ((x_row_bytes | ea_row_bytes | y_row_bytes) & 3) == 0,
                 "glam_collate: row sizes must be multiples of 4 bytes");
    const void* const* d = ds_host;
    void* const* o = out_host;
    for (int i = 0; i < GLAM_COLLATE_FIELDS; ++i)
        GLAM_REQUIRE(aligned_to(d[i], 4) && aligned_to(o[i], i == 1 || i == 4 || i == 5 ? 8 : 4), "glam_collate: misaligned pointer (field %d)", i);
    GLAM_REQUIRE(aligned_to(table, 4), "glam_collate: misaligned table");
    // what every batch has: ptr (both widths), the row pointers of both directions; a batch with slots reads the dataset's prefix sums
    GLAM_REQUIRE(o[5] && o[6] && o[7] && o[10] && (B == 0 || (d[4] && d[5] && d[6])), "glam_collate: null pointer (ptr / rowptr / colptr / prefix sums)");
    GLAM_REQUIRE(N == 0 || (o[4] && d[7] && d[10] && (x_row_bytes == 0 || (d[0] && o[0]))), "glam_collate: null pointer (node fields)");
    GLAM_REQUIRE(E == 0 || (d[1] && o[1] && d[8] && d[9] && d[11] && d[12] && o[8] && o[9] && o[11] && o[12] && (ea_row_bytes == 0 || (d[2] && o[2]))),
                 "glam_collate: null pointer (edge fields)");
    GLAM_REQUIRE(Y == 0 || y_row_bytes == 0 || (d[3] && o[3]), "glam_collate: null pointer (y)");
    GLAM_REQUIRE(N > 0 || E == 0, "glam_collate: edges without nodes");
    // an ELL pair is written when the caller passes its outputs: both tensors of the pair, from both tensors of the dataset's, 16-byte rows
    for (int i = 13; i < 17; i += 2) {
        GLAM_REQUIRE((o[i] != nullptr) == (o[i + 1] != nullptr), "glam_collate: one tensor of an ELL pair without the other");
        GLAM_REQUIRE(!o[i] || (d[i] && d[i + 1]), "glam_collate: ELL output without the dataset's ELL records");
        GLAM_REQUIRE(!o[i] || (aligned16(o[i]) && aligned16(o[i + 1]) && aligned16(d[i]) && aligned16(d[i + 1])), "glam_collate: misaligned ELL pointer");
    }
    CollateArgs a = {};
    a.x = (const uint32_t*)d[0]; a.ei = (const int*)d[1]; a.ea = (const uint32_t*)d[2]; a.y = (const uint32_t*)d[3];
    a.node_ptr = (const int*)d[4]; a.edge_ptr = (const int*)d[5]; a.y_ptr = (const int*)d[6];
    a.rowptr = (const int*)d[7]; a.src = (const int*)d[8]; a.eid = (const int*)d[9];
    a.colptr = (const int*)d[10]; a.dst = (const int*)d[11]; a.eid_t = (const int*)d[12];
    a.ell_src = (const int4*)d[13]; a.ell_eid = (const int4*)d[14]; a.ell_dst = (const int4*)d[15]; a.ell_eid_t = (const int4*)d[16];
    a.ids = table; a.node_off = table + (B + 1); a.edge_off = table + 2 * (B + 1); a.y_off = table + 3 * (B + 1);
    a.ox = (uint32_t*)o[0]; a.oei = (int64_t*)o[1]; a.oea = (uint32_t*)o[2]; a.oy = (uint32_t*)o[3];
    a.obatch = (int64_t*)o[4]; a.optr64 = (int64_t*)o[5]; a.optr32 = (int*)o[6];
    a.orowptr = (int*)o[7]; a.osrc = (int*)o[8]; a.oeid = (int*)o[9]; a.ocolptr = (int*)o[10]; a.odst = (int*)o[11]; a.oeid_t = (int*)o[12];
    a.oell_src = (int4*)o[13]; a.oell_eid = (int4*)o[14]; a.oell_dst = (int4*)o[15]; a.oell_eid_t = (int4*)o[16];
    a.B = (int)B; a.N = (int)N; a.E = (int)E; a.Y = (int)Y; a.Ed = (int)Ed;
    // a row stream moves 16-byte units where the rows are whole units and both sides start on one (then every row does), dwords otherwise
    const int rb[3] = {x_row_bytes, ea_row_bytes, y_row_bytes};
    const int64_t rows[3] = {N, E, Y};
    int w[3], vec[3];
    int64_t count[6];
    for (int k = 0; k < 3; ++k) {
        vec[k] = rb[k] > 0 && rb[k] % 16 == 0 && aligned16(d[k == 0 ? 0 : k + 1]) && aligned16(o[k == 0 ? 0 : k + 1]);
        w[k] = rb[k] / (vec[k] ? 16 : 4);
        count[k] = rows[k] * w[k];
    }
    a.xw = w[0]; a.eaw = w[1]; a.yw = w[2];
    a.xvec = vec[0]; a.eavec = vec[1]; a.yvec = vec[2];
    count[3] = N + 1; count[4] = E; count[5] = B + 1;
    int64_t items = 0;
    for (int s = 0; s < 6; ++s) {
        // the kernel indexes the elements of a stream, item padding included, with an int
        if (count[s] >= INT32_MAX - kCollateItem) return fail(GLAM_E_UNSUPPORTED, "glam_collate: a field of the batch has 2^31 elements or more");
        a.first[s] = (int)items;
        items += (count[s] + kCollateItem - 1) / kCollateItem;
    }
    a.first[6] = (int)items;
    const int grid = grid_for(items, 1, kCollateBlocks);
    if (B <= kCollateSlots) hipLaunchKernelGGL(k_collate<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_collate<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    GLAM_LAUNCH_CHECK("glam_collate");
    return GLAM_OK;
}

// both entry points of the fixed-capacity collate: K phantom graphs (glam_collate_padded is K = 1)
static int collate_padded(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t K, int64_t N_cap,
                          int64_t E_cap, int64_t y_rows, int64_t Ed, int32_t x_row_bytes, int32_t x_out_stride_bytes,
                          int32_t ea_row_bytes, int32_t y_row_bytes, void* stream) {
    GLAM_REQUIRE(ds_host && out_host && table, "glam_collate_padded: null pointer (ds_host / out_host / table)");
    GLAM_REQUIRE(B >= 1 && N_cap >= 1 && E_cap >= 0 && Ed >= 0 && B < INT32_MAX - 1 && N_cap < INT32_MAX && E_cap < INT32_MAX && Ed < INT32_MAX,
                 "glam_collate_padded: B / N_cap / E_cap / Ed out of range (B >= 1, N_cap >= 1 for the phantom node, all below 2^31 - 1)");
    GLAM_REQUIRE(K >= 1 && K <= N_cap && B + K < INT32_MAX - 1,
                 "glam_collate_padded: K out of range (1 <= K <= N_cap: every phantom graph owns a node; B + K below 2^31 - 1)");
    GLAM_REQUIRE(x_row_bytes >= 0 && ea_row_bytes >= 0 && y_row_bytes >= 0 && ((x_row_bytes | ea_row_bytes | y_row_bytes) & 3) == 0,
                 "glam_collate_padded: row sizes must be multiples of 4 bytes");
    GLAM_REQUIRE(x_out_stride_bytes >= x_row_bytes && x_out_stride_bytes % 16 == 0,
                 "glam_collate_padded: the output row stride of x must be a multiple of 16 bytes, at least x_row_bytes");
    const void* const* d = ds_host;
    void* const* o = out_host;
    const bool has_y = y_row_bytes > 0 && o[3];
    GLAM_REQUIRE(!has_y || (y_rows >= 1 && B * y_rows < INT32_MAX), "glam_collate_padded: y rows per graph must be a positive integer");
    GLAM_REQUIRE(E_cap == 0 || Ed > 0, "glam_collate_padded: phantom edges copy the dataset's edge row 0: a dataset without edges has E_cap = 0");
    for (int i = 0; i < GLAM_COLLATE_FIELDS; ++i)
        GLAM_REQUIRE(aligned_to(d[i], 4) && aligned_to(o[i], i == 1 || i == 4 || i == 5 ? 8 : 4), "glam_collate_padded: misaligned pointer (field %d)", i);
    GLAM_REQUIRE(aligned_to(table, 4), "glam_collate_padded: misaligned table");
    GLAM_REQUIRE(o[4] && o[5] && o[6] && o[7] && o[10] && d[4] && d[5] && d[6] && d[7] && d[10] && (x_row_bytes == 0 || (d[0] && o[0] && aligned16(o[0]))),
                 "glam_collate_padded: null pointer (batch / ptr / rowptr / colptr / prefix sums / x), or x output off a 16-byte boundary");
    GLAM_REQUIRE(E_cap == 0 || (d[1] && o[1] && d[8] && d[9] && d[11] && d[12] && o[8] && o[9] && o[11] && o[12] && (ea_row_bytes == 0 || (d[2] && o[2]))),
                 "glam_collate_padded: null pointer (edge fields)");
    GLAM_REQUIRE(!has_y || d[3], "glam_collate_padded: null pointer (y)");
    for (int i = 13; i < 17; i += 2) {
        GLAM_REQUIRE((o[i] != nullptr) == (o[i + 1] != nullptr), "glam_collate_padded: one tensor of an ELL pair without the other");
        GLAM_REQUIRE(!o[i] || (d[i] && d[i + 1]), "glam_collate_padded: ELL output without the dataset's ELL records");
        GLAM_REQUIRE(!o[i] || (aligned16(o[i]) && aligned16(o[i + 1]) && aligned16(d[i]) && aligned16(d[i + 1])), "glam_collate_padded: misaligned ELL pointer");
    }
    CollatePadArgs pa = {};
    CollateArgs& a = pa.c;
    a.x = (const uint32_t*)d[0]; a.ei = (const int*)d[1]; a.ea = (const uint32_t*)d[2]; a.y = (const uint32_t*)d[3];
    a.node_ptr = (const int*)d[4]; a.edge_ptr = (const int*)d[5]; a.y_ptr = (const int*)d[6];
    a.rowptr = (const int*)d[7]; a.src = (const int*)d[8]; a.eid = (const int*)d[9];
    a.colptr = (const int*)d[10]; a.dst = (const int*)d[11]; a.eid_t = (const int*)d[12];
    a.ell_src = (const int4*)d[13]; a.ell_eid = (const int4*)d[14]; a.ell_dst = (const int4*)d[15]; a.ell_eid_t = (const int4*)d[16];
    a.ids = table; a.node_off = table + (B + 1); a.edge_off = table + 2 * (B + 1); a.y_off = table + 3 * (B + 1);
    a.ox = (uint32_t*)o[0]; a.oei = (int64_t*)o[1]; a.oea = (uint32_t*)o[2]; a.oy = (uint32_t*)o[3];
    a.obatch = (int64_t*)o[4]; a.optr64 = (int64_t*)o[5]; a.optr32 = (int*)o[6];
    a.orowptr = (int*)o[7]; a.osrc = (int*)o[8]; a.oeid = (int*)o[9]; a.ocolptr = (int*)o[10]; a.odst = (int*)o[11]; a.oeid_t = (int*)o[12];
    a.oell_src = (int4*)o[13]; a.oell_eid = (int4*)o[14]; a.oell_dst = (int4*)o[15]; a.oell_eid_t = (int4*)o[16];
    a.B = (int)B; a.Ed = (int)Ed;
    pa.N_cap = (int)N_cap; pa.E_cap = (int)E_cap; pa.K = (int)K;
    // units as in glam_collate; the output rows of x are whole 16-byte units by contract, so x moves as units where its input rows are
    const int Y = has_y ? (int)(B * y_rows) : 0;
    a.xvec = x_row_bytes > 0 && x_row_bytes % 16 == 0 && aligned16(d[0]);
    a.xw = x_row_bytes / (a.xvec ? 16 : 4);
    pa.xwo = x_out_stride_bytes / (a.xvec ? 16 : 4);
    a.eavec = ea_row_bytes > 0 && ea_row_bytes % 16 == 0 && aligned16(d[2]) && aligned16(o[2]);
    a.eaw = ea_row_bytes / (a.eavec ? 16 : 4);
    a.yvec = has_y && y_row_bytes % 16 == 0 && aligned16(d[3]) && aligned16(o[3]);
    a.yw = has_y ? y_row_bytes / (a.yvec ? 16 : 4) : 0;
    const int64_t count[6] = {x_row_bytes > 0 ? N_cap * pa.xwo : 0, o[2] ? E_cap * a.eaw : 0, (int64_t)Y * a.yw, N_cap + 1, E_cap, B + K + 1};
    int64_t items = 0;
    for (int s = 0; s < 6; ++s) {
        if (count[s] >= INT32_MAX - kCollateItem) return fail(GLAM_E_UNSUPPORTED, "glam_collate_padded: a field of the batch has 2^31 elements or more");
        a.first[s] = (int)items;
        items += (count[s] + kCollateItem - 1) / kCollateItem;
    }
    a.first[6] = (int)items;
    const int grid = grid_for(items, 1, kCollateBlocks);
    if (B <= kCollateSlots) hipLaunchKernelGGL(k_collate_padded<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, pa);
    else hipLaunchKernelGGL(k_collate_padded<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, pa);
    GLAM_LAUNCH_CHECK("glam_collate_padded");
    return GLAM_OK;
}

extern "C" int glam_collate_padded(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t N_cap,
                                   int64_t E_cap, int64_t y_rows, int64_t Ed, int32_t x_row_bytes, int32_t x_out_stride_bytes,
                                   int32_t ea_row_bytes, int32_t y_row_bytes, void* stream) {
    return collate_padded(ds_host, out_host, table, B, 1, N_cap, E_cap, y_rows, Ed, x_row_bytes, x_out_stride_bytes, ea_row_bytes, y_row_bytes,
                          stream);
}

extern "C" int glam_collate_padded_split(const void* const* ds_host, void* const* out_host, const int32_t* table, int64_t B, int64_t K,
                                         int64_t N_cap, int64_t E_cap, int64_t y_rows, int64_t Ed, int32_t x_row_bytes,
                                         int32_t x_out_stride_bytes, int32_t ea_row_bytes, int32_t y_row_bytes, void* stream) {
    return collate_padded(ds_host, out_host, table, B, K, N_cap, E_cap, y_rows, Ed, x_row_bytes, x_out_stride_bytes, ea_row_bytes, y_row_bytes,
                          stream);
}
