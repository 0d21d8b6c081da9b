// The optimizer step of the training loop that drives the path: `Adam(self.model.parameters(), lr=args.lr)` (reference
// src_1gp/trainer.py:49-50, stepped once per batch at trainer.py:301; lr moved by ReduceLROnPlateau, trainer.py:55,85).
// A default-shaped model has 36 parameter tensors between 1 and 307 200 elements (355 k in all).  The library's multi-tensor kernel cuts
// them into 65 536-element chunks — 9 workgroups on a 256-CU device, in double precision because its hyper-parameters are doubles — and
// took 45 us per step (6 % of a 0.79 ms step before this file existed).  Here: ONE launch over all tensors, 1 024-element
// chunks (one float4 per thread, one round trip), fp32 arithmetic: 5.3 us (tools/bench_adam.py).
//   step s = *step + 1                                   (device counter: a captured launch replays correctly)
//   g' = g + weight_decay * p
//   m  = m + (1 - beta1) (g' - m)          v = beta2 v + (1 - beta2) g'^2
//   p  = p - lr / (1 - beta1^s) * m / (sqrt(v) / sqrt(1 - beta2^s) + eps)
// The tensor addresses travel by value in the kernel arguments (gradients are fresh allocations every eager step: no table in device
// memory to keep in sync).  The step counter is written by the LAST workgroup to finish (a two-level ticket), after every workgroup has read it.
#include "common.h"

namespace glam {

constexpr int kAdamMaxTensors = 40;
constexpr int kAdamChunk = 4 * kBlock;

struct AdamArgs {
    float* p[kAdamMaxTensors]; const float* g[kAdamMaxTensors]; float* m[kAdamMaxTensors]; float* v[kAdamMaxTensors];
    int numel[kAdamMaxTensors];
    int chunk_end[kAdamMaxTensors];      // running count of chunks: tensor t owns workgroups [chunk_end[t-1], chunk_end[t])
    int n;
    float* step; const float* lr_dev; unsigned* ticket;
    double lr, beta1, beta2, eps, weight_decay;
    int bump;                            // last launch of a step: advance *step
};

// Every workgroup has consumed *step (it fed the values it stored) before it takes its ticket; the last one to arrive writes the new
// count and re-arms the tickets.  Two levels as in rng_end (rng.h): workgroup b checks in at sub-counter b % 16 (one 128-byte line
// each), the last of a sub-group at the main ticket — a single counter serialises every workgroup of the launch at the coherent point
// (13 of k_adam's 16 us), and a release fence per workgroup costs an L2 write-back each.  Called by one thread per workgroup after a
// barrier.  ticket: u32[GLAM_ADAM_TICKET_WORDS].
__device__ __forceinline__ void step_ticket(float* step, unsigned* ticket, float s) {
    const unsigned g = gridDim.x, sidx = blockIdx.x & 15u;
    const unsigned in_sub = (g - sidx + 15u) >> 4, nsub = g < 16u ? g : 16u;
    unsigned* sub = ticket + 32 * (1 + sidx);
    if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_sub - 1) {
        __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsub - 1) {
            __hip_atomic_store(step, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float omb1, float b2, float omb2, float step_size,
                                         float bc2_sqrt, float eps, float wd) {
    if (wd != 0.f) g = g + wd * p;
    m = m + omb1 * (g - m);
    v = b2 * v + omb2 * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

__global__ void __launch_bounds__(kBlock) k_adam(AdamArgs a) {
    const int tid = threadIdx.x, b = blockIdx.x;
    // owner of this workgroup: lane l compares against chunk_end[l] (one vector load from the argument block), the count of passed
    // boundaries is the tensor index — a scalar walk over the table is a chain of up to 40 dependent scalar loads
    const int lane = tid & 63;
    const bool passed = lane < a.n - 1 && b >= a.chunk_end[lane];
    const int t = __builtin_popcountll(__ballot(passed));
    const int first = t ? a.chunk_end[t - 1] : 0;
    const int off = (b - first) * kAdamChunk + 4 * tid, numel = a.numel[t];
    float* p = a.p[t]; const float* g = a.g[t]; float* m = a.m[t]; float* v = a.v[t];
    // agent-scope atomic loads, as the RNG position is read (rng.h): the previous launch's last workgroup published the count with an
    // agent-scope store and no fence, and a plain load may be served a line cached before that update — a stale count would give
    // some workgroups the bias correction of step s - 1, and a stale ticket winner would store the old count again
    const float s = __hip_atomic_load(a.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1.f;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && off + 4 <= numel;
    float4 pv = f4zero(), gv = f4zero(), mv = f4zero(), vv = f4zero();
    if (vec) { pv = ld4(p + off); gv = ld4(g + off); mv = ld4(m + off); vv = ld4(v + off); }
    else {
        float* pp = &pv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (off + i < numel) { pp[i] = p[off + i]; gp[i] = g[off + i]; mp[i] = m[off + i]; vp[i] = v[off + i]; }
    }
    const double lr = a.lr_dev ? (double)__hip_atomic_load(a.lr_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.lr;
    // 1 - beta^s = -expm1(s ln beta): fp32 keeps 1e-7 relative accuracy at every s (1 - powf(beta, s) would lose four digits at s = 1),
    // and the double-precision pow / divide / sqrt of the direct form cost 0.8 us of a 6 us launch
    const float step_size = (float)lr / -expm1f(s * (float)log(a.beta1));
    const float bc2_sqrt = sqrtf(-expm1f(s * (float)log(a.beta2)));
    const float omb1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, omb2 = (float)(1.0 - a.beta2), eps = (float)a.eps,
                wd = (float)a.weight_decay;
    adam_one(pv.x, gv.x, mv.x, vv.x, omb1, b2, omb2, step_size, bc2_sqrt, eps, wd);
    adam_one(pv.y, gv.y, mv.y, vv.y, omb1, b2, omb2, step_size, bc2_sqrt, eps, wd);
    adam_one(pv.z, gv.z, mv.z, vv.z, omb1, b2, omb2, step_size, bc2_sqrt, eps, wd);
    adam_one(pv.w, gv.w, mv.w, vv.w, omb1, b2, omb2, step_size, bc2_sqrt, eps, wd);
    if (vec) { st4(p + off, pv); st4(m + off, mv); st4(v + off, vv); }
    else {
        const float* pp = &pv.x; const float* mp = &mv.x; const float* vp = &vv.x;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (off + i < numel) { p[off + i] = pp[i]; m[off + i] = mp[i]; v[off + i] = vp[i]; }
    }
    if (a.bump) {
        __syncthreads();
        if (tid == 0) step_ticket(a.step, a.ticket, s);
    }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Ranger (reference src_1gp/ranger.py:117-205): RAdam + Lookahead + gradient centralisation, the optimizer the reference's search
// draws in half its trials ('optim': choice(['Adam', 'Ranger'])).  One launch over all tensors, per tensor in the reference's order:
//   gc_loc:   g = g - mean_row(g)           (written back: the reference centralises p.grad in place)
//   v = beta2 v + (1 - beta2) g^2            m = beta1 m + (1 - beta1) g
//   rectified (N_sma(s) > threshold):  G = m / (sqrt(v) + eps), step_size = sqrt(...) / (1 - beta1^s)
//   otherwise:                         G = m (an alias: wd / late centralisation below also land in m), step_size = 1 / (1 - beta1^s)
//   G += wd p;   !gc_loc: G = G - mean_row(G);   p -= step_size lr G
//   s % k == 0:  slow += alpha (p - slow);  p = slow
// A row is every index of dimension 0 of a centralised tensor (numel / size(0) elements).  The unit of work is one WAVE per row: the
// row mean is a wave reduction in a fixed order (no LDS, no atomics, no second launch), and a row of any length is walked in passes of
// 256 elements (a float4 per lane) — once for the mean, once for the update, which re-reads the row from L2.  A tensor that is not
// centralised is cut into segments of kRangerFlat elements and walked the same way without the first pass.  Rows of the default
// model are at most 1 024 elements (1 024 rows of 300 in mol_flat): 1 700 waves, 430 workgroups.
// The RAdam rectification is computed in double: N_sma = N_sma_max - 2 s beta2^s / (1 - beta2^s) is the difference of two numbers
// near 2 / (1 - beta2) (2 000) that leaves s, so fp32 would keep 4 significant digits of it — and N_sma(5) = 4.996 sits 0.004 below
// the default threshold.  Everything per element is fp32.
constexpr int kRangerMaxTensors = 40;
constexpr int kRangerPass = 4 * 64;     // elements one wave covers per pass
constexpr int kRangerFlat = 4 * kRangerPass;
static_assert(kRangerMaxTensors <= 64, "one bit per tensor in the 64-bit masks, one lane per tensor boundary in the owner ballot");

struct RangerArgs {
    float* p[kRangerMaxTensors]; float* g[kRangerMaxTensors]; float* m[kRangerMaxTensors]; float* v[kRangerMaxTensors];
    float* slow[kRangerMaxTensors];
    int numel[kRangerMaxTensors];
    int seg[kRangerMaxTensors];          // segment length: the row length of a centralised tensor, kRangerFlat otherwise
    int task_end[kRangerMaxTensors];     // running count of segments: tensor t owns waves [task_end[t-1], task_end[t])
    uint64_t gc_mask, vec_mask;          // bit t: tensor t is centralised / every address and segment start is 16-byte aligned
    int n, tasks;
    float* step; const float* lr_dev; unsigned* ticket;
    double lr, beta1, beta2, eps, weight_decay, alpha, threshold;
    int k, gc_loc, bump;
};

__device__ __forceinline__ void ranger_load(const float* x, int j, int len, bool vec, float (&r)[4]) {
    if (vec && j + 4 <= len) { const float4 t = ld4(x + j); r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = j + i < len ? x[j + i] : 0.f;
    }
}

__device__ __forceinline__ void ranger_store(float* x, int j, int len, bool vec, const float (&r)[4]) {
    if (vec && j + 4 <= len) st4(x + j, make_float4(r[0], r[1], r[2], r[3]));
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (j + i < len) x[j + i] = r[i];
    }
}

// the same fp32 sum in every lane: a butterfly leaves lane-dependent rounding, lane 0's value is broadcast
__device__ __forceinline__ float ranger_wave_sum(float x) { return __shfl(group_sum<64>(x), 0, 64); }

struct RangerScalars { float b1, omb1, b2, omb2, eps, wd, alpha, neg_lr_step; bool rect; };

// G of one element from the updated moments (m, v already advanced)
__device__ __forceinline__ float ranger_G(const RangerScalars& c, float p, float m, float v) {
    float G = c.rect ? m / (sqrtf(v) + c.eps) : m;
    if (c.wd != 0.f) G = G + c.wd * p;
    return G;
}

__global__ void __launch_bounds__(kBlock) k_ranger(RangerArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = blockIdx.x * (kBlock / 64) + (tid >> 6);
    const float s = __hip_atomic_load(a.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1.f;   // agent scope: see k_adam
    if (w < a.tasks) {
        const bool passed = lane < a.n - 1 && w >= a.task_end[lane];
        const int t = __builtin_popcountll(__ballot(passed));
        const int first = t ? a.task_end[t - 1] : 0;
        const int seg = a.seg[t], start = (w - first) * seg, len = min(seg, a.numel[t] - start);
        float* p = a.p[t] + start; float* g = a.g[t] + start; float* m = a.m[t] + start; float* v = a.v[t] + start;
        float* slow = a.slow[t] + start;
        const bool gc = (a.gc_mask >> t) & 1ull, vec = (a.vec_mask >> t) & 1ull;

        RangerScalars c;
        {
            const double sd = s, b2t = pow(a.beta2, sd), n_max = 2.0 / (1.0 - a.beta2) - 1.0;
            const double n_sma = n_max - 2.0 * sd * b2t / (1.0 - b2t);
            const double bc1 = 1.0 - pow(a.beta1, sd);
            c.rect = n_sma > a.threshold;
            // the reference's expression, evaluated left to right as Python does
            const double step_size = c.rect ? sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) / bc1
                                            : 1.0 / bc1;
            const double lr = a.lr_dev ? (double)__hip_atomic_load(a.lr_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.lr;
            c.neg_lr_step = (float)(-step_size * lr);
            c.b1 = (float)a.beta1; c.omb1 = (float)(1.0 - a.beta1); c.b2 = (float)a.beta2; c.omb2 = (float)(1.0 - a.beta2);
            c.eps = (float)a.eps; c.wd = (float)a.weight_decay; c.alpha = (float)a.alpha;
        }
        const bool look = ((int)s % a.k) == 0;
        const bool gc_early = gc && a.gc_loc, gc_late = gc && !a.gc_loc;

        float mean = 0.f;
        if (gc) {                            // pass 1: the row mean of g (gc_loc) or of G (late centralisation)
            float acc = 0.f;
            for (int j = 4 * lane; j < len; j += kRangerPass) {
                float gr[4];
                ranger_load(g, j, len, vec, gr);
                if (gc_early) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc += gr[i];
                } else {
                    float pr[4], mr[4], vr[4];
                    ranger_load(p, j, len, vec, pr); ranger_load(m, j, len, vec, mr); ranger_load(v, j, len, vec, vr);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (j + i >= len) continue;
                        const float vn = c.b2 * vr[i] + c.omb2 * gr[i] * gr[i], mn = c.b1 * mr[i] + c.omb1 * gr[i];
                        acc += ranger_G(c, pr[i], mn, vn);
                    }
                }
            }
            mean = ranger_wave_sum(acc) / (float)len;
        }
        for (int j = 4 * lane; j < len; j += kRangerPass) {     // pass 2: the update
            float pr[4], gr[4], mr[4], vr[4], sr[4];
            ranger_load(p, j, len, vec, pr); ranger_load(g, j, len, vec, gr);
            ranger_load(m, j, len, vec, mr); ranger_load(v, j, len, vec, vr);
            if (look) ranger_load(slow, j, len, vec, sr);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float gi = gr[i];
                if (gc_early) gi = gi - mean;
                gr[i] = gi;
                vr[i] = c.b2 * vr[i] + c.omb2 * gi * gi;
                mr[i] = c.b1 * mr[i] + c.omb1 * gi;
                float G = ranger_G(c, pr[i], mr[i], vr[i]);
                if (gc_late) G = G - mean;
                if (!c.rect) mr[i] = G;              // G aliases exp_avg in the un-rectified branch
                pr[i] = pr[i] + c.neg_lr_step * G;
                if (look) { sr[i] = sr[i] + c.alpha * (pr[i] - sr[i]); pr[i] = sr[i]; }
            }
            ranger_store(p, j, len, vec, pr); ranger_store(m, j, len, vec, mr); ranger_store(v, j, len, vec, vr);
            if (gc_early) ranger_store(g, j, len, vec, gr);
            if (look) ranger_store(slow, j, len, vec, sr);
        }
    }
    if (a.bump) {
        __syncthreads();
        if (tid == 0) step_ticket(a.step, a.ticket, s);
    }
}

}  // namespace glam

using namespace glam;

extern "C" int glam_adam_max_tensors(void) { return kAdamMaxTensors; }

extern "C" int glam_adam_step(const uint64_t* table, const int64_t* numel, int n, float* step, unsigned* ticket, const float* lr_dev,
                              double lr, double beta1, double beta2, double eps, double weight_decay, void* stream) {
    GLAM_REQUIRE(n >= 0 && (n == 0 || (table && numel)) && step && ticket, "glam_adam_step: null pointer / negative count");
    GLAM_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 && weight_decay >= 0, "glam_adam_step: bad hyper-parameters");
    int done = 0;
    // tensors with no elements take no workgroup; the step counter advances even when nothing is left to launch for
    int last_nonempty = -1;
    for (int i = 0; i < n; ++i) {
        GLAM_REQUIRE(numel[i] >= 0 && numel[i] < ((int64_t)1 << 31) - kAdamChunk, "glam_adam_step: tensor too large for 32-bit offsets");
        if (numel[i] > 0) {
            GLAM_REQUIRE(table[4 * i] && table[4 * i + 1] && table[4 * i + 2] && table[4 * i + 3], "glam_adam_step: null tensor pointer");
            last_nonempty = i;
        }
    }
    if (last_nonempty < 0) return GLAM_OK;
    while (done <= last_nonempty) {
        AdamArgs a{};
        int k = 0, chunks = 0;
        while (done <= last_nonempty && k < kAdamMaxTensors) {
            const int i = done++;
            if (numel[i] == 0) continue;
            a.p[k] = (float*)table[4 * i]; a.g[k] = (const float*)table[4 * i + 1];
            a.m[k] = (float*)table[4 * i + 2]; a.v[k] = (float*)table[4 * i + 3];
            a.numel[k] = (int)numel[i];
            chunks += (int)((numel[i] + kAdamChunk - 1) / kAdamChunk);
            a.chunk_end[k] = chunks;
            ++k;
        }
        if (k == 0) break;
        a.n = k; a.step = step; a.lr_dev = lr_dev; a.ticket = ticket;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
        a.bump = done > last_nonempty ? 1 : 0;
        hipLaunchKernelGGL(k_adam, dim3(chunks), dim3(kBlock), 0, (hipStream_t)stream, a);
        GLAM_LAUNCH_CHECK("glam_adam_step");
    }
    return GLAM_OK;
}

extern "C" int glam_ranger_max_tensors(void) { return kRangerMaxTensors; }

extern "C" int glam_ranger_step(const uint64_t* table, const int64_t* numel, const int64_t* row, int n, float* step, unsigned* ticket,
                                const float* lr_dev, double lr, double beta1, double beta2, double eps, double weight_decay,
                                double alpha, int k, double n_sma_threshold, int gc_loc, void* stream) {
    GLAM_REQUIRE(n >= 0 && (n == 0 || (table && numel && row)) && step && ticket, "glam_ranger_step: null pointer / negative count");
    GLAM_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0 && weight_decay >= 0 && alpha >= 0 && alpha <= 1 && k >= 1 &&
                 n_sma_threshold == n_sma_threshold, "glam_ranger_step: bad hyper-parameters");
    int last_nonempty = -1;
    for (int i = 0; i < n; ++i) {
        GLAM_REQUIRE(numel[i] >= 0 && numel[i] < ((int64_t)1 << 31) - kRangerFlat, "glam_ranger_step: tensor too large for 32-bit offsets");
        GLAM_REQUIRE(row[i] >= 0 && (row[i] == 0 || numel[i] % row[i] == 0), "glam_ranger_step: row length does not divide the tensor");
        if (numel[i] > 0) {
            for (int c = 0; c < 5; ++c) GLAM_REQUIRE(table[5 * i + c], "glam_ranger_step: null tensor pointer");
            last_nonempty = i;
        }
    }
    if (last_nonempty < 0) return GLAM_OK;
    int done = 0;
    while (done <= last_nonempty) {
        RangerArgs a{};
        int t = 0;
        int64_t tasks = 0;
        while (done <= last_nonempty && t < kRangerMaxTensors) {
            const int i = done++;
            if (numel[i] == 0) continue;
            a.p[t] = (float*)table[5 * i]; a.g[t] = (float*)table[5 * i + 1]; a.m[t] = (float*)table[5 * i + 2];
            a.v[t] = (float*)table[5 * i + 3]; a.slow[t] = (float*)table[5 * i + 4];
            a.numel[t] = (int)numel[i];
            a.seg[t] = row[i] > 0 ? (int)row[i] : kRangerFlat;
            if (row[i] > 0) a.gc_mask |= 1ull << t;
            uint64_t addr = 0;
            for (int c = 0; c < 5; ++c) addr |= table[5 * i + c];
            if ((addr & 15) == 0 && a.seg[t] % 4 == 0) a.vec_mask |= 1ull << t;
            tasks += (numel[i] + a.seg[t] - 1) / a.seg[t];
            GLAM_REQUIRE(tasks < ((int64_t)1 << 31) - 64, "glam_ranger_step: too many rows for one launch");
            a.task_end[t] = (int)tasks;
            ++t;
        }
        if (t == 0) break;
        a.n = t; a.tasks = (int)tasks; a.step = step; a.lr_dev = lr_dev; a.ticket = ticket;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.alpha = alpha;
        a.threshold = n_sma_threshold; a.k = k; a.gc_loc = gc_loc ? 1 : 0;
        a.bump = done > last_nonempty ? 1 : 0;
        const int waves_per_block = kBlock / 64;
        hipLaunchKernelGGL(k_ranger, dim3((unsigned)((tasks + waves_per_block - 1) / waves_per_block)), dim3(kBlock), 0, (hipStream_t)stream, a);
        GLAM_LAUNCH_CHECK("glam_ranger_step");
    }
    return GLAM_OK;
}
