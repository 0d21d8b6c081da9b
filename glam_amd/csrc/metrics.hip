// Evaluation metrics of the reference's trainers (src_1gp/metrics.py, src_2gi_ddi/utils.py: binary_metrics,
// binary_metrics_multi_target_nan, regression_metrics / cal_ci, screening_metrics / bedroc_score / enrichment_factor_single,
// multi_class_metrics), scored on the device instead of by sklearn and an O(n^2) Python loop.
//
// Counts, not sorts.  Every order-based metric is a function of per-sample counts.  For a valid sample i of one task, over the valid j
// of that task (i itself included in the "equal" counts):
//   gt_all, gt_pos   samples with a strictly higher score (all / positives)
//   eq_all, eq_pos   samples with an equal score
//   eq_before        samples with an equal score and j < i
// ROC-AUC   = sum over negatives of (gt_pos + eq_pos / 2) / (P N)                       (sklearn's trapezoid, ties included)
// PR-AUC    = sum over the first sample of each distinct score (eq_before == 0) of
//             eq_pos / P * (prec_ge + prec_gt) / 2, prec_ge = (gt_pos + eq_pos) / (gt_all + eq_all), prec_gt = gt_pos / gt_all
//             (1 when nothing scores higher: sklearn's appended (recall 0, precision 1) point)
// rank      = 1 + gt_all + eq_before: the descending rank in the STABLE order (ties: lower index first).  BEDROC sums
//             exp(-alpha rank / n) over the positives; EF@p counts the positives with rank <= int(n_valid p).
// CI        over (y, f): pairs = #{j: y_j < y_i}, of those less = #{f_j < f_i}, equal = #{f_j == f_i}; CI = (less + equal / 2) / pairs.
// One thread per sample i walks all j of its task through LDS tiles (every lane reads the same LDS word: a broadcast); the counts stay
// in int32 registers and are never stored.  Each block writes one partial record (integer sums, fp64 sums in a fixed order: wave
// butterfly, then the waves in order); a one-block finish kernel folds the partials of each task in block order and writes the call's
// result record.  Two launches per call; results are bit-identical run to run.
//
// Keys stay in the caller's dtype (float or double: fp64 labels or targets rounded to fp32 would tie where the reference sees none);
// labels / predictions arrive as float or double.  A label outside {0, 1} ({-1, 0, 1} when masked, -1 = missing) or a non-finite
// score of a valid sample sets the record's bad flag; the host raises the reference's ValueError for it.
#include "common.h"

#include <math.h>

namespace glam {

constexpr int kMetBlock = 256;            // samples i per block = LDS tile of j
constexpr int kMetFinish = 1024;          // threads of the finish kernels
constexpr int kMetMaxPct = 5;             // EF percentiles per call (screening_metrics asks for 5)
constexpr int kMcBlocks = 256;            // blocks of the multi-class count kernel
constexpr int kMcMaxClass = 4096;         // LDS: 3 int32 counters per class

struct MetPartial {                       // one block of one task
    long long c[16];
    double d[4];
};
struct MetRecord {                        // the call's result (GLAM_METRICS_RECORD_BYTES)
    long long i[16];
    double d[16];
};
static_assert(sizeof(MetRecord) == GLAM_METRICS_RECORD_BYTES, "record size");

struct MetPct {
    double p[kMetMaxPct];
    int n;
};

// partial slots (binary form)
enum { PB_NVALID = 0, PB_POS, PB_AUC2, PB_TP, PB_FP, PB_TN, PB_FN, PB_EF0, PB_BAD = PB_EF0 + kMetMaxPct };
// partial slots (CI / regression form)
enum { PR_PAIRS = 0, PR_LESS, PR_EQUAL, PR_BAD };

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// block sum in a fixed order: butterfly within each wave, then the waves' results in wave order (every thread gets the total)
template <int NT>
__device__ __forceinline__ double block_sum_f64(double v, double* s) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < NT / 64; ++w) r += s[w];
    return r;
}
template <int NT>
__device__ __forceinline__ long long block_sum_i64(long long v, long long* s) {
    v = wave_sum_i64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < NT / 64; ++w) r += s[w];
    return r;
}

template <typename T> __device__ __forceinline__ T met_nan();
template <> __device__ __forceinline__ float met_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double met_nan<double>() { return __builtin_nan(""); }

// ---- binary forms: one thread per sample i of task t, all j of the task through LDS ------------------------------------------
// score, label, pred: [n, tasks] row-major (task stride `tasks`); pred may be null (pred_mode 1: score >= thr, 2: score > thr).
template <typename T, typename L>
__global__ void __launch_bounds__(kMetBlock) k_metrics_binary_pairs(const T* __restrict__ score, const L* __restrict__ label,
                                                                   const L* __restrict__ pred, long long n, long long tasks, int nb,
                                                                   int masked, int pred_mode, T thr, double alpha, MetPct pct,
                                                                   MetPartial* __restrict__ part) {
    __shared__ T s_key[kMetBlock];
    __shared__ unsigned char s_pos[kMetBlock];
    __shared__ double s_d[kMetBlock / 64];
    __shared__ long long s_i[kMetBlock / 64];
    const int tid = threadIdx.x, b = blockIdx.x % nb;
    const long long t = blockIdx.x / nb;
    const long long i = (long long)b * kMetBlock + tid;

    // this thread's own sample: key, class, prediction
    T ki = met_nan<T>();
    int li = -1, bad = 0, pi = 0;
    if (i < n) {
        const L y = label[i * tasks + t];
        const T s = score[i * tasks + t];
        if (y == (L)0 || y == (L)1) {
            li = y == (L)1;
            ki = s;
            if (!isfinite(s)) bad = 1;
            if (pred_mode == 0) {
                const L p = pred[i * tasks + t];
                if (p == (L)0 || p == (L)1) pi = p == (L)1; else bad = 1;
            } else {
                pi = pred_mode == 1 ? s >= thr : s > thr;
            }
        } else if (!(masked && y == (L)-1)) {
            bad = 1;
        }
    }

    int gt_all = 0, gt_pos = 0, eq_all = 0, eq_pos = 0, eq_before = 0;
    long long n_valid = 0, n_pos = 0;
    for (long long j0 = 0; j0 < n; j0 += kMetBlock) {
        const long long j = j0 + tid;
        T k = met_nan<T>();          // missing rows (and padding) compare false against everything
        int p = 0, v = 0;
        if (j < n) {
            const L y = label[j * tasks + t];
            if (y == (L)0 || y == (L)1) { k = score[j * tasks + t]; p = y == (L)1; v = 1; }
        }
        s_key[tid] = k;
        s_pos[tid] = (unsigned char)p;
        n_valid += __syncthreads_count(v);       // barrier: the tile is visible after it
        n_pos += __syncthreads_count(p);
        const int m = n - j0 < kMetBlock ? (int)(n - j0) : kMetBlock;
        const long long rel = i - j0;            // j < i  <=>  q < rel
        for (int q = 0; q < m; ++q) {
            const T kj = s_key[q];
            const int pj = s_pos[q];
            const int gt = kj > ki, eq = kj == ki;
            gt_all += gt; gt_pos += gt & pj;
            eq_all += eq; eq_pos += eq & pj;
            eq_before += eq & (q < rel);
        }
        __syncthreads();
    }

    long long auc2 = 0, tp = 0, fp = 0, tn = 0, fn = 0, ef[kMetMaxPct] = {0, 0, 0, 0, 0};
    double pr = 0.0, bed = 0.0;
    if (li >= 0) {
        if (li == 0) auc2 = 2LL * gt_pos + eq_pos;
        if (eq_before == 0 && eq_pos > 0 && n_pos > 0) {
            const double prec_ge = (double)(gt_pos + eq_pos) / (double)(gt_all + eq_all);
            const double prec_gt = gt_all > 0 ? (double)gt_pos / (double)gt_all : 1.0;
            pr = (double)eq_pos / (double)n_pos * (prec_ge + prec_gt) / 2.0;
        }
        if (li == 1) {
            const long long rank = 1LL + gt_all + eq_before;
            bed = exp(-alpha * (double)rank / (double)n);
            for (int k = 0; k < pct.n; ++k) ef[k] = rank <= (long long)((double)n_valid * pct.p[k]);
        }
        tp = li & pi; fn = li & (pi ^ 1); fp = (li ^ 1) & pi; tn = (li ^ 1) & (pi ^ 1);
    }
    const long long vals[PB_BAD + 1] = {0, 0, auc2, tp, fp, tn, fn, ef[0], ef[1], ef[2], ef[3], ef[4], bad};
    MetPartial* out = part + t * nb + b;
    for (int s = PB_AUC2; s <= PB_BAD; ++s) {
        const long long v = block_sum_i64<kMetBlock>(vals[s], s_i);
        if (tid == 0) out->c[s] = v;
    }
    pr = block_sum_f64<kMetBlock>(pr, s_d);
    bed = block_sum_f64<kMetBlock>(bed, s_d);
    if (tid == 0) {
        out->c[PB_NVALID] = n_valid;
        out->c[PB_POS] = n_pos;
        out->d[0] = pr;
        out->d[1] = bed;
    }
}

// Per task (thread-strided): fold the partials in block order and derive the task's metrics; the sums over the kept tasks (the
// reference's `sum(list) / len(list)`) then run as a fixed-order block sum.  Task 0's raw counts go into the record too (single-task
// forms).
__global__ void __launch_bounds__(kMetFinish) k_metrics_binary_finish(const MetPartial* __restrict__ part, long long tasks, int nb,
                                                                     MetRecord* __restrict__ rec) {
    __shared__ double s_d[kMetFinish / 64];
    __shared__ long long s_i[kMetFinish / 64];
    long long kept = 0, skipped = 0, bad = 0;
    double s_auc = 0.0, s_acc = 0.0, s_prec = 0.0, s_rec = 0.0;
    for (long long t = threadIdx.x; t < tasks; t += kMetFinish) {
        long long c[PB_BAD + 1] = {};
        double pr = 0.0, bed = 0.0;
        for (int b = 0; b < nb; ++b) {
            const MetPartial& p = part[t * nb + b];
            for (int s = PB_AUC2; s <= PB_BAD; ++s) c[s] += p.c[s];
            pr += p.d[0];
            bed += p.d[1];
        }
        if (nb > 0) { c[PB_NVALID] = part[t * nb].c[PB_NVALID]; c[PB_POS] = part[t * nb].c[PB_POS]; }   // every block counts all j
        const long long P = c[PB_POS], N = c[PB_NVALID] - c[PB_POS];
        bad |= c[PB_BAD] != 0;
        if (P > 0 && N > 0) {
            ++kept;
            s_auc += (double)c[PB_AUC2] / (2.0 * (double)P * (double)N);
            s_acc += (double)(c[PB_TP] + c[PB_TN]) / (double)(P + N);
            s_prec += c[PB_TP] + c[PB_FP] > 0 ? (double)c[PB_TP] / (double)(c[PB_TP] + c[PB_FP]) : 0.0;
            s_rec += (double)c[PB_TP] / (double)P;
        } else {
            ++skipped;
        }
        if (t == 0) {
            rec->i[3] = P; rec->i[4] = N;
            rec->i[5] = c[PB_TP]; rec->i[6] = c[PB_FP]; rec->i[7] = c[PB_TN]; rec->i[8] = c[PB_FN];
            for (int k = 0; k < kMetMaxPct; ++k) rec->i[9 + k] = c[PB_EF0 + k];
            rec->i[14] = c[PB_AUC2];
            rec->d[4] = pr; rec->d[5] = bed;
        }
    }
    kept = block_sum_i64<kMetFinish>(kept, s_i);
    skipped = block_sum_i64<kMetFinish>(skipped, s_i);
    bad = block_sum_i64<kMetFinish>(bad, s_i);
    s_auc = block_sum_f64<kMetFinish>(s_auc, s_d);
    s_acc = block_sum_f64<kMetFinish>(s_acc, s_d);
    s_prec = block_sum_f64<kMetFinish>(s_prec, s_d);
    s_rec = block_sum_f64<kMetFinish>(s_rec, s_d);
    if (threadIdx.x == 0) {
        rec->i[0] = kept; rec->i[1] = skipped; rec->i[2] = bad != 0;
        rec->d[0] = s_auc; rec->d[1] = s_acc; rec->d[2] = s_prec; rec->d[3] = s_rec;
    }
}

// ---- regression: CI pair counts plus the squared-error partials ------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kMetBlock) k_metrics_ci_pairs(const T* __restrict__ y, const T* __restrict__ f, long long n,
                                                               MetPartial* __restrict__ part) {
    __shared__ T s_y[kMetBlock], s_f[kMetBlock];
    __shared__ double s_d[kMetBlock / 64];
    __shared__ long long s_i[kMetBlock / 64];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMetBlock + tid;
    T yi = met_nan<T>(), fi = met_nan<T>();
    double sy = 0.0, se = 0.0;
    int bad = 0;
    if (i < n) {
        yi = y[i]; fi = f[i];
        bad = !isfinite(yi) || !isfinite(fi);
        const double d = (double)yi - (double)fi;
        sy = (double)yi;
        se = d * d;
    }
    int pairs = 0, less = 0, equal = 0;
    for (long long j0 = 0; j0 < n; j0 += kMetBlock) {
        const long long j = j0 + tid;
        s_y[tid] = j < n ? y[j] : met_nan<T>();
        s_f[tid] = j < n ? f[j] : met_nan<T>();
        __syncthreads();
        const int m = n - j0 < kMetBlock ? (int)(n - j0) : kMetBlock;
        for (int q = 0; q < m; ++q) {
            const T yj = s_y[q], fj = s_f[q];
            const int lt = yj < yi;
            pairs += lt;
            less += lt & (fj < fi);
            equal += lt & (fj == fi);
        }
        __syncthreads();
    }
    const long long vals[PR_BAD + 1] = {pairs, less, equal, bad};
    MetPartial* out = part + blockIdx.x;
    for (int s = 0; s <= PR_BAD; ++s) {
        const long long v = block_sum_i64<kMetBlock>(vals[s], s_i);
        if (tid == 0) out->c[s] = v;
    }
    sy = block_sum_f64<kMetBlock>(sy, s_d);
    se = block_sum_f64<kMetBlock>(se, s_d);
    if (tid == 0) { out->d[0] = sy; out->d[1] = se; }
}

// folds the partials in block order, then the second pass sum (y - mean)^2 over all samples (r2_score's denominator)
template <typename T>
__global__ void __launch_bounds__(kMetFinish) k_metrics_ci_finish(const T* __restrict__ y, long long n, const MetPartial* __restrict__ part,
                                                                 int nb, MetRecord* __restrict__ rec) {
    __shared__ double s_d[kMetFinish / 64];
    __shared__ double s_mean;
    if (threadIdx.x == 0) {
        long long c[PR_BAD + 1] = {};
        double sy = 0.0, se = 0.0;
        for (int b = 0; b < nb; ++b) {
            for (int s = 0; s <= PR_BAD; ++s) c[s] += part[b].c[s];
            sy += part[b].d[0];
            se += part[b].d[1];
        }
        for (int s = 0; s <= PR_BAD; ++s) rec->i[s] = c[s];
        rec->d[0] = se;
        rec->d[2] = sy;
        s_mean = n > 0 ? sy / (double)n : 0.0;
    }
    __syncthreads();
    const double mean = s_mean;
    double st = 0.0;
    for (long long i = threadIdx.x; i < n; i += kMetFinish) {
        const double d = (double)y[i] - mean;
        st += d * d;
    }
    st = block_sum_f64<kMetFinish>(st, s_d);
    if (threadIdx.x == 0) rec->d[1] = st;
}

// ---- multi-class: argmax per row (ties: the first maximum, a NaN wins as in np.argmax), per-class counts --------------------------
template <typename T>
__device__ __forceinline__ bool mc_better(T va, int ia, T vb, int ib) {
    const bool na = va != va, nbn = vb != vb;
    if (na != nbn) return na;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}

// counts per block: ws[b][0][c] rows with label c, [1][c] rows predicted c, [2][c] rows with both; bad[b]
template <typename T, typename L>
__global__ void __launch_bounds__(kMetBlock) k_metrics_mc_counts(const T* __restrict__ score, const L* __restrict__ label,
                                                                const L* __restrict__ pred, long long n, int n_class,
                                                                int* __restrict__ counts, int* __restrict__ bad_out) {
    extern __shared__ int s_cnt[];     // [3][n_class]
    __shared__ int s_bad;
    for (int c = threadIdx.x; c < 3 * n_class; c += kMetBlock) s_cnt[c] = 0;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, waves = kMetBlock / 64;
    for (long long r = (long long)blockIdx.x * waves + (threadIdx.x >> 6); r < n; r += (long long)gridDim.x * waves) {
        int p = 0;
        if (pred == nullptr) {
            T bv = met_nan<T>();
            int bi = 0x7fffffff;
            for (int c = lane; c < n_class; c += 64) {
                const T v = score[r * n_class + c];
                if (bi == 0x7fffffff || mc_better(v, c, bv, bi)) { bv = v; bi = c; }
            }
            for (int m = 32; m >= 1; m >>= 1) {
                const T ov = __shfl_xor(bv, m, 64);
                const int oi = __shfl_xor(bi, m, 64);
                if (oi != 0x7fffffff && (bi == 0x7fffffff || mc_better(ov, oi, bv, bi))) { bv = ov; bi = oi; }
            }
            p = bi;
        }
        if (lane == 0) {
            const L y = label[r];
            int ok = y >= (L)0 && y < (L)n_class && y == (L)(long long)y;
            if (pred != nullptr) {
                const L q = pred[r];
                const int okp = q >= (L)0 && q < (L)n_class && q == (L)(long long)q;
                ok &= okp;
                p = okp ? (int)q : 0;
            }
            if (ok) {
                const int yc = (int)y;
                atomicAdd(&s_cnt[yc], 1);
                atomicAdd(&s_cnt[n_class + p], 1);
                if (yc == p) atomicAdd(&s_cnt[2 * n_class + yc], 1);
            } else {
                atomicOr(&s_bad, 1);
            }
        }
    }
    __syncthreads();
    int* out = counts + (long long)blockIdx.x * 3 * n_class;
    for (int c = threadIdx.x; c < 3 * n_class; c += kMetBlock) out[c] = s_cnt[c];
    if (threadIdx.x == 0) bad_out[blockIdx.x] = s_bad;
}

// per class (thread-strided) over the blocks; the averages over the classes seen (labels or predictions) as fixed-order block sums
__global__ void __launch_bounds__(kMetFinish) k_metrics_mc_finish(const int* __restrict__ counts, const int* __restrict__ bad_in, int nb,
                                                                 long long n, int n_class, MetRecord* __restrict__ rec) {
    __shared__ double s_d[kMetFinish / 64];
    __shared__ long long s_i[kMetFinish / 64];
    long long seen = 0, correct = 0, bad = 0;
    double sp = 0.0, sr = 0.0, sf = 0.0;
    for (int c = threadIdx.x; c < n_class; c += kMetFinish) {
        long long tr = 0, pr = 0, tp = 0;
        for (int b = 0; b < nb; ++b) {
            const int* q = counts + (long long)b * 3 * n_class;
            tr += q[c]; pr += q[n_class + c]; tp += q[2 * n_class + c];
        }
        correct += tp;
        if (tr + pr == 0) continue;
        ++seen;
        sp += pr > 0 ? (double)tp / (double)pr : 0.0;
        sr += tr > 0 ? (double)tp / (double)tr : 0.0;
        sf += 2.0 * (double)tp / (double)(tr + pr);
    }
    for (int b = threadIdx.x; b < nb; b += kMetFinish) bad |= bad_in[b];
    seen = block_sum_i64<kMetFinish>(seen, s_i);
    correct = block_sum_i64<kMetFinish>(correct, s_i);
    bad = block_sum_i64<kMetFinish>(bad, s_i);
    sp = block_sum_f64<kMetFinish>(sp, s_d);
    sr = block_sum_f64<kMetFinish>(sr, s_d);
    sf = block_sum_f64<kMetFinish>(sf, s_d);
    if (threadIdx.x == 0) {
        rec->i[0] = correct; rec->i[1] = seen; rec->i[2] = bad != 0; rec->i[3] = n;
        rec->d[0] = sp; rec->d[1] = sr; rec->d[2] = sf;
    }
}

static inline long long met_blocks(long long n) { return (n + kMetBlock - 1) / kMetBlock; }
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int mc_blocks(long long n) {
    long long g = (n + 3) / 4;
    return (int)(g < 1 ? 1 : g > kMcBlocks ? kMcBlocks : g);
}

}  // namespace glam

using namespace glam;

extern "C" size_t glam_metrics_workspace_bytes(int64_t n, int64_t tasks, int n_class) {
    if (n < 0 || n >= GLAM_METRICS_MAX_N || tasks < 1 || n_class < 0 || n_class > kMcMaxClass) return 0;
    if (n_class > 0)
        return align256((size_t)mc_blocks(n) * 3 * n_class * sizeof(int)) + align256((size_t)mc_blocks(n) * sizeof(int));
    return align256((size_t)(met_blocks(n) > 0 ? met_blocks(n) : 1) * tasks * sizeof(MetPartial));
}

extern "C" int glam_metrics_binary(const void* score, const void* label, const void* pred, int key_dtype, int label_dtype, int64_t n,
                                   int64_t tasks, int masked, int pred_mode, double threshold, double alpha, const double* pct_host,
                                   int n_pct, void* ws, size_t ws_bytes, void* record, void* stream) {
    GLAM_REQUIRE(n >= 0 && n < GLAM_METRICS_MAX_N, "glam_metrics_binary: n = %lld outside [0, 2^31 - 1)", (long long)n);
    GLAM_REQUIRE(tasks >= 1 && met_blocks(n) * tasks < ((int64_t)1 << 31), "glam_metrics_binary: bad task count %lld", (long long)tasks);
    GLAM_REQUIRE((key_dtype == 0 || key_dtype == 1) && (label_dtype == 0 || label_dtype == 1), "glam_metrics_binary: bad dtype");
    GLAM_REQUIRE(pred_mode >= 0 && pred_mode <= 2 && n_pct >= 0 && n_pct <= kMetMaxPct && (n_pct == 0 || pct_host),
                 "glam_metrics_binary: bad prediction mode / percentiles");
    GLAM_REQUIRE(record && (n == 0 || (score && label && (pred_mode != 0 || pred))), "glam_metrics_binary: null pointer");
    GLAM_REQUIRE(ws && ws_bytes >= glam_metrics_workspace_bytes(n, tasks, 0), "glam_metrics_binary: workspace too small");
    const long long nbl = met_blocks(n);
    MetPartial* part = (MetPartial*)ws;
    MetPct pct = {};
    for (int k = 0; k < n_pct; ++k) pct.p[k] = pct_host[k];
    pct.n = n_pct;
    hipStream_t s = (hipStream_t)stream;
    const void* pr = pred_mode == 0 ? pred : nullptr;
    if (nbl > 0) {
        const dim3 grid((unsigned)(nbl * tasks));
#define GLAM_MET_PAIRS(T, L)                                                                                                   \
        hipLaunchKernelGGL((k_metrics_binary_pairs<T, L>), grid, dim3(kMetBlock), 0, s, (const T*)score, (const L*)label,     \
                           (const L*)pr, (long long)n, (long long)tasks, (int)nbl, masked, pred_mode, (T)threshold, alpha, pct, part)
        if (key_dtype == 0 && label_dtype == 0) GLAM_MET_PAIRS(float, float);
        else if (key_dtype == 0) GLAM_MET_PAIRS(float, double);
        else if (label_dtype == 0) GLAM_MET_PAIRS(double, float);
        else GLAM_MET_PAIRS(double, double);
#undef GLAM_MET_PAIRS
        GLAM_LAUNCH_CHECK("glam_metrics_binary");
    }
    hipLaunchKernelGGL(k_metrics_binary_finish, dim3(1), dim3(kMetFinish), 0, s, part, (long long)tasks, (int)nbl, (MetRecord*)record);
    GLAM_LAUNCH_CHECK("glam_metrics_binary");
    return GLAM_OK;
}

extern "C" int glam_metrics_regression(const void* y, const void* f, int dtype, int64_t n, void* ws, size_t ws_bytes, void* record,
                                       void* stream) {
    GLAM_REQUIRE(n >= 0 && n < GLAM_METRICS_MAX_N, "glam_metrics_regression: n = %lld outside [0, 2^31 - 1)", (long long)n);
    GLAM_REQUIRE(dtype == 0 || dtype == 1, "glam_metrics_regression: bad dtype");
    GLAM_REQUIRE(record && (n == 0 || (y && f)), "glam_metrics_regression: null pointer");
    GLAM_REQUIRE(ws && ws_bytes >= glam_metrics_workspace_bytes(n, 1, 0), "glam_metrics_regression: workspace too small");
    const long long nbl = met_blocks(n);
    MetPartial* part = (MetPartial*)ws;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0) {
        if (nbl > 0) hipLaunchKernelGGL(k_metrics_ci_pairs<float>, dim3((unsigned)nbl), dim3(kMetBlock), 0, s, (const float*)y, (const float*)f, (long long)n, part);
        GLAM_LAUNCH_CHECK("glam_metrics_regression");
        hipLaunchKernelGGL(k_metrics_ci_finish<float>, dim3(1), dim3(kMetFinish), 0, s, (const float*)y, (long long)n, part, (int)nbl, (MetRecord*)record);
    } else {
        if (nbl > 0) hipLaunchKernelGGL(k_metrics_ci_pairs<double>, dim3((unsigned)nbl), dim3(kMetBlock), 0, s, (const double*)y, (const double*)f, (long long)n, part);
        GLAM_LAUNCH_CHECK("glam_metrics_regression");
        hipLaunchKernelGGL(k_metrics_ci_finish<double>, dim3(1), dim3(kMetFinish), 0, s, (const double*)y, (long long)n, part, (int)nbl, (MetRecord*)record);
    }
    GLAM_LAUNCH_CHECK("glam_metrics_regression");
    return GLAM_OK;
}

extern "C" int glam_metrics_multiclass(const void* score, const void* label, const void* pred, int key_dtype, int label_dtype, int64_t n,
                                       int n_class, void* ws, size_t ws_bytes, void* record, void* stream) {
    GLAM_REQUIRE(n >= 0 && n < GLAM_METRICS_MAX_N, "glam_metrics_multiclass: n = %lld outside [0, 2^31 - 1)", (long long)n);
    GLAM_REQUIRE(n_class >= 1 && n_class <= kMcMaxClass, "glam_metrics_multiclass: n_class = %d outside [1, %d]", n_class, kMcMaxClass);
    GLAM_REQUIRE((key_dtype == 0 || key_dtype == 1) && (label_dtype == 0 || label_dtype == 1), "glam_metrics_multiclass: bad dtype");
    GLAM_REQUIRE(record && (n == 0 || (label && (score || pred))), "glam_metrics_multiclass: null pointer");
    GLAM_REQUIRE(ws && ws_bytes >= glam_metrics_workspace_bytes(n, 1, n_class), "glam_metrics_multiclass: workspace too small");
    const int nb = mc_blocks(n);
    int* counts = (int*)ws;
    int* bad = (int*)((char*)ws + align256((size_t)nb * 3 * n_class * sizeof(int)));
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)3 * n_class * sizeof(int);
#define GLAM_MET_MC(T, L)                                                                                                     \
    hipLaunchKernelGGL((k_metrics_mc_counts<T, L>), dim3(nb), dim3(kMetBlock), lds, s, (const T*)score, (const L*)label, (const L*)pred, \
                       (long long)n, n_class, counts, bad)
    if (key_dtype == 0 && label_dtype == 0) GLAM_MET_MC(float, float);
    else if (key_dtype == 0) GLAM_MET_MC(float, double);
    else if (label_dtype == 0) GLAM_MET_MC(double, float);
    else GLAM_MET_MC(double, double);
#undef GLAM_MET_MC
    GLAM_LAUNCH_CHECK("glam_metrics_multiclass");
    hipLaunchKernelGGL(k_metrics_mc_finish, dim3(1), dim3(kMetFinish), 0, s, counts, bad, nb, (long long)n, n_class, (MetRecord*)record);
    GLAM_LAUNCH_CHECK("glam_metrics_multiclass");
    return GLAM_OK;
}
