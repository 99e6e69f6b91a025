// hit@k and NDCG@k of generated semantic ids in one launch (reference evaluate/metrics.py:17-30 TopKAccumulator.accumulate and :63-91
// NDCGAccumulator.accumulate): for every batch row, every slice :i+1 and every position i < D, does beam j repeat the true item's ids
// there, and what do the matching beams' ranks add to each k's hit count and NDCG sum.
//
// Relevance is binary, so a row's relevance vector under one predicate is a K-bit set and both metrics have a closed form on it
// (mask: the set, first = ctz(mask), m = popcount(mask), disc[j] = 1 / log2(j + 2)):
//     hit@k   = mask != 0 and first < k
//     NDCG@k  = sum_{j < k, j in mask} disc[j] / sum_{j < min(m, k)} disc[j]       (0 when m = 0; not computed at all when k > K)
// m counts the matches among all K beams: the reference sorts the whole relevance row before it truncates the ideal ordering.
//
// One wave per batch row, a lane per beam (K <= 64): the lane loads its beam's D ids, a __ballot per predicate gives the 2 D masks,
// and then the lanes change roles: lane e (and e + 64) owns the accumulator of entry e = ((kind * D + i) * nk + kidx), picks its
// predicate's mask out of the ballots and adds the row's term to a register.  Nothing in fp64 but the adds and one division: the
// discount table (disc[0 .. 64), then its running sums cum[0 .. 64]) is computed on the host and read through LDS.
//
// Determinism: a wave walks its rows in ascending order, a workgroup adds its 16 waves' sums in wave order and stores one partial per
// entry; the workgroup that arrives last adds the partials onto the state, sixteen consecutive workgroups' at a time and those sums in
// order.  The grid is a function of B alone, so two calls on the same inputs add the same numbers in the same order.  The hit counts
// are integers and go to the state with integer atomics.
#include "common.h"

namespace {

constexpr int RM_WAVES = HIDVAE_METRICS_ROWS_PER_BLOCK;  // one wave per batch row at a time
constexpr int RM_THREADS = RM_WAVES * HV_WAVE;
constexpr int RM_SLOTS = 2 * HIDVAE_METRICS_MAX_D * HIDVAE_METRICS_MAX_KS;  // entries of the state, and of one workgroup's partial
constexpr int RM_TABLE = 2 * HIDVAE_BEAM_MAX_K + 1;                         // disc[64], cum[65]
constexpr int RM_CHUNK = HIDVAE_METRICS_MAX_BLOCKS / (RM_THREADS / RM_SLOTS);  // partials one thread of the last workgroup adds
static_assert(RM_SLOTS == 2 * HV_WAVE, "a lane owns the entries e and e + 64");
static_assert(RM_THREADS % RM_SLOTS == 0 && RM_CHUNK * (RM_THREADS / RM_SLOTS) == HIDVAE_METRICS_MAX_BLOCKS && RM_THREADS / RM_SLOTS <= RM_WAVES,
              "the last workgroup's thread groups cover every workgroup's partial and fit the LDS rows");

struct MetricArgs {
    const void *actual;  // [B, D], row stride lda
    int64_t lda;
    const void *top;     // [B, K, D], row stride ldr, beam stride ldb
    int64_t ldr, ldb, B;
    int K, D, nk, want_hits, want_ndcg;
    int ks[HIDVAE_METRICS_MAX_KS];
    const double *table;       // device: disc[0 .. 64), cum[0 .. 64]
    unsigned long long *hits;  // [2][8][8]
    double *ndcg;              // [2][8][8]
    unsigned long long *rows;
    unsigned *counter;         // arrivals; zero on entry, zero on return
    double *partials;          // [gridDim.x][RM_SLOTS]
};

// state slot of entry e = (kind * D + i) * nk + kidx: ((kind * 8) + i) * 8 + kidx, whatever D and nk this call has
__device__ __forceinline__ int state_slot(int e, int D, int nk) {
    const int p = e / nk, kidx = e - p * nk, kind = p >= D ? 1 : 0, i = p - kind * D;
    return (kind * HIDVAE_METRICS_MAX_D + i) * HIDVAE_METRICS_MAX_KS + kidx;
}

template <typename TA, typename TB>
__global__ __launch_bounds__(RM_THREADS) void retrieval_metrics_kernel(MetricArgs a) {
    __shared__ double s_table[RM_TABLE];
    __shared__ double s_sum[RM_WAVES][RM_SLOTS];
    __shared__ unsigned s_hit[RM_WAVES][RM_SLOTS];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, D = a.D, nk = a.nk, nE = 2 * D * nk;
    if (a.want_ndcg)  // (hits alone need no discounts: the table pointer may be null)
        for (int i = tid; i < RM_TABLE; i += RM_THREADS) s_table[i] = a.table[i];

    // the two entries this lane accumulates: their predicate (slice :i+1 -> i, position i -> D + i) and their k
    int pred[2], kk[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int e = lane + u * HV_WAVE;
        pred[u] = e < nE ? e / nk : -1;
        const int kidx = e < nE ? e - pred[u] * nk : -1;
        kk[u] = 0;
#pragma unroll
        for (int j = 0; j < HIDVAE_METRICS_MAX_KS; j++) kk[u] = kidx == j ? a.ks[j] : kk[u];
    }
    __syncthreads();

    double sum[2] = {0.0, 0.0};
    unsigned hit[2] = {0u, 0u};
    const TA *actual = reinterpret_cast<const TA *>(a.actual);
    const TB *top = reinterpret_cast<const TB *>(a.top);
    const bool beam = lane < K;
    const int64_t stride = (int64_t)gridDim.x * RM_WAVES;
    for (int64_t b = (int64_t)blockIdx.x * RM_WAVES + wave; b < a.B; b += stride) {
        const TA *arow = actual + b * a.lda;
        const TB *trow = top + b * a.ldr + (beam ? lane : 0) * a.ldb;
        uint64_t mask[2] = {0, 0};
        bool run = beam;
#pragma unroll
        for (int d = 0; d < HIDVAE_METRICS_MAX_D; d++) {
            if (d < D) {
                const bool eq = beam && (int64_t)trow[d] == (int64_t)arow[d];  // ids are compared as the integers they are, never indexed with
                run = run && eq;
                const uint64_t m_slice = __ballot(run), m_pos = __ballot(eq);
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    mask[u] = pred[u] == d ? m_slice : mask[u];
                    mask[u] = pred[u] == D + d ? m_pos : mask[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint64_t m = mask[u];
            if (pred[u] < 0 || m == 0) continue;
            const int k = kk[u];
            if (a.want_hits && __builtin_ctzll(m) < k) hit[u]++;
            if (a.want_ndcg && k <= K) {
                uint64_t low = k >= 64 ? m : (m & ((1ull << k) - 1ull));
                double dcg = 0.0;
                while (low) {  // ascending rank
                    dcg += s_table[__builtin_ctzll(low)];
                    low &= low - 1;
                }
                const int n = __popcll(m);
                sum[u] += dcg / s_table[HIDVAE_BEAM_MAX_K + (n < k ? n : k)];
            }
        }
    }

#pragma unroll
    for (int u = 0; u < 2; u++) {
        s_sum[wave][lane + u * HV_WAVE] = sum[u];
        s_hit[wave][lane + u * HV_WAVE] = hit[u];
    }
    __syncthreads();
    if (tid < nE) {
        double t = s_sum[0][tid];
        unsigned h = s_hit[0][tid];
#pragma unroll
        for (int w = 1; w < RM_WAVES; w++) t += s_sum[w][tid], h += s_hit[w][tid];
        if (a.want_hits && h) atomicAdd(a.hits + state_slot(tid, D, nk), (unsigned long long)h);
        if (a.want_ndcg) a.partials[(int64_t)blockIdx.x * RM_SLOTS + tid] = t;
    }
    if (blockIdx.x == 0 && tid == 0) atomicAdd(a.rows, (unsigned long long)a.B);
    if (!a.want_ndcg) return;

    // the partial is published, the arrival counted; whoever arrives last adds all of them in workgroup order
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        s_last = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    }
    __syncthreads();
    // eight groups of threads add sixteen workgroups' partials each, their loads in flight together, then the groups' sums are added
    // in group order: still one fixed order, without 127 dependent round trips to memory
    {
        const int e = tid & (RM_SLOTS - 1), c = tid / RM_SLOTS;
        double v[RM_CHUNK];
#pragma unroll
        for (int j = 0; j < RM_CHUNK; j++) {
            const unsigned g = c * RM_CHUNK + j;
            v[j] = (e < nE && g < gridDim.x)
                       ? __hip_atomic_load(a.partials + (int64_t)g * RM_SLOTS + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                       : 0.0;
        }
        double t = v[0];
#pragma unroll
        for (int j = 1; j < RM_CHUNK; j++) t += v[j];
        s_sum[c][e] = t;
    }
    __syncthreads();
    if (tid < nE) {
        double t = s_sum[0][tid];
        for (unsigned c = 1; c * RM_CHUNK < gridDim.x; c++) t += s_sum[c][tid];
        a.ndcg[state_slot(tid, D, nk)] += t;
    }
    if (tid == 0) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // clean for the next launch
}

// (the workspace formula of api.cpp counts the same workgroups)
int64_t metric_blocks(int64_t B) {
    const int64_t g = hv_cdiv(B, RM_WAVES);
    return g < 1 ? 1 : (g > HIDVAE_METRICS_MAX_BLOCKS ? HIDVAE_METRICS_MAX_BLOCKS : g);
}

template <typename TA, typename TB>
int launch(const MetricArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((retrieval_metrics_kernel<TA, TB>), dim3((unsigned)metric_blocks(a.B)), dim3(RM_THREADS), 0, s, a);
    HV_LAUNCH_CHECK("retrieval_metrics");
    return HIDVAE_OK;
}

}  // namespace

extern "C" int hidvae_retrieval_metrics(const void *actual, int actual_bytes, int64_t lda, const void *top_k, int top_k_bytes, int64_t ld_row,
                                        int64_t ld_beam, int64_t B, int K, int D, const int32_t *ks_host, int nk, int flags,
                                        const double *discounts, int64_t *hits, double *ndcg, int64_t *rows, void *workspace, void *stream) {
    HV_REQUIRE((actual_bytes == 4 || actual_bytes == 8) && (top_k_bytes == 4 || top_k_bytes == 8),
               "retrieval_metrics: ids of %d / %d bytes (int32 or int64)", actual_bytes, top_k_bytes);
    HV_REQUIRE(K >= 1 && K <= HIDVAE_BEAM_MAX_K, "retrieval_metrics: K = %d beams (1 .. %d)", K, HIDVAE_BEAM_MAX_K);
    HV_REQUIRE(D >= 1 && D <= HIDVAE_METRICS_MAX_D, "retrieval_metrics: D = %d id positions (1 .. %d)", D, HIDVAE_METRICS_MAX_D);
    HV_REQUIRE(nk >= 1 && nk <= HIDVAE_METRICS_MAX_KS && ks_host, "retrieval_metrics: %d values of k (1 .. %d)", nk, HIDVAE_METRICS_MAX_KS);
    for (int j = 0; j < nk; j++) HV_REQUIRE(ks_host[j] >= 1, "retrieval_metrics: k = %d (>= 1)", (int)ks_host[j]);
    HV_REQUIRE(flags != 0 && (flags & ~(HIDVAE_METRICS_HITS | HIDVAE_METRICS_NDCG)) == 0, "retrieval_metrics: flags %d (HITS | NDCG)", flags);
    HV_REQUIRE(B >= 0 && B <= INT32_MAX && lda >= 0 && ld_row >= 0 && ld_beam >= 0, "retrieval_metrics: bad arguments");
    HV_REQUIRE(rows && (!(flags & HIDVAE_METRICS_HITS) || hits) && (!(flags & HIDVAE_METRICS_NDCG) || (ndcg && discounts && workspace)),
               "retrieval_metrics: a state, table or workspace pointer the flags ask for is null");
    if (B == 0) return HIDVAE_OK;
    HV_REQUIRE(actual && top_k, "retrieval_metrics: bad arguments");
    MetricArgs a;
    a.actual = actual, a.lda = lda, a.top = top_k, a.ldr = ld_row, a.ldb = ld_beam, a.B = B;
    a.K = K, a.D = D, a.nk = nk;
    a.want_hits = (flags & HIDVAE_METRICS_HITS) != 0, a.want_ndcg = (flags & HIDVAE_METRICS_NDCG) != 0;
    for (int j = 0; j < HIDVAE_METRICS_MAX_KS; j++) a.ks[j] = j < nk ? ks_host[j] : 0;
    a.table = discounts;
    a.hits = reinterpret_cast<unsigned long long *>(hits), a.ndcg = ndcg, a.rows = reinterpret_cast<unsigned long long *>(rows);
    a.counter = reinterpret_cast<unsigned *>(workspace);
    a.partials = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(workspace) + 8);
    const hipStream_t s = (hipStream_t)stream;
    if (actual_bytes == 4) return top_k_bytes == 4 ? launch<int32_t, int32_t>(a, s) : launch<int32_t, int64_t>(a, s);
    return top_k_bytes == 4 ? launch<int64_t, int32_t>(a, s) : launch<int64_t, int64_t>(a, s);
}
