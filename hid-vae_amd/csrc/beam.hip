// One constrained beam-search step in one launch (reference modules/model.py:200-226, generate_next_sem_id's loop body): the
// log-softmax of each parent beam's logits row at its candidate ids, the validity of parent + candidate in the prefix index
// (prefix.h), the score (-10000 * (not valid) + logp) + parent log-probability, and the k best of the k_prev * C candidates of a batch
// item, ordered by (score descending, flat index j * C + c ascending), with the parents' ids carried along.
//
// One 1024-thread workgroup per batch item (at B = 256 one per CU; the step is bound by the latency of dependent binary-search loads,
// so 16 waves hide more of it than 4 would).  One thread per parent finds the parent's key range [a, b) in the sorted keys; one wave
// per parent row takes the running max / sum of exp over the V logits (one pass, 16-byte loads); both go to LDS.  Then the threads
// walk the flat candidate index, seven candidates per thread at a time with their searches interleaved, and leave each score in LDS as
// an order-preserving 32-bit key and each validity as one bit.  The selection is k rounds of workgroup arg-max over 64-bit (score key,
// ~flat index) words: every thread keeps the best of the slots it owns (flat index mod 1024) in a register, a round is one wave
// reduction + one 16-entry LDS exchange, and only the winner's owner rescans its n / 1024 slots.  With k <= 64 of up to 32768 scores
// that reads LDS k * n / 1024 times per thread at the worst, where a bitonic sort of the padded array would move all n scores
// log^2(n) / 2 times (105 passes at n = 32768) to order 32768 entries of which k are wanted, and a per-parent top-k followed by a
// merge would need k * k_prev staging slots and a second selection for the same result.
#include <float.h>
#include "prefix.h"

namespace {

constexpr int BEAM_THREADS = 1024;
constexpr int BEAM_WAVES = BEAM_THREADS / HV_WAVE;
constexpr int BEAM_UNROLL = 7;  // candidates a thread searches for at a time (7 x 1024 >= 32 x 200: one pass at the reference's shape)
// LDS head: 2 x 16 reduction slots, the k winners, then per parent its key, key range, row max, log sum exp and log-probability
constexpr int BEAM_HEAD_BYTES = (2 * BEAM_WAVES + HIDVAE_BEAM_MAX_K) * 8 + HIDVAE_BEAM_MAX_K * (3 * 8 + 3 * 4);

struct BeamArgs {
    const float *logits;      // [B * k_prev, V], row stride ld_logits
    int64_t ld_logits, V;
    const void *cand;         // [B * k_prev, C] int32 / int64, row stride ldc; unused when the candidate is its own id
    int64_t ldc;
    int C;
    const int64_t *generated; // [B * k_prev, w], row stride ldg; unused at w = 0
    int64_t ldg;
    const float *log_probas;  // [B * k_prev] or nullptr (zeros)
    int k_prev, w, k;
    float temperature;
    int vec4;                 // every logits row is 16-byte aligned and V % 4 == 0
    int64_t lo_w, radix_w, span_w, span_next;
    const int64_t *keys;
    int64_t n_keys;
    int64_t *out_ids;         // [B, k, w + 1]
    float *out_logp;          // [B, k]
    int64_t *out_parents;     // [B, k]
    uint8_t *out_valid;       // [B, k]
};

// float -> uint32 whose unsigned order is the float order (-0 and +0 were made one value before); 0 is kept for "taken"
__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return o ? o : 1u;
}
__device__ __forceinline__ float order_value(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// max over the wave, the same value in every lane.  Data-parallel-primitive moves (lanes swapped inside quads, rows rotated by 4 and
// 8, then lane 15 / 31 broadcast into the following rows) leave the maximum in lane 63: six register moves per half instead of six
// trips through the LDS crossbar, on a chain that every one of the k selection rounds waits for.
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_max_step(uint64_t v) {
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);  // (a lane without a source keeps its own)
    const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    const uint64_t other = ((uint64_t)ohi << 32) | olo;
    return other > v ? other : v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    v = dpp_max_step<0xb1>(v);   // quad_perm:[1,0,3,2]
    v = dpp_max_step<0x4e>(v);   // quad_perm:[2,3,0,1]
    v = dpp_max_step<0x124>(v);  // row_ror:4
    v = dpp_max_step<0x128>(v);  // row_ror:8
    v = dpp_max_step<0x142>(v);  // row_bcast:15
    v = dpp_max_step<0x143>(v);  // row_bcast:31
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

// the parent's key range: lower_bound of x0 and of x1 >= x0 over [0, n), both searches advancing together
__device__ __forceinline__ void lower_bound_pair(const int64_t *keys, int64_t n, int64_t x0, int64_t x1, int64_t &r0, int64_t &r1) {
    int64_t a0 = 0, b0 = n, a1 = 0, b1 = n;
    while (a0 < b0 || a1 < b1) {
        const int64_t m0 = a0 + ((b0 - a0) >> 1), m1 = a1 + ((b1 - a1) >> 1);
        const bool g0 = a0 < b0, g1 = a1 < b1;
        const int64_t k0 = g0 ? keys[m0] : 0, k1 = g1 ? keys[m1] : 0;
        if (g0 && k0 < x0) a0 = m0 + 1;
        else if (g0) b0 = m0;
        if (g1 && k1 < x1) a1 = m1 + 1;
        else if (g1) b1 = m1;
    }
    r0 = a0, r1 = a1;
}

__device__ __forceinline__ void softmax_update(float t, float &m, float &s) {
    if (t > m) {
        s = s * expf(m - t) + 1.0f;
        m = t;
    } else {
        s += expf(t - m);
    }
}

template <int CB>
__device__ __forceinline__ int64_t candidate_id(const void *cand, int64_t at, int c) {
    if (CB == 4) return (int64_t) reinterpret_cast<const int32_t *>(cand)[at];
    if (CB == 8) return reinterpret_cast<const int64_t *>(cand)[at];
    return c;
}

// CB: bytes of a candidate entry (4, 8), or 0 when candidate c of a row is the id c
template <int CB>
__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(BeamArgs a, PrefixPlan p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char beam_lds[];
    uint64_t *red = reinterpret_cast<uint64_t *>(beam_lds);          // [2][BEAM_WAVES]
    uint64_t *win = red + 2 * BEAM_WAVES;                            // [HIDVAE_BEAM_MAX_K]
    int64_t *pkey = reinterpret_cast<int64_t *>(win + HIDVAE_BEAM_MAX_K);  // per parent: key, then the key range [plo, phi) (empty: none)
    int64_t *plo = pkey + HIDVAE_BEAM_MAX_K, *phi = plo + HIDVAE_BEAM_MAX_K;
    float *pmax = reinterpret_cast<float *>(phi + HIDVAE_BEAM_MAX_K), *plse = pmax + HIDVAE_BEAM_MAX_K, *pbase = plse + HIDVAE_BEAM_MAX_K;
    uint32_t *sc = reinterpret_cast<uint32_t *>(beam_lds + BEAM_HEAD_BYTES);  // [n] score keys
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, n = a.k_prev * C;
    uint32_t *vbits = sc + n;                                        // [ceil(n / 32)] validity bits
    const int64_t b = blockIdx.x;
    const float T = a.temperature;

    for (int i = tid; i < (n + 31) / 32; i += BEAM_THREADS) vbits[i] = 0u;
    // one thread per parent: its key range in the index
    if (tid < a.k_prev) {
        const int64_t row = b * a.k_prev + tid;
        int64_t key = 0, lo = 0, hi = a.n_keys;
        if (a.w > 0) {
            if (pack_row<true>(a.generated + row * a.ldg, a.w, p, key)) {
                lower_bound_pair(a.keys, a.n_keys, key * a.span_w, (key + 1) * a.span_w, lo, hi);
            } else {
                hi = 0;
            }
        }
        pkey[tid] = key, plo[tid] = lo, phi[tid] = hi;
        pbase[tid] = a.log_probas ? a.log_probas[row] : 0.0f;
    }
    // one wave per parent row: running max and sum of exp of logits / T
    for (int j = wave; j < a.k_prev; j += BEAM_WAVES) {
        const float *x = a.logits + (b * a.k_prev + j) * a.ld_logits;
        float m = -FLT_MAX, s = 0.0f;
        if (a.vec4) {
            const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x);
            for (int64_t v = lane; v < (a.V >> 2); v += HV_WAVE) {
                const f32x4 q = x4[v];
                softmax_update(q.x / T, m, s);
                softmax_update(q.y / T, m, s);
                softmax_update(q.z / T, m, s);
                softmax_update(q.w / T, m, s);
            }
        } else {
            for (int64_t v = lane; v < a.V; v += HV_WAVE) softmax_update(x[v] / T, m, s);
        }
        const float M = hv_wave_max(m);
        const float lse = logf(hv_wave_sum(s * expf(m - M)));
        if (lane == 0) pmax[j] = M, plse[j] = lse;
    }
    __syncthreads();

    // the candidates, BEAM_UNROLL per thread at a time: their binary searches advance together, so their loads are in flight together
    for (int f0 = tid; f0 < n; f0 += BEAM_THREADS * BEAM_UNROLL) {
        int64_t slo[BEAM_UNROLL], shi[BEAM_UNROLL], start[BEAM_UNROLL];
        float part[BEAM_UNROLL];  // logp: the penalty and the parent's log-probability follow once validity is known
        int par[BEAM_UNROLL];
#pragma unroll
        for (int u = 0; u < BEAM_UNROLL; u++) {
            const int flat = f0 + u * BEAM_THREADS;
            slo[u] = shi[u] = 0;
            start[u] = -1;  // (no search: the id is outside the logits row or the column's range)
            part[u] = -INFINITY;
            par[u] = 0;
            if (flat < n) {
                const int j = flat / C, c = flat - j * C;
                const int64_t row = b * a.k_prev + j;
                const int64_t id = candidate_id<CB>(a.cand, row * a.ldc + c, c);
                const bool in_v = id >= 0 && id < a.V;  // (an id outside the logits row is never an index)
                if (in_v) part[u] = (a.logits[row * a.ld_logits + id] / T - pmax[j]) - plse[j];
                const int64_t d = id - a.lo_w;
                par[u] = j;
                if (in_v && d >= 0 && d < a.radix_w) {
                    start[u] = (pkey[j] * a.radix_w + d) * a.span_next;
                    slo[u] = plo[j], shi[u] = phi[j];
                }
            }
        }
        for (;;) {
            int64_t mid[BEAM_UNROLL], at[BEAM_UNROLL];
            bool go[BEAM_UNROLL], any = false;
#pragma unroll
            for (int u = 0; u < BEAM_UNROLL; u++) {
                go[u] = slo[u] < shi[u];
                mid[u] = slo[u] + ((shi[u] - slo[u]) >> 1);
                at[u] = go[u] ? a.keys[mid[u]] : 0;
                any = any || go[u];
            }
            if (!any) break;
#pragma unroll
            for (int u = 0; u < BEAM_UNROLL; u++) {
                if (go[u] && at[u] < start[u]) slo[u] = mid[u] + 1;
                else if (go[u]) shi[u] = mid[u];
            }
        }
#pragma unroll
        for (int u = 0; u < BEAM_UNROLL; u++) {
            const int flat = f0 + u * BEAM_THREADS;
            if (flat < n) {
                const bool valid = start[u] >= 0 && slo[u] < phi[par[u]] && a.keys[slo[u]] < start[u] + a.span_next;
                const float score = ((valid ? 0.0f : -10000.0f) + part[u]) + pbase[par[u]];
                sc[flat] = order_key(score + 0.0f);
                if (valid) atomicOr(&vbits[flat >> 5], 1u << (flat & 31));
            }
        }
    }
    __syncthreads();

    // k rounds of arg-max over (score key, ~flat index): thread t owns the slots t, t + 1024, ...
    auto scan = [&]() {
        uint64_t best = 0;
        for (int i = tid; i < n; i += BEAM_THREADS) {
            const uint32_t v = sc[i];
            const uint64_t e = ((uint64_t)v << 32) | (uint32_t)~(uint32_t)i;
            best = (v != 0u && e > best) ? e : best;
        }
        return best;
    };
    uint64_t mine = scan();
    for (int r = 0; r < a.k; r++) {
        const uint64_t wv = wave_max_u64(mine);
        uint64_t *slot = red + (r & 1) * BEAM_WAVES;
        if (lane == 0) slot[wave] = wv;
        __syncthreads();
        uint64_t best = slot[0];
#pragma unroll
        for (int i = 1; i < BEAM_WAVES; i++) best = slot[i] > best ? slot[i] : best;
        if (tid == 0) win[r] = best;
        const uint32_t idx = ~(uint32_t)best;
        if (best != 0 && (int)(idx & (BEAM_THREADS - 1)) == tid) {  // (best is 0 only if k > n, which the entry point refuses)
            sc[idx] = 0u;
            mine = scan();
        }
    }
    __syncthreads();

    const int w1 = a.w + 1;
    for (int e = tid; e < a.k * w1; e += BEAM_THREADS) {
        const int r = e / w1, col = e - r * w1;
        const uint64_t best = win[r];
        const int idx = best ? (int)~(uint32_t)best : 0;
        const int j = idx / C, c = idx - j * C;
        const int64_t row = b * a.k_prev + j;
        int64_t v;
        if (col < a.w) v = a.generated[row * a.ldg + col];
        else v = candidate_id<CB>(a.cand, row * a.ldc + c, c);
        a.out_ids[(b * a.k + r) * w1 + col] = v;
        if (col == a.w) {
            a.out_logp[b * a.k + r] = order_value((uint32_t)(best >> 32));
            a.out_parents[b * a.k + r] = j;
            a.out_valid[b * a.k + r] = (uint8_t)((vbits[idx >> 5] >> (idx & 31)) & 1u);
        }
    }
}

template <int CB>
int launch(const BeamArgs &a, const PrefixPlan &p, int64_t B, size_t lds, hipStream_t s) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&beam_step_kernel<CB>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       BEAM_HEAD_BYTES + HIDVAE_BEAM_MAX_CANDIDATES * 4 + HIDVAE_BEAM_MAX_CANDIDATES / 8);
    HV_REQUIRE(attr == hipSuccess, "beam_step: could not size the LDS of beam_step_kernel");
    hipLaunchKernelGGL(beam_step_kernel<CB>, dim3((unsigned)B), dim3(BEAM_THREADS), lds, s, a, p);
    HV_LAUNCH_CHECK("beam_step");
    return HIDVAE_OK;
}

}  // namespace

extern "C" int hidvae_beam_step(const float *logits, int64_t ld_logits, int64_t B, int64_t k_prev, int64_t V, const void *cand, int cand_bytes,
                                int64_t ldc, int64_t C, const int64_t *generated, int64_t ldg, const float *log_probas, int w, int k,
                                float temperature, const int64_t *lo_host, const int64_t *radix_host, int W, const int64_t *keys,
                                int64_t n_keys, int64_t *out_ids, float *out_logp, int64_t *out_parents, uint8_t *out_valid, void *stream) {
    PrefixPlan p;
    int64_t spans[HIDVAE_PREFIX_MAX_W + 1];
    const int rc = read_plan(lo_host, radix_host, W, p, spans);
    if (rc != HIDVAE_OK) return rc;
    HV_REQUIRE(cand_bytes == 0 || cand_bytes == 4 || cand_bytes == 8, "beam_step: candidate entries of %d bytes (int32, int64, or 0: the id is the index)",
               cand_bytes);
    HV_REQUIRE(B >= 0 && B <= INT32_MAX && k_prev >= 1 && V >= 1 && C >= 1 && ld_logits >= V && n_keys >= 0 && (n_keys == 0 || keys),
               "beam_step: bad arguments");
    HV_REQUIRE(cand_bytes != 0 || C == V, "beam_step: without candidates every id is one, C = V (got C %lld, V %lld)", (long long)C, (long long)V);
    HV_REQUIRE(k >= 1 && k <= HIDVAE_BEAM_MAX_K, "beam_step: k = %d beams (1 .. %d)", k, HIDVAE_BEAM_MAX_K);
    HV_REQUIRE(C <= HIDVAE_BEAM_MAX_CANDIDATES && k_prev <= HIDVAE_BEAM_MAX_CANDIDATES / C,
               "beam_step: %lld parents x %lld candidates per batch item, the in-LDS selection holds %d", (long long)k_prev, (long long)C,
               HIDVAE_BEAM_MAX_CANDIDATES);
    HV_REQUIRE(k_prev <= HIDVAE_BEAM_MAX_K, "beam_step: %lld parent beams (the parents are an earlier step's at most %d beams)",
               (long long)k_prev, HIDVAE_BEAM_MAX_K);
    HV_REQUIRE(k <= k_prev * C, "beam_step: k = %d beams out of %lld candidates", k, (long long)(k_prev * C));
    HV_REQUIRE(w >= 0 && w < W, "beam_step: position %d, the next id needs %d > position indexed columns", w, W);
    HV_REQUIRE(temperature > 0.0f, "beam_step: temperature %g (> 0)", (double)temperature);
    HV_REQUIRE(w == 0 || ldg >= w, "beam_step: bad arguments");
    if (B == 0) return HIDVAE_OK;
    HV_REQUIRE(logits && (cand_bytes == 0 || (cand && ldc >= C)) && (w == 0 || generated) && out_ids && out_logp && out_parents && out_valid,
               "beam_step: bad arguments");
    BeamArgs a;
    a.logits = logits, a.ld_logits = ld_logits, a.V = V;
    a.cand = cand, a.ldc = ldc, a.C = (int)C;
    a.generated = generated, a.ldg = ldg, a.log_probas = log_probas;
    a.k_prev = (int)k_prev, a.w = w, a.k = k, a.temperature = temperature;
    a.vec4 = (V % 4 == 0) && (ld_logits % 4 == 0) && ((uintptr_t)logits % 16 == 0);
    a.lo_w = p.lo[w], a.radix_w = p.radix[w], a.span_w = spans[w], a.span_next = spans[w + 1];
    a.keys = keys, a.n_keys = n_keys;
    a.out_ids = out_ids, a.out_logp = out_logp, a.out_parents = out_parents, a.out_valid = out_valid;
    const int64_t n = k_prev * C;
    const size_t lds = (size_t)BEAM_HEAD_BYTES + (size_t)n * 4 + (size_t)((n + 31) / 32) * 4;
    const hipStream_t s = (hipStream_t)stream;
    if (cand_bytes == 0) return launch<0>(a, p, B, lds, s);
    if (cand_bytes == 4) return launch<4>(a, p, B, lds, s);
    return launch<8>(a, p, B, lds, s);
}
