// Prefix index of the corpus id cache for constrained decoding (reference modules/tokenizer/h_semids.py:199-239 exists_prefix,
// the stage-2 decoder's inference_verifier_fn, model.py:200-219).  Every cache row's first W columns become one mixed-radix key
// (column j: digit id - lo[j] in [0, radix[j]), first column most significant); the keys are sorted and deduplicated once per cache
// (plumbing, outside the decode loop).  A prefix p of width w then owns the key range [key(p) * S_w, (key(p) + 1) * S_w) with
// S_w = prod_{i >= w} radix[i]: it exists iff a key lies in that range (one lower_bound), and digit d may follow it iff a key lies in
// [(key(p) * radix[w] + d) * S_{w+1}, ... + S_{w+1}).  So one index answers every width, and every call is one launch.  The plan and the
// search helpers live in prefix.h (beam.hip reads the same index).
#include "prefix.h"

namespace {

__global__ __launch_bounds__(256) void prefix_pack_kernel(const int64_t *ids, int64_t n, int64_t ld, int W, PrefixPlan p, int64_t *keys) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int64_t key;
    const bool ok = pack_row<false>(ids + r * ld, W, p, key);
    keys[r] = ok ? key : -1;  // (a row outside the plan can match no query: query keys are >= 0)
}

// one thread per query row: rows at or past n_covered are written False without being read
template <typename T>
__global__ __launch_bounds__(256) void prefix_exists_kernel(const T *q, int64_t n_q, int64_t ldq, int w, PrefixPlan p, int64_t span,
                                                            const int64_t *keys, int64_t n_keys, int64_t n_covered, uint8_t *out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_q) return;
    uint8_t hit = 0;
    if (r < n_covered) {
        int64_t key;
        if (pack_row<true>(q + r * ldq, w, p, key)) {
            const int64_t i = lower_bound(keys, 0, n_keys, key * span);
            hit = i < n_keys && keys[i] < (key + 1) * span;
        }
    }
    out[r] = hit;
}

// one wave per query row: the prefix's key range [a, b) once, then one lane per candidate next id v (digit v - lo_w) searches it
template <typename T>
__global__ __launch_bounds__(256) void prefix_next_kernel(const T *q, int64_t n_q, int64_t ldq, int w, PrefixPlan p, int64_t lo_w,
                                                          int64_t radix_w, int64_t span_w, int64_t span_next, const int64_t *keys,
                                                          int64_t n_keys, int64_t V, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_q) return;
    int64_t key = 0, a = 0, b = n_keys;
    bool ok = true;
    if (w > 0) {
        ok = pack_row<true>(q + r * ldq, w, p, key);
        if (ok) {
            a = lower_bound(keys, 0, n_keys, key * span_w);
            b = lower_bound(keys, a, n_keys, (key + 1) * span_w);
        }
    }
    ok = ok && a < b;
    uint8_t *o = out + r * V;
    for (int64_t v = lane; v < V; v += HV_WAVE) {
        uint8_t hit = 0;
        const int64_t d = v - lo_w;
        if (ok && d >= 0 && d < radix_w) {
            const int64_t start = (key * radix_w + d) * span_next;
            const int64_t i = lower_bound(keys, a, b, start);
            hit = i < b && keys[i] < start + span_next;
        }
        o[v] = hit;
    }
}

}  // namespace

extern "C" int hidvae_prefix_pack(const int64_t *ids, int64_t n, int64_t ld, int W, const int64_t *lo_host, const int64_t *radix_host,
                                  int64_t *keys, void *stream) {
    PrefixPlan p;
    int64_t spans[HIDVAE_PREFIX_MAX_W + 1];
    const int rc = read_plan(lo_host, radix_host, W, p, spans);
    if (rc != HIDVAE_OK) return rc;
    HV_REQUIRE(n >= 0 && ld >= W && (n == 0 || (ids && keys)), "prefix_pack: bad arguments");
    if (n == 0) return HIDVAE_OK;
    hipLaunchKernelGGL(prefix_pack_kernel, dim3((unsigned)hv_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, ids, n, ld, W, p, keys);
    HV_LAUNCH_CHECK("prefix_pack");
    return HIDVAE_OK;
}

extern "C" int hidvae_prefix_exists(const void *q, int q_bytes, int64_t n_q, int64_t ldq, int w, const int64_t *lo_host,
                                    const int64_t *radix_host, int W, const int64_t *keys, int64_t n_keys, int64_t n_covered, uint8_t *out,
                                    void *stream) {
    PrefixPlan p;
    int64_t spans[HIDVAE_PREFIX_MAX_W + 1];
    const int rc = read_plan(lo_host, radix_host, W, p, spans);
    if (rc != HIDVAE_OK) return rc;
    HV_REQUIRE(q_bytes == 4 || q_bytes == 8, "prefix_exists: query entries of %d bytes (int32 or int64)", q_bytes);
    HV_REQUIRE(w >= 1 && w <= W, "prefix_exists: width %d of %d indexed columns", w, W);
    HV_REQUIRE(n_q >= 0 && ldq >= w && n_keys >= 0 && (n_q == 0 || (q && out)) && (n_keys == 0 || keys), "prefix_exists: bad arguments");
    if (n_q == 0) return HIDVAE_OK;
    const dim3 grid((unsigned)hv_cdiv(n_q, 256));
    const hipStream_t s = (hipStream_t)stream;
    if (q_bytes == 8)
        hipLaunchKernelGGL(prefix_exists_kernel<int64_t>, grid, dim3(256), 0, s, (const int64_t *)q, n_q, ldq, w, p, spans[w], keys, n_keys,
                           n_covered, out);
    else
        hipLaunchKernelGGL(prefix_exists_kernel<int32_t>, grid, dim3(256), 0, s, (const int32_t *)q, n_q, ldq, w, p, spans[w], keys, n_keys,
                           n_covered, out);
    HV_LAUNCH_CHECK("prefix_exists");
    return HIDVAE_OK;
}

extern "C" int hidvae_prefix_next(const void *q, int q_bytes, int64_t n_q, int64_t ldq, int w, const int64_t *lo_host, const int64_t *radix_host,
                                  int W, const int64_t *keys, int64_t n_keys, int64_t V, uint8_t *out, void *stream) {
    PrefixPlan p;
    int64_t spans[HIDVAE_PREFIX_MAX_W + 1];
    const int rc = read_plan(lo_host, radix_host, W, p, spans);
    if (rc != HIDVAE_OK) return rc;
    HV_REQUIRE(q_bytes == 4 || q_bytes == 8, "prefix_next: query entries of %d bytes (int32 or int64)", q_bytes);
    HV_REQUIRE(w >= 0 && w < W, "prefix_next: width %d, the next id needs %d > width indexed columns", w, W);
    HV_REQUIRE(n_q >= 0 && V >= 0 && ldq >= w && n_keys >= 0 && (w == 0 || n_q == 0 || q) && (n_q == 0 || V == 0 || out) &&
                   (n_keys == 0 || keys), "prefix_next: bad arguments");
    if (n_q == 0 || V == 0) return HIDVAE_OK;
    const dim3 grid((unsigned)hv_cdiv(n_q, 4));
    const hipStream_t s = (hipStream_t)stream;
    if (q_bytes == 8)
        hipLaunchKernelGGL(prefix_next_kernel<int64_t>, grid, dim3(256), 0, s, (const int64_t *)q, n_q, ldq, w, p, p.lo[w], p.radix[w],
                           spans[w], spans[w + 1], keys, n_keys, V, out);
    else
        hipLaunchKernelGGL(prefix_next_kernel<int32_t>, grid, dim3(256), 0, s, (const int32_t *)q, n_q, ldq, w, p, p.lo[w], p.radix[w],
                           spans[w], spans[w + 1], keys, n_keys, V, out);
    HV_LAUNCH_CHECK("prefix_next");
    return HIDVAE_OK;
}
