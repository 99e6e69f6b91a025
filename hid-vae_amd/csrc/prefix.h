// The mixed-radix key plan of a prefix index and the device helpers that read it, shared by the index's own kernels (prefix.hip) and the
// constrained beam-search step (beam.hip).  A cache row's first W columns are one key (column j: digit id - lo[j] in [0, radix[j]), first
// column most significant); a prefix of width w owns the key range [key(p) * S_w, (key(p) + 1) * S_w), S_w = prod_{i >= w} radix[i].
#pragma once
#include "common.h"

struct PrefixPlan {
    int64_t lo[HIDVAE_PREFIX_MAX_W];
    int64_t radix[HIDVAE_PREFIX_MAX_W];
};

// key of the first w columns of `row`; false when an entry lies outside its column's [lo, lo + radix) (QUERY: or is negative)
template <bool QUERY, typename T>
__device__ __forceinline__ bool pack_row(const T *row, int w, const PrefixPlan &p, int64_t &key) {
    int64_t k = 0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < HIDVAE_PREFIX_MAX_W; j++) {
        if (j >= w) break;  // (w is uniform: the unrolled loop keeps the plan in scalar registers)
        const int64_t v = (int64_t)row[j];
        const int64_t d = v - p.lo[j];
        ok = ok && d >= 0 && d < p.radix[j] && (!QUERY || v >= 0);
        k = k * p.radix[j] + (ok ? d : 0);
    }
    key = k;
    return ok;
}

// first index in [a, b) whose key is >= x (b when none)
__device__ __forceinline__ int64_t lower_bound(const int64_t *keys, int64_t a, int64_t b, int64_t x) {
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (keys[mid] < x) a = mid + 1;
        else b = mid;
    }
    return a;
}

// validates the host plan of the first W columns; spans[w] = prod_{w <= i < W} radix[i] (< 2^62 by construction)
static inline int read_plan(const int64_t *lo_host, const int64_t *radix_host, int W, PrefixPlan &p, int64_t *spans) {
    HV_REQUIRE(lo_host && radix_host && W >= 1 && W <= HIDVAE_PREFIX_MAX_W, "prefix: %d indexed columns (1 .. %d)", W, HIDVAE_PREFIX_MAX_W);
    p = PrefixPlan{};
    int64_t prod = 1;
    for (int j = W - 1; j >= 0; j--) {
        HV_REQUIRE(radix_host[j] >= 1 && lo_host[j] <= 0, "prefix: column %d has radix %lld, offset %lld (radix >= 1, offset <= 0)", j,
                   (long long)radix_host[j], (long long)lo_host[j]);
        HV_REQUIRE(prod <= (HIDVAE_PREFIX_KEY_LIMIT - 1) / radix_host[j], "prefix: the radix product of %d columns reaches 2^62", W);
        spans[j + 1] = prod;
        prod *= radix_host[j];
        p.lo[j] = lo_host[j];
        p.radix[j] = radix_host[j];
    }
    spans[0] = prod;
    return HIDVAE_OK;
}
