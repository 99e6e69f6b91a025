// Jagged (variable-length) multi-head attention FORWARD for the stage-2 decode loop (reference modules/transformer/attention.py:113-124:
// F.scaled_dot_product_attention on jagged NestedTensors).  fp32 in, fp32 out, fp32 accumulation on v_mfma_f32_32x32x2_f32; online
// softmax over 32-token kv tiles, the score matrix is never materialised; no dropout (the decode and evaluation paths run in eval).
//
// Decomposition.  Query ROW SPACE is cut into tiles of 32 rows; one wave owns (one tile, one head), a workgroup of 4 waves takes 4
// heads of the same tile.  The grid depends on (total_q, H) alone.  A tile may cross any number of segments (a segment = the kv_group
// consecutive query sequences that share one kv sequence, a contiguous row block): the wave finds the first one by a binary search on
// the device offsets and notes, per row, the kv rows that row may see.  The kv sequences of consecutive segments lie back to back, so
// the tile walks the UNION of its segments' kv rows once, 32 at a time, and a per-element mask (the row's own range, cut at the
// diagonal when causal) keeps the segments apart: a masked score is -inf, p = 0, and the row's running max is untouched.
//
// Per kv tile (all fragment maps from the ISA's 32x32x2 f32 form: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31],
// C/D column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)):
//   S^T = K Q^T   A = K, B = Q^T.  The sum over d has no prescribed order, so lane half h takes d = h Dh/2 + step: a lane reads Dh/2
//                 CONTIGUOUS floats of its K row (16-byte loads) and holds the same slice of its q row for the whole tile walk.
//   softmax       lane (q = lane & 31, h) holds 16 scores of ITS q row: the row reduction is 15 in-lane ops + one cross-half shuffle.
//   O^T = V^T P^T A = V^T, B = P^T.  k-step r sums kv rows (crow(r, 0), crow(r, 1)): exactly what register r of the two lane halves
//                 holds, so P feeds the second product with no lane movement and no LDS.  V is read as 128-byte row pieces.
// The result O^T[d][q] has 4 consecutive d per register quad: one 16-byte store each.
//
// Determinism: one wave produces an output row, kv tiles ascending, a fixed order inside a tile; no atomics.
#include "common.h"

namespace {

constexpr int ATT_TILE = 32;        // query rows per wave = kv rows per tile (the MFMA's 32 x 32 result)
constexpr int ATT_WAVES = 4;        // heads per workgroup
constexpr float ATT_LOG2E = 1.44269504088896341f;

__device__ __forceinline__ int att_crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int DH>
__global__ __launch_bounds__(ATT_WAVES * 64) void jagged_attention_kernel(const float *__restrict__ q, int64_t ldq, const float *__restrict__ k,
                                                                          int64_t ldk, const float *__restrict__ v, int64_t ldv,
                                                                          float *__restrict__ out, int64_t ldo, const int64_t *__restrict__ q_offsets,
                                                                          const int64_t *__restrict__ kv_offsets, int64_t nkv, int64_t total_q,
                                                                          int64_t total_kv, int H, int64_t g, int causal, float scale_log2e) {
    constexpr int HALF = DH / 2;   // d values per lane half in the first product
    constexpr int DB = DH / 32;    // 32-wide d blocks of the second product
    const int lane = threadIdx.x & 63, col = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y * ATT_WAVES + (threadIdx.x >> 6);
    if (head >= H) return;  // (whole waves leave; the kernel has no barrier)
    const int64_t r0 = (int64_t)blockIdx.x * ATT_TILE;
    const int64_t r1 = r0 + ATT_TILE < total_q ? r0 + ATT_TILE : total_q;
    const int64_t row = r0 + col;  // this lane's query row
    const int64_t hoff = (int64_t)head * DH;

    // the lane's slice of its q row, kept for the whole walk
    float qf[HALF];
    {
        const bool ok = row < r1;
        const float4 *src = reinterpret_cast<const float4 *>(q + (ok ? row : r0) * ldq + hoff + hh * HALF);
#pragma unroll
        for (int i = 0; i < HALF / 4; i++) {
            float4 t = ok ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            qf[4 * i] = t.x; qf[4 * i + 1] = t.y; qf[4 * i + 2] = t.z; qf[4 * i + 3] = t.w;
        }
    }

    f32x16 o[DB];
#pragma unroll
    for (int b = 0; b < DB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.f;
    float m = -INFINITY, l = 0.f;  // m: the row's running maximum (both lane halves agree); l: THIS lane's share of the running sum
    bool written = false;

    // first segment j with segment end > r0 (segments are row blocks [q_offsets[j g], q_offsets[(j + 1) g]))
    int64_t lo = 0, hi = nkv;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (q_offsets[(mid + 1) * g] > r0) hi = mid; else lo = mid + 1;
    }
    // the tile's segments: every lane notes the kv rows ITS row may see, [vis_lo, vis_hi) in absolute kv rows; the wave notes the union
    // [kmin, kmax) of them.  kv sequences lie back to back, so the union is one row range, walked ONCE for all the tile's segments with a
    // per-element mask: a tile of 32 rows over eight 4-token sequences costs two kv tiles, not eight.
    int vis_lo = 0, vis_hi = 0;
    int64_t kmin = total_kv, kmax = 0;
    for (int64_t j = lo; j < nkv; j++) {
        const int64_t s0 = q_offsets[j * g], s1 = q_offsets[(j + 1) * g];
        if (s0 >= r1) break;
        const int64_t a0 = s0 > r0 ? s0 : r0, a1 = s1 < r1 ? s1 : r1;  // the segment's rows inside this tile
        if (a1 <= a0) continue;
        int64_t k0 = kv_offsets[j], k1 = kv_offsets[j + 1];
        k0 = k0 < 0 ? 0 : (k0 > total_kv ? total_kv : k0);  // (offsets are the caller's; no read leaves the buffers whatever they hold)
        k1 = k1 < k0 ? k0 : (k1 > total_kv ? total_kv : k1);
        // causal (kv_group == 1, the segment IS the sequence): row s0 + i sees kv 0 .. i, the tile's last row of it a1 - s0 - 1
        const int64_t kend = (causal && k0 + (a1 - s0) < k1) ? k0 + (a1 - s0) : k1;
        if (kend > k0) {
            kmin = k0 < kmin ? k0 : kmin;
            kmax = kend > kmax ? kend : kmax;
        }
        if (row >= a0 && row < a1) {
            written = true;
            const int64_t mine_end = (causal && k0 + (row - s0) + 1 < k1) ? k0 + (row - s0) + 1 : k1;
            vis_lo = (int)k0;
            vis_hi = (int)mine_end;
        }
    }
    for (int64_t kb = kmin; kb < kmax; kb += ATT_TILE) {
        // ---- S^T = K Q^T
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] = 0.f;
        {
            const bool ok = kb + col < kmax;
            const float4 *src = reinterpret_cast<const float4 *>(k + (ok ? kb + col : kb) * ldk + hoff + hh * HALF);
#pragma unroll
            for (int i = 0; i < HALF / 4; i++) {
                const float4 t = ok ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(t.x, qf[4 * i], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(t.y, qf[4 * i + 1], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(t.z, qf[4 * i + 2], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(t.w, qf[4 * i + 3], s, 0, 0, 0);
            }
        }
        // ---- online softmax of this lane's q row (scores in log2 units: p = 2^(s - m))
        const int kv0 = (int)kb + 4 * hh;
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kv = kv0 + att_crow(r, 0);
            s[r] = (kv >= vis_lo && kv < vis_hi) ? s[r] * scale_log2e : -INFINITY;
            tmax = fmaxf(tmax, s[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax);
        // mn == -inf: the row has seen no visible score yet (tiles of other segments, or no kv at all): nothing to rescale and every p
        // is 0; no exp of (-inf) - (-inf) is formed
        const bool live = mn > -INFINITY;
        const float alpha = (live && m > -INFINITY) ? __builtin_amdgcn_exp2f(m - mn) : (live ? 0.f : 1.f);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            s[r] = (live && s[r] > -INFINITY) ? __builtin_amdgcn_exp2f(s[r] - mn) : 0.f;
            psum += s[r];
        }
        l = l * alpha + psum;
        m = mn;
#pragma unroll
        for (int b = 0; b < DB; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[b][r] *= alpha;
        // ---- O^T += V^T P^T
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int64_t kv = kb + att_crow(r, hh);
            const bool ok = kv < kmax;
            const float *src = v + (ok ? kv : kb) * ldv + hoff + col;
#pragma unroll
            for (int b = 0; b < DB; b++) {
                const float t = ok ? src[32 * b] : 0.f;
                o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(t, s[r], o[b], 0, 0, 0);
            }
        }
    }

    // ---- normalise and store: an empty kv sequence (l == 0) gives zero rows
    const float lt = l + __shfl_xor(l, 32);
    const float inv = lt > 0.f ? 1.0f / lt : 0.f;
    if (written) {
        float *dst = out + row * ldo + hoff + 4 * hh;
#pragma unroll
        for (int b = 0; b < DB; b++)
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                float4 t;
                t.x = o[b][4 * gq] * inv; t.y = o[b][4 * gq + 1] * inv; t.z = o[b][4 * gq + 2] * inv; t.w = o[b][4 * gq + 3] * inv;
                *reinterpret_cast<float4 *>(dst + 32 * b + 8 * gq) = t;
            }
    }
}

}  // namespace

extern "C" int hidvae_jagged_attention_fwd(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv, float *out,
                                           int64_t ldo, const int64_t *q_offsets, int64_t nq, int64_t total_q, const int64_t *kv_offsets,
                                           int64_t nkv, int64_t total_kv, int num_heads, int head_dim, int kv_group, int causal, float scale,
                                           void *stream) {
    HV_REQUIRE(head_dim == 32 || head_dim == 64 || head_dim == 128, "jagged_attention_fwd: head_dim %d (32, 64 or 128)", head_dim);
    HV_REQUIRE(num_heads >= 1 && kv_group >= 1 && nq >= 1 && nkv >= 1 && total_q >= 0 && total_kv >= 0,
               "jagged_attention_fwd: bad sizes (heads %d, kv_group %d, nq %lld, nkv %lld)", num_heads, kv_group, (long long)nq, (long long)nkv);
    HV_REQUIRE(nq == nkv * kv_group, "jagged_attention_fwd: nq %lld is not nkv %lld x kv_group %d", (long long)nq, (long long)nkv, kv_group);
    HV_REQUIRE(!causal || (kv_group == 1 && nq == nkv), "jagged_attention_fwd: causal needs kv_group == 1 (got %d)", kv_group);
    HV_REQUIRE(total_q < (int64_t(1) << 31) && total_kv < (int64_t(1) << 31) && nq < (int64_t(1) << 31),
               "jagged_attention_fwd: %lld query rows, %lld kv rows (below 2^31 each)", (long long)total_q, (long long)total_kv);
    HV_REQUIRE(q_offsets && kv_offsets, "jagged_attention_fwd: null offsets");
    if (total_q == 0) return HIDVAE_OK;
    const int64_t d = (int64_t)num_heads * head_dim;
    HV_REQUIRE(q && out && (total_kv == 0 || (k && v)), "jagged_attention_fwd: null tensor");
    HV_REQUIRE(ldq >= d && ldk >= d && ldv >= d && ldo >= d && ((ldq | ldk | ldv | ldo) & 3) == 0,
               "jagged_attention_fwd: leading dimensions (%lld, %lld, %lld, %lld) must be >= %lld and multiples of 4", (long long)ldq,
               (long long)ldk, (long long)ldv, (long long)ldo, (long long)d);
    HV_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
               "jagged_attention_fwd: q, k, v and out must be 16-byte aligned");
    const dim3 grid((unsigned)hv_cdiv(total_q, ATT_TILE), (unsigned)hv_cdiv(num_heads, ATT_WAVES)), block(ATT_WAVES * 64);
    HV_REQUIRE(grid.y <= 65535, "jagged_attention_fwd: %d heads", num_heads);
    const float sl = scale * ATT_LOG2E;
    hipStream_t s = (hipStream_t)stream;
#define ATT_LAUNCH(DH)                                                                                                                   \
    hipLaunchKernelGGL((jagged_attention_kernel<DH>), grid, block, 0, s, q, ldq, k, ldk, v, ldv, out, ldo, q_offsets, kv_offsets, nkv, total_q, \
                       total_kv, num_heads, (int64_t)kv_group, causal, sl)
    if (head_dim == 32) ATT_LAUNCH(32);
    else if (head_dim == 64) ATT_LAUNCH(64);
    else ATT_LAUNCH(128);
#undef ATT_LAUNCH
    HV_LAUNCH_CHECK("jagged_attention_fwd");
    return HIDVAE_OK;
}
