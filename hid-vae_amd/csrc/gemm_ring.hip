// Linear backward (dW = g^T x, dX = epi(g W), db = colsum(g)) on an LDS-DMA ring: every layer of the tag heads and of the encoder /
// decoder (reference modules/h_rqvae.py:132-188,322-331; modules/encoder.py:23-36) from 0.2 GFLOP on (rules.h), at every batch size.
//
// What differs from gemm_mid_sk_kernel (gemm.hip), which stages every operand global -> VGPR -> ds_write, runs sixteen (eight) waves per
// 64x64 tile in four (two) k-groups whose partial tiles meet in LDS at every segment end, and restarts its pipeline at every segment:
//   * a workgroup is FOUR waves, one 32x32 quarter of a 64x64 tile each and the whole K range of its segment: one accumulator chain
//     per wave, no k-groups, nothing to add up in LDS;
//   * operands go global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no VGPR, no ds_write, one instruction per KiB), into a ring
//     of RB_NS stages of 32 k; the loads of step s + 3 are issued right after the barrier of step s and run through segment and tile
//     boundaries -- the ring never drains inside a workgroup's range except where a partial tile is handed over; counted
//     s_waitcnt vmcnt(N), one raw s_barrier per step;
//   * the work is gemm_mid_sk_kernel's list of k-steps cut into equal contiguous ranges (every SIMD the same number of MFMAs whatever
//     the tile count; partial tiles through the workspace, the last arriver adds them in ascending k order: deterministic), over a
//     tile list ordered in square-ish bands;
//   * the loader state (buffer descriptors, per-lane offsets, the cursor) lives in registers and is rebuilt only at a tile change:
//     indexing the argument struct by a run-time product index turns every field into a scalar load from the argument segment, eight
//     dependent ones per step (the first build: 1.7 us per step of nothing but that).
// Measured (scratch/r4): alone, 10-25 % faster than gemm_mid_sk_kernel on most shapes from B = 1024 up (1024 x 691 x 768:
// 31.6 vs 37.5 us; 2048 x 768 x 691: 55.6 vs 64.0 us = 0.50 of the fp32 MFMA peak; 4096 x 768 x 512: 71.8 vs 80.6 = 0.57; 8192 x 512 x 256:
// 51.9 vs 60.8; slower on 1024 x 768 x 512: 27.4 vs 22.9).  Inside the step it first replaced gemm_mid_sk_kernel from B = 2048 (tagged step
// 2.008 -> 1.881 ms, the B = 8192 shard 0.870 -> 0.830 ms) and tied at B = 1024; what moved the B = 1024 step was giving it the layers
// of 0.2-0.9 GFLOP that the per-wave pair kernels had (those run 1.5-2x slower in the three-lane step than alone): 1.156 -> 1.088 ms
// (profiles/r04_ring_threshold_ab.log).  Variants that were built, tested and NOT kept (sources: scratch/r4/gemm_ring_v3c.hip.txt): a
// chunk-major step list (L2 hits 39 % -> 81 %, fabric traffic 114 -> 27 MB per launch) with pieces parked in slabs and a second,
// combining launch -- slower in the step for the second launch's gap; two dedicated loader waves beside four MFMA waves -- no change:
// what does not overlap is not the DMA instructions' issue (ablation: MFMAs + LDS reads alone 17.4 us above the launch's fixed 8 us =
// the matrix pipe's floor at the ~2.0 GHz the chip holds; DMAs alone 9.7 us; together 23.6).
// LDS images (a stage = 16 KB = operand A, then operand B):
//   k-major operand (g and x of dW; W of dX), element (k, c) at P[k * ld + c]:   [32 k][64 c] floats, filled by 8 pieces of 4 k-rows;
//       the MFMA fragment of k-pair j is the dword at row 2j + h: 32 consecutive dwords per half-wave, conflict-free ds_read_b32;
//   k-contiguous operand (g of dX), element (m, k) at P[m * ld + k]:             [64 m][32 k], 128-byte rows, filled by 8 pieces of
//       8 rows; the 16-byte chunk c of row m sits at position c ^ ((m >> 1) & 7) -- the permutation is applied to the SOURCE address
//       of the DMA (its LDS side is lane-linear) and again on the read: conflict-free ds_read_b128.
// Edges: k rows past K are aimed out of the buffer (LDS-DMA writes zeros for them: scratch/r4/probe.hip); a 16-byte chunk of a
// k-contiguous row that straddles K brings in finite neighbours which meet those zeros; rows / columns past M / N only reach
// accumulator rows / columns that are never stored; the hardware's range check is per dword (same probe).  16-byte DMA needs dword
// alignment only, so 691-wide rows are fine.
// Not the ORDER-G16 chain: gradients only (their tests compare against float64 and demand launch-to-launch bit identity).
//
// bf16-operand forms (the amp mode): the same ring, the same fp32 LDS images, tile order and hand-over; only the read of a
// step differs.  Each lane takes the sixteen fp32 values per operand the fp32 form reads, rounds them to bf16 (v_cvt_pk_bf16_f32:
// round to nearest even, as torch's .bfloat16()) and feeds two v_mfma_f32_32x32x16_bf16 instead of sixteen v_mfma_f32_32x32x2_f32.
// Inside a 32x32x16 fragment lane l holds k = 8 (l >> 5) + j of its row / column in element j; any permutation of the sixteen k of a
// fragment is the same product as long as both operands use it, so element j of half h is the k the fp32 form reads at that position
// (k-major image: k = 2j + h of the fragment's 16; k-contiguous image: k = 8t + 4h + e with j = 4 (t & 1) + e).  The C/D layout is the
// fp32 one.  A step that reaches past K zeroes the operand values at k >= K at the read: a k-contiguous chunk straddling K brings in
// whatever follows the row (the next row, or a strided view's padding), and in the NT form both operands have such chunks.
//   gemm_ring_bwd_bf16_kernel  dW = g^T x, dX = epi(g W), db, every shape hidvae_linear_bwd takes (hidvae_linear_bwd_bf16);
//   gemm_ring_fwd_bf16_kernel  y = epi(x W^T + b) [* dropout]: the forward NT product with the epilogues of hidvae_gemm_f32, both
//                              operands k-contiguous in the swizzled [64][32] image (hidvae_gemm_bf16).
#include "common.h"
#include "rules.h"
#include "gemm_ring.h"

namespace {

constexpr int RB_BK = 32;            // k per step
constexpr int RB_NS = 4;             // ring stages
constexpr int RB_D = 3;              // steps the loads run ahead
constexpr int RB_STAGE = 4096;       // floats per stage: A image (2048) then B image (2048)
constexpr int RB_LDS_FLOATS = RB_NS * RB_STAGE + 64;  // + the flag word and the column sums' partials
constexpr int RB_OOB = 0x7FFFFFF0;   // a byte offset no buffer reaches
#define RB_LDSP(p) ((__attribute__((address_space(3))) void *)(p))

struct RingProb {
    const float *A, *B;
    float *C;
    const float *aux;
    int lda, ldb, ldc, ldaux;
    int M, N, K;
    int nbx, nby, ntiles, nsteps, bh;  // 64x64 tiles, steps of RB_BK per tile, band height of the tile order
    int epilogue, accumulate;
    float scale;
    unsigned a_bytes, b_bytes;
};

struct RingArgs {
    RingProb p[2];  // p[0]: TN (dW = g^T x), p[1]: NN (dX = g W; ntiles == 0: absent)
    const float *cs_x;
    float *cs_out;
    int cs_ld, cs_rows, cs_cols, cs_accumulate;
    int nbc, cu;    // column-sum units (32 columns each) and their price in steps
    int S, q, G;    // total steps, steps per workgroup, workgroups
    float *slabs;   // [G][2][4096] partial tiles (accumulator layout)
    int *counters;  // [ntiles0 + ntiles1], zero between launches
};

// what the forward form (p[0] = NT, p[1] absent) adds: bias, dropout (a keep-mask tensor or the in-kernel decision), accumulate into C
struct RingFwd {
    const float *bias;
    const float *mask;
    int ldmask;
    float mask_scale;
    HvDrop drop;  // element index row * N + col, as hidvae_gemm_f32
    int row_base; // the first row of this launch in the caller's matrix (a launch takes at most HV_SK_COUNTERS tiles)
};

typedef __bf16 hv_bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

// eight fp32 operand values -> one bf16 fragment (v_cvt_pk_bf16_f32, round to nearest even)
__device__ __forceinline__ hv_bf16x8 ring_bf16(f32x8 v) { return __builtin_convertvector(v, hv_bf16x8); }

// tile t of the band order -> (by, bx): bands of `bh` tile rows, column-major inside a band
__device__ __forceinline__ void ring_tile_xy(const RingProb &P, int t, int &by, int &bx) {
    const int band_sz = P.bh * P.nbx;
    const int band = t / band_sz, r = t - band * band_sz;
    int hb = P.nby - band * P.bh;
    hb = hb < P.bh ? hb : P.bh;
    bx = r / hb;
    by = band * P.bh + (r - bx * hb);
}

struct Cursor {  // a position in the workgroup's list of k-steps (all wave-uniform)
    int prob, tile, ks;
};

__device__ __forceinline__ Cursor ring_locate(const RingArgs &a, int step) {
    Cursor c;
    const int S0 = a.p[0].ntiles * a.p[0].nsteps;
    c.prob = step >= S0 ? 1 : 0;
    const int rel = step - (c.prob ? S0 : 0), nT = a.p[c.prob].nsteps;
    c.tile = rel / nT;
    c.ks = rel - c.tile * nT;
    return c;
}
// The loader: where the DMA stream stands (it runs RB_D steps ahead of the MFMAs, through segment and tile boundaries), with everything a
// step needs held in registers -- the kernel arguments are read again only when the stream moves to another tile (indexing a.p[prob] at
// run time makes every field a scalar load from the argument segment: eight dependent ones per step cost more than the step's MFMAs)
struct Loader {
    int prob, tile, ks;       // cursor (wave-uniform)
    int nsteps, ntiles, K;    // of the cursor's problem
    int stepA, stepB;         // bytes per step
    __amdgpu_buffer_rsrc_t ra, rb;
    int voffA[2], voffB[2];   // per lane: byte offsets of this wave's two pieces per operand at k0 = 0 (RB_OOB: a row outside the matrix)
    int kA[2], kB[2];         // per lane: the piece's first k relative to the step (for the K edge)
};

template <bool FWD>
__device__ __forceinline__ void loader_tile(const RingArgs &a, Loader &L, int wave, int lane) {
    const RingProb &P = a.p[L.prob];
    const bool NN = FWD || L.prob != 0;  // operand A k-contiguous (NN of the backward, NT of the forward)
    L.nsteps = P.nsteps; L.ntiles = P.ntiles; L.K = P.K;
    L.ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.A), 0, (int)P.a_bytes, 0x00020000);
    L.rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.B), 0, (int)P.b_bytes, 0x00020000);
    int by, bx;
    ring_tile_xy(P, L.tile, by, bx);
    const int m0 = 64 * by, n0 = 64 * bx, lda = P.lda, ldb = P.ldb, M = P.M;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int p = wave + 4 * i;
        const int kr = 4 * p + (lane >> 4), c4 = 4 * (lane & 15);  // k-major image: row kr of the step, columns c4 .. c4 + 3
        const int row = 8 * p + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);  // k-contiguous image: row, source chunk
        if (FWD) {  // NT: operand B (W [N, K]) k-contiguous too
            L.kB[i] = 4 * c;
            L.voffB[i] = n0 + row < P.N ? 4 * ((n0 + row) * ldb + 4 * c) : RB_OOB;
        } else {
            L.kB[i] = kr;
            L.voffB[i] = 4 * (kr * ldb + n0 + c4);
        }
        L.kA[i] = NN ? 4 * c : kr;
        L.voffA[i] = NN ? (m0 + row < M ? 4 * ((m0 + row) * lda + 4 * c) : RB_OOB) : 4 * (kr * lda + m0 + c4);
    }
    L.stepA = NN ? 4 * RB_BK : 4 * RB_BK * lda;
    L.stepB = FWD ? 4 * RB_BK : 4 * RB_BK * ldb;
}

// the wave's four DMA instructions of the loader's step into ring buffer `buf`, then the cursor moves on
template <bool FWD>
__device__ __forceinline__ void loader_issue(const RingArgs &a, Loader &L, int wave, int lane, float *lds, int buf) {
    float *dst = lds + buf * RB_STAGE;
    const int k0 = L.ks * RB_BK;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int p = wave + 4 * i;
        // (the whole byte offset rides in the VECTOR offset: the hardware's per-dword range check covers voffset, not soffset, so
        //  anything past the end of the matrix -- the overhang of its last rows' last chunks -- reads as zero instead of leaving the buffer)
        const int va = (k0 + L.kA[i] < L.K && L.voffA[i] != RB_OOB) ? L.voffA[i] + L.ks * L.stepA : RB_OOB;
        const int vb = (k0 + L.kB[i] < L.K && (!FWD || L.voffB[i] != RB_OOB)) ? L.voffB[i] + L.ks * L.stepB : RB_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(L.ra, RB_LDSP(dst + 256 * p), 16, va, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(L.rb, RB_LDSP(dst + 2048 + 256 * p), 16, vb, 0, 0, 0);
    }
    if (++L.ks == L.nsteps) {
        L.ks = 0;
        if (++L.tile == L.ntiles) {
            L.tile = 0;
            L.prob++;
        }
        if (L.prob < (FWD ? 1 : 2)) loader_tile<FWD>(a, L, wave, lane);  // (past the last problem the stream has ended: nothing is issued any more)
    }
}

// one step's sixteen MFMAs of the wave's quarter from ring buffer `buf`
template <bool NN>
__device__ __forceinline__ void ring_mfma(const float *lds, int buf, int wm, int wn, int i32, int h, f32x16 &acc) {
    const float *As = lds + buf * RB_STAGE, *Bs = As + 2048;
    if (NN) {
        const int m = 32 * wm + i32, f = (m >> 1) & 7;
        f32x4 x[4];
#pragma unroll
        for (int t = 0; t < 4; t++) x[t] = *reinterpret_cast<const f32x4 *>(As + m * 32 + 4 * ((2 * t + h) ^ f));
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float b = Bs[(8 * t + 4 * h + e) * 64 + 32 * wn + i32];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[t][e], b, acc, 0, 0, 0);
            }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const float a = As[(2 * j + h) * 64 + 32 * wm + i32];
            const float b = Bs[(2 * j + h) * 64 + 32 * wn + i32];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
}

// the bf16 form of a step: the same LDS reads, two v_mfma_f32_32x32x16_bf16.  LAY: 0 = TN (both operands k-major), 1 = NN (A
// k-contiguous, B k-major), 2 = NT (both k-contiguous).  kv = K - (the step's first k): values at k >= kv are zeroed (only a step
// that reaches past K, wave-uniform).  In the k-major image rows past K are zeros already (the DMA was aimed out of the buffer).
template <int LAY>
__device__ __forceinline__ void ring_mfma_bf16(const float *lds, int buf, int wm, int wn, int i32, int h, int kv, f32x16 &acc) {
    const float *As = lds + buf * RB_STAGE, *Bs = As + 2048;
    f32x8 a[2], b[2];
    if (LAY == 0) {
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                a[s][j] = As[(16 * s + 2 * j + h) * 64 + 32 * wm + i32];
                b[s][j] = Bs[(16 * s + 2 * j + h) * 64 + 32 * wn + i32];
            }
    } else {
        const int m = 32 * wm + i32, f = (m >> 1) & 7;
        f32x4 x[4];
#pragma unroll
        for (int t = 0; t < 4; t++) x[t] = *reinterpret_cast<const f32x4 *>(As + m * 32 + 4 * ((2 * t + h) ^ f));
        if (LAY == 2) {
            const int n = 32 * wn + i32, fn = (n >> 1) & 7;
            f32x4 y[4];
#pragma unroll
            for (int t = 0; t < 4; t++) y[t] = *reinterpret_cast<const f32x4 *>(Bs + n * 32 + 4 * ((2 * t + h) ^ fn));
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int e = 0; e < 4; e++) b[t >> 1][4 * (t & 1) + e] = y[t][e];
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int e = 0; e < 4; e++) b[t >> 1][4 * (t & 1) + e] = Bs[(8 * t + 4 * h + e) * 64 + 32 * wn + i32];
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int e = 0; e < 4; e++) a[t >> 1][4 * (t & 1) + e] = x[t][e];
        if (kv < RB_BK) {  // k = 8t + 4h + e at or past K: the tail of a straddling chunk
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (8 * t + 4 * h + e >= kv) {
                        a[t >> 1][4 * (t & 1) + e] = 0.0f;
                        if (LAY == 2) b[t >> 1][4 * (t & 1) + e] = 0.0f;
                    }
        }
    }
#pragma unroll
    for (int s = 0; s < 2; s++) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring_bf16(a[s]), ring_bf16(b[s]), acc, 0, 0, 0);
}

// write-through stores / cache-bypassing loads for the partial tiles (the hand-over of gemm_mid_sk_kernel: gemm.hip, sk_store_through)
__device__ __forceinline__ void ring_store_through(float *p, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ f32x4 ring_load_through(const float *p) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// epilogue + store of the wave's quarter.  C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// Every load and store is a buffer operation whose lanes outside the matrix are aimed out of range (loads give 0, stores are dropped):
// sixteen back-to-back loads per input and sixteen stores, no branch per element (a per-element "load or not" makes the compiler wait
// for every element's round trip on its own).
template <int EPI>
__device__ __forceinline__ void ring_output_epi(const RingProb &P, int m0, int n0, int wm, int wn, int i32, int h, const f32x16 &acc) {
    const int col = n0 + 32 * wn + i32, row0 = m0 + 32 * wm + 4 * h;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(P.C, 0, (int)(4 * ((int64_t)(P.M - 1) * P.ldc + P.N)), 0x00020000);
    int offc[16];
    float ax[16], old[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        offc[r] = (row < P.M && col < P.N) ? 4 * (row * P.ldc + col) : RB_OOB;
    }
    if (EPI != HIDVAE_EPI_NONE) {
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P.aux), 0,
                                                                            (int)(4 * ((int64_t)(P.M - 1) * P.ldaux + P.N)), 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = row0 + (r & 3) + 8 * (r >> 2);
            ax[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (row < P.M && col < P.N) ? 4 * (row * P.ldaux + col) : RB_OOB, 0, 0));
        }
    }
    if (P.accumulate) {
#pragma unroll
        for (int r = 0; r < 16; r++) old[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, offc[r], 0, 0));
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
        float v = EPI == HIDVAE_EPI_NONE ? acc[r] : hv_apply_epilogue(EPI, acc[r], &ax[r], 0, P.scale);
        if (P.accumulate) v = old[r] + v;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rc, offc[r], 0, 0);
    }
}
__device__ __forceinline__ void ring_output(const RingProb &P, int m0, int n0, int wm, int wn, int i32, int h, const f32x16 &acc) {
    switch (P.epilogue) {  // (uniform)
        case HIDVAE_EPI_DSILU: ring_output_epi<HIDVAE_EPI_DSILU>(P, m0, n0, wm, wn, i32, h, acc); break;
        case HIDVAE_EPI_DRELU: ring_output_epi<HIDVAE_EPI_DRELU>(P, m0, n0, wm, wn, i32, h, acc); break;
        case HIDVAE_EPI_DGELU: ring_output_epi<HIDVAE_EPI_DGELU>(P, m0, n0, wm, wn, i32, h, acc); break;
        case HIDVAE_EPI_DSIGMOID: ring_output_epi<HIDVAE_EPI_DSIGMOID>(P, m0, n0, wm, wn, i32, h, acc); break;
        default: ring_output_epi<HIDVAE_EPI_NONE>(P, m0, n0, wm, wn, i32, h, acc); break;
    }
}

// the forward form's epilogue, element for element what hidvae_gemm_f32 applies: v = acc + bias; the pre-activation into aux (SiLU,
// GELU, ...: any forward code but NONE, when aux is given); the activation; dropout (keep-mask * scale, or the in-kernel decision at
// element index row * N + col); accumulate.
template <int EPI>
__device__ __forceinline__ void ring_output_fwd_epi(const RingProb &P, const RingFwd &F, int m0, int n0, int wm, int wn, int i32, int h,
                                                    const f32x16 &acc) {
    const int col = n0 + 32 * wn + i32, row0 = m0 + 32 * wm + 4 * h;
    if (col >= P.N) return;
    const float bias = F.bias != nullptr ? F.bias[col] : 0.0f;
    const bool drop = F.mask != nullptr || F.drop.state != nullptr;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        if (row >= P.M) continue;
        float v = acc[r] + bias;
        if (EPI != HIDVAE_EPI_NONE && P.aux != nullptr) const_cast<float *>(P.aux)[(int64_t)row * P.ldaux + col] = v;
        v = hv_apply_epilogue(EPI, v, nullptr, 0, 1.0f);
        if (drop)
            v = v * (F.mask != nullptr ? F.mask[(int64_t)row * F.ldmask + col] * F.mask_scale
                                       : (hv_drop_keep(F.drop, (unsigned long long)((int64_t)(F.row_base + row) * P.N + col)) ? F.mask_scale : 0.0f));
        float *dst = P.C + (int64_t)row * P.ldc + col;
        *dst = P.accumulate ? *dst + v : v;
    }
}
__device__ __forceinline__ void ring_output_fwd(const RingProb &P, const RingFwd &F, int m0, int n0, int wm, int wn, int i32, int h,
                                                const f32x16 &acc) {
    switch (P.epilogue) {  // (uniform)
        case HIDVAE_EPI_SILU: ring_output_fwd_epi<HIDVAE_EPI_SILU>(P, F, m0, n0, wm, wn, i32, h, acc); break;
        case HIDVAE_EPI_RELU: ring_output_fwd_epi<HIDVAE_EPI_RELU>(P, F, m0, n0, wm, wn, i32, h, acc); break;
        case HIDVAE_EPI_GELU: ring_output_fwd_epi<HIDVAE_EPI_GELU>(P, F, m0, n0, wm, wn, i32, h, acc); break;
        case HIDVAE_EPI_SIGMOID: ring_output_fwd_epi<HIDVAE_EPI_SIGMOID>(P, F, m0, n0, wm, wn, i32, h, acc); break;
        default: ring_output_fwd_epi<HIDVAE_EPI_NONE>(P, F, m0, n0, wm, wn, i32, h, acc); break;
    }
}

// one finished 64x64 tile (or, in the hand-over, the sum of its pieces) out through the form's epilogue
template <bool FWD>
__device__ __forceinline__ void ring_finish(const RingProb &P, const RingFwd *F, int m0, int n0, int wm, int wn, int i32, int h,
                                            const f32x16 &acc) {
    if (FWD) ring_output_fwd(P, *F, m0, n0, wm, wn, i32, h, acc);
    else ring_output(P, m0, n0, wm, wn, i32, h, acc);
}

// end of a segment: steps [ks0, ks0 + len) of tile `tile` (global steps from tstart, nT of them) are in `acc`
template <bool FWD>
__device__ __forceinline__ void ring_flush(const RingArgs &a, const RingFwd *F, const RingProb &P, int tile, int counter, int ks0, int len,
                                           int tstart, int v, int wave, int lane, f32x16 &acc, int *flag) {
    const int wm = wave >> 1, wn = wave & 1, i32 = lane & 31, h = lane >> 5;
    int by, bx;
    ring_tile_xy(P, tile, by, bx);
    const int m0 = 64 * by, n0 = 64 * bx, nT = P.nsteps;
    if (ks0 == 0 && len == nT) {  // the whole tile
        ring_finish<FWD>(P, F, m0, n0, wm, wn, i32, h, acc);
        return;
    }
    // a piece of the tile: park it (slot 2v: the tile began before this range; 2v + 1: it begins here and goes on), count arrivals
    float *mine = a.slabs + ((int64_t)2 * v + (ks0 == 0 ? 1 : 0)) * 4096 + (wave * 4 * 64 + lane) * 4;
#pragma unroll
    for (int gi = 0; gi < 4; gi++) {
        f32x4 w = {acc[4 * gi], acc[4 * gi + 1], acc[4 * gi + 2], acc[4 * gi + 3]};
        ring_store_through(mine + gi * 256, w);
    }
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");  // this thread's piece has been acknowledged by memory (and every DMA has landed)
    __syncthreads();                                     // ... and so has every thread's
    const int v_first = tstart / a.q, v_last = (tstart + nT - 1) / a.q;
    if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(a.counters + counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const bool last = *flag == v_last - v_first;
    if (last) {  // last to arrive: every piece is in memory; ascending k, whoever finishes
        f32x16 sum;
        for (int u = v_first; u <= v_last; u++) {
            const float *src = a.slabs + ((int64_t)2 * u + (u * a.q <= tstart ? 1 : 0)) * 4096 + (wave * 4 * 64 + lane) * 4;
            f32x4 w[4];
#pragma unroll
            for (int gi = 0; gi < 4; gi++) w[gi] = ring_load_through(src + gi * 256);
#pragma unroll
            for (int gi = 0; gi < 4; gi++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(w[gi]) : : "memory");  // (ties the uses of w to the wait)
#pragma unroll
            for (int gi = 0; gi < 4; gi++)
#pragma unroll
                for (int e = 0; e < 4; e++) sum[4 * gi + e] = u == v_first ? w[gi][e] : sum[4 * gi + e] + w[gi][e];
        }
        ring_finish<FWD>(P, F, m0, n0, wm, wn, i32, h, sum);
        if (threadIdx.x == 0) __hip_atomic_store(a.counters + counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // clean for the next launch
    }
    __syncthreads();  // the flag word is free again
}

// bias gradient db[c] = sum_b g[b, c]: 32 columns per unit.  Thread t takes the column quad 4 (t & 7) of the unit and the rows
// t >> 3, t >> 3 + 32, ...: sixteen-byte loads, eight in flight, each thread's rows added in ascending order; the 32 row groups' partials
// are then added in ascending group order through LDS (fixed order: bit-reproducible).  Memory latency, not arithmetic: ~2.5 us per unit
// at 1024 rows, which is what a.cu prices.
__device__ __forceinline__ void ring_colsum32(const RingArgs &a, int c0, float *part) {
    const int cq = threadIdx.x & 7, rg = threadIdx.x >> 3;  // 8 column quads x 32 row groups
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.cs_x), 0,
                                                                        (int)(4 * ((int64_t)(a.cs_rows - 1) * a.cs_ld + a.cs_cols)), 0x00020000);
    const int col = c0 + 4 * cq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = rg; r0 < a.cs_rows; r0 += 8 * 32) {
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int r = r0 + 32 * j;
            v[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (r < a.cs_rows && col < a.cs_cols) ? 4 * (r * a.cs_ld + col) : RB_OOB, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) acc = acc + v[j];
    }
    *reinterpret_cast<f32x4 *>(part + (rg * 8 + cq) * 4) = acc;
    __syncthreads();
    if (threadIdx.x < 32 && c0 + (int)threadIdx.x < a.cs_cols) {
        float v = part[threadIdx.x];
        for (int j = 1; j < 32; j++) v += part[j * 32 + threadIdx.x];
        float *dst = a.cs_out + c0 + threadIdx.x;
        *dst = a.cs_accumulate ? *dst + v : v;
    }
    __syncthreads();
}

__device__ __forceinline__ int ring_xcd_slot(int slot, int nslots) {  // XCD j works on the j-th contiguous eighth of the step list
    return (nslots & 7) == 0 ? (slot & 7) * (nslots >> 3) + (slot >> 3) : slot;
}

// the steps [ks0, ks0 + len) of one tile: the tight loop.  `s` = the workgroup's step counter (ring position), `nst` its total.
// BF16 / FWD: the operand precision and the forward form; LAY of the bf16 read: 0 TN, 1 NN, 2 NT (K, ks0: for the edge of the last step).
template <bool NN, bool BF16 = false, bool FWD = false>
__device__ __forceinline__ void ring_segment(const RingArgs &a, Loader &L, int len, int &s, int nst, int wave, int lane, float *lds, f32x16 &acc,
                                             int K = 0, int ks0 = 0) {
    const int wm = wave >> 1, wn = wave & 1, i32 = lane & 31, h = lane >> 5;
    for (int i = 0; i < len; i++, s++) {
        // stage s has landed once at most the younger stages' DMAs (4 per stage and wave) are outstanding
        const int rem = nst - 1 - s;
        if (rem >= 2) asm volatile("s_waitcnt vmcnt(8)" : : : "memory");
        else if (rem == 1) asm volatile("s_waitcnt vmcnt(4)" : : : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        __builtin_amdgcn_s_barrier();  // every wave's share of stage s is in LDS; everybody is done reading stage s - 1
        if (s + RB_D < nst) loader_issue<FWD>(a, L, wave, lane, lds, (s + RB_D) % RB_NS);
        if (BF16) ring_mfma_bf16<FWD ? 2 : (NN ? 1 : 0)>(lds, s % RB_NS, wm, wn, i32, h, K - (ks0 + i) * RB_BK, acc);
        else ring_mfma<NN>(lds, s % RB_NS, wm, wn, i32, h, acc);
    }
}

__global__ __launch_bounds__(256) void gemm_ring_bwd_kernel(RingArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ring_lds[];
    int *flag = reinterpret_cast<int *>(ring_lds + RB_NS * RB_STAGE);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int v = ring_xcd_slot((int)blockIdx.x, a.G);
    const int lo = v * a.q;
    const int hi = lo + a.q < a.S ? lo + a.q : a.S;
    const int n0 = a.p[0].nsteps, n1 = a.p[1].nsteps, T0 = a.p[0].ntiles;
    const int S0 = T0 * n0, Sg = S0 + a.p[1].ntiles * n1;
    const int ghi = hi < Sg ? hi : Sg;
    const int nst = ghi - lo;  // GEMM steps of this workgroup
    if (nst > 0) {
        Loader L;
        {
            const Cursor c = ring_locate(a, lo);
            L.prob = c.prob; L.tile = c.tile; L.ks = c.ks;
            loader_tile<false>(a, L, wave, lane);
        }
        int prob = L.prob, tile = L.tile, ks = L.ks;  // the consumer's position
#pragma unroll
        for (int i = 0; i < RB_D; i++)
            if (i < nst) loader_issue<false>(a, L, wave, lane, ring_lds, i);
        int s = 0;
        while (s < nst) {
            const int nT = prob ? n1 : n0;
            int len = nT - ks;
            if (len > nst - s) len = nst - s;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.0f;
            if (prob) ring_segment<true>(a, L, len, s, nst, wave, lane, ring_lds, acc);
            else ring_segment<false>(a, L, len, s, nst, wave, lane, ring_lds, acc);
            ring_flush<false>(a, nullptr, a.p[prob], tile, (prob ? T0 : 0) + tile, ks, len, (prob ? S0 : 0) + tile * nT, v, wave, lane, acc, flag);
            ks += len;
            if (ks == nT) {
                ks = 0;
                if (++tile == (prob ? a.p[1].ntiles : T0)) {
                    tile = 0;
                    prob++;
                }
            }
        }
    }
    // bias column sums: a unit belongs to the range that holds its first step
    if (hi > Sg && a.nbc > 0) {
        __syncthreads();
        int step = lo > Sg ? lo : Sg;
        while (step < hi) {
            const int rel = step - Sg, u = (rel + a.cu - 1) / a.cu;
            if (u >= a.nbc || Sg + u * a.cu >= hi) break;
            ring_colsum32(a, u * 32, ring_lds);
            step = Sg + u * a.cu + 1;
        }
    }
}

// the whole launch: the workgroup's range of the step list (then, for the backward, its bias column sums)
template <bool BF16, bool FWD>
__device__ __forceinline__ void ring_body(const RingArgs &a, const RingFwd *F) {
    extern __shared__ __attribute__((aligned(16))) float ring_lds[];
    int *flag = reinterpret_cast<int *>(ring_lds + RB_NS * RB_STAGE);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int v = ring_xcd_slot((int)blockIdx.x, a.G);
    const int lo = v * a.q;
    const int hi = lo + a.q < a.S ? lo + a.q : a.S;
    const int n0 = a.p[0].nsteps, n1 = a.p[1].nsteps, T0 = a.p[0].ntiles;
    const int S0 = T0 * n0, Sg = S0 + a.p[1].ntiles * n1;
    const int ghi = hi < Sg ? hi : Sg;
    const int nst = ghi - lo;  // GEMM steps of this workgroup
    if (nst > 0) {
        Loader L;
        {
            const Cursor c = ring_locate(a, lo);
            L.prob = c.prob; L.tile = c.tile; L.ks = c.ks;
            loader_tile<FWD>(a, L, wave, lane);
        }
        int prob = L.prob, tile = L.tile, ks = L.ks;  // the consumer's position
#pragma unroll
        for (int i = 0; i < RB_D; i++)
            if (i < nst) loader_issue<FWD>(a, L, wave, lane, ring_lds, i);
        int s = 0;
        while (s < nst) {
            const int nT = prob ? n1 : n0;
            int len = nT - ks;
            if (len > nst - s) len = nst - s;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.0f;
            if (!BF16) {
                if (prob) ring_segment<true>(a, L, len, s, nst, wave, lane, ring_lds, acc);
                else ring_segment<false>(a, L, len, s, nst, wave, lane, ring_lds, acc);
            } else if (prob) ring_segment<true, true, false>(a, L, len, s, nst, wave, lane, ring_lds, acc, a.p[1].K, ks);
            else ring_segment<false, true, FWD>(a, L, len, s, nst, wave, lane, ring_lds, acc, a.p[0].K, ks);
            ring_flush<FWD>(a, F, a.p[prob], tile, (prob ? T0 : 0) + tile, ks, len, (prob ? S0 : 0) + tile * nT, v, wave, lane, acc, flag);
            ks += len;
            if (ks == nT) {
                ks = 0;
                if (++tile == (prob ? a.p[1].ntiles : T0)) {
                    tile = 0;
                    prob++;
                }
            }
        }
    }
    // bias column sums: a unit belongs to the range that holds its first step
    if (!FWD && hi > Sg && a.nbc > 0) {
        __syncthreads();
        int step = lo > Sg ? lo : Sg;
        while (step < hi) {
            const int rel = step - Sg, u = (rel + a.cu - 1) / a.cu;
            if (u >= a.nbc || Sg + u * a.cu >= hi) break;
            ring_colsum32(a, u * 32, ring_lds);
            step = Sg + u * a.cu + 1;
        }
    }
}

__global__ __launch_bounds__(256) void gemm_ring_bwd_bf16_kernel(RingArgs a) { ring_body<true, false>(a, nullptr); }
__global__ __launch_bounds__(256) void gemm_ring_fwd_bf16_kernel(RingArgs a, RingFwd f) { ring_body<true, true>(a, &f); }

}  // namespace

namespace {

int ring_band(int tiles, int nby) {  // band height ~ sqrt(tiles / 8): the eighth of the list an XCD takes is then about square
    int bh = 1;
    while ((bh + 1) * (bh + 1) * 8 <= tiles) bh++;
    return bh < nby ? bh : nby;
}

// the TN problem dW [n_out, n_in] (+)= g^T x of RingArgs::p[0]
void ring_prob_dw(RingProb &p0, const float *g, int64_t ldg, const float *x, int64_t ldx, int64_t B, int64_t n_out, int64_t n_in, float *dW,
                  int64_t lddw, int accumulate_dw) {
    p0.A = g; p0.lda = (int)ldg; p0.B = x; p0.ldb = (int)ldx; p0.C = dW; p0.ldc = (int)lddw;
    p0.M = (int)n_out; p0.N = (int)n_in; p0.K = (int)B;
    p0.nbx = (int)hv_cdiv(n_in, 64); p0.nby = (int)hv_cdiv(n_out, 64); p0.ntiles = p0.nbx * p0.nby; p0.nsteps = (int)hv_cdiv(B, RB_BK);
    p0.bh = ring_band(p0.ntiles, p0.nby);
    p0.epilogue = HIDVAE_EPI_NONE; p0.scale = 1.0f; p0.accumulate = accumulate_dw; p0.aux = nullptr; p0.ldaux = 0;
    p0.a_bytes = (unsigned)(4 * ((B - 1) * ldg + n_out)); p0.b_bytes = (unsigned)(4 * ((B - 1) * ldx + n_in));
}

// the NN problem dX [B, n_in] = epi(g W) of RingArgs::p[1]
void ring_prob_dx(RingProb &p1, const float *g, int64_t ldg, const float *W, int64_t ldw, int64_t B, int64_t n_out, int64_t n_in, float *dX,
                  int64_t lddx, int dx_epilogue, float *aux, int64_t ldaux, float dx_scale, int accumulate = 0) {
    p1.A = g; p1.lda = (int)ldg; p1.B = W; p1.ldb = (int)ldw; p1.C = dX; p1.ldc = (int)lddx;
    p1.M = (int)B; p1.N = (int)n_in; p1.K = (int)n_out;
    p1.nbx = (int)hv_cdiv(n_in, 64); p1.nby = (int)hv_cdiv(B, 64); p1.ntiles = p1.nbx * p1.nby; p1.nsteps = (int)hv_cdiv(n_out, RB_BK);
    p1.bh = ring_band(p1.ntiles, p1.nby);
    p1.epilogue = dx_epilogue; p1.aux = aux; p1.ldaux = aux ? (int)ldaux : 0; p1.scale = dx_scale; p1.accumulate = accumulate;
    p1.a_bytes = (unsigned)(4 * ((B - 1) * ldg + n_out)); p1.b_bytes = (unsigned)(4 * ((n_out - 1) * ldw + n_in));
}

void ring_prob_absent(RingProb &p) {
    p.ntiles = 0; p.nsteps = 1; p.nbx = p.nby = p.bh = 1;
}

// the even split of the step list over at most `slots` workgroups; -> false when the arrival counters or the slabs do not suffice
bool ring_split(RingArgs &a, int slots, float *workspace) {
    a.S = a.p[0].ntiles * a.p[0].nsteps + a.p[1].ntiles * a.p[1].nsteps + a.nbc * a.cu;
    if (a.p[0].ntiles + a.p[1].ntiles > HV_SK_COUNTERS) return false;
    constexpr int minq = 8;  // shortest range worth a workgroup (steps of 32 k)
    int G = a.S / minq;
    if (G > slots) G = slots;
    if (G > HV_SK_MAX_G) G = (int)HV_SK_MAX_G;
    if (G < 1) G = 1;
    a.q = (int)hv_cdiv(a.S, G);
    a.G = (int)hv_cdiv(a.S, a.q);
    a.counters = reinterpret_cast<int *>(workspace);
    a.slabs = workspace + HV_SK_COUNTERS;
    return true;
}

constexpr size_t RB_LDS_BYTES = (size_t)RB_LDS_FLOATS * 4;

int ring_lds_attr(const void *kernel, const char *name, const char *kernel_name) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RB_LDS_BYTES) != hipSuccess)
        return hv_fail(HIDVAE_ELAUNCH, "%s: could not size the LDS of %s", name, kernel_name);
    return HIDVAE_OK;
}

}  // namespace

int hv_ring_linear_bwd(const float *g, int64_t ldg, const float *x, int64_t ldx, const float *W, int64_t ldw, int64_t B, int64_t n_out,
                       int64_t n_in, float *dW, int64_t lddw, int accumulate_dw, float *dX, int64_t lddx, int dx_epilogue, float *aux,
                       int64_t ldaux, float dx_scale, float *db, int accumulate_db, float *workspace, int slots, hipStream_t stream) {
    RingArgs a{};
    ring_prob_dw(a.p[0], g, ldg, x, ldx, B, n_out, n_in, dW, lddw, accumulate_dw);
    if (dX != nullptr) ring_prob_dx(a.p[1], g, ldg, W, ldw, B, n_out, n_in, dX, lddx, dx_epilogue, aux, ldaux, dx_scale);
    else ring_prob_absent(a.p[1]);
    a.cs_x = g; a.cs_ld = (int)ldg; a.cs_rows = (int)B; a.cs_cols = (int)n_out; a.cs_out = db; a.cs_accumulate = accumulate_db;
    a.nbc = db != nullptr ? (int)hv_cdiv(n_out, 32) : 0;
    a.cu = 4 + (int)hv_cdiv(B, 512);  // a 32-column strip of B rows: latency-bound, ~2 us + 0.5 us per 512 rows, in steps of ~0.45 us
    if (!ring_split(a, slots, workspace)) return 1;
    static const int attr = ring_lds_attr(reinterpret_cast<const void *>(&gemm_ring_bwd_kernel), "linear_bwd ring", "gemm_ring_bwd_kernel");
    if (attr != HIDVAE_OK) return attr;
    hipLaunchKernelGGL(gemm_ring_bwd_kernel, dim3((unsigned)a.G), dim3(256), RB_LDS_BYTES, stream, a);
    HV_LAUNCH_CHECK("linear_bwd ring");
    return HIDVAE_OK;
}

// ---- the bf16-operand entry points (include/hidvae.h) -------------------------------------------------------------------------------
namespace {

constexpr int RB_BF16_SLOTS = 512;  // workgroups a bf16 launch may use: two per CU (the fp32 ring's choice inside hidvae_linear_bwd)

// a buffer descriptor's byte offsets are 32-bit: every operand view of a launch stays below 2^29 floats; a launch's step list stays an int
constexpr int64_t RB_MAX_ELEMS = ((int64_t)1 << 29) - 1;
constexpr int64_t RB_MAX_STEPS = (int64_t)1 << 28;

bool ring_bytes_ok(int64_t rows, int64_t ld, int64_t cols) { return rows >= 1 && (rows - 1) * ld + cols <= RB_MAX_ELEMS; }

int64_t ring_min(int64_t a, int64_t b) { return a < b ? a : b; }

// rows of a view of leading dimension ld that keep it below 2^29 floats, a multiple of `unit` (0: not even `unit` rows fit)
int64_t ring_rows_fit(int64_t ld, int64_t unit) { return (RB_MAX_ELEMS / (ld > 0 ? ld : 1)) / unit * unit; }

int linear_bwd_bf16_impl(const float *g, int64_t ldg, const float *x, int64_t ldx, const float *W, int64_t ldw, int64_t B, int64_t n_out,
                         int64_t n_in, float *dW, int64_t lddw, int accumulate_dw, float *dX, int64_t lddx, int dx_epilogue, float *aux,
                         int64_t ldaux, float dx_scale, float *db, int accumulate_db, float *workspace, hipStream_t stream, const char *name) {
    HV_REQUIRE(g && x && dW && B >= 1 && n_out >= 1 && n_in >= 1, "%s: bad arguments", name);
    HV_REQUIRE(ldg >= n_out && ldx >= n_in && lddw >= n_in, "%s: leading dimension too small", name);
    HV_REQUIRE(dX == nullptr || (W != nullptr && ldw >= n_in && lddx >= n_in), "%s: dX needs W", name);
    HV_REQUIRE(dX == nullptr || dx_epilogue == HIDVAE_EPI_NONE || (dx_epilogue >= HIDVAE_EPI_DSILU && aux != nullptr && ldaux >= n_in),
               "%s: dX epilogue %d", name, dx_epilogue);
    HV_REQUIRE(workspace != nullptr, "%s: needs its workspace (hidvae_query_workspace(HIDVAE_WS_LINEAR_BWD_BF16))", name);
    static const int attr = ring_lds_attr(reinterpret_cast<const void *>(&gemm_ring_bwd_bf16_kernel), name, "gemm_ring_bwd_bf16_kernel");
    if (attr != HIDVAE_OK) return attr;
    const int64_t nbx = hv_cdiv(n_in, 64), t0 = hv_cdiv(n_out, 64) * nbx, t1 = dX != nullptr ? hv_cdiv(B, 64) * nbx : 0;
    auto launch = [&](const RingArgs &a0) -> int {
        RingArgs a = a0;
        if (!ring_split(a, RB_BF16_SLOTS, workspace)) return hv_fail(HIDVAE_EINVAL, "%s: too many tiles", name);
        hipLaunchKernelGGL(gemm_ring_bwd_bf16_kernel, dim3((unsigned)a.G), dim3(256), RB_LDS_BYTES, stream, a);
        HV_LAUNCH_CHECK(name);
        return HIDVAE_OK;
    };
    auto colsums = [&](RingArgs &a, const float *gv, int64_t rows, int64_t cols, float *out, int acc) {
        if (db == nullptr) return;
        a.cs_x = gv; a.cs_ld = (int)ldg; a.cs_rows = (int)rows; a.cs_cols = (int)cols; a.cs_out = out; a.cs_accumulate = acc;
        a.nbc = (int)hv_cdiv(cols, 32);
        a.cu = 4 + (int)hv_cdiv(rows, 512);
    };
    // the common case: dW, dX and db in ONE launch
    const bool whole = t0 + t1 <= HV_SK_COUNTERS && ring_bytes_ok(B, ldg, n_out) && ring_bytes_ok(B, ldx, n_in) && ring_bytes_ok(n_out, lddw, n_in) &&
                       (dX == nullptr || (ring_bytes_ok(n_out, ldw, n_in) && ring_bytes_ok(B, lddx, n_in) && (aux == nullptr || ring_bytes_ok(B, ldaux, n_in)))) &&
                       (t0 * hv_cdiv(B, RB_BK) + t1 * hv_cdiv(n_out, RB_BK)) <= RB_MAX_STEPS;
    if (whole) {
        RingArgs a{};
        ring_prob_dw(a.p[0], g, ldg, x, ldx, B, n_out, n_in, dW, lddw, accumulate_dw);
        if (dX != nullptr) ring_prob_dx(a.p[1], g, ldg, W, ldw, B, n_out, n_in, dX, lddx, dx_epilogue, aux, ldaux, dx_scale);
        else ring_prob_absent(a.p[1]);
        colsums(a, g, B, n_out, db, accumulate_db);
        return launch(a);
    }
    // otherwise in pieces, each within the arrival counters, the 32-bit byte offsets and an int step list:
    //   dW + db: bands of dW rows (n_out) x chunks of the batch (dW's K), the later chunks accumulating (fixed order: deterministic);
    //   dX:      chunks of rows x chunks of n_out (dX's K), the later ones accumulating (every D* epilogue is linear in the product)
    HV_REQUIRE(nbx <= HV_SK_COUNTERS && ring_rows_fit(ldg, 64) >= 64 && ring_rows_fit(ldx, 64) >= 64 &&
               ring_rows_fit(lddw, 64) >= 64 && (dX == nullptr || (ring_rows_fit(ldw, RB_BK) >= RB_BK && ring_rows_fit(lddx, 64) >= 64 &&
               (aux == nullptr || ring_rows_fit(ldaux, 64) >= 64))),
               "%s: rows of more than 2^23 floats or more than 262144 columns", name);
    {
        int64_t band = ring_min((HV_SK_COUNTERS / nbx) * 64, ring_rows_fit(lddw, 64));
        band = ring_min(band, hv_cdiv(n_out, 64) * 64);
        const int64_t tb = hv_cdiv(band, 64) * nbx;
        int64_t kc = ring_min(ring_min(ring_rows_fit(ldg, RB_BK), ring_rows_fit(ldx, RB_BK)), (RB_MAX_STEPS / tb) * RB_BK);
        kc = ring_min(kc, B);
        for (int64_t o0 = 0; o0 < n_out; o0 += band) {
            const int64_t Ro = ring_min(band, n_out - o0);
            for (int64_t k0 = 0; k0 < B; k0 += kc) {
                const int64_t Kc = ring_min(kc, B - k0);
                RingArgs a{};
                ring_prob_dw(a.p[0], g + k0 * ldg + o0, ldg, x + k0 * ldx, ldx, Kc, Ro, n_in, dW + o0 * lddw, lddw, accumulate_dw || k0 > 0);
                ring_prob_absent(a.p[1]);
                colsums(a, g + k0 * ldg + o0, Kc, Ro, db != nullptr ? db + o0 : nullptr, accumulate_db || k0 > 0);
                const int rc = launch(a);
                if (rc != HIDVAE_OK) return rc;
            }
        }
    }
    if (dX == nullptr) return HIDVAE_OK;
    int64_t rows = ring_min(ring_min((HV_SK_COUNTERS / nbx) * 64, ring_rows_fit(ldg, 64)), ring_rows_fit(lddx, 64));
    if (aux != nullptr) rows = ring_min(rows, ring_rows_fit(ldaux, 64));
    rows = ring_min(rows, hv_cdiv(B, 64) * 64);
    const int64_t tr = hv_cdiv(rows, 64) * nbx;
    const int64_t kc = ring_min(ring_min(ring_rows_fit(ldw, RB_BK), (RB_MAX_STEPS / tr) * RB_BK), n_out);
    for (int64_t r0 = 0; r0 < B; r0 += rows) {
        const int64_t R = ring_min(rows, B - r0);
        for (int64_t k0 = 0; k0 < n_out; k0 += kc) {
            const int64_t Kc = ring_min(kc, n_out - k0);
            RingArgs a{};
            ring_prob_absent(a.p[0]);
            ring_prob_dx(a.p[1], g + r0 * ldg + k0, ldg, W + k0 * ldw, ldw, R, Kc, n_in, dX + r0 * lddx, lddx, dx_epilogue,
                         aux ? aux + r0 * ldaux : nullptr, ldaux, dx_scale, k0 > 0);
            const int rc = launch(a);
            if (rc != HIDVAE_OK) return rc;
        }
    }
    return HIDVAE_OK;
}

}  // namespace

extern "C" int hidvae_linear_bwd_bf16(const float *g, int64_t ldg, const float *x, int64_t ldx, const float *W, int64_t ldw, int64_t B,
                                      int64_t n_out, int64_t n_in, float *dW, int64_t lddw, int accumulate_dw, float *dX, int64_t lddx,
                                      int dx_epilogue, float *aux, int64_t ldaux, float dx_scale, float *db, int accumulate_db,
                                      float *workspace, void *stream) {
    return linear_bwd_bf16_impl(g, ldg, x, ldx, W, ldw, B, n_out, n_in, dW, lddw, accumulate_dw, dX, lddx, dx_epilogue, aux, ldaux, dx_scale,
                                db, accumulate_db, workspace, (hipStream_t)stream, "linear_bwd_bf16");
}

extern "C" int hidvae_linear_bwd_group_bf16(const hidvae_linear_bwd_problem *pr, int n, void *stream) {
    HV_REQUIRE(pr != nullptr && n >= 1, "linear_bwd_group_bf16: bad arguments");
    for (int i = 0; i < n; i++) {  // one ring launch per problem, in order (stream-serialised: one workspace may serve them all)
        const hidvae_linear_bwd_problem &q = pr[i];
        const int rc = linear_bwd_bf16_impl(q.g, q.ldg, q.x, q.ldx, q.W, q.ldw, q.B, q.n_out, q.n_in, q.dW, q.lddw, q.accumulate_dw, q.dX,
                                            q.lddx, q.dx_epilogue, q.aux, q.ldaux, 1.0f, q.db, q.accumulate_db, q.workspace, (hipStream_t)stream,
                                            "linear_bwd_group_bf16");
        if (rc != HIDVAE_OK) return rc;
    }
    return HIDVAE_OK;
}

extern "C" int hidvae_gemm_bf16(int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias,
                                float *C, int64_t ldc, int epilogue, float *aux, int64_t ldaux, const float *mask, int64_t ldmask,
                                float mask_scale, const unsigned long long *rng_state, unsigned rng_site, unsigned drop_threshold,
                                float *workspace, int accumulate, void *stream) {
    HV_REQUIRE(M >= 1 && N >= 1 && K >= 1, "gemm_bf16: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    HV_REQUIRE(A && B && C, "gemm_bf16: null operand");
    HV_REQUIRE(lda >= K && ldb >= K && ldc >= N, "gemm_bf16: leading dimension too small (lda=%lld ldb=%lld ldc=%lld)", (long long)lda,
               (long long)ldb, (long long)ldc);
    HV_REQUIRE(epilogue >= HIDVAE_EPI_NONE && epilogue <= HIDVAE_EPI_SIGMOID, "gemm_bf16: epilogue %d (forward codes only)", epilogue);
    HV_REQUIRE(aux == nullptr || ldaux >= N, "gemm_bf16: ldaux=%lld", (long long)ldaux);
    HV_REQUIRE(!(mask && rng_state), "gemm_bf16: a keep-mask OR the in-kernel generator, not both");
    HV_REQUIRE(mask == nullptr || ldmask >= N, "gemm_bf16: ldmask=%lld", (long long)ldmask);
    HV_REQUIRE(workspace != nullptr, "gemm_bf16: needs its workspace (hidvae_query_workspace(HIDVAE_WS_GEMM_BF16))");
    HV_REQUIRE(ring_bytes_ok(N, ldb, K), "gemm_bf16: a weight of %lld x %lld passes 2^29 elements (32-bit byte offsets)", (long long)N, (long long)K);
    RingFwd f{};
    f.bias = bias; f.mask = mask; f.ldmask = mask ? (int)ldmask : 0; f.mask_scale = mask_scale;
    f.drop = HvDrop{rng_state, rng_site, drop_threshold};
    static const int attr = ring_lds_attr(reinterpret_cast<const void *>(&gemm_ring_fwd_bf16_kernel), "gemm_bf16", "gemm_ring_fwd_bf16_kernel");
    if (attr != HIDVAE_OK) return attr;
    // row chunks of at most HV_SK_COUNTERS tiles (M > 21845 at N = 768), every view of them below 2^29 floats, and an int step list
    const int64_t nbx = hv_cdiv(N, 64);
    int64_t rows = ring_min(ring_min((HV_SK_COUNTERS / nbx) * 64, ring_rows_fit(lda, 64)), ring_rows_fit(ldc, 64));
    if (aux != nullptr) rows = ring_min(rows, ring_rows_fit(ldaux, 64));
    if (mask != nullptr) rows = ring_min(rows, ring_rows_fit(ldmask, 64));
    rows = ring_min(rows, (RB_MAX_STEPS / (nbx * hv_cdiv(K, RB_BK))) * 64);
    HV_REQUIRE(rows >= 64, "gemm_bf16: N=%lld / rows of more than 2^23 floats are refused", (long long)N);
    for (int64_t r0 = 0; r0 < M; r0 += rows) {
        const int64_t R = M - r0 < rows ? M - r0 : rows;
        RingArgs a{};
        RingProb &p = a.p[0];
        p.A = A + r0 * lda; p.lda = (int)lda; p.B = B; p.ldb = (int)ldb; p.C = C + r0 * ldc; p.ldc = (int)ldc;
        p.M = (int)R; p.N = (int)N; p.K = (int)K;
        p.nbx = (int)nbx; p.nby = (int)hv_cdiv(R, 64); p.ntiles = p.nbx * p.nby; p.nsteps = (int)hv_cdiv(K, RB_BK);
        p.bh = ring_band(p.ntiles, p.nby);
        p.epilogue = epilogue; p.aux = aux ? aux + r0 * ldaux : nullptr; p.ldaux = aux ? (int)ldaux : 0; p.scale = 1.0f; p.accumulate = accumulate;
        p.a_bytes = (unsigned)(4 * ((R - 1) * lda + K)); p.b_bytes = (unsigned)(4 * ((N - 1) * ldb + K));
        ring_prob_absent(a.p[1]);
        RingFwd fc = f;
        if (mask != nullptr) fc.mask = mask + r0 * ldmask;
        fc.row_base = (int)r0;  // (the in-kernel decision indexes an element by its row in the whole matrix)
        if (!ring_split(a, RB_BF16_SLOTS, workspace)) return hv_fail(HIDVAE_EINVAL, "gemm_bf16: too many tiles");
        hipLaunchKernelGGL(gemm_ring_fwd_bf16_kernel, dim3((unsigned)a.G), dim3(256), RB_LDS_BYTES, (hipStream_t)stream, a, fc);
        HV_LAUNCH_CHECK("gemm_bf16");
    }
    return HIDVAE_OK;
}
