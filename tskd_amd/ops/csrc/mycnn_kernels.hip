// MyCNN fused inference kernels — hand-written CDNA4 (gfx950 / MI355X) HIP.
//
// Replaces the reference's PyTorch ATen CPU ops (reference bin/models.py:22-36;
// SURVEY.md §2.6 K1-K9). Geometry, pack offsets and the small device helpers
// shared with the other two libraries are in tskd_common.h.
//
//   1. Conv stack: (SN, CIN, 120) windows -> (SN, LIN) features. Fuses
//      Conv1d(CIN,4,K1) + tanh + MaxPool1d(PK,PS) + Conv1d(4,1,5) + tanh +
//      pool into ONE kernel, one 64-lane wavefront per window; the pooled
//      tail (conv_tail) is shared. Dropout sites are identity in eval (K5).
//        1a conv_stack_kernel — fp32 input (exact-numerics path): direct
//           VALU cross-correlation.
//        1b conv_stack_mfma_kernel — bf16 (SN, CIN, L) input: conv1 as an
//           MFMA im2col-GEMM. The window is staged TRANSPOSED in LDS as bf16
//           (xt[t][i]), which makes the im2col matrix A[s][kk]
//           (kk = k*CIN + i) a shifted view xt_flat[s*CIN + kk] — A
//           fragments are contiguous LDS reads, no gather. B = conv weights
//           pre-packed host-side in MFMA fragment order (4 used columns of a
//           16-col tile); the v_mfma_f32_16x16x32_bf16 accumulator chains
//           over KK/32 k-steps; the epilogue folds the bias and lands RAW
//           rows in LDS for the pool (tanh is applied after each pool).
//        1c conv_stack_mfma_tlast_kernel — bf16 time-last (SN, L, CIN)
//           input, even CIN: the same GEMM with A fragments read straight
//           from global, one wave per TWO windows.
//
//   2. lstm_head_kernel: (S, N, LIN) features -> (S, N) logits/probs.
//      Fuses the 2-layer LSTM(LIN,16) *batch-axis-as-time* scan (the
//      reference's 2-D-input quirk: hidden state flows across the N windows
//      of a batch — SURVEY.md §2.3) with the Linear(16,1) head, the age gate
//      relu(age*eps+1) and optional sigmoid. One wavefront per sequence:
//      the 64 lanes are the 64 gate-unit rows (4 gates x 16 hidden),
//      per-lane weight rows live in VGPRs, the full h vectors of both layers
//      are collected into per-lane registers with 16 INDEPENDENT shuffles
//      per layer (dependency-chain broken: the serial-scan critical path is
//      ~2 shuffle round-trips per layer, not 32), features prefetched into
//      LDS in 32-step chunks.
//
//   3. serve_tail_kernel: the serving trigger (one window per stream) as one
//      kernel — window gather from the fp32 ring + 1b's conv + ONE LSTM step
//      + head. MyCNN5/MyCNN4 (even CIN).
//
//   4. serve_tail_occlude_kernel: channel attribution — kernel 3 on C + 1
//      variants of a listed stream's window (one channel held flat or zeroed
//      per variant), the ring window read once per stream.
//
//   5. serve_tail_history_kernel: risk history — kernel 3 on K past window
//      positions of a listed stream that the ring still holds.
//
//   debug_mfma_kernel: one 16x16x32 bf16 MFMA tile, the fragment-map ground
//   truth for the tests.
//
// Numerics: fp32 accumulation throughout (MFMA accumulator is fp32).
// Wavefront size is 64 on CDNA4 (not 32) — all lane math assumes it.

#include <hip/hip_runtime.h>

#include "tskd_common.h"

#define WG_WAVES 4
#define WG_THREADS (WAVE * WG_WAVES)

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// One lane's MFMA operand fragment: 8 bf16 = 4 dwords.
union BU { unsigned int d[4]; unsigned short u[8]; bf16x8 v; };

// Preload this lane's B fragments for all k-steps: one dwordx4 per step
// from the host-packed [KSTEPS][64][8] bf16 array.
template <class G>
__device__ __forceinline__ void load_bfrags(
    const unsigned short* bfrag, int lane, bf16x8 (&bfr)[G::KSTEPS])
{
    #pragma unroll
    for (int st = 0; st < G::KSTEPS; ++st) {
        BU bu;
        #pragma unroll
        for (int q = 0; q < 4; ++q)
            bu.d[q] = ((const unsigned int*)bfrag)[(st * WAVE + lane) * 4 + q];
        bfr[st] = bu.v;
    }
}

// ---------------------------------------------------------------------------
// Shared epilogue: pool1 -> conv2 -> tanh -> pool2 -> feature store.
// Reads lds_c1 (4 x C1 conv1 rows), uses lds_p1/lds_c2 scratch.
//
// TANH_AT_POOL: tanh is monotone, so tanh(max(a,b)) == max(tanh(a), tanh(b))
// — the MFMA path stores RAW conv1 pre-activations (bias folded) and applies
// tanh AFTER each pool, cutting transcendental count ~2x (444->220, 51->25)
// and keeping every lane active.
// ---------------------------------------------------------------------------
template <class G, bool TANH_AT_POOL>
__device__ __forceinline__ void conv_tail(
    int lane, const float* __restrict__ lds_w, float* c1w, float* p1w,
    float* c2w, float* __restrict__ feat, long win)
{
    const float* w2 = lds_w + G::OW2;
    const float  b2 = lds_w[G::OB2];
    // pool1 (PK, PS)
    for (int o = lane; o < 4 * G::P1; o += WAVE) {
        const int c = o / G::P1, q = o % G::P1;
        const float* src = c1w + c * G::C1 + q * G::PS;
        float m = src[0];
        #pragma unroll
        for (int k = 1; k < G::PK; ++k) m = fmaxf(m, src[k]);
        p1w[o] = TANH_AT_POOL ? tanhf_(m) : m;
    }
    wave_sync();
    // conv2 (+ tanh here only when pool1 already produced tanh'd inputs and
    // pool2 will apply the second tanh)
    for (int s = lane; s < G::C2; s += WAVE) {
        float acc = b2;
        #pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float* pr = p1w + c * G::P1 + s;
            #pragma unroll
            for (int k = 0; k < 5; ++k)
                acc = fmaf(w2[c * 5 + k], pr[k], acc);
        }
        c2w[s] = TANH_AT_POOL ? acc : tanhf_(acc);
    }
    wave_sync();
    // pool2 -> feature vector
    for (int q = lane; q < G::LIN; q += WAVE) {
        const float* src = c2w + q * G::PS;
        float m = src[0];
        #pragma unroll
        for (int k = 1; k < G::PK; ++k) m = fmaxf(m, src[k]);
        feat[win * G::LIN + q] = TANH_AT_POOL ? tanhf_(m) : m;
    }
    wave_sync();  // before the next window overwrites scratch
}

// ---------------------------------------------------------------------------
// Kernel 1a (fp32 path): direct VALU conv stack — exact fp32 numerics.
// ---------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(WG_THREADS) void conv_stack_kernel(
    const float* __restrict__ x,  // (SN, CIN, L)
    float* __restrict__ feat,     // (SN, LIN)
    const float* __restrict__ wpack,
    int SN)
{
    __shared__ float lds_w[G::NW];
    __shared__ float lds_x[WG_WAVES][G::CIN * G::L];
    __shared__ float lds_c1[WG_WAVES][4 * G::C1];
    __shared__ float lds_p1[WG_WAVES][4 * G::P1];
    __shared__ float lds_c2[WG_WAVES][G::C2];

    for (int i = threadIdx.x; i < G::NW; i += WG_THREADS) lds_w[i] = wpack[i];
    __syncthreads();

    const float* w1 = lds_w + G::OW1;
    const float* b1 = lds_w + G::OB1;
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    float* xw = lds_x[wave];

    for (long win = blockIdx.x * WG_WAVES + wave; win < SN;
         win += (long)gridDim.x * WG_WAVES) {
        const float* xin = x + win * (G::CIN * G::L);
        for (int i = lane; i < G::CIN * G::L; i += WAVE) xw[i] = xin[i];
        wave_sync();
        for (int o = lane; o < 4 * G::C1; o += WAVE) {
            const int c = o / G::C1, s = o % G::C1;
            // two independent partial accumulators (even/odd input channel)
            // halve the 100-deep dependent fma chain
            float acc = b1[c], acc2 = 0.f;
            const float* wr = w1 + c * (G::CIN * G::K1);
            #pragma unroll
            for (int i = 0; i < G::CIN; i += 2) {
                const float* xr = xw + i * G::L + s;
                const float* xr2 = xw + (i + 1) * G::L + s;
                #pragma unroll
                for (int k = 0; k < G::K1; ++k) {
                    acc = fmaf(wr[i * G::K1 + k], xr[k], acc);
                    if (i + 1 < G::CIN)
                        acc2 = fmaf(wr[(i + 1) * G::K1 + k], xr2[k], acc2);
                }
            }
            lds_c1[wave][o] = tanhf_(acc + acc2);
        }
        wave_sync();
        conv_tail<G, false>(lane, lds_w, lds_c1[wave], lds_p1[wave],
                            lds_c2[wave], feat, win);
    }
}

// ---------------------------------------------------------------------------
// Kernel 1b (bf16 path): conv1 as MFMA im2col-GEMM (16x16x32 bf16).
//
// Fragment maps (gfx950 v_mfma_f32_16x16x32_bf16; verified on-device by
// tskd_debug_mfma16x16x32 + tests/test_hip_mycnn.py):
//   A: lane l holds A[row = l&15][k = (l>>4)*8 + j], j = 0..7
//   B: lane l holds B[k = (l>>4)*8 + j][col = l&15]
//   C: lane l holds C[row = (l>>4)*4 + r][col = l&15], r = 0..3
// ---------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(WG_THREADS) void conv_stack_mfma_kernel(
    const unsigned short* __restrict__ x,   // (SN, CIN, L) bf16 bits
    float* __restrict__ feat,               // (SN, LIN)
    const float* __restrict__ wpack,
    const unsigned short* __restrict__ bfrag,  // [KSTEPS][64][8] bf16 bits
    int SN)
{
    __shared__ float lds_w[G::NW];
    __shared__ unsigned short lds_xt[WG_WAVES][G::XTSZ];  // transposed window
    __shared__ float lds_c1[WG_WAVES][4 * G::C1];
    __shared__ float lds_p1[WG_WAVES][4 * G::P1];
    __shared__ float lds_c2[WG_WAVES][G::C2];

    for (int i = threadIdx.x; i < G::NW; i += WG_THREADS) lds_w[i] = wpack[i];
    __syncthreads();

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const float* b1 = lds_w + G::OB1;
    unsigned short* xt = lds_xt[wave];

    bf16x8 bfr[G::KSTEPS];
    // Preload B fragments (per-lane, all k-steps): one dwordx4 per step.
    // Written out rather than load_bfrags(): the helper's loop form changes
    // this kernel's instruction schedule.
    #pragma unroll
    for (int st = 0; st < G::KSTEPS; ++st) {
        BU bu;
        bu.d[0] = ((const unsigned int*)bfrag)[(st * WAVE + lane) * 4 + 0];
        bu.d[1] = ((const unsigned int*)bfrag)[(st * WAVE + lane) * 4 + 1];
        bu.d[2] = ((const unsigned int*)bfrag)[(st * WAVE + lane) * 4 + 2];
        bu.d[3] = ((const unsigned int*)bfrag)[(st * WAVE + lane) * 4 + 3];
        bfr[st] = bu.v;
    }

    for (long win = blockIdx.x * WG_WAVES + wave; win < SN;
         win += (long)gridDim.x * WG_WAVES) {
        const unsigned short* xin = x + win * (G::CIN * G::L);
        // Stage TRANSPOSED: xt[t*CIN + i] = x[i*L + t]. Coalesced 8-byte
        // global reads (L % 4 == 0 so a quad never crosses a channel row),
        // scattered 2-byte LDS writes.
        static_assert(G::L % 4 == 0, "quad staging needs L % 4 == 0");
        for (int q = lane; q < G::CIN * G::L / 4; q += WAVE) {
            const int f = q * 4;
            const int i = f / G::L, t0 = f % G::L;
            union { unsigned long long u; unsigned short h[4]; } v;
            v.u = *(const unsigned long long*)(xin + f);
            #pragma unroll
            for (int j = 0; j < 4; ++j)
                xt[(t0 + j) * G::CIN + i] = v.h[j];
        }
        for (int i = G::XTN + lane; i < G::XTSZ; i += WAVE) xt[i] = 0;
        wave_sync();

        // conv1 = A(im2col view of xt) x B(weights), one 16-row tile at a time
        #pragma unroll 1
        for (int mt = 0; mt < G::MTILES; ++mt) {
            const int s = mt * 16 + (lane & 15);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int st = 0; st < G::KSTEPS; ++st) {
                const int base = s * G::CIN + st * 32 + (lane >> 4) * 8;
                BU au;
                if constexpr (G::CIN % 2 == 0) {
                    // base is even: 4-byte-aligned LDS reads land directly
                    // in the fragment dwords (little-endian bf16 pairs).
                    const unsigned int* xtu = (const unsigned int*)xt;
                    au.d[0] = xtu[base / 2];
                    au.d[1] = xtu[base / 2 + 1];
                    au.d[2] = xtu[base / 2 + 2];
                    au.d[3] = xtu[base / 2 + 3];
                } else {
                    #pragma unroll
                    for (int j = 0; j < 8; ++j) au.u[j] = xt[base + j];
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(au.v, bfr[st],
                                                              acc, 0, 0, 0);
            }
            const int c = lane & 15;
            if (c < 4) {
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mt * 16 + (lane >> 4) * 4 + r;
                    if (row < G::C1)
                        lds_c1[wave][c * G::C1 + row] = acc[r] + b1[c];
                }
            }
        }
        wave_sync();
        conv_tail<G, true>(lane, lds_w, lds_c1[wave], lds_p1[wave],
                           lds_c2[wave], feat, win);
    }
}

// ---------------------------------------------------------------------------
// Kernel 1c (bf16 TIME-LAST layout): conv1 MFMA im2col with A-fragments read
// STRAIGHT FROM GLOBAL — no LDS staging, no transpose pass.
//
// Input layout (SN, L, CIN) ("timelast"): the im2col row A[s][kk]
// (kk = k*CIN + i) is the contiguous global range x[win*L*CIN + s*CIN + kk],
// so each lane's 8-element fragment is 4 dword loads through the vector-
// memory path (L1-resident: a window is 2.4 KB). PMC showed the staged
// variant spends 39% of cycles waiting on LDS (profiles/r01) — this variant
// keeps LDS only for the small pooled tail.
//
// NOTE: fragment reads overrun a window by up to (KSTEPS*32 - KK + C1%16
// rows) elements into the NEXT window; callers must allocate the x buffer
// with TLAST_SLACK trailing elements (tskd_amd/ops wrapper does). Only the
// last M-tile reaches that far, and only at reduction indices kk >= KK, where
// the B rows are zero. A zero B row does not discard a NaN or an Inf
// (0 x NaN = NaN), so the last tile clears those A half-words first: the
// next window's (or the slack's) contents never reach a conv1 row. A finite
// value cleared this way contributed +-0 to an accumulator that starts at
// +0 and is never -0, so finite inputs give the same bits as without it.
// The mask also clears the window's OWN kk >= KK words, in the last tile
// only: a non-finite value late in a window still turns that window's rows
// of the earlier tiles into NaN (same patient's score; docs/PARITY.md).
// ---------------------------------------------------------------------------
#define TLAST_SLACK 256  // trailing bf16 elements required after the tensor
template <class G>
__global__ __launch_bounds__(WG_THREADS) void conv_stack_mfma_tlast_kernel(
    const unsigned short* __restrict__ x,   // (SN, L, CIN) bf16 bits
    float* __restrict__ feat,               // (SN, LIN)
    const float* __restrict__ wpack,
    const unsigned short* __restrict__ bfrag,  // [KSTEPS][64][8] bf16 bits
    int SN)
{
    __shared__ float lds_w[G::NW];
    __shared__ float lds_c1[WG_WAVES][4 * G::C1];
    __shared__ float lds_p1[WG_WAVES][4 * G::P1];
    __shared__ float lds_c2[WG_WAVES][G::C2];

    for (int i = threadIdx.x; i < G::NW; i += WG_THREADS) lds_w[i] = wpack[i];
    __syncthreads();

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const float* b1 = lds_w + G::OB1;

    bf16x8 bfr[G::KSTEPS];
    load_bfrags<G>(bfrag, lane, bfr);
    // per-lane fragment base within a window (dwords): rows l&15, k-group l>>4
    const int lane_dw = ((lane & 15) * G::CIN + (lane >> 4) * 8) / 2;
    __shared__ float lds_c1b[WG_WAVES][4 * G::C1];  // 2nd window of the pair
    // Last-tile A masks for the k-steps that reach past KK: dword q of step
    // st holds kk = st*32 + (lane>>4)*8 + 2q and kk + 1.
    constexpr int ST0 = G::KK / 32;   // first k-step with a kk >= KK
    unsigned int kmask[G::KSTEPS - ST0 > 0 ? G::KSTEPS - ST0 : 1][4];
    #pragma unroll
    for (int st = ST0; st < G::KSTEPS; ++st) {
        #pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kk = st * 32 + (lane >> 4) * 8 + 2 * q;
            kmask[st - ST0][q] = (kk < G::KK ? 0x0000ffffu : 0u)
                               | (kk + 1 < G::KK ? 0xffff0000u : 0u);
        }
    }

    // TWO windows per wave: the pair's MFMA/load chains are independent, so
    // the in-order wave covers one chain's global-load latency with the
    // other's MFMAs (the single-window chain was latency-exposed).
    for (long win = (blockIdx.x * WG_WAVES + wave) * 2; win < SN;
         win += (long)gridDim.x * WG_WAVES * 2) {
        const long win1 = win + 1;
        const bool has1 = win1 < SN;
        const unsigned int* xwa =
            (const unsigned int*)(x + win * (long)(G::L * G::CIN));
        const unsigned int* xwb =
            (const unsigned int*)(x + (has1 ? win1 : win) *
                                  (long)(G::L * G::CIN));
        #pragma unroll 1
        for (int mt = 0; mt < G::MTILES; ++mt) {
            f32x4 acca = {0.f, 0.f, 0.f, 0.f};
            f32x4 accb = {0.f, 0.f, 0.f, 0.f};
            const unsigned int* basea = xwa + (long)mt * (16 * G::CIN / 2)
                                        + lane_dw;
            const unsigned int* baseb = xwb + (long)mt * (16 * G::CIN / 2)
                                        + lane_dw;
            #pragma unroll
            for (int st = 0; st < G::KSTEPS; ++st) {
                BU aa, ab;
                aa.d[0] = basea[st * 16 + 0];
                aa.d[1] = basea[st * 16 + 1];
                aa.d[2] = basea[st * 16 + 2];
                aa.d[3] = basea[st * 16 + 3];
                ab.d[0] = baseb[st * 16 + 0];
                ab.d[1] = baseb[st * 16 + 1];
                ab.d[2] = baseb[st * 16 + 2];
                ab.d[3] = baseb[st * 16 + 3];
                if (st >= ST0 && mt == G::MTILES - 1) {   // uniform
                    #pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        aa.d[q] &= kmask[st - ST0][q];
                        ab.d[q] &= kmask[st - ST0][q];
                    }
                }
                acca = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aa.v, bfr[st],
                                                               acca, 0, 0, 0);
                accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ab.v, bfr[st],
                                                               accb, 0, 0, 0);
            }
            const int c = lane & 15;
            if (c < 4) {
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mt * 16 + (lane >> 4) * 4 + r;
                    if (row < G::C1) {
                        lds_c1[wave][c * G::C1 + row] = acca[r] + b1[c];
                        lds_c1b[wave][c * G::C1 + row] = accb[r] + b1[c];
                    }
                }
            }
        }
        wave_sync();
        conv_tail<G, true>(lane, lds_w, lds_c1[wave], lds_p1[wave],
                           lds_c2[wave], feat, win);
        if (has1)
            conv_tail<G, true>(lane, lds_w, lds_c1b[wave], lds_p1[wave],
                               lds_c2[wave], feat, win1);
    }
}

// ---------------------------------------------------------------------------
// Kernel 2: fused LSTM (batch-as-time) + Linear head + age gate (+sigmoid)
// (K6+K7+K8+K9 of SURVEY.md §2.6)
// ---------------------------------------------------------------------------
// Lane layout: lane l owns gate-unit row l of both LSTM layers, where rows
// 0-15 = input gate i, 16-31 = forget f, 32-47 = cell g, 48-63 = output o
// (PyTorch gate order) for hidden units u = l & 15.  After each step the
// full 16-wide h vectors are collected into per-lane register arrays with
// 16 independent shuffles, so the next step's h-dots are register FMAs.
template <class G>
__global__ __launch_bounds__(WG_THREADS) void lstm_head_kernel(
    const float* __restrict__ feat,  // (S, N, LIN)
    const float* __restrict__ age,   // (S, N) or nullptr
    float* __restrict__ out,         // (S, N)
    const float* __restrict__ wpack,
    int S, int N, float age_eps, int apply_sigmoid)
{
    constexpr int LIN = G::LIN;
    constexpr int CHUNK = 32;  // feature-prefetch steps (64 measured equal)
    constexpr int PRE_R = (CHUNK * LIN + WAVE - 1) / WAVE;  // regs per lane
    __shared__ float lds_feat[WG_WAVES][CHUNK * LIN];

    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int unit = lane & 15;

    // Per-lane weight rows -> registers (broadcast through L2; once).
    float wih1[LIN], whh1[16], wih2[16], whh2[16];
    const float bl1 = wpack[G::OBL1 + lane];
    const float bl2 = wpack[G::OBL2 + lane];
    #pragma unroll
    for (int i = 0; i < LIN; ++i) wih1[i] = wpack[G::OWIH1 + lane * LIN + i];
    #pragma unroll
    for (int i = 0; i < 16; ++i) {
        whh1[i] = wpack[G::OWHH1 + lane * 16 + i];
        wih2[i] = wpack[G::OWIH2 + lane * 16 + i];
        whh2[i] = wpack[G::OWHH2 + lane * 16 + i];
    }
    const float outb = wpack[G::OOUTB];
    const bool is_cell_gate = (lane >= 32 && lane < 48);

    float* fw = lds_feat[wave];

    for (long seq = blockIdx.x * WG_WAVES + wave; seq < S;
         seq += (long)gridDim.x * WG_WAVES) {
        const float* fseq = feat + seq * (long)N * LIN;
        const float* aseq = age ? age + seq * N : nullptr;
        float h1v[16], h2v[16];   // full h vectors, replicated per lane
        float c1 = 0.f, c2 = 0.f; // own-unit cell state
        #pragma unroll
        for (int u = 0; u < 16; ++u) h1v[u] = h2v[u] = 0.f;

        // Double-buffered chunk pipeline: chunk c+1's global loads are
        // ISSUED before chunk c's compute (their s_waitcnt lands at the LDS
        // write after the compute), so the scan never stalls on HBM latency
        // at chunk boundaries.
        const long ntot = (long)N * LIN;
        float pre[PRE_R];
        #pragma unroll
        for (int r = 0; r < PRE_R; ++r) {
            const long idx = (long)r * WAVE + lane;
            pre[r] = idx < ntot ? fseq[idx] : 0.f;
        }
        for (int t0 = 0; t0 < N; t0 += CHUNK) {
            const int tn = min(CHUNK, N - t0);
            #pragma unroll
            for (int r = 0; r < PRE_R; ++r) {
                const int j = r * WAVE + lane;
                if (j < CHUNK * LIN) fw[j] = pre[r];
            }
            wave_sync();
            if (t0 + CHUNK < N) {
                const long base = (long)(t0 + CHUNK) * LIN;
                #pragma unroll
                for (int r = 0; r < PRE_R; ++r) {
                    const long idx = base + (long)r * WAVE + lane;
                    pre[r] = idx < ntot ? fseq[idx] : 0.f;
                }
            }

            for (int tt = 0; tt < tn; ++tt) {
                const float* xt = fw + tt * LIN;
                // ----- layer 1: LIN-dim x-dot (LDS broadcast, 2 partial
                //       accumulators) + 16-dim h-dot (register FMA) -----
                float ga = bl1, gb = 0.f;
                #pragma unroll
                for (int i = 0; i < LIN; i += 2) {
                    ga = fmaf(wih1[i], xt[i], ga);
                    if (i + 1 < LIN) gb = fmaf(wih1[i + 1], xt[i + 1], gb);
                }
                #pragma unroll
                for (int u = 0; u < 16; u += 2) {
                    ga = fmaf(whh1[u], h1v[u], ga);
                    gb = fmaf(whh1[u + 1], h1v[u + 1], gb);
                }
                float g = ga + gb;
                float a = is_cell_gate ? tanhf_(g) : sigmoidf_(g);
                {
                    const float iu = __shfl(a, unit);
                    const float fu = __shfl(a, unit + 16);
                    const float gu = __shfl(a, unit + 32);
                    const float ou = __shfl(a, unit + 48);
                    c1 = fmaf(fu, c1, iu * gu);
                    const float h = ou * tanhf_(c1);
                    #pragma unroll
                    for (int u = 0; u < 16; ++u) h1v[u] = __shfl(h, u);
                }
                // ----- layer 2: both dots are register FMAs -----
                ga = bl2; gb = 0.f;
                #pragma unroll
                for (int u = 0; u < 16; u += 2) {
                    ga = fmaf(wih2[u], h1v[u], ga);
                    gb = fmaf(wih2[u + 1], h1v[u + 1], gb);
                    ga = fmaf(whh2[u], h2v[u], ga);
                    gb = fmaf(whh2[u + 1], h2v[u + 1], gb);
                }
                g = ga + gb;
                a = is_cell_gate ? tanhf_(g) : sigmoidf_(g);
                {
                    const float iu = __shfl(a, unit);
                    const float fu = __shfl(a, unit + 16);
                    const float gu = __shfl(a, unit + 32);
                    const float ou = __shfl(a, unit + 48);
                    c2 = fmaf(fu, c2, iu * gu);
                    const float h = ou * tanhf_(c2);
                    #pragma unroll
                    for (int u = 0; u < 16; ++u) h2v[u] = __shfl(h, u);
                }
                // ----- head (every lane has h2v: reduce-free dot) -----
                if (lane == 0) {
                    float y = outb;
                    #pragma unroll
                    for (int u = 0; u < 16; ++u)
                        y = fmaf(wpack[G::OOUTW + u], h2v[u], y);
                    const float ag = aseq ? aseq[t0 + tt] : 0.f;
                    y *= fmaxf(fmaf(ag, age_eps, 1.0f), 0.0f);
                    if (apply_sigmoid) y = sigmoidf_(y);
                    out[seq * N + t0 + tt] = y;
                }
            }
            wave_sync();  // before overwriting the feature chunk
        }
    }
}

// ---------------------------------------------------------------------------
// Kernel 3 (serving tail, B = 1, N = 1): window gather + conv stack + ONE
// LSTM step + head in one kernel, straight from the StreamEngine's fp32
// `proc` ring. Replaces window_gather_tlast2 -> conv_stack_mfma_tlast ->
// lstm_head for the one-window-per-stream trigger: the bf16 (120, C) window
// and the (S, LIN) feature tensor never touch global memory.
//
// Schedule = kernel 1c's: one wave per TWO streams, grid-stride. Per pair:
//   stage   lanes take consecutive t (coalesced per channel row of the
//           ring), RNE f32->bf16, two channels packed per dword store into
//           the per-wave time-major image xt[t*CIN + c] (row stride CIN/2
//           = 5 dwords: conflict-free). The window starts at
//           (end - 120) mod ring and wraps at most once.
//   conv1   kernel 1b's even-CIN MFMA im2col loop, A-fragments from LDS,
//           the pair's chains interleaved, one c1 row set per window.
//   tail    conv_tail<G, true> unchanged, its feature row pointed at LDS.
//           The pair shares one p1/c2/feature scratch, and that scratch
//           lives in window a's image, dead after the MFMA loop: 35.7 KB
//           of LDS per workgroup (MyCNN5) keeps 4 workgroups per CU. Every
//           hand-over between the image's two uses crosses a wave_sync().
//   lstm    lstm_head_kernel's lane layout and operation order for a single
//           step from h0 = c0 = 0: the whh FMAs and the f*c term are exact
//           zeros there and are omitted (whh1/whh2 are never loaded); every
//           kept term keeps its order, so results match the unfused chain.
// ---------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(WG_THREADS, 4) void serve_tail_kernel(
    const float* __restrict__ proc,   // (S, CIN, ring) fp32 processed ring
    const float* __restrict__ age,    // (S) or nullptr
    float* __restrict__ out,          // (S)
    const float* __restrict__ wpack,
    const unsigned short* __restrict__ bfrag,  // [KSTEPS][64][8] bf16 bits
    int S, int ring, long end_in, const long long* __restrict__ dstate,
    int end_extra, float age_eps, int apply_sigmoid)
{
    static_assert(G::CIN % 2 == 0, "packed staging needs an even CIN");
    static_assert(G::XTSZ % 8 == 0 && G::XTN % 2 == 0, "");
    constexpr int LIN = G::LIN;
    constexpr int CD  = G::CIN / 2;    // dwords per time-major row
    constexpr int XTD = G::XTSZ / 2;   // padded image, dwords
    __shared__ float lds_w[G::NW];
    __shared__ unsigned int lds_xt[WG_WAVES][2][XTD];
    __shared__ float lds_c1[WG_WAVES][2][4 * G::C1];
    // pool/conv2 scratch and the feature row live in window a's image, which
    // is dead once the MFMA loop has read it (and is restaged every pair)
    static_assert(4 * G::P1 + G::C2 + LIN <= G::XTN / 2, "scratch > image");

    for (int i = threadIdx.x; i < G::NW; i += WG_THREADS) lds_w[i] = wpack[i];
    __syncthreads();

    // wave index is uniform: say so, so ring rows and LDS bases are scalar
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const int unit = lane & 15;
    const float* b1 = lds_w + G::OB1;
    unsigned int* xta = lds_xt[wave][0];
    unsigned int* xtb = lds_xt[wave][1];
    float* c1a = lds_c1[wave][0];
    float* c1b = lds_c1[wave][1];
    float* p1w = (float*)xta;
    float* c2w = p1w + 4 * G::P1;
    float* fw = c2w + G::C2;

    bf16x8 bfr[G::KSTEPS];
    load_bfrags<G>(bfrag, lane, bfr);
    // LSTM / head rows (lane = gate row), once per wave. No whh blocks.
    float wih1[LIN], wih2[16], outw[16];
    const float bl1 = wpack[G::OBL1 + lane];
    const float bl2 = wpack[G::OBL2 + lane];
    #pragma unroll
    for (int i = 0; i < LIN; ++i) wih1[i] = wpack[G::OWIH1 + lane * LIN + i];
    #pragma unroll
    for (int i = 0; i < 16; ++i) {
        wih2[i] = wpack[G::OWIH2 + lane * 16 + i];
        outw[i] = wpack[G::OOUTW + i];   // uniform address
    }
    const float outb = wpack[G::OOUTB];
    const bool is_cell_gate = (lane >= 32 && lane < 48);

    // Ring position of the window (uniform): a short ring gives the all-
    // zero window, like the gather's `ok` predicate at B = 1.
    const long end = dstate ? (long)dstate[1] + end_extra : end_in;
    const bool full = end >= G::L;
    const int start = full ? (int)((end - G::L) % ring) : 0;

    // The A-fragment overread past t = L-1 lands in this zeroed tail of the
    // wave's own image; staging never writes it, so zero it once.
    for (int i = G::XTN / 2 + lane; i < XTD; i += WAVE) xta[i] = xtb[i] = 0u;

    // Per-lane byte offsets into a channel row for t = lane + 64*h.
    constexpr int NT = (G::L + WAVE - 1) / WAVE;
    unsigned int goff[NT];
    #pragma unroll
    for (int h = 0; h < NT; ++h) {
        unsigned int gi = start + lane + h * WAVE;
        if (gi >= (unsigned int)ring) gi -= ring;   // at most one wrap
        goff[h] = gi * 4u;
    }

    auto stage = [&](unsigned int* xt, long s, bool live) {
        // uniform row base + 32-bit lane offset; all loads issued first
        const char* pr = (const char*)(proc + s * ((long)G::CIN * ring));
        float v[NT][G::CIN];
        #pragma unroll
        for (int h = 0; h < NT; ++h) {
            #pragma unroll
            for (int c = 0; c < G::CIN; ++c) v[h][c] = 0.f;
        }
        if (live) {
            #pragma unroll
            for (int h = 0; h < NT; ++h) {
                if (lane + h * WAVE < G::L) {
                    #pragma unroll
                    for (int c = 0; c < G::CIN; ++c)
                        v[h][c] = *(const float*)(pr + (long)c * ring * 4
                                                  + goff[h]);
                }
            }
        }
        #pragma unroll
        for (int h = 0; h < NT; ++h) {
            if (lane + h * WAVE < G::L) {
                #pragma unroll
                for (int c = 0; c < G::CIN; c += 2)
                    xt[(lane + h * WAVE) * CD + (c >> 1)] =
                        (unsigned int)f32_to_bf16(v[h][c]) |
                        ((unsigned int)f32_to_bf16(v[h][c + 1]) << 16);
            }
        }
    };

    auto c1_store = [&](float* c1w, const f32x4& acc, int mt) {
        const int c = lane & 15;
        if (c < 4) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + (lane >> 4) * 4 + r;
                if (row < G::C1) c1w[c * G::C1 + row] = acc[r] + b1[c];
            }
        }
    };

    // One LSTM step from zero state + head for stream s (feature row in fw).
    auto lstm_step = [&](long s) {
        float h1v[16], h2v[16];
        float ga = bl1, gb = 0.f;
        #pragma unroll
        for (int i = 0; i < LIN; i += 2) {
            ga = fmaf(wih1[i], fw[i], ga);
            if (i + 1 < LIN) gb = fmaf(wih1[i + 1], fw[i + 1], gb);
        }
        float g = ga + gb;
        float a = is_cell_gate ? tanhf_(g) : sigmoidf_(g);
        {
            const float iu = __shfl(a, unit);
            const float gu = __shfl(a, unit + 32);
            const float ou = __shfl(a, unit + 48);
            const float h = ou * tanhf_(iu * gu);
            #pragma unroll
            for (int u = 0; u < 16; ++u) h1v[u] = __shfl(h, u);
        }
        ga = bl2; gb = 0.f;
        #pragma unroll
        for (int u = 0; u < 16; u += 2) {
            ga = fmaf(wih2[u], h1v[u], ga);
            gb = fmaf(wih2[u + 1], h1v[u + 1], gb);
        }
        g = ga + gb;
        a = is_cell_gate ? tanhf_(g) : sigmoidf_(g);
        {
            const float iu = __shfl(a, unit);
            const float gu = __shfl(a, unit + 32);
            const float ou = __shfl(a, unit + 48);
            const float h = ou * tanhf_(iu * gu);
            #pragma unroll
            for (int u = 0; u < 16; ++u) h2v[u] = __shfl(h, u);
        }
        if (lane == 0) {
            float y = outb;
            #pragma unroll
            for (int u = 0; u < 16; ++u) y = fmaf(outw[u], h2v[u], y);
            const float ag = age ? age[s] : 0.f;
            y *= fmaxf(fmaf(ag, age_eps, 1.0f), 0.0f);
            if (apply_sigmoid) y = sigmoidf_(y);
            out[s] = y;
        }
        wave_sync();  // feature-row reads done before the next tail's store
    };

    for (long win = (blockIdx.x * WG_WAVES + wave) * 2; win < S;
         win += (long)gridDim.x * WG_WAVES * 2) {
        const long win1 = win + 1;
        const bool has1 = win1 < S;
        stage(xta, win, full);
        stage(xtb, has1 ? win1 : win, full && has1);
        wave_sync();

        #pragma unroll 1
        for (int mt = 0; mt < G::MTILES; ++mt) {
            f32x4 acca = {0.f, 0.f, 0.f, 0.f};
            f32x4 accb = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int st = 0; st < G::KSTEPS; ++st) {
                // even element offset: aligned dwords are fragment dwords
                const int bd = ((mt * 16 + (lane & 15)) * G::CIN + st * 32
                                + (lane >> 4) * 8) / 2;
                BU aa, ab;
                #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    aa.d[q] = xta[bd + q];
                    ab.d[q] = xtb[bd + q];
                }
                acca = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    aa.v, bfr[st], acca, 0, 0, 0);
                accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    ab.v, bfr[st], accb, 0, 0, 0);
            }
            c1_store(c1a, acca, mt);
            c1_store(c1b, accb, mt);
        }
        wave_sync();  // both images are dead from here: scratch may land
        conv_tail<G, true>(lane, lds_w, c1a, p1w, c2w, fw, 0);
        lstm_step(win);
        if (has1) {
            conv_tail<G, true>(lane, lds_w, c1b, p1w, c2w, fw, 0);
            lstm_step(win1);
        }
    }
}

// ---------------------------------------------------------------------------
// Kernel 4 (channel attribution): occlusion scores of listed streams' latest
// windows straight from the ring. Variant 0 is the window as it stands (what
// serve_tail_kernel scores); variant k = 1..CIN has channel k-1 replaced for
// all 120 t by one constant: +0.0 (OCCLUDE_ZERO, "the channel never
// arrived") or the window's oldest point (OCCLUDE_HOLD, "the lead fell off
// ten minutes ago": the forward-fill carry). out is (n, CIN + 1).
//
// Schedule: the wave's pair of images is two variants of one stream, so the
// CIN + 1 = 11 variants take 6 rounds (the twelfth image is skipped). One
// wave per (listed stream, round) item, ONE flat grid-stride loop: a
// workgroup's 4 waves take consecutive rounds, mostly of the same stream, so
// HBM sees a stream's 4.8 KB window once and the other rounds read it from
// L1/L2. A round reads the window once (serve_tail_kernel's coalesced read
// and unwrap), packs it to bf16 pairs in 10 VGPRs and stages both images
// from those: the constant replaces fp32 ring values before the RNE
// conversion, which for one value is the conversion of that value, so only
// the occluded channel's half-word of a packed dword changes. conv1,
// conv_tail and the LSTM step are serve_tail_kernel's, operation for
// operation, and weights, biases and B fragments stay in registers across
// the loop. Keeping the packed window in registers across a stream's 6
// rounds (a round loop nested in the stream loop) was built first and
// spilled 56 B per lane at 128 VGPRs; the flat loop has serve_tail_kernel's
// shape and does not (126 VGPRs, MyCNN5).
//
// Tail<G> below holds serve_tail_kernel's pieces as functions. That kernel
// keeps its own in-place copies: built from these functions it computes the
// same values but the compiler allocates 128 instead of 123 VGPRs and
// schedules it differently (as with load_bfrags in kernel 1b), and its
// measured schedule is the one the serving step is tuned on.
// ---------------------------------------------------------------------------
#define OCCLUDE_HOLD 0
#define OCCLUDE_ZERO 1

template <class G>
struct Tail {
    static_assert(G::CIN % 2 == 0, "packed staging needs an even CIN");
    static_assert(G::XTSZ % 8 == 0 && G::XTN % 2 == 0, "");
    static constexpr int LIN = G::LIN;
    static constexpr int CD  = G::CIN / 2;    // dwords per time-major row
    static constexpr int XTD = G::XTSZ / 2;   // padded image, dwords
    static constexpr int NT  = (G::L + WAVE - 1) / WAVE;  // t's per lane
    // pool/conv2 scratch and the feature row live in window a's image, which
    // is dead once the MFMA loop has read it (and is restaged every pair)
    static_assert(4 * G::P1 + G::C2 + LIN <= G::XTN / 2, "scratch > image");

    // B fragments and LSTM / head rows (lane = gate row), once per wave. No
    // whh blocks.
    bf16x8 bfr[G::KSTEPS];
    float wih1[LIN], wih2[16], outw[16];
    float bl1, bl2, outb;

    __device__ __forceinline__ void load(const float* __restrict__ wpack,
                                         const unsigned short* bfrag,
                                         int lane) {
        load_bfrags<G>(bfrag, lane, bfr);
        bl1 = wpack[G::OBL1 + lane];
        bl2 = wpack[G::OBL2 + lane];
        #pragma unroll
        for (int i = 0; i < LIN; ++i)
            wih1[i] = wpack[G::OWIH1 + lane * LIN + i];
        #pragma unroll
        for (int i = 0; i < 16; ++i) {
            wih2[i] = wpack[G::OWIH2 + lane * 16 + i];
            outw[i] = wpack[G::OOUTW + i];   // uniform address
        }
        outb = wpack[G::OOUTB];
    }

    // Per-lane byte offsets into a channel row for t = lane + 64*h; the
    // window starts at ring slot `start` and wraps at most once.
    static __device__ __forceinline__ void ring_offsets(
        int start, int ring, int lane, unsigned int (&goff)[NT])
    {
        #pragma unroll
        for (int h = 0; h < NT; ++h) {
            unsigned int gi = start + lane + h * WAVE;
            if (gi >= (unsigned int)ring) gi -= ring;   // at most one wrap
            goff[h] = gi * 4u;
        }
    }

    // Stream s's window as packed bf16 pairs, pk[h][c/2] = channels c, c+1
    // at t = lane + 64*h (RNE): uniform row base + 32-bit lane offset, all
    // loads issued first. Not live: the all-zero window.
    static __device__ __forceinline__ void ring_load(
        const float* __restrict__ proc, long s, int ring,
        const unsigned int (&goff)[NT], int lane, bool live,
        unsigned int (&pk)[NT][CD])
    {
        const char* pr = (const char*)(proc + s * ((long)G::CIN * ring));
        float v[NT][G::CIN];
        #pragma unroll
        for (int h = 0; h < NT; ++h) {
            #pragma unroll
            for (int c = 0; c < G::CIN; ++c) v[h][c] = 0.f;
        }
        if (live) {
            #pragma unroll
            for (int h = 0; h < NT; ++h) {
                if (lane + h * WAVE < G::L) {
                    #pragma unroll
                    for (int c = 0; c < G::CIN; ++c)
                        v[h][c] = *(const float*)(pr + (long)c * ring * 4
                                                  + goff[h]);
                }
            }
        }
        #pragma unroll
        for (int h = 0; h < NT; ++h) {
            #pragma unroll
            for (int c = 0; c < G::CIN; c += 2)
                pk[h][c >> 1] =
                    (unsigned int)f32_to_bf16(v[h][c]) |
                    ((unsigned int)f32_to_bf16(v[h][c + 1]) << 16);
        }
    }

    // Packed window -> the time-major image xt[t*CIN + c] (row stride CD
    // dwords); the zeroed tail past t = L-1 is never written.
    static __device__ __forceinline__ void image_store(
        unsigned int* xt, int lane, const unsigned int (&pk)[NT][CD])
    {
        #pragma unroll
        for (int h = 0; h < NT; ++h) {
            if (lane + h * WAVE < G::L) {
                #pragma unroll
                for (int cd = 0; cd < CD; ++cd)
                    xt[(lane + h * WAVE) * CD + cd] = pk[h][cd];
            }
        }
    }

    static __device__ __forceinline__ void c1_store(
        float* c1w, const float* b1, const f32x4& acc, int mt, int lane)
    {
        const int c = lane & 15;
        if (c < 4) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + (lane >> 4) * 4 + r;
                if (row < G::C1) c1w[c * G::C1 + row] = acc[r] + b1[c];
            }
        }
    }

    // conv1 of the two images: kernel 1b's even-CIN MFMA im2col loop, the
    // pair's chains interleaved, one c1 row set per image.
    __device__ __forceinline__ void conv1_pair(
        const unsigned int* xta, const unsigned int* xtb, float* c1a,
        float* c1b, const float* b1, int lane) const
    {
        #pragma unroll 1
        for (int mt = 0; mt < G::MTILES; ++mt) {
            f32x4 acca = {0.f, 0.f, 0.f, 0.f};
            f32x4 accb = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int st = 0; st < G::KSTEPS; ++st) {
                // even element offset: aligned dwords are fragment dwords
                const int bd = ((mt * 16 + (lane & 15)) * G::CIN + st * 32
                                + (lane >> 4) * 8) / 2;
                BU aa, ab;
                #pragma unroll
                for (int q = 0; q < 4; ++q) {
                    aa.d[q] = xta[bd + q];
                    ab.d[q] = xtb[bd + q];
                }
                acca = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    aa.v, bfr[st], acca, 0, 0, 0);
                accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    ab.v, bfr[st], accb, 0, 0, 0);
            }
            c1_store(c1a, b1, acca, mt, lane);
            c1_store(c1b, b1, accb, mt, lane);
        }
    }

    // One LSTM step from zero state + head on the feature row fw; lane 0
    // reads age[ai] (age may be null) and writes out[oi].
    __device__ __forceinline__ void lstm_step(
        const float* fw, int lane, const float* __restrict__ age, long ai,
        float* __restrict__ out, long oi, float age_eps,
        int apply_sigmoid) const
    {
        const int unit = lane & 15;
        const bool is_cell_gate = (lane >= 32 && lane < 48);
        float h1v[16], h2v[16];
        float ga = bl1, gb = 0.f;
        #pragma unroll
        for (int i = 0; i < LIN; i += 2) {
            ga = fmaf(wih1[i], fw[i], ga);
            if (i + 1 < LIN) gb = fmaf(wih1[i + 1], fw[i + 1], gb);
        }
        float g = ga + gb;
        float a = is_cell_gate ? tanhf_(g) : sigmoidf_(g);
        {
            const float iu = __shfl(a, unit);
            const float gu = __shfl(a, unit + 32);
            const float ou = __shfl(a, unit + 48);
            const float h = ou * tanhf_(iu * gu);
            #pragma unroll
            for (int u = 0; u < 16; ++u) h1v[u] = __shfl(h, u);
        }
        ga = bl2; gb = 0.f;
        #pragma unroll
        for (int u = 0; u < 16; u += 2) {
            ga = fmaf(wih2[u], h1v[u], ga);
            gb = fmaf(wih2[u + 1], h1v[u + 1], gb);
        }
        g = ga + gb;
        a = is_cell_gate ? tanhf_(g) : sigmoidf_(g);
        {
            const float iu = __shfl(a, unit);
            const float gu = __shfl(a, unit + 32);
            const float ou = __shfl(a, unit + 48);
            const float h = ou * tanhf_(iu * gu);
            #pragma unroll
            for (int u = 0; u < 16; ++u) h2v[u] = __shfl(h, u);
        }
        if (lane == 0) {
            float y = outb;
            #pragma unroll
            for (int u = 0; u < 16; ++u) y = fmaf(outw[u], h2v[u], y);
            const float ag = age ? age[ai] : 0.f;
            y *= fmaxf(fmaf(ag, age_eps, 1.0f), 0.0f);
            if (apply_sigmoid) y = sigmoidf_(y);
            out[oi] = y;
        }
        wave_sync();  // feature-row reads done before the next tail's store
    }
};

template <class G>
__global__ __launch_bounds__(WG_THREADS, 4) void serve_tail_occlude_kernel(
    const float* __restrict__ proc,   // (S, CIN, ring) fp32 processed ring
    const int* __restrict__ sids,     // (n) stream ids
    const float* __restrict__ age,    // (n) or nullptr
    float* __restrict__ out,          // (n, CIN + 1)
    const float* __restrict__ wpack,
    const unsigned short* __restrict__ bfrag,  // [KSTEPS][64][8] bf16 bits
    int S, int n, int ring, long end, int baseline, float age_eps,
    int apply_sigmoid)
{
    using T = Tail<G>;
    constexpr int NV = G::CIN + 1;    // variants per stream
    __shared__ float lds_w[G::NW];
    __shared__ unsigned int lds_xt[WG_WAVES][2][T::XTD];
    __shared__ float lds_c1[WG_WAVES][2][4 * G::C1];

    for (int i = threadIdx.x; i < G::NW; i += WG_THREADS) lds_w[i] = wpack[i];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const float* b1 = lds_w + G::OB1;
    unsigned int* xta = lds_xt[wave][0];
    unsigned int* xtb = lds_xt[wave][1];
    float* c1a = lds_c1[wave][0];
    float* c1b = lds_c1[wave][1];
    float* p1w = (float*)xta;
    float* c2w = p1w + 4 * G::P1;
    float* fw = c2w + G::C2;

    T tw;
    tw.load(wpack, bfrag, lane);

    // the launcher guarantees L <= end and L <= ring: a full window
    const int start = (int)((end - G::L) % ring);
    for (int i = G::XTN / 2 + lane; i < T::XTD; i += WAVE)
        xta[i] = xtb[i] = 0u;
    unsigned int goff[T::NT];
    T::ring_offsets(start, ring, lane, goff);

    // Image of variant k from the packed window: channel occ = k - 1 (none
    // for k = 0) holds the baseline's bf16 bits `ins` in its half-word of
    // dword occ / 2. occ, keep and ins are uniform.
    auto stage = [&](unsigned int* xt, const unsigned int (&pk)[T::NT][T::CD],
                     const unsigned int (&pk0)[T::CD], int k) {
        const int occ = k - 1;
        const bool hi = occ & 1;
        unsigned int base = 0u;
        if (baseline == OCCLUDE_HOLD) {
            #pragma unroll
            for (int cd = 0; cd < T::CD; ++cd)
                if (cd == (occ >> 1)) base = pk0[cd];
        }
        const unsigned int keep = hi ? 0x0000ffffu : 0xffff0000u;
        const unsigned int ins = hi ? (base & 0xffff0000u) : (base & 0xffffu);
        unsigned int q[T::NT][T::CD];
        #pragma unroll
        for (int h = 0; h < T::NT; ++h) {
            #pragma unroll
            for (int cd = 0; cd < T::CD; ++cd)
                q[h][cd] = (occ >= 0 && cd == (occ >> 1))
                    ? ((pk[h][cd] & keep) | ins) : pk[h][cd];
        }
        T::image_store(xt, lane, q);
    };

    // One item = one round of one listed stream = variants ka, ka + 1.
    constexpr int NR = (NV + 1) / 2;
    for (long item = blockIdx.x * WG_WAVES + wave; item < (long)n * NR;
         item += (long)gridDim.x * WG_WAVES) {
        const long i = item / NR;
        const int ka = (int)(item % NR) * 2, kb = ka + 1;
        const bool hasb = kb < NV;
        // uniform: say so, so the ring row base is scalar
        const long s = __builtin_amdgcn_readfirstlane(sids[i]);
        if (s < 0 || s >= S) continue;    // the host refuses these ids
        unsigned int pk[T::NT][T::CD], pk0[T::CD];
        T::ring_load(proc, s, ring, goff, lane, true, pk);
        // the window's oldest point, t = 0, is lane 0's first row
        #pragma unroll
        for (int cd = 0; cd < T::CD; ++cd)
            pk0[cd] = __builtin_amdgcn_readfirstlane(pk[0][cd]);
        stage(xta, pk, pk0, ka);
        stage(xtb, pk, pk0, hasb ? kb : 0);
        wave_sync();

        tw.conv1_pair(xta, xtb, c1a, c1b, b1, lane);
        wave_sync();  // both images are dead from here: scratch may land
        conv_tail<G, true>(lane, lds_w, c1a, p1w, c2w, fw, 0);
        tw.lstm_step(fw, lane, age, i, out, i * NV + ka, age_eps,
                     apply_sigmoid);
        if (hasb) {
            conv_tail<G, true>(lane, lds_w, c1b, p1w, c2w, fw, 0);
            tw.lstm_step(fw, lane, age, i, out, i * NV + kb, age_eps,
                         apply_sigmoid);
        }
    }
}

// ---------------------------------------------------------------------------
// Kernel 5 (risk history): scores of listed streams at K past window
// positions straight from the ring. Column j is the window ending at
// e_j = end - (K-1-j)*stride (oldest first, the order of the window gather's
// batch axis), scored as serve_tail_kernel scores it at end = e_j: its own
// one-step sequence. Columns j < jmin reach below what the ring still holds;
// they get a quiet NaN and none of their addresses is formed. out is (n, K).
//
// Schedule: kernel 4's flat loop, the wave's pair of images being two
// consecutive columns of one stream: one wave per (listed stream, round)
// item, (K + 1) / 2 rounds per stream. Each image has its own ring read
// (uniform start, one compare-and-subtract wrap); at stride 12 two
// neighbouring windows share 108 of their 120 points and a workgroup's 4
// waves mostly take rounds of one stream, so L1/L2 serve the repeats. A
// round with one column below jmin stages the zero image for it
// (ring_load(live = false)) and skips its tail; a round with both below
// jmin only writes the NaNs. Odd K's last round has the newest column alone:
// its absent partner is a zero image without a tail, too.
// ---------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(WG_THREADS, 4) void serve_tail_history_kernel(
    const float* __restrict__ proc,   // (S, CIN, ring) fp32 processed ring
    const int* __restrict__ sids,     // (n) stream ids
    const float* __restrict__ age,    // (n) or nullptr
    float* __restrict__ out,          // (n, K)
    const float* __restrict__ wpack,
    const unsigned short* __restrict__ bfrag,  // [KSTEPS][64][8] bf16 bits
    int S, int n, int ring, long end, int K, int stride, int jmin,
    float age_eps, int apply_sigmoid)
{
    using T = Tail<G>;
    __shared__ float lds_w[G::NW];
    __shared__ unsigned int lds_xt[WG_WAVES][2][T::XTD];
    __shared__ float lds_c1[WG_WAVES][2][4 * G::C1];

    for (int i = threadIdx.x; i < G::NW; i += WG_THREADS) lds_w[i] = wpack[i];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const float* b1 = lds_w + G::OB1;
    unsigned int* xta = lds_xt[wave][0];
    unsigned int* xtb = lds_xt[wave][1];
    float* c1a = lds_c1[wave][0];
    float* c1b = lds_c1[wave][1];
    float* p1w = (float*)xta;
    float* c2w = p1w + 4 * G::P1;
    float* fw = c2w + G::C2;

    T tw;
    tw.load(wpack, bfrag, lane);

    for (int i = G::XTN / 2 + lane; i < T::XTD; i += WAVE)
        xta[i] = xtb[i] = 0u;

    // The launcher guarantees L <= e_jmin, (K-1)*stride < 2^30 and ring <=
    // 2^29: the newest window's start slot, and per column the distance back
    // from it, are 32-bit.
    const int start_new = (int)((end - G::L) % ring);
    const float qnan = __builtin_nanf("");

    // One item = one round of one listed stream = columns ja, ja + 1.
    const int NR = (K + 1) / 2;
    for (long item = blockIdx.x * WG_WAVES + wave; item < (long)n * NR;
         item += (long)gridDim.x * WG_WAVES) {
        const long i = item / NR;
        const int ja = (int)(item % NR) * 2, jb = ja + 1;
        const bool hasb = jb < K;
        const bool livea = ja >= jmin, liveb = hasb && jb >= jmin;
        // uniform: say so, so the ring row base is scalar
        const long s = __builtin_amdgcn_readfirstlane(sids[i]);
        if (s < 0 || s >= S) continue;    // the host refuses these ids
        // jmin <= K - 1 and the unavailable columns are a prefix: a round
        // without a live column has both, and a live a has a live b or none
        if (!livea && !liveb) {
            if (lane == 0) out[i * K + ja] = out[i * K + jb] = qnan;
            continue;
        }
        // slot of a live column's oldest point; 0 for one that is not live
        // (nothing is read through its offsets)
        auto start_of = [&](int j, bool live) {
            if (!live) return 0;
            const int back = (int)((unsigned int)((K - 1 - j) * stride)
                                   % (unsigned int)ring);
            const int st = start_new - back;
            return st < 0 ? st + ring : st;
        };
        // image a is staged completely before image b's offsets are formed:
        // with both reads issued first the 40 loads are hoisted together
        // and MyCNN5 spills 3 VGPRs at the 128 of these launch bounds
        auto stage = [&](unsigned int* xt, int j, bool live) {
            unsigned int goff[T::NT], pk[T::NT][T::CD];
            T::ring_offsets(start_of(j, live), ring, lane, goff);
            T::ring_load(proc, s, ring, goff, lane, live, pk);
            T::image_store(xt, lane, pk);
        };
        stage(xta, ja, livea);
        stage(xtb, jb, liveb);
        wave_sync();

        tw.conv1_pair(xta, xtb, c1a, c1b, b1, lane);
        wave_sync();  // both images are dead from here: scratch may land
        if (livea) {
            conv_tail<G, true>(lane, lds_w, c1a, p1w, c2w, fw, 0);
            tw.lstm_step(fw, lane, age, i, out, i * K + ja, age_eps,
                         apply_sigmoid);
        } else if (lane == 0) {
            out[i * K + ja] = qnan;
        }
        if (liveb) {
            conv_tail<G, true>(lane, lds_w, c1b, p1w, c2w, fw, 0);
            tw.lstm_step(fw, lane, age, i, out, i * K + jb, age_eps,
                         apply_sigmoid);
        }
    }
}

// ---------------------------------------------------------------------------
// Debug: one 16x16x32 bf16 MFMA tile (fragment-map ground truth for tests)
// ---------------------------------------------------------------------------
__global__ void debug_mfma_kernel(const unsigned short* __restrict__ A,
                                  const unsigned short* __restrict__ B,
                                  float* __restrict__ C) {
    const int lane = threadIdx.x;
    BU a, b;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = (lane >> 4) * 8 + j;
        a.u[j] = A[(lane & 15) * 32 + k];   // A[row][k], row-major 16x32
        b.u[j] = B[k * 16 + (lane & 15)];   // B[k][col], row-major 32x16
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
    #pragma unroll
    for (int r = 0; r < 4; ++r)
        C[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

// ---------------------------------------------------------------------------
// extern "C" launchers (ctypes API; stream owned by caller -> hipGraph-safe)
// ---------------------------------------------------------------------------
namespace {

template <class G>
int launch_conv(const void* x, int x_is_bf16, int x_timelast, float* feat,
                const float* wpack, const void* bfrag, int SN,
                hipStream_t stream) {
    if (SN <= 0) return 0;
    int grid = (SN + WG_WAVES - 1) / WG_WAVES;
    if (grid > 8192) grid = 8192;
    if (x_is_bf16) {
        if (!bfrag) return -2;  // bf16 path requires packed B fragments
        if (x_timelast) {
            if constexpr (G::CIN % 2 == 0) {
                // one wave per two windows
                int g1 = (SN / 2 + WG_WAVES - 1) / WG_WAVES;
                if (g1 < 1) g1 = 1;
                if (g1 > 8192) g1 = 8192;
                hipLaunchKernelGGL((conv_stack_mfma_tlast_kernel<G>),
                                   dim3(g1), dim3(WG_THREADS), 0, stream,
                                   (const unsigned short*)x, feat, wpack,
                                   (const unsigned short*)bfrag, SN);
                return (int)hipGetLastError();
            }
            return -4;  // odd-CIN variants: use the staged layout
        }
        hipLaunchKernelGGL((conv_stack_mfma_kernel<G>), dim3(grid),
                           dim3(WG_THREADS), 0, stream,
                           (const unsigned short*)x, feat, wpack,
                           (const unsigned short*)bfrag, SN);
    } else {
        if (x_timelast) return -4;  // fp32 path is (C, L) only
        hipLaunchKernelGGL((conv_stack_kernel<G>), dim3(grid),
                           dim3(WG_THREADS), 0, stream, (const float*)x, feat,
                           wpack, SN);
    }
    return (int)hipGetLastError();
}

template <class G>
int launch_lstm(const float* feat, const float* age, float* out,
                const float* wpack, int S, int N, float age_eps,
                int apply_sigmoid, hipStream_t stream) {
    if (S <= 0 || N <= 0) return 0;
    int grid = (S + WG_WAVES - 1) / WG_WAVES;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL((lstm_head_kernel<G>), dim3(grid), dim3(WG_THREADS), 0,
                       stream, feat, age, out, wpack, S, N, age_eps,
                       apply_sigmoid);
    return (int)hipGetLastError();
}

// Fused serving tail: even-CIN variants whose CIN equals the ring's channel
// count; anything else is SERVE_TAIL_UNSUPPORTED and launches nothing.
#define SERVE_TAIL_UNSUPPORTED (-6)
template <class G>
int launch_serve_tail(const float* proc, int S, int C, int ring, long end_in,
                      const long long* dstate, int end_extra,
                      const float* age, float* out, const float* wpack,
                      const void* bfrag, float age_eps, int apply_sigmoid,
                      hipStream_t stream) {
    if constexpr (G::CIN % 2 != 0) {
        return SERVE_TAIL_UNSUPPORTED;
    } else {
        if (C != G::CIN) return SERVE_TAIL_UNSUPPORTED;
        // a window must fit the ring; row byte offsets are 32-bit
        if (ring < G::L || ring > (1 << 29)) return -5;
        if (!bfrag) return -2;
        if (S <= 0) return 0;
        // grid as launch_conv's 1-wave-per-2-windows branch
        int g1 = (S / 2 + WG_WAVES - 1) / WG_WAVES;
        if (g1 < 1) g1 = 1;
        if (g1 > 8192) g1 = 8192;
        hipLaunchKernelGGL((serve_tail_kernel<G>), dim3(g1),
                           dim3(WG_THREADS), 0, stream, proc, age, out, wpack,
                           (const unsigned short*)bfrag, S, ring, end_in,
                           dstate, end_extra, age_eps, apply_sigmoid);
        return (int)hipGetLastError();
    }
}

// Channel attribution: serve_tail's coverage and codes; a window end before
// the first full window is -5 as well, an unknown baseline -7.
template <class G>
int launch_serve_tail_occlude(const float* proc, int S, int C, int ring,
                              long end, const int* sids, int n,
                              const float* age, int baseline, float* out,
                              const float* wpack, const void* bfrag,
                              float age_eps, int apply_sigmoid,
                              hipStream_t stream) {
    if constexpr (G::CIN % 2 != 0) {
        return SERVE_TAIL_UNSUPPORTED;
    } else {
        if (C != G::CIN) return SERVE_TAIL_UNSUPPORTED;
        if (ring < G::L || ring > (1 << 29) || end < G::L) return -5;
        if (baseline != OCCLUDE_HOLD && baseline != OCCLUDE_ZERO) return -7;
        if (!bfrag) return -2;
        if (n <= 0) return 0;
        // one wave per (stream, round of two variants)
        const long items = (long)n * ((G::CIN + 2) / 2);
        const int g1 = (int)((items < 4 * 8192L ? items : 4 * 8192L)
                             + WG_WAVES - 1) / WG_WAVES;
        hipLaunchKernelGGL((serve_tail_occlude_kernel<G>), dim3(g1),
                           dim3(WG_THREADS), 0, stream, proc, sids, age, out,
                           wpack, (const unsigned short*)bfrag, S, n, ring,
                           end, baseline, age_eps, apply_sigmoid);
        return (int)hipGetLastError();
    }
}

// Risk history: serve_tail's coverage and codes. -5 as well for a column
// geometry the kernel's 32-bit slot arithmetic does not take and for a jmin
// whose column would read an overwritten or negative ring position.
template <class G>
int launch_serve_tail_history(const float* proc, int S, int C, int ring,
                              long end, const int* sids, int n,
                              const float* age, int K, int stride, int jmin,
                              float* out, const float* wpack,
                              const void* bfrag, float age_eps,
                              int apply_sigmoid, hipStream_t stream) {
    if constexpr (G::CIN % 2 != 0) {
        return SERVE_TAIL_UNSUPPORTED;
    } else {
        if (C != G::CIN) return SERVE_TAIL_UNSUPPORTED;
        if (ring < G::L || ring > (1 << 29)) return -5;
        if (K < 1 || stride < 1 || (long)(K - 1) * stride >= (1L << 30))
            return -5;
        if (jmin < 0 || jmin > K - 1) return -5;
        const long lo = end - ring > 0 ? end - ring : 0;
        if (end - (long)(K - 1 - jmin) * stride - G::L < lo) return -5;
        if (!bfrag) return -2;
        if (n <= 0) return 0;
        // one wave per (stream, round of two columns)
        const long items = (long)n * ((K + 1) / 2);
        const int g1 = (int)((items < 4 * 8192L ? items : 4 * 8192L)
                             + WG_WAVES - 1) / WG_WAVES;
        hipLaunchKernelGGL((serve_tail_history_kernel<G>), dim3(g1),
                           dim3(WG_THREADS), 0, stream, proc, sids, age, out,
                           wpack, (const unsigned short*)bfrag, S, n, ring,
                           end, K, stride, jmin, age_eps, apply_sigmoid);
        return (int)hipGetLastError();
    }
}

}  // namespace

extern "C" {

// variant (everywhere below): 0 = MyCNN5, 1 = MyCNN2/3, 2 = MyCNN4

// Scores (n, K) of the listed streams at K window positions of the (S, C, G)
// fp32 ring: column j ends at end - (K-1-j)*stride; columns below jmin are
// NaN and read nothing; age is (n) or null.
int tskd_serve_tail_history_fwd(const float* proc, int S, int C, int G,
                                long end, const int* sids, int n,
                                const float* age, int K, int stride, int jmin,
                                float* out, const float* wpack,
                                const void* bfrag, float age_eps,
                                int apply_sigmoid, int variant,
                                void* stream) {
    return dispatch_variant(variant, [&](auto g) {
        return launch_serve_tail_history<typename decltype(g)::type>(
            proc, S, C, G, end, sids, n, age, K, stride, jmin, out, wpack,
            bfrag, age_eps, apply_sigmoid, (hipStream_t)stream);
    });
}

// Occlusion scores (n, C + 1) of the listed streams' latest windows ending at
// `end` in the (S, C, G) fp32 ring; baseline 0 = hold, 1 = zero; age is (n)
// or null.
int tskd_serve_tail_occlude_fwd(const float* proc, int S, int C, int G,
                                long end, const int* sids, int n,
                                const float* age, int baseline, float* out,
                                const float* wpack, const void* bfrag,
                                float age_eps, int apply_sigmoid, int variant,
                                void* stream) {
    return dispatch_variant(variant, [&](auto g) {
        return launch_serve_tail_occlude<typename decltype(g)::type>(
            proc, S, C, G, end, sids, n, age, baseline, out, wpack, bfrag,
            age_eps, apply_sigmoid, (hipStream_t)stream);
    });
}

// Window gather + conv + one LSTM step + head from the (S, C, G) fp32 ring;
// end = dstate ? dstate[1] + end_extra : end_in (as in the window gather).
int tskd_serve_tail_fwd(const float* proc, int S, int C, int G, long end_in,
                        const long long* dstate, int end_extra,
                        const float* age, float* out, const float* wpack,
                        const void* bfrag, float age_eps, int apply_sigmoid,
                        int variant, void* stream) {
    return dispatch_variant(variant, [&](auto g) {
        return launch_serve_tail<typename decltype(g)::type>(
            proc, S, C, G, end_in, dstate, end_extra, age, out, wpack, bfrag,
            age_eps, apply_sigmoid, (hipStream_t)stream);
    });
}

int tskd_conv_fwd(const void* x, int x_is_bf16, int x_timelast, float* feat,
                  const float* wpack, const void* bfrag, int SN, int variant,
                  void* stream) {
    return dispatch_variant(variant, [&](auto g) {
        return launch_conv<typename decltype(g)::type>(
            x, x_is_bf16, x_timelast, feat, wpack, bfrag, SN,
            (hipStream_t)stream);
    });
}

int tskd_lstm_head_fwd(const float* feat, const float* age, float* out,
                       const float* wpack, int S, int N, float age_eps,
                       int apply_sigmoid, int variant, void* stream) {
    return dispatch_variant(variant, [&](auto g) {
        return launch_lstm<typename decltype(g)::type>(
            feat, age, out, wpack, S, N, age_eps, apply_sigmoid,
            (hipStream_t)stream);
    });
}

int tskd_debug_mfma16x16x32(const unsigned short* A, const unsigned short* B,
                            float* C, void* stream) {
    hipLaunchKernelGGL(debug_mfma_kernel, dim3(1), dim3(WAVE), 0,
                       (hipStream_t)stream, A, B, C);
    return (int)hipGetLastError();
}

int tskd_pack_size(int variant) {
    return dispatch_variant(
        variant, [](auto g) { return decltype(g)::type::NPACK; });
}

int tskd_feat_len(int variant) {
    return dispatch_variant(
        variant, [](auto g) { return decltype(g)::type::LIN; });
}

// MFMA B-fragment pack geometry for python (ksteps per variant).
int tskd_conv_ksteps(int variant) {
    return dispatch_variant(
        variant, [](auto g) { return decltype(g)::type::KSTEPS; });
}

}  // extern "C"
