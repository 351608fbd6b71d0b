// Pieces shared by the three HIP libraries (mycnn / preprocess / train):
// model geometry and packed-parameter layout, the same-wave LDS fence, the
// fast activations, bf16 conversion and the variant dispatch.
#pragma once

#include <hip/hip_runtime.h>

#define WAVE 64  // wavefront size on CDNA4 — all lane math assumes it

// ---------------------------------------------------------------------------
// Geometry per model variant (lengths from SURVEY.md §2.3 forward semantics)
// ---------------------------------------------------------------------------
template <int CIN_, int K1_, int PK_, int PS_, int L_ = 120>
struct Geom {
    static constexpr int CIN = CIN_;
    static constexpr int K1  = K1_;
    static constexpr int PK  = PK_;
    static constexpr int PS  = PS_;
    static constexpr int L   = L_;
    static constexpr int C1  = L - K1 + 1;            // conv1 out len
    static constexpr int P1  = (C1 - PK) / PS + 1;    // pool1 out len
    static constexpr int C2  = P1 - 5 + 1;            // conv2 out len (k=5)
    static constexpr int LIN = (C2 - PK) / PS + 1;    // pool2 out len = LSTM in
    // MFMA im2col geometry
    static constexpr int KK     = CIN * K1;           // reduction length
    static constexpr int KSTEPS = (KK + 31) / 32;     // mfma k-steps (K=32)
    static constexpr int MTILES = (C1 + 15) / 16;     // 16-row output tiles
    static constexpr int XTN    = CIN * L;            // transposed window elems
    static constexpr int XTSZ   = ((MTILES * 16 - 1) * CIN + KSTEPS * 32 + 7)
                                  / 8 * 8;            // padded LDS extent
    // fp32 weight-pack offsets (must match tskd_amd/ops/pack.py)
    static constexpr int OW1   = 0;                   // [4][CIN][K1]
    static constexpr int OB1   = OW1 + 4 * CIN * K1;  // [4]
    static constexpr int OW2   = OB1 + 4;             // [4][5]
    static constexpr int OB2   = OW2 + 20;            // [1]
    static constexpr int NW    = OB2 + 1;             // conv-stack words
    static constexpr int OWIH1 = OB2 + 1;             // [64][LIN]
    static constexpr int OWHH1 = OWIH1 + 64 * LIN;    // [64][16]
    static constexpr int OBL1  = OWHH1 + 64 * 16;     // [64] (b_ih + b_hh)
    static constexpr int OWIH2 = OBL1 + 64;           // [64][16]
    static constexpr int OWHH2 = OWIH2 + 64 * 16;     // [64][16]
    static constexpr int OBL2  = OWHH2 + 64 * 16;     // [64]
    static constexpr int OOUTW = OBL2 + 64;           // [16]
    static constexpr int OOUTB = OOUTW + 16;          // [1]
    static constexpr int NPACK = OOUTB + 1;
    // training conv stash layout (per window, fp32/int32 words)
    static constexpr int SC_C1T = 0;                 // [4*C1] tanh(conv1)
    static constexpr int SC_C2T = SC_C1T + 4 * C1;   // [C2]  tanh(conv2)
    static constexpr int SC_I1 = SC_C2T + C2;        // [4*P1] pool1 argmax
    static constexpr int SC_I2 = SC_I1 + 4 * P1;     // [LIN] pool2 argmax
    static constexpr int SC_M1 = SC_I2 + LIN;        // [4*P1] dropout1 mult
    static constexpr int SC_M2 = SC_M1 + 4 * P1;     // [LIN] dropout2 mult
    static constexpr int SC_SIZE = SC_M2 + LIN;
    // training lstm stash layout (per step, fp32 words)
    static constexpr int SL_A1 = 0;    // [64] layer1 activated gates
    static constexpr int SL_C1 = 64;   // [16]
    static constexpr int SL_H1 = 80;   // [16]
    static constexpr int SL_A2 = 96;   // [64]
    static constexpr int SL_C2 = 160;  // [16]
    static constexpr int SL_H2 = 176;  // [16]
    static constexpr int SL_SIZE = 192;
};

using GeomCNN5 = Geom<10, 10, 3, 2>;  // MyCNN5: 111/55/51/25
using GeomCNN2 = Geom<7, 5, 2, 2>;    // MyCNN2/3: 116/58/54/27
using GeomCNN4 = Geom<10, 5, 2, 2>;   // MyCNN4: same lens as CNN2, 10 ch

static_assert(GeomCNN5::LIN == 25, "MyCNN5 feature length must be 25");
static_assert(GeomCNN2::LIN == 27, "MyCNN2 feature length must be 27");
static_assert(GeomCNN5::KSTEPS == 4 && GeomCNN2::KSTEPS == 2, "");

// variant: 0 = MyCNN5, 1 = MyCNN2/3, 2 = MyCNN4. Calls f(GeomTag<G>{}) for
// the variant's geometry and returns its result; -1 for an unknown variant.
template <class G> struct GeomTag { using type = G; };

template <class F>
inline int dispatch_variant(int variant, F&& f) {
    switch (variant) {
        case 0: return f(GeomTag<GeomCNN5>{});
        case 1: return f(GeomTag<GeomCNN2>{});
        case 2: return f(GeomTag<GeomCNN4>{});
    }
    return -1;
}

// Same-wave LDS read-after-write fence: LDS ops of one wave complete in
// order once lgkmcnt drains; the asm "memory" clobber stops compiler
// reordering, wave_barrier stops scheduler migration across it.
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float sigmoidf_(float x) {
    return 1.0f / (1.0f + __expf(-x));
}

__device__ __forceinline__ float tanhf_(float x) {
    // tanh(x) = 2*sigmoid(2x) - 1; fast-exp based, fp32-accurate to ~1e-7 rel.
    return 2.0f / (1.0f + __expf(-2.0f * x)) - 1.0f;
}

__device__ __forceinline__ float bf16_to_f32(unsigned short u) {
    union { unsigned int i; float f; } v;
    v.i = ((unsigned int)u) << 16;
    return v.f;
}

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    union { float f; unsigned int i; } u;
    u.f = f;
    const unsigned int r = u.i + 0x7fffu + ((u.i >> 16) & 1);  // RNE
    return (unsigned short)(r >> 16);
}
