// Fused streaming-preprocess kernels — CDNA4 (gfx950) HIP.
//
// Replaces the reference's Spark Structured Streaming stage (reference
// bin/processStream.py:105-218 + predictStream.py window assembly :96-142;
// SURVEY.md §2.6 K13) with GPU-resident per-(stream, channel) ring buffers
// and three kernels:
//
//   1. ingest_dense / ingest_events: raw samples -> 5-s bucket (sum, count).
//      Dense path: one wavefront per bucket, coalesced strided loads +
//      wave shuffle reduction. Sparse path (irregular event batches, the
//      real numerics records at fs=1/60 Hz): atomicAdd into buckets.
//      Both have a GATED instantiation (signal-quality gate): per-channel
//      plausibility bounds, rejected samples counted into rej (S, C) int64.
//
//   2. window_fill: the Spark groupBy(key, channel, window(180 s, 5 s))
//      .agg(avg) — a window STARTING at grid g covers buckets [g, g+36) and
//      its average is sum(raw)/count(raw) over those buckets — followed by
//      the reference's ffill -> bfill -> fillna(0) (processStream.py:114-123).
//      ffill carries state ACROSS trigger batches (documented improvement
//      over the reference, whose ffill restarts per 60-s micro-batch).
//
//   3. window_gather: assemble model windows (S, B, C, 120) from the last
//      120 processed grid points per stream (predictStream.py's 600 s/60 s
//      window -> (1, 10, 120) tensor), batched B windows back at a given
//      grid stride. Missing channels come out zero (never-filled grid = 0).
//
// Ring-buffer layout (all fp32, indexed mod G):
//   bsum, bcnt : (S, C, G)  raw-sample sum / count per 5-s bucket
//   proc       : (S, C, G)  processed (filled) window averages by START grid
//   last_val   : (S, C)     ffill carry (NaN = no value seen yet)
// Head indices live on the host (python StreamEngine); kernels take them as
// arguments so the whole trigger step can be captured in a hipGraph.

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <math.h>

#include "tskd_common.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_;
typedef __attribute__((ext_vector_type(4))) float f32x4_;

// Device-resident ring indices (hipGraph mode): dstate[0]=head,
// dstate[1]=nproc. A null dstate falls back to the host-passed values.
__device__ __forceinline__ long ring_head(const long long* dstate, long h) {
    return dstate ? (long)dstate[0] : h;
}
__device__ __forceinline__ long ring_nproc(const long long* dstate, long p) {
    return dstate ? (long)dstate[1] : p;
}

__global__ void advance_state_kernel(long long* dstate, int nb, int np) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        dstate[0] += nb;
        dstate[1] += np;
    }
}

typedef float f32x2p_ __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------
// 1a. Dense ingest: raw (S, CIN, T) -> NB = T/bucket_len new buckets/channel
// ---------------------------------------------------------------------------
// One wave processes FOUR consecutive buckets of one (stream, channel) row
// in 16-lane groups — a 625-sample bucket is 78 oct-loads, so a whole-wave
// bucket wastes 39% of lanes on the ragged tail; 16-lane groups keep ~95%
// busy (78/16 = 4.9 balanced iterations per group).
#define ING_GRP 4   // buckets per wave
#define ING_GL 16   // lanes per bucket group

// One sample into a lane's accumulators. Ungated: present iff not NaN.
// GATED (signal-quality gate, docs/PARITY.md divergence 15): accepted iff
// lo <= f <= hi in fp32 — false for NaN, and with infinite bounds true for
// exactly the samples !isnan accepts, ±inf included. A sample that is
// neither accepted nor NaN is rejected: it reaches neither sum nor cnt and
// adds 1 to rej.
template <bool GATED>
__device__ __forceinline__ void ingest_acc(float f, float lo, float hi,
                                           float& sum, float& cnt, int& rej) {
    if constexpr (GATED) {
        // selects, not branches: a rejected sample adds +0 (sum never
        // holds -0, so that leaves it bit for bit alone) and the kernel
        // stays straight-line code
        const bool acc = (lo <= f) & (f <= hi);
        sum += acc ? f : 0.f;
        cnt += acc ? 1.f : 0.f;
        rej += (int)(!acc & !isnan(f));
    } else {
        if (!isnan(f)) { sum += f; cnt += 1.f; }
    }
}

// Both dense kernels. The gate's two arguments travel as a parameter pack
// (empty when !GATED), so the ungated instantiation keeps the argument list
// and the code it had before the gate existed. GATED adds: the row's bounds
// (by wire channel, wave-uniform: a wave's four buckets share one (s, cin)
// row) loaded once per task, a third per-lane accumulator reduced over the
// wave (its four bucket groups count into the same rej[s, c]), and ONE 64-bit
// atomicAdd per task into rej[s, c], issued by lane 0 and only when the wave
// rejected something — a clean stream costs no atomics. Every mask that
// keeps a sample out of sum/cnt (boundary chunks, the tensor-final scalar
// tail) keeps it out of rej: all three go through ingest_acc.
__device__ __forceinline__ const float* gate_bounds(const float* b,
                                                    long long*) { return b; }
__device__ __forceinline__ long long* gate_rej(const float*, long long* r) {
    return r;
}

template <class DT, bool GATED, class... GA>
__global__ void ingest_dense_kernel(
    const DT* __restrict__ raw,     // (S, CIN, T)
    float* __restrict__ bsum,       // (S, C, G), element stride BST
    float* __restrict__ bcnt,       // (= bsum+1 when packed (sum,cnt) pairs)
    const int* __restrict__ chan_map,  // (CIN) raw row -> wire channel
    int S, int CIN, int C, int T, int G,
    int bucket_len, long head_in,   // buckets written at [head, head+NB)
    const long long* __restrict__ dstate, int BST,
    GA... gate)  // GATED: const float* bounds (C, 2), long long* rej (S, C)
{
    const long head = ring_head(dstate, head_in);
    const int head_mod = (int)(head % G);  // hoisted: no 64-bit mod per task
    const int NB = T / bucket_len;
    const int NBG = (NB + ING_GRP - 1) / ING_GRP;
    const long nwaves = (long)S * CIN * NBG;
    const int wlane = threadIdx.x % WAVE;
    const int grp = wlane / ING_GL;     // which of the wave's 4 buckets
    const int lane = wlane % ING_GL;    // lane within the bucket group
    for (long w = (long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
         w < nwaves; w += (long)gridDim.x * (blockDim.x / WAVE)) {
        // 32-bit decode: nwaves < 2^31 in any real config; 64-bit div/mod
        // per task measured as a visible fraction of the wave's cycle
        // budget (12 tasks x ~5 KB each)
        const int wi = (int)w;
        const int bg = wi % NBG;
        const int wrem = wi / NBG;
        const int cin = wrem % CIN;
        const int s = wrem / CIN;
        const int b = bg * ING_GRP + grp;
        const bool active = b < NB;
        const DT* src = raw + ((long)s * CIN + cin) * T +
                        (long)(active ? b : 0) * bucket_len;
        float sum = 0.f, cnt = 0.f;
        float lo = 0.f, hi = 0.f;
        int rej = 0, cg = 0;
        if constexpr (GATED) {
            // the row is the wave's: say so, and channel and bounds come
            // through the scalar cache into scalar registers
            const float* bounds = gate_bounds(gate...);
            cg = chan_map[__builtin_amdgcn_readfirstlane(cin)];
            lo = bounds[2 * cg];
            hi = bounds[2 * cg + 1];
        }
        // 16B-aligned vector body (bucket offsets like 625 samples are not
        // 16B-aligned): bf16 masks the boundary chunks, fp32 peels them.
        if (active) {
            if constexpr (sizeof(DT) == 2) {
                // peel-free: cover the bucket with ALIGNED oct-chunks and
                // mask the (at most two) boundary chunks in-register —
                // removes both scalar peel loops per bucket
                const unsigned short* su = (const unsigned short*)src;
                const int mis = (int)(((size_t)su & 15) / 2);  // elems before
                const u32x4_* vp = (const u32x4_*)(su - mis);
                // ceil: the final partial chunk is loaded and masked
                // in-register (measured 4% faster than a scalar tail) —
                // EXCEPT for the very last bucket of the whole tensor,
                // where the <= 14 B over-read would pass the allocation:
                // that one task floors the chunk count and takes the
                // scalar tail. When mis + bucket_len < 8 the floor is 0
                // chunks and the tail is the whole bucket: it starts at
                // sample 0, never before it. The masked head read-back
                // (<= 14 B before the bucket) stays inside the raw tensor
                // for every bucket but (0,0,0), where it stays inside the
                // aligned 16 B chunk that holds the tensor's first sample
                // (mis = 0 when the tensor starts its allocation).
                const bool at_end = s == S - 1 && cin == CIN - 1 &&
                                    b == NB - 1;
                const int nch = (mis + bucket_len + (at_end ? 0 : 7)) / 8;
                for (int base = lane; base < nch; base += 5 * ING_GL) {
                    union { u32x4_ q; unsigned short h[8]; } v[5];
                    #pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        const int pp = base + u * ING_GL;
                        v[u].q = __builtin_nontemporal_load(
                            &vp[pp < nch ? pp : 0]);
                    }
                    #pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        const int pp = base + u * ING_GL;
                        if (pp >= nch) continue;
                        const int idx0 = pp * 8 - mis;  // sample idx of h[0]
                        if (idx0 >= 0 && idx0 + 8 <= bucket_len) {
                            #pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const float f = bf16_to_f32(v[u].h[j]);
                                ingest_acc<GATED>(f, lo, hi, sum, cnt, rej);
                            }
                        } else {  // boundary chunk: mask by sample index
                            #pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const unsigned k = (unsigned)(idx0 + j);
                                if (k < (unsigned)bucket_len) {
                                    const float f = bf16_to_f32(v[u].h[j]);
                                    ingest_acc<GATED>(f, lo, hi, sum, cnt,
                                                      rej);
                                }
                            }
                        }
                    }
                }
                if (at_end)
                    for (int i = max(nch * 8 - mis, 0) + lane;
                         i < bucket_len;
                         i += ING_GL) {  // tensor-final bucket only
                        const float f = bf16_to_f32(su[i]);
                        ingest_acc<GATED>(f, lo, hi, sum, cnt, rej);
                    }
            } else {
                int pre = (int)(((16 - ((size_t)src & 15)) & 15) / 4);
                if (pre > bucket_len) pre = bucket_len;
                for (int i = lane; i < pre; i += ING_GL) {
                    const float f = (float)src[i];
                    ingest_acc<GATED>(f, lo, hi, sum, cnt, rej);
                }
                const int quad = (bucket_len - pre) / 4;
                const f32x4_* vp = (const f32x4_*)((const float*)src + pre);
                for (int base = lane; base < quad; base += 5 * ING_GL) {
                    f32x4_ v[5];
                    #pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        const int pp = base + u * ING_GL;
                        v[u] = __builtin_nontemporal_load(
                            &vp[pp < quad ? pp : 0]);
                    }
                    #pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        if (base + u * ING_GL < quad) {
                            ingest_acc<GATED>(v[u].x, lo, hi, sum, cnt, rej);
                            ingest_acc<GATED>(v[u].y, lo, hi, sum, cnt, rej);
                            ingest_acc<GATED>(v[u].z, lo, hi, sum, cnt, rej);
                            ingest_acc<GATED>(v[u].w, lo, hi, sum, cnt, rej);
                        }
                    }
                }
                for (int i = pre + quad * 4 + lane; i < bucket_len; i += ING_GL) {
                    const float f = (float)src[i];
                    ingest_acc<GATED>(f, lo, hi, sum, cnt, rej);
                }
            }
        }
        // reduce within each 16-lane bucket group
        #pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            sum += __shfl_xor(sum, off);
            cnt += __shfl_xor(cnt, off);
        }
        if (lane == 0 && active) {
            const int c = chan_map[cin];
            int bi = head_mod + b;
            if (bi >= G) bi -= G;      // b < NB <= G: one subtract suffices
            const long idx = (((long)s * C + c) * G + bi) * BST;
            bsum[idx] = sum;
            bcnt[idx] = cnt;
        }
        if constexpr (GATED) {
            // the wave's four groups count into the same rej[s, c]
            // (inactive groups hold 0): reduce over the whole wave
            #pragma unroll
            for (int off = WAVE / 2; off > 0; off >>= 1)
                rej += __shfl_xor(rej, off);
            if (wlane == 0 && rej > 0)
                atomicAdd((unsigned long long*)gate_rej(gate...)
                              + ((long)s * C + cg),
                          (unsigned long long)rej);
        }
    }
}

// ---------------------------------------------------------------------------
// 1b. Sparse ingest: event tuples (stream, chan, grid_bucket, value)
// ---------------------------------------------------------------------------
// GATED: late drop first (a late event is never counted as rejected), then
// the channel's bounds: one extra compare, and one extra 64-bit atomic on the
// rare rejected event.
template <bool GATED, class... GA>
__global__ void ingest_events_kernel(
    const int* __restrict__ ev_stream, const int* __restrict__ ev_chan,
    const long* __restrict__ ev_bucket, const float* __restrict__ ev_val,
    float* __restrict__ bsum, float* __restrict__ bcnt,
    int C, int G, long n_events, long min_bucket, int BST,
    GA... gate)  // GATED: const float* bounds (C, 2), long long* rej (S, C)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_events;
         i += (long)gridDim.x * blockDim.x) {
        const long b = ev_bucket[i];
        if (b < min_bucket) continue;  // behind the watermark: dropped (late data)
        const float v = ev_val[i];
        if (isnan(v)) continue;
        if constexpr (GATED) {
            const float* bounds = gate_bounds(gate...);
            const int c = ev_chan[i];
            if (!(bounds[2 * c] <= v && v <= bounds[2 * c + 1])) {
                atomicAdd((unsigned long long*)gate_rej(gate...)
                              + ((long)ev_stream[i] * C + c), 1ull);
                continue;
            }
        }
        const long idx = (((long)ev_stream[i] * C + ev_chan[i]) * G
                          + b % G) * BST;
        atomicAdd(&bsum[idx], v);
        atomicAdd(&bcnt[idx], 1.f);
    }
}

// Zero the bucket slots about to be (re)used: [head, head+nb) mod G.
__global__ void clear_buckets_kernel(
    float* __restrict__ bsum, float* __restrict__ bcnt,
    int S, int C, int G, long head, int nb, int BST)
{
    const long n = (long)S * C * nb;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % nb);
        const long sc = i / nb;
        const long idx = (sc * G + (head + j) % G) * BST;
        bsum[idx] = 0.f;
        bcnt[idx] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// 1c. Stream reset: return the listed stream slots to the never-used state
//     (bucket sums/counts and processed points 0, fill carry NaN) so that a
//     slot given up by one patient carries nothing over to the next.
// ---------------------------------------------------------------------------
// A stream owns up to three contiguous float regions of per-stream length
// len[r] at base[r] + sid * len[r]: the packed (sum,cnt) pairs (2*C*G) and
// proc (C*G), or bsum, bcnt and proc (C*G each). blockIdx.y strides over the
// id list, blockIdx.x over the stream's store units; a region whose length is
// a multiple of 4 floats (and whose base is 16 B-aligned — the launcher
// checks) is written with 16 B stores, any other with dword stores. Reads no
// ring position, so it may run between graph replays.
struct ResetRegions {
    float* base[3];
    int len[3];     // floats per stream
    int vec[3];     // 1: 16 B stores
    int units[3];   // store units per stream (len/4 or len; 0 = unused)
};

__global__ __launch_bounds__(256) void reset_streams_kernel(
    const int* __restrict__ sids, int n, ResetRegions rg,
    float* __restrict__ last_val, int S, int C)
{
    const int total = rg.units[0] + rg.units[1] + rg.units[2];
    const f32x4_ z4 = {0.f, 0.f, 0.f, 0.f};
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        const int s = sids[k];
        if ((unsigned)s >= (unsigned)S) continue;  // host range-checks too
        // 64-bit stride: total may be close to 2^31 (the launcher's bound)
        for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total;
             u += (long)gridDim.x * blockDim.x) {
            // constant indices only: the region table stays in scalar
            // registers (a lane-indexed table would go to scratch)
            float* base = rg.base[0];
            int len = rg.len[0], vec = rg.vec[0], v = (int)u;
            if (v >= rg.units[0]) {
                v -= rg.units[0];
                base = rg.base[1]; len = rg.len[1]; vec = rg.vec[1];
                if (v >= rg.units[1]) {
                    v -= rg.units[1];
                    base = rg.base[2]; len = rg.len[2]; vec = rg.vec[2];
                }
            }
            float* p = base + (long)s * len;
            if (vec) ((f32x4_*)p)[v] = z4;
            else p[v] = 0.f;
        }
        if (blockIdx.x == 0)
            for (int c = threadIdx.x; c < C; c += blockDim.x)
                last_val[(long)s * C + c] = NAN;
    }
}

// ---------------------------------------------------------------------------
// 1d. Stream snapshot / restore (warm restart): only a short tail of each
//     ring is live — buckets [nproc, nproc+nbk) not yet consumed by the fill,
//     the last `keep` processed points [nproc-keep, nproc) that model windows
//     still read, and the fill carry. snapshot_streams compacts that tail of
//     the listed streams into one record each; restore_streams scatters
//     records back into a (fresh) engine whose G, S or bucket packing may
//     differ from the source's.
// ---------------------------------------------------------------------------
// Record of stream k, C x R fp32 with R = 2*nbk + keep + 1, per channel:
//   [sum0, cnt0, sum1, cnt1, ...](nbk pairs) [proc](keep) [last_val]
// in LINEAR grid order: ring slot = start + j, minus G once past the end
// (b0, p0 < G and nbk, keep <= G, so a range wraps at most once). The pair
// layout is the same for BST=2 (packed) and BST=1 (split) engines. Lane u of
// a record walks one channel's ring row with consecutive lanes on consecutive
// addresses. blockIdx.y strides the id list, blockIdx.x the record. Ring
// positions arrive by value (no device state block is read), so both kernels
// may run between graph replays. Offsets into rings and records are 64-bit.
template <bool RESTORE>
__global__ __launch_bounds__(256) void snapshot_streams_kernel(
    const int* __restrict__ sids, int n, float* bsum, float* bcnt,
    float* proc, float* last_val, int S, int C, int G, int BST,
    int b0, int p0, int nbk, int keep, float* rec_base)
{
    const int R = 2 * nbk + keep + 1;
    const long total = (long)C * R;  // < 2^31 (the launcher's bound)
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        const int s = sids[k];
        if ((unsigned)s >= (unsigned)S) continue;  // host range-checks too
        float* rec = rec_base + (long)k * total;
        for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < total;
             u += (long)gridDim.x * blockDim.x) {
            const int c = (int)(u / R), r = (int)(u - (long)c * R);
            const long row = (long)s * C + c;
            float* p;
            if (r < 2 * nbk) {
                int g = b0 + (r >> 1);
                if (g >= G) g -= G;
                p = ((r & 1) ? bcnt : bsum) + (row * G + g) * BST;
            } else if (r < 2 * nbk + keep) {
                int g = p0 + (r - 2 * nbk);
                if (g >= G) g -= G;
                p = proc + row * G + g;
            } else {
                p = last_val + row;
            }
            if (RESTORE) *p = rec[u];
            else rec[u] = *p;
        }
    }
}

// ---------------------------------------------------------------------------
// 1e. Window coverage: how much of the latest model window rests on samples.
//     The window's L grid points [lo, lo+L) (lo = nproc - L) average buckets
//     [lo, lo+span), span = L + W - 1. Bucket j of the span is PRESENT iff
//     j < nfloor (below a restored engine's floor: state unknown, counted as
//     present) or its count is > 0. Per (stream, channel) row, int32 x 3:
//       present  present buckets in the span
//       imputed  grid points i in [0, L) with no present bucket in [i, i+W)
//       stale    run of non-present buckets ending at the span's last one
// ---------------------------------------------------------------------------
// One wave per row, grid-strided. Lane l loads the counts of span buckets
// l, l+64, l+128 (stride BST floats, so packed and split rings both work;
// the span wraps at most once: g0 < G and span <= G), all three loads before
// the first use. Three ballots give the row's presence as a wave-uniform
// 192-bit mask m[0..2]; present is three popcounts, stale a leading-zero
// count down from bit span-1 (bits from span on are 0 by construction), and
// for imputed lane l of round q tests bits [64q+l, 64q+l+W) — a funnel shift
// of m[q], m[q+1] by l — then a ballot and a popcount. No LDS, no atomics;
// lane 0 stores the three results. Positions arrive by value (no device
// state block is read). Row offsets are 64-bit.
#define COV_MAXSPAN 192

__global__ __launch_bounds__(256) void window_coverage_kernel(
    const float* __restrict__ bcnt, int BST, const int* __restrict__ sids,
    int n, int S, int C, int G, int g0, int nfloor, int L, int W,
    int* __restrict__ out)
{
    typedef unsigned long long u64;
    const int lane = threadIdx.x & (WAVE - 1);
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const long nwaves = (long)gridDim.x * blockDim.x / WAVE;
    const int span = L + W - 1;
    const u64 wmask = W >= 64 ? ~0ull : (1ull << W) - 1;
    const long rows = (long)n * C;
    for (long r = wave; r < rows; r += nwaves) {
        const int k = (int)(r / C), c = (int)(r - (long)k * C);
        const int s = sids ? sids[k] : k;
        if ((unsigned)s >= (unsigned)S) continue;  // host range-checks too
        const float* row = bcnt + ((long)s * C + c) * G * BST;
        float v[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            // lanes past the span re-read its last bucket (masked below):
            // an unconditional load keeps the three in flight together
            int g = g0 + min(lane + WAVE * q, span - 1);
            if (g >= G) g -= G;
            v[q] = row[(long)g * BST];
        }
        u64 m[4];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int j = lane + WAVE * q;
            m[q] = __ballot((j < span) & ((j < nfloor) | (v[q] > 0.f)));
        }
        m[3] = 0;
        const int present = __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]);
        int top = -1;  // highest present bucket of the span
        if (m[2]) top = 191 - __clzll(m[2]);
        else if (m[1]) top = 127 - __clzll(m[1]);
        else if (m[0]) top = 63 - __clzll(m[0]);
        int imputed = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            // bits [64q + lane, 64q + lane + 64) of the mask
            const u64 x = lane ? (m[q] >> lane) | (m[q + 1] << (WAVE - lane))
                               : m[q];
            imputed += __popcll(__ballot((lane + WAVE * q < L) &
                                         ((x & wmask) == 0)));
        }
        if (lane == 0) {
            int* o = out + r * 3;
            o[0] = present;
            o[1] = imputed;
            o[2] = span - 1 - top;
        }
    }
}

// ---------------------------------------------------------------------------
// 2. Sliding-window average + ffill/bfill/zero-fill
//    Processes proc grid points [phead, phead+np): window starting at grid j
//    averages buckets [j, j+win_buckets). The fill is an order-dependent
//    scan per (s, c) row: tiny np per trigger, large only in replay catch-up.
//    Three kernels (general, fill16, staged fill16) share the pieces below.
// ---------------------------------------------------------------------------
// Longest window any fill kernel accepts (the launcher refuses others): it
// sizes the general kernel's LDS rows.
#define FILL_MAXW 64

// Serial ffill scan of window values lv[0, n), in place, by ONE lane. After
// ffill-with-carry, NaNs can only be a PREFIX of the batch (once any value
// is seen, carry is set forever), so bfill reduces to: fill the prefix with
// the first valid value (or 0). nan_prefix accumulates over calls (the
// general kernel scans one 64-point chunk per call); first_val is the value
// that ended the prefix.
__device__ __forceinline__ void fill_scan(float* lv, int n, float& carry,
                                          int& nan_prefix, float& first_val) {
    for (int j = 0; j < n; ++j) {
        const float v = lv[j];
        if (isnan(v)) {
            if (isnan(carry)) ++nan_prefix;  // still before the first value
            else lv[j] = carry;
        } else {
            if (isnan(carry)) first_val = v;
            carry = v;
        }
    }
}

// Window (sum, cnt) over two linear segments of pairs — a window that wraps
// the ring is p1[0, first) then p2[0, rem). Four independent accumulators (a
// single dependent add chain was the lane's critical path) in a fixed
// association that every caller shares bit for bit: segment 1 dealt
// round-robin into a0..a3 with the < 4 remainder into a0, segment 2 again
// from a0, then (a0 + a1) + (a2 + a3).
__device__ __forceinline__ f32x2p_ window_sum2(const f32x2p_* p1, int first,
                                               const f32x2p_* p2, int rem) {
    f32x2p_ a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
    f32x2p_ a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
    int k = 0;
    for (; k + 4 <= first; k += 4) {
        a0 += p1[k];     a1 += p1[k + 1];
        a2 += p1[k + 2]; a3 += p1[k + 3];
    }
    for (; k < first; ++k) a0 += p1[k];
    int j = 0;
    for (; j + 4 <= rem; j += 4) {
        a0 += p2[j];     a1 += p2[j + 1];
        a2 += p2[j + 2]; a3 += p2[j + 3];
    }
    for (; j < rem; ++j) a0 += p2[j];
    return (a0 + a1) + (a2 + a3);
}

// Window value of a (sum, cnt) total: the mean, NaN for an empty window.
__device__ __forceinline__ float window_mean(f32x2p_ t) {
    return (t.y > 0.f) ? t.x / t.y : NAN;
}

// fill16 epilogue: lane gl of a 16-lane group holds window value `val` of
// row sc (NaN = empty window); lv is the group's 16-float LDS row. Lane 0 of
// the group scans, the group takes the bfill | fillna(0) prefix from it and
// stores its np points at proc[sc, (phead + gl) mod G]; the row's carry goes
// back to last_val. Whole waves call it (it syncs the wave three times).
__device__ __forceinline__ void fill16_finish(
    float* lv, float val, float carry, bool live, long sc, int grp, int gl,
    int np, long phead, int G, float* __restrict__ proc,
    float* __restrict__ last_val)
{
    float first_val = NAN;
    int nan_prefix = 0;
    lv[gl] = val;
    wave_sync();
    if (live && gl == 0) {
        fill_scan(lv, np, carry, nan_prefix, first_val);
        last_val[sc] = carry;
    }
    wave_sync();
    if (live && gl < np) {
        nan_prefix = __shfl(nan_prefix, grp * 16);
        first_val = __shfl(first_val, grp * 16);
        float outv = lv[gl];
        if (gl < nan_prefix)
            outv = isnan(first_val) ? 0.f : first_val;
        proc[sc * G + (phead + gl) % G] = outv;
    }
    wave_sync();                          // lv reads done before reuse
}

// General kernel (np > 16: catch-up refills). One WAVE per (stream,
// channel): coalesced bucket loads, LDS-staged sliding sums (each lane owns
// one output point per 64-point chunk), the order-dependent ffill scan runs
// on lane 0 over LDS.
__global__ __launch_bounds__(256) void window_fill_kernel(
    const float* __restrict__ bsum, const float* __restrict__ bcnt,
    float* __restrict__ proc, float* __restrict__ last_val,
    int S, int C, int G, long phead_in, int np, int win_buckets,
    const long long* __restrict__ dstate, int BST)
{
    const long phead = ring_nproc(dstate, phead_in);
    constexpr int CHUNK = 64;             // output points per iteration
    // bucket sums / counts: CHUNK + win_buckets - 1 <= CHUNK + FILL_MAXW used
    __shared__ float lds_s[4][CHUNK + FILL_MAXW];
    __shared__ float lds_c[4][CHUNK + FILL_MAXW];
    __shared__ float lds_v[4][CHUNK];       // window values / filled output
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    float* ls = lds_s[wave];
    float* lc = lds_c[wave];
    float* lv = lds_v[wave];

    const long nsc = (long)S * C;
    for (long sc = (long)blockIdx.x * 4 + wave; sc < nsc;
         sc += (long)gridDim.x * 4) {
        const float* bs = bsum + sc * G * BST;
        const float* bc = bcnt + sc * G * BST;
        float* pr = proc + sc * G;
        float carry = last_val[sc];
        int nan_prefix = 0;
        float first_val = NAN;

        for (int j0 = 0; j0 < np; j0 += CHUNK) {
            const int jn = min(CHUNK, np - j0);
            const int nload = jn + win_buckets - 1;
            // coalesced bucket loads into LDS
            for (int i = lane; i < nload; i += WAVE) {
                const long idx = (phead + j0 + i) % G;
                if (BST == 2) {  // packed (sum,cnt) pair: one 8 B load
                    const f32x2p_ v = *(const f32x2p_*)(bs + idx * 2);
                    ls[i] = v.x;
                    lc[i] = v.y;
                } else {
                    ls[i] = bs[idx];
                    lc[i] = bc[idx];
                }
            }
            wave_sync();
            // lane j: sliding raw-sample mean of window starting at j0+j
            if (lane < jn) {
                float sum = 0.f, cnt = 0.f;
                for (int k = 0; k < win_buckets; ++k) {
                    sum += ls[lane + k];
                    cnt += lc[lane + k];
                }
                lv[lane] = (cnt > 0.f) ? sum / cnt : NAN;
            }
            wave_sync();
            // lane 0: ffill scan (order-dependent; jn <= 64 steps)
            if (lane == 0) fill_scan(lv, jn, carry, nan_prefix, first_val);
            wave_sync();
            if (lane < jn) pr[(phead + j0 + lane) % G] = lv[lane];
            wave_sync();
            carry = __shfl(carry, 0);
        }
        nan_prefix = __shfl(nan_prefix, 0);
        first_val = __shfl(first_val, 0);
        if (nan_prefix > 0) {
            const float fill = isnan(first_val) ? 0.f : first_val;  // bfill|0
            for (int i = lane; i < nan_prefix; i += WAVE)
                pr[(phead + i) % G] = fill;
        }
        if (lane == 0) last_val[sc] = carry;
    }
}

// Timelast gather v2: one thread per (s, b, t) writes ALL C channels of
// one timepoint. In the (S, B, WIN, C) layout the channel axis is
// CONTIGUOUS, so the stores are C/2 packed dwords (vs v1's 2-byte
// scattered stores — profile: 72 us vs the std-layout gather's 30 us at
// S=16384); the reads coalesce per channel (consecutive t lanes hit
// consecutive proc addresses). Even C only (wire space is 10).
template <class OT>
__global__ void window_gather_tlast2_kernel(
    const float* __restrict__ proc, OT* __restrict__ out,  // (S, B, WIN, C)
    int S, int C, int G, int B, int WIN, int stride, long end_in,
    const long long* __restrict__ dstate, int end_extra)
{
    const long end = dstate ? (long)dstate[1] + end_extra : end_in;
    const long n = (long)S * B * WIN;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i % WIN);
        const int b = (int)((i / WIN) % B);
        const int s = (int)(i / ((long)WIN * B));
        const long wend = end - (long)(B - 1 - b) * stride;
        const long g = wend - WIN + t;
        const bool ok = g >= 0 && g < end && wend - WIN >= 0 && wend <= end;
        const int gi = ok ? (int)(g % G) : 0;
        const float* pr = proc + (long)s * C * G + gi;
        if constexpr (sizeof(OT) == 2) {
            unsigned int* od = (unsigned int*)(out + i * C);
            for (int c = 0; c < C; c += 2) {
                const unsigned int lo =
                    ok ? f32_to_bf16(pr[(long)c * G]) : 0u;
                const unsigned int hi =
                    ok ? f32_to_bf16(pr[(long)(c + 1) * G]) : 0u;
                od[c >> 1] = lo | (hi << 16);
            }
        } else {
            OT* od = out + i * C;
            for (int c = 0; c < C; ++c)
                od[c] = ok ? (OT)pr[(long)c * G] : (OT)0;
        }
    }
}

// Steady-state variant (np <= 16): the general kernel leaves 52 of 64 lanes
// idle when a trigger yields only NB=12 new grid points. Pack FOUR
// (stream, channel) rows per wave in 16-lane groups; the <= 51 bucket
// reads per row are consecutive-address (coalesced within the group) and
// L1-resident, so no LDS staging — only the 16-value ffill scan goes
// through LDS. Dispatch in tskd_preproc_window_fill.
__global__ __launch_bounds__(256) void window_fill16_kernel(
    const float* __restrict__ bsum, const float* __restrict__ bcnt,
    float* __restrict__ proc, float* __restrict__ last_val,
    int S, int C, int G, long phead_in, int np, int win_buckets,
    const long long* __restrict__ dstate, int BST)
{
    const long phead = ring_nproc(dstate, phead_in);
    __shared__ float lds_v[4][64];        // per wave: 4 groups x 16 values
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int grp = lane / 16, gl = lane % 16;
    float* lv = lds_v[wave] + grp * 16;

    const long nsc = (long)S * C;
    for (long sc0 = ((long)blockIdx.x * 4 + wave) * 4; sc0 < nsc;
         sc0 += (long)gridDim.x * 16) {
        const long sc = sc0 + grp;
        const bool live = sc < nsc;
        float carry = NAN, val = NAN;
        if (live) {
            carry = last_val[sc];
            if (gl < np && BST == 2) {
                // packed (sum,cnt) pairs: ONE f32x2 load and ONE packed add
                // per bucket — half the loads and adds of the split-array
                // layout (the whole point of TSKD_PACKED_BUCKETS)
                const f32x2p_* pk = (const f32x2p_*)(bsum + sc * G * 2);
                const int start = (int)((phead + gl) % G);
                const int first = min(win_buckets, G - start);
                val = window_mean(window_sum2(pk + start, first, pk,
                                              win_buckets - first));
            } else if (gl < np) {
                const float* bs = bsum + sc * G;
                const float* bc = bcnt + sc * G;
                // split the (possibly wrapping) 36-bucket window into two
                // linear segments and sum with 4 independent accumulators:
                // the single dependent add chain was the lane's critical
                // path (the loads are L1/L2 hits shared across the group)
                const int start = (int)((phead + gl) % G);
                const int first = min(win_buckets, G - start);
                const int rem = win_buckets - first;
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
                const float* p1 = bs + start;
                const float* q1 = bc + start;
                int k = 0;
                for (; k + 4 <= first; k += 4) {
                    a0 += p1[k];     c0 += q1[k];
                    a1 += p1[k + 1]; c1 += q1[k + 1];
                    a2 += p1[k + 2]; c2 += q1[k + 2];
                    a3 += p1[k + 3]; c3 += q1[k + 3];
                }
                for (; k < first; ++k) { a0 += p1[k]; c0 += q1[k]; }
                int j = 0;
                for (; j + 4 <= rem; j += 4) {
                    a0 += bs[j];     c0 += bc[j];
                    a1 += bs[j + 1]; c1 += bc[j + 1];
                    a2 += bs[j + 2]; c2 += bc[j + 2];
                    a3 += bs[j + 3]; c3 += bc[j + 3];
                }
                for (; j < rem; ++j) { a0 += bs[j]; c0 += bc[j]; }
                const float sum = (a0 + a1) + (a2 + a3);
                const float cnt = (c0 + c1) + (c2 + c3);
                val = (cnt > 0.f) ? sum / cnt : NAN;
            }
        }
        fill16_finish(lv, val, carry, live, sc, grp, gl, np, phead, G, proc,
                      last_val);
    }
}

// Staged steady-state fill (packed layout, the default): the loop above has
// every lane fetch its own 36 pairs from L1 — 48 lanes x 288 B requested for
// ~1.5 KB of distinct data per wave, in nine dependent round trips. Here each
// 16-lane group loads its row's span (np + win_buckets - 1 pairs, 47 in
// steady state) ONCE, all of a lane's loads issued back to back, into a
// per-group LDS row; slot j holds ring element (phead + j) mod G. Every lane
// then sums its window from LDS in window_sum2's association, so the two
// kernels agree bit for bit.
// When no lane of the launch wraps (uniform) and win_buckets is the
// compile-time WB, the sum is WB unrolled LDS reads and packed adds. A wave's
// next task's loads are issued before the current task's sums, so they are
// in flight across its scan and store.
// Row stride 80 pairs = 160 dwords = 32 mod 64 banks: the two groups of a
// 32-lane ds_read_b64 half hit disjoint banks.
#define F16_SLOTS 64    // pair slots a group's LDS row holds (span limit)
#define F16_STRIDE 80   // row stride, pairs
// NQ = loads per lane = ceil(span / 16), a launch constant so the loads and
// the LDS stores are straight-line code.
template <int WB, int NQ>
__global__ __launch_bounds__(256) void window_fill16_staged_kernel(
    const float* __restrict__ bsum, float* __restrict__ proc,
    float* __restrict__ last_val, int S, int C, int G, long phead_in, int np,
    int win_buckets, const long long* __restrict__ dstate)
{
    static_assert(WB % 4 == 0 && WB + 15 <= F16_SLOTS, "");
    static_assert(NQ >= 1 && NQ * 16 <= F16_SLOTS, "");
    const long phead = ring_nproc(dstate, phead_in);
    const int wb = WB ? WB : win_buckets;
    __shared__ f32x2p_ lds_p[4][4][F16_STRIDE];
    __shared__ float lds_v[4][64];        // per wave: 4 groups x 16 values
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int grp = lane / 16, gl = lane % 16;
    float* lv = lds_v[wave] + grp * 16;
    f32x2p_* row = lds_p[wave][grp];

    const int s0 = (int)(phead % G);
    const int span = np + wb - 1;         // <= 16 NQ, <= G (launcher)
    const bool nowrap = s0 + span <= G;   // uniform over the grid
    // ring element of slot gl + 16 q, unwrapped once (span <= G)
    int eidx[NQ];
    #pragma unroll
    for (int q = 0; q < NQ; ++q) {
        int e = s0 + gl + 16 * q;
        if (e >= G) e -= G;
        eidx[q] = gl + 16 * q < span ? e : 0;
    }

    const long nsc = (long)S * C;
    const long stride = (long)gridDim.x * 16;
    long sc0 = ((long)blockIdx.x * 4 + wave) * 4;
    // a task's loads are issued one task ahead: they fly over the previous
    // task's sums, scan and store
    f32x2p_ ld[NQ];
    float carry_ld = NAN;
    auto fetch = [&](long base) {
        const long sc = base + grp;
        if (sc < nsc) {
            const f32x2p_* pk = (const f32x2p_*)(bsum + sc * G * 2);
            #pragma unroll
            for (int q = 0; q < NQ; ++q) ld[q] = pk[eidx[q]];
            carry_ld = last_val[sc];
        }
    };
    if (sc0 < nsc) fetch(sc0);
    for (; sc0 < nsc; sc0 += stride) {
        const long sc = sc0 + grp;
        const bool live = sc < nsc;
        float carry = NAN, val = NAN;
        if (live) {
            carry = carry_ld;
            #pragma unroll
            for (int q = 0; q < NQ; ++q) row[gl + 16 * q] = ld[q];
        }
        if (sc0 + stride < nsc) fetch(sc0 + stride);
        wave_sync();
        if (live && gl < np) {
            const f32x2p_* p1 = row + gl;
            f32x2p_ t;
            if (WB && nowrap) {           // window_sum2 with rem = 0, unrolled
                f32x2p_ a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
                f32x2p_ a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
                #pragma unroll
                for (int k = 0; k < WB; k += 4) {
                    a0 += p1[k];     a1 += p1[k + 1];
                    a2 += p1[k + 2]; a3 += p1[k + 3];
                }
                t = (a0 + a1) + (a2 + a3);
            } else {                      // segment 2 follows in the LDS row
                const int start = (int)((phead + gl) % G);
                const int first = min(wb, G - start);
                t = window_sum2(p1, first, p1 + first, wb - first);
            }
            val = window_mean(t);
        }
        // its last sync: row and lv reads are done before the next task's
        fill16_finish(lv, val, carry, live, sc, grp, gl, np, phead, G, proc,
                      last_val);
    }
}

// ---------------------------------------------------------------------------
// 3. Window gather: (S, B, C, WIN) model inputs from processed grid.
//    Window b (b = 0..B-1) covers grid [end - (B-1-b)*stride - WIN,
//    end - (B-1-b)*stride). Grid points never produced (g < 0) read as 0.
// ---------------------------------------------------------------------------

// Vectorized: each thread emits 4 consecutive time points (WIN % 4 == 0),
// reading contiguous proc and writing one 8 B (bf16) / 16 B (f32) store.
// TLAST: emit (S, B, WIN, C) instead — the layout the LDS-free MFMA conv
// kernel consumes (scalar scattered stores; the read side stays coalesced).
template <class OT, bool TLAST = false>
__global__ void window_gather_kernel(
    const float* __restrict__ proc,
    OT* __restrict__ out,            // (S, B, C, WIN) or (S, B, WIN, C)
    int S, int C, int G, int B, int WIN, int stride, long end_in,
    const long long* __restrict__ dstate, int end_extra)
{
    const long end = dstate ? (long)dstate[1] + end_extra : end_in;
    const int WQ = WIN / 4;
    const long n = (long)S * B * C * WQ;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        const int tq = (int)(i % WQ);
        const int c = (int)((i / WQ) % C);
        const int b = (int)((i / ((long)WQ * C)) % B);
        const int s = (int)(i / ((long)WQ * C * B));
        const long wend = end - (long)(B - 1 - b) * stride;
        const long g0 = wend - WIN + tq * 4;
        const float* pr = proc + ((long)s * C + c) * G;
        float v[4];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long g = g0 + j;
            v[j] = (g >= 0 && g < end && wend - WIN >= 0 && wend <= end)
                       ? pr[g % G] : 0.f;
        }
        if constexpr (TLAST) {
            const long ob = ((long)s * B + b) * C * WIN;
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long o = ob + (long)(tq * 4 + j) * C + c;
                if constexpr (sizeof(OT) == 2) out[o] = f32_to_bf16(v[j]);
                else out[o] = (OT)v[j];
            }
        } else {
            const long o = (((long)s * B + b) * C + c) * WIN + (long)tq * 4;
            if constexpr (sizeof(OT) == 2) {
                union { unsigned short h[4]; unsigned long long u; } pk;
                #pragma unroll
                for (int j = 0; j < 4; ++j) pk.h[j] = f32_to_bf16(v[j]);
                *(unsigned long long*)(out + o) = pk.u;
            } else {
                float4 pk = {v[0], v[1], v[2], v[3]};
                *(float4*)((float*)out + o) = pk;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Optional per-window z-normalization (BASELINE.json names a z-normalize
// stage; the REFERENCE has none — SURVEY.md §7 fidelity note — so this is
// an opt-in post-pass, off by default): each (stream, batch, channel) row of
// WIN points is normalized to (v - mean) / max(std, eps) in place.
// One wave per row: shuffle-reduced mean/var, vectorized rewrite.
// ---------------------------------------------------------------------------
template <class OT>
__global__ void window_znorm_kernel(OT* __restrict__ w,  // (rows, WIN)
                                    long rows, int WIN, float eps)
{
    const int lane = threadIdx.x % WAVE;
    for (long r = (long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
         r < rows; r += (long)gridDim.x * (blockDim.x / WAVE)) {
        OT* row = w + r * WIN;
        float sum = 0.f, sq = 0.f;
        for (int t = lane; t < WIN; t += WAVE) {
            float v;
            if constexpr (sizeof(OT) == 2) v = bf16_to_f32((unsigned short)row[t]);
            else v = (float)row[t];
            sum += v;
            sq = fmaf(v, v, sq);
        }
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_xor(sum, off);
            sq += __shfl_xor(sq, off);
        }
        const float mean = sum / WIN;
        const float var = fmaxf(sq / WIN - mean * mean, 0.f);
        const float inv = 1.0f / fmaxf(sqrtf(var), eps);
        for (int t = lane; t < WIN; t += WAVE) {
            float v;
            if constexpr (sizeof(OT) == 2) v = bf16_to_f32((unsigned short)row[t]);
            else v = (float)row[t];
            v = (v - mean) * inv;
            if constexpr (sizeof(OT) == 2) row[t] = (OT)f32_to_bf16(v);
            else row[t] = (OT)v;
        }
    }
}

// ---------------------------------------------------------------------------
// extern "C" launchers
// ---------------------------------------------------------------------------
static inline int grid_for(long n, int block) {
    long g = (n + block - 1) / block;
    if (g > 16384) g = 16384;
    if (g < 1) g = 1;
    return (int)g;
}

extern "C" {

// Shared launcher of the two dense entry points: bounds == null launches the
// ungated kernels with their own (unchanged) argument list.
static int launch_ingest_dense(const void* raw, int raw_is_bf16, float* bsum,
                               float* bcnt, const int* chan_map, int S,
                               int CIN, int C, int T, int G, int bucket_len,
                               long head, const long long* dstate, int bst,
                               const float* bounds, long long* rej,
                               hipStream_t st) {
    const int NB = T / bucket_len;
    if (NB <= 0 || S <= 0) return 0;
    const long nwaves = (long)S * CIN * ((NB + ING_GRP - 1) / ING_GRP);
    // read-ceiling probe: 32768 blocks measures ~3% above the 16384 cap.
    // TSKD_INGEST_GRID caps the block count: the probe saturates HBM from
    // ~2048 blocks, so a small grid leaves CU wave slots free for a
    // co-scheduled model chain (TriggerGraph overlap mode).
    long cap = 32768;
    if (const char* gc = getenv("TSKD_INGEST_GRID")) cap = atol(gc);
    long blocks = (nwaves + 3) / 4;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    const int grid = (int)blocks;
    // bf16: 5-deep load ILP with masked boundary chunks (no scalar peel);
    // fp32: 5-deep load ILP with a scalar head/tail peel.
    if (bounds && raw_is_bf16)
        hipLaunchKernelGGL((ingest_dense_kernel<unsigned short, true,
                                                const float*, long long*>),
                           dim3(grid), dim3(256), 0, st,
                           (const unsigned short*)raw, bsum, bcnt, chan_map,
                           S, CIN, C, T, G, bucket_len, head, dstate, bst,
                           bounds, rej);
    else if (bounds)
        hipLaunchKernelGGL((ingest_dense_kernel<float, true, const float*,
                                                long long*>), dim3(grid),
                           dim3(256), 0, st, (const float*)raw, bsum, bcnt,
                           chan_map, S, CIN, C, T, G, bucket_len, head, dstate,
                           bst, bounds, rej);
    else if (raw_is_bf16)
        hipLaunchKernelGGL((ingest_dense_kernel<unsigned short, false>),
                           dim3(grid), dim3(256), 0, st,
                           (const unsigned short*)raw, bsum, bcnt, chan_map,
                           S, CIN, C, T, G, bucket_len, head, dstate, bst);
    else
        hipLaunchKernelGGL((ingest_dense_kernel<float, false>), dim3(grid),
                           dim3(256), 0, st, (const float*)raw, bsum, bcnt,
                           chan_map, S, CIN, C, T, G, bucket_len, head, dstate,
                           bst);
    return (int)hipGetLastError();
}

int tskd_preproc_ingest_dense(const void* raw, int raw_is_bf16,
                              float* bsum, float* bcnt, const int* chan_map,
                              int S, int CIN, int C, int T, int G,
                              int bucket_len, long head,
                              const long long* dstate, int bst,
                              void* stream) {
    return launch_ingest_dense(raw, raw_is_bf16, bsum, bcnt, chan_map, S, CIN,
                               C, T, G, bucket_len, head, dstate, bst, nullptr,
                               nullptr, (hipStream_t)stream);
}

// Signal-quality gate: the same launch with per-wire-channel bounds (C, 2)
// fp32 [lo, hi] and the cumulative (S, C) int64 rejected counter. -4: a null
// bounds or counter pointer.
int tskd_preproc_ingest_dense_gated(const void* raw, int raw_is_bf16,
                                    float* bsum, float* bcnt,
                                    const int* chan_map, int S, int CIN,
                                    int C, int T, int G, int bucket_len,
                                    long head, const long long* dstate,
                                    int bst, const float* bounds,
                                    long long* rej, void* stream) {
    if (!bounds || !rej) return -4;
    return launch_ingest_dense(raw, raw_is_bf16, bsum, bcnt, chan_map, S, CIN,
                               C, T, G, bucket_len, head, dstate, bst, bounds,
                               rej, (hipStream_t)stream);
}

int tskd_preproc_ingest_events(const int* ev_stream, const int* ev_chan,
                               const long* ev_bucket, const float* ev_val,
                               float* bsum, float* bcnt, int C, int G,
                               long n_events, long min_bucket, int bst,
                               void* stream) {
    if (n_events <= 0) return 0;
    hipLaunchKernelGGL((ingest_events_kernel<false>),
                       dim3(grid_for(n_events, 256)), dim3(256), 0,
                       (hipStream_t)stream, ev_stream, ev_chan, ev_bucket,
                       ev_val, bsum, bcnt, C, G, n_events, min_bucket, bst);
    return (int)hipGetLastError();
}

int tskd_preproc_ingest_events_gated(const int* ev_stream, const int* ev_chan,
                                     const long* ev_bucket,
                                     const float* ev_val, float* bsum,
                                     float* bcnt, int C, int G, long n_events,
                                     long min_bucket, int bst,
                                     const float* bounds, long long* rej,
                                     void* stream) {
    if (!bounds || !rej) return -4;
    if (n_events <= 0) return 0;
    hipLaunchKernelGGL((ingest_events_kernel<true, const float*,
                                             long long*>),
                       dim3(grid_for(n_events, 256)), dim3(256), 0,
                       (hipStream_t)stream, ev_stream, ev_chan, ev_bucket,
                       ev_val, bsum, bcnt, C, G, n_events, min_bucket, bst,
                       bounds, rej);
    return (int)hipGetLastError();
}

int tskd_preproc_clear_buckets(float* bsum, float* bcnt, int S, int C, int G,
                               long head, int nb, int bst, void* stream) {
    if (nb <= 0) return 0;
    const long n = (long)S * C * nb;
    hipLaunchKernelGGL(clear_buckets_kernel, dim3(grid_for(n, 256)), dim3(256),
                       0, (hipStream_t)stream, bsum, bcnt, S, C, G, head, nb,
                       bst);
    return (int)hipGetLastError();
}

int tskd_preproc_reset_streams(const int* sids, int n, float* bsum,
                               float* bcnt, float* proc, float* last_val,
                               int S, int C, int G, int bst, void* stream) {
    if (n <= 0) return 0;
    const long cg = (long)C * G;
    if (S <= 0 || cg <= 0 || 3 * cg > 0x7fffffffL) return -4;
    if (bst == 2 && bcnt != bsum + 1) return -5;  // not (sum,cnt) pairs
    ResetRegions rg = {};
    int nreg = 0;
    auto add = [&](float* base, long len) {
        rg.base[nreg] = base;
        rg.len[nreg] = (int)len;
        rg.vec[nreg] = len % 4 == 0 && ((size_t)base & 15) == 0;
        rg.units[nreg] = (int)(rg.vec[nreg] ? len / 4 : len);
        ++nreg;
    };
    if (bst == 2) {
        add(bsum, 2 * cg);  // one contiguous run of (sum,cnt) pairs
    } else {
        add(bsum, cg);
        add(bcnt, cg);
    }
    add(proc, cg);
    const int total = rg.units[0] + rg.units[1] + rg.units[2];
    // ~4096 blocks over (ids x chunks): enough to fill the chip for one
    // stream, no more launch tail than that for thousands
    const int gy = n < 4096 ? n : 4096;
    int gx = (total + 255) / 256;
    if (gx > 4096 / gy) gx = 4096 / gy;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(reset_streams_kernel, dim3(gx, gy), dim3(256), 0,
                       (hipStream_t)stream, sids, n, rg, last_val, S, C);
    return (int)hipGetLastError();
}

// Shared launcher of snapshot_streams / restore_streams. -4: a shape or range
// the kernels do not cover; -5: bst=2 without (sum,cnt) pairs.
static int launch_snapshot(bool restore, const int* sids, int n, float* bsum,
                           float* bcnt, float* proc, float* last_val, int S,
                           int C, int G, int bst, long nproc, int nbk,
                           int keep, float* rec, hipStream_t st) {
    if (n <= 0) return 0;
    if (S <= 0 || C <= 0 || G <= 0 || nproc < 0) return -4;
    if (nbk < 0 || keep < 0 || nbk > G || keep > G || keep > nproc) return -4;
    if (bst != 1 && bst != 2) return -5;
    if (bst == 2 && bcnt != bsum + 1) return -5;
    const long total = (long)C * (2L * nbk + keep + 1);
    if (total > 0x7fffffffL) return -4;
    const int b0 = (int)(nproc % G), p0 = (int)((nproc - keep) % G);
    // ~8192 blocks over (ids x record chunks), as reset_streams sizes its grid
    const int gy = n < 8192 ? n : 8192;
    long gx = (total + 255) / 256;
    if (gx > 8192 / gy) gx = 8192 / gy;
    if (gx < 1) gx = 1;
    if (restore)
        hipLaunchKernelGGL((snapshot_streams_kernel<true>), dim3((int)gx, gy),
                           dim3(256), 0, st, sids, n, bsum, bcnt, proc,
                           last_val, S, C, G, bst, b0, p0, nbk, keep, rec);
    else
        hipLaunchKernelGGL((snapshot_streams_kernel<false>),
                           dim3((int)gx, gy), dim3(256), 0, st, sids, n, bsum,
                           bcnt, proc, last_val, S, C, G, bst, b0, p0, nbk,
                           keep, rec);
    return (int)hipGetLastError();
}

int tskd_preproc_snapshot_streams(const int* sids, int n, const float* bsum,
                                  const float* bcnt, const float* proc,
                                  const float* last_val, int S, int C, int G,
                                  int bst, long nproc, int nbk, int keep,
                                  float* out, void* stream) {
    return launch_snapshot(false, sids, n, (float*)bsum, (float*)bcnt,
                           (float*)proc, (float*)last_val, S, C, G, bst,
                           nproc, nbk, keep, out, (hipStream_t)stream);
}

int tskd_preproc_restore_streams(const int* sids, int n, float* bsum,
                                 float* bcnt, float* proc, float* last_val,
                                 int S, int C, int G, int bst, long nproc,
                                 int nbk, int keep, const float* in,
                                 void* stream) {
    return launch_snapshot(true, sids, n, bsum, bcnt, proc, last_val, S, C, G,
                           bst, nproc, nbk, keep, (float*)in,
                           (hipStream_t)stream);
}

// Coverage of the model window ending at nproc: out (n, C, 3) int32 =
// [present, imputed, stale] per row of the listed streams (sids null: all S,
// n = S). -4: a shape or position the kernel does not cover (span above
// COV_MAXSPAN or G, W outside [1, 64], nproc < L); -5: a stride other than
// 1 or 2.
int tskd_preproc_window_coverage(const float* bcnt, int bst, const int* sids,
                                 int n, int S, int C, int G, long nproc, int L,
                                 int W, long floor, int* out, void* stream) {
    if (S <= 0 || C <= 0 || G <= 0 || L < 1 || W < 1 || W > 64) return -4;
    const int span = L + W - 1;
    if (span > COV_MAXSPAN || span > G || nproc < L) return -4;
    if (bst != 1 && bst != 2) return -5;
    if (!sids && n != S) return -4;
    if (n <= 0) return 0;
    const long lo = nproc - L;
    long nfloor = floor - lo;  // span buckets below the restore floor
    if (nfloor < 0) nfloor = 0;
    if (nfloor > span) nfloor = span;
    const long nthreads = (long)n * C * WAVE;  // one wave per row
    hipLaunchKernelGGL(window_coverage_kernel, dim3(grid_for(nthreads, 256)),
                       dim3(256), 0, (hipStream_t)stream, bcnt, bst, sids, n,
                       S, C, G, (int)(lo % G), (int)nfloor, L, W, out);
    return (int)hipGetLastError();
}

int tskd_preproc_window_fill(const float* bsum, const float* bcnt, float* proc,
                             float* last_val, int S, int C, int G, long phead,
                             int np, int win_buckets,
                             const long long* dstate, int bst, void* stream) {
    // -4: a window the general kernel's LDS rows do not hold (every np)
    if (win_buckets < 1 || win_buckets > FILL_MAXW) return -4;
    if (np <= 0) return 0;
    if (np <= 16) {
        // steady-state: 4 (stream, channel) rows per wave, 16-lane groups
        const long nsc4 = ((long)S * C + 15) / 16;
        // TSKD_FILL16_STAGED (default 1, read per launch so both live in one
        // process): packed rows whose span fits the LDS row and the ring are
        // staged once per group; 0 keeps the per-lane L1 loop below.
        const char* sk = getenv("TSKD_FILL16_STAGED");
        const int span = np + win_buckets - 1;
        if (bst == 2 && span <= F16_SLOTS && span <= G &&
            !(sk && atoi(sk) == 0)) {
            const dim3 grid(grid_for(nsc4, 1));
#define FILL16_STAGED(WB, NQ)                                                 \
    hipLaunchKernelGGL((window_fill16_staged_kernel<WB, NQ>), grid,           \
                       dim3(256), 0, (hipStream_t)stream, bsum, proc,         \
                       last_val, S, C, G, phead, np, win_buckets, dstate)
            if (win_buckets == 36 && span <= 48) FILL16_STAGED(36, 3);
            else if (win_buckets == 36) FILL16_STAGED(36, 4);
            else FILL16_STAGED(0, 4);
#undef FILL16_STAGED
            return (int)hipGetLastError();
        }
        hipLaunchKernelGGL(window_fill16_kernel, dim3(grid_for(nsc4, 1)),
                           dim3(256), 0, (hipStream_t)stream, bsum, bcnt,
                           proc, last_val, S, C, G, phead, np, win_buckets,
                           dstate, bst);
        return (int)hipGetLastError();
    }
    const long nsc = (long)S * C * WAVE;  // one wave per (stream, channel)
    hipLaunchKernelGGL(window_fill_kernel, dim3(grid_for(nsc, 256)), dim3(256),
                       0, (hipStream_t)stream, bsum, bcnt, proc, last_val, S,
                       C, G, phead, np, win_buckets, dstate, bst);
    return (int)hipGetLastError();
}

int tskd_preproc_advance_state(long long* dstate, int nb, int np,
                               void* stream) {
    hipLaunchKernelGGL(advance_state_kernel, dim3(1), dim3(64), 0,
                       (hipStream_t)stream, dstate, nb, np);
    return (int)hipGetLastError();
}

int tskd_preproc_window_gather(const float* proc, void* out, int out_is_bf16,
                               int out_timelast, int S, int C, int G, int B,
                               int WIN, int stride, long end,
                               const long long* dstate, int end_extra,
                               void* stream) {
    if (WIN % 4 != 0) return -3;  // vectorized gather needs WIN % 4 == 0
    const long n = (long)S * B * C * (WIN / 4);
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool tlast2 = C % 2 == 0;  // v2 packs channel pairs into dwords
    const long n2 = (long)S * B * WIN;  // v2: thread per (s, b, t)
    if (out_is_bf16) {
        if (out_timelast && tlast2)
            hipLaunchKernelGGL((window_gather_tlast2_kernel<unsigned short>),
                               dim3(grid_for(n2, 256)), dim3(256), 0, st,
                               proc, (unsigned short*)out, S, C, G, B, WIN,
                               stride, end, dstate, end_extra);
        else if (out_timelast)
            hipLaunchKernelGGL((window_gather_kernel<unsigned short, true>),
                               dim3(grid_for(n, 256)), dim3(256), 0, st, proc,
                               (unsigned short*)out, S, C, G, B, WIN, stride,
                               end, dstate, end_extra);
        else
            hipLaunchKernelGGL((window_gather_kernel<unsigned short>),
                               dim3(grid_for(n, 256)), dim3(256), 0, st, proc,
                               (unsigned short*)out, S, C, G, B, WIN, stride,
                               end, dstate, end_extra);
    } else {
        if (out_timelast && tlast2)
            hipLaunchKernelGGL((window_gather_tlast2_kernel<float>),
                               dim3(grid_for(n2, 256)), dim3(256), 0, st,
                               proc, (float*)out, S, C, G, B, WIN, stride,
                               end, dstate, end_extra);
        else if (out_timelast)
            hipLaunchKernelGGL((window_gather_kernel<float, true>),
                               dim3(grid_for(n, 256)), dim3(256), 0, st, proc,
                               (float*)out, S, C, G, B, WIN, stride, end,
                               dstate, end_extra);
        else
            hipLaunchKernelGGL((window_gather_kernel<float>),
                               dim3(grid_for(n, 256)), dim3(256), 0, st, proc,
                               (float*)out, S, C, G, B, WIN, stride, end,
                               dstate, end_extra);
    }
    return (int)hipGetLastError();
}

int tskd_preproc_window_znorm(void* w, int is_bf16, long rows, int win,
                              float eps, void* stream) {
    if (rows <= 0) return 0;
    const int grid = grid_for(rows * WAVE, 256);
    if (is_bf16)
        hipLaunchKernelGGL((window_znorm_kernel<unsigned short>), dim3(grid),
                           dim3(256), 0, (hipStream_t)stream,
                           (unsigned short*)w, rows, win, eps);
    else
        hipLaunchKernelGGL((window_znorm_kernel<float>), dim3(grid), dim3(256),
                           0, (hipStream_t)stream, (float*)w, rows, win, eps);
    return (int)hipGetLastError();
}

}  // extern "C"
