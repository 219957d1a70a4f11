// assoc.hip -- the association network's forward pass on gfx950.
//
// Reference (likojack/ODAM src/models/associator.py:163-312): keypoint encoder MLP, sine frame-index encoding,
// 2 self-attention GNN layers over each track's time steps, average pooling over time, 8 alternating self/cross
// GNN layers between tracks and detections (4 heads of 64), final projection, score matrix / 16, 100 Sinkhorn
// iterations in log space.  The reference runs ~300 tiny PyTorch kernels per frame for this; here every Conv1d(k=1)
// is a conv_gemm launch (fp32 MFMA), attention is the fused kernel with head dimension 64, and the whole Sinkhorn
// loop is ONE single-workgroup kernel (assoc_sinkhorn.hip).  Beside this file: the track-window store that builds the network's
// track input (assoc_trackwin.hip) and the Hungarian / attach step behind it (assoc_match.hip).
//
// Layout: token-major rows.  A token set lives in a [N, 512] buffer "cat": columns 0..255 hold x, columns
// 256..511 receive the attention message, so cat([x, message]) (associator.py:97) needs no copy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/odam_assoc.h"
#include "assoc_internal.h"
#include "conv_gemm.h"
#include "detr_kernels.h"
#include "odam_config.h"
#include "odam_err.h"
#include "wave_ops.h"

using namespace odam_assoc_internal;      // launch_sinkhorn, PG_GROUPS, PG_BAR_WORDS
using odam_cg::ConvGemmArgs;

namespace {

constexpr int D = 256, NF = 79, NT = 100, ND = 30, FPAD = 128;

// ---- kernels ------------------------------------------------------------------------------------------------------
// in [n_seq, 79, L] channel-first (row 0 = frame index, rows 1..78 features) ->
// feat [n_seq*L, 128] (features, zero padded) and cat[:, 0:256] = sine encoding of the frame index
// A second input (in2: n_tok2 tokens of sequences of length L2) continues the token rows behind the first: tracks and detections in
// one launch.
__global__ __launch_bounds__(256) void prepare_kernel(const float* __restrict__ in, int L, int n_tok,
                                                      const float* __restrict__ div_term, float* __restrict__ feat,
                                                      float* __restrict__ cat, const float* __restrict__ in2 = nullptr, int L2 = 1, int n_tok2 = 0) {
    const int tok = blockIdx.x;
    if (tok >= n_tok + n_tok2) return;
    if (tok >= n_tok) { in = in2; L = L2; }
    const int t = tok >= n_tok ? tok - n_tok : tok;
    const int s = t / L, l = t - s * L;
    const float* src = in + (size_t)s * NF * L + l;
    const int c = threadIdx.x;
    if (c < FPAD) feat[(size_t)tok * FPAD + c] = (c < NF - 1) ? src[(size_t)(c + 1) * L] : 0.0f;
    const float pos = src[0];
    const float a = pos * div_term[c >> 1];                    // associator.py:325-326
    cat[(size_t)tok * 512 + c] = (c & 1) ? cosf(a) : sinf(a);
}

// F.avg_pool1d over the L time steps of each track: out[s, c] = mean_l cat[(s*L + l), c]   (associator.py:231-232)
// ... and blocks T .. T + n_tail - 1 move the rows that follow the n_seq sequences in `cat` (the encoded detections, which went through
// the encoder launches as 30 more rows of the same matrix) behind the means: out becomes the [T + 30] row block of the matching GNN
__global__ __launch_bounds__(256) void time_mean_kernel(const float* __restrict__ cat, int L, float* __restrict__ out, int n_seq) {
    const int s = blockIdx.x, c = threadIdx.x;
    if (s >= n_seq) {
        out[(size_t)s * 512 + c] = cat[((size_t)n_seq * L + (s - n_seq)) * 512 + c];
        return;
    }
    const float* p = cat + (size_t)s * L * 512 + c;
    float acc = 0.0f;
    int l = 0;
    for (; l + 10 <= L; l += 10) {          // ten rows in flight, added in order (the sum is the sequential one)
        float v[10];
#pragma unroll
        for (int i = 0; i < 10; i++) v[i] = p[(size_t)(l + i) * 512];
#pragma unroll
        for (int i = 0; i < 10; i++) acc += v[i];
    }
    for (; l < L; l++) acc += p[(size_t)l * 512];
    out[(size_t)s * 512 + c] = acc / (float)L;
}

// ---- the matching GNN + final projection as ONE persistent launch ----------------------------------------
// At 40 tracks the GNN is 8 layers x 6 launches on <= 70 rows: every launch is a dispatch and a memory round trip long
// (~10 us) however little it computes.  This kernel keeps PG_WG workgroups resident (one per CU) and walks the same stages
// with a device-wide barrier in between (5 per layer).  A stage is a few hundred independent 16x16 output blocks, ONE per
// single-wave workgroup: the data path of a CU, not the arithmetic, is what a stage costs (a block reads 16 rows of the
// input and 16 rows of the weights, 32-64 KB; with 8 blocks per CU a stage took 11 us), so the blocks are spread over all
// CUs and half a block's operand bytes are in flight before the first v_mfma_f32_16x16x4_f32 issues.
//
// Coherence without cache maintenance: bytes one workgroup writes and another reads later in the launch are stored and
// loaded with sc1 (agent-coherent: written through / fetched past the non-coherent L1 and L2 lines), the stores are
// drained (vmcnt(0)) before the barrier's counter is touched, and the counters are relaxed agent-scope atomics
// (MI355X_MICROARCH.md, inter-workgroup visibility, second valid form).  Release / acquire fences at the barrier instead
// write back and invalidate the whole L2 40 times per launch, weights included.  The weights are read-only: plain loads.
// Barrier: two levels -- 8 group counters (workgroup id % 8; 32 arrivals each on its own line), the last arrival of a group
// bumps the global generation every workgroup polls; the spin is bounded so a lost workgroup cannot hang the device.
constexpr int PG_WG = 256, PG_NT = 256, PG_NW = PG_NT / 64, PG_MAXL = 16;      // PG_GROUPS, PG_BAR_WORDS (the barrier words): assoc_internal.h
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct GnnLayerW { const float *qkv_w, *qkv_b, *mg_w, *mg_b, *m0_w, *m0_b, *m2_w, *m2_b; int cross; };
struct GnnArgs {
    GnnLayerW L[PG_MAXL];
    int n_layers;
    const float *fin_w, *fin_b;
    float *X, *kv, *att, *h, *mT;     // [MX][512], [MX][768], [MX][256], [MX][512], [MX + 2][256]
    float* kv2;                       // second [MX][768] (the row-partitioned kernel alternates between the two by layer)
    int T;
    unsigned* bar;                    // [0] generation, [1] error flag (a barrier timed out), [32 (1 + g)] group counters; zeroed before every launch
    unsigned long long timeout_ticks; // bound of one barrier wait in 100 MHz ticks (0: give up at the first barrier -- tests)
    unsigned long long* stamps;       // diagnostics (odam_assoc_stage_stamps): 100 MHz timer of workgroup 0 after every stage, or null
    int fake_misplaced;               // tests (odam_assoc_debug_misplace): gnn_rowpart_kernel's placement check behaves as if a group straddled XCDs
};

constexpr int SC1 = 16;      // cache-policy bit of the buffer intrinsics on gfx94x / gfx950
__device__ __forceinline__ __amdgpu_buffer_rsrc_t coh_buf(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ float4 coh_ld4(__amdgpu_buffer_rsrc_t r, int float_idx) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, float_idx * 4, 0, SC1));
}
__device__ __forceinline__ float coh_ld(__amdgpu_buffer_rsrc_t r, int float_idx) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, float_idx * 4, 0, SC1));
}
__device__ __forceinline__ void coh_st(__amdgpu_buffer_rsrc_t r, int float_idx, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, float_idx * 4, 0, SC1);
}

// Returns false when the launch is lost: this workgroup waited longer than the bound (not every workgroup became resident:
// a foreign kernel holds CUs, or the device is smaller than the host's gate assumed), or another one said so.  A lost launch
// is abandoned at once -- every workgroup returns at its next barrier instead of spinning through the remaining stages --
// and reported: the flag turns Z into NaN in the Sinkhorn kernel and bumps a host-visible counter, and the host re-runs the
// frame through the launch sequence (odam_assoc_forward_sequence).  The counters are zeroed before every launch, so one
// lost launch does not poison the next.
__device__ __forceinline__ bool grid_barrier(unsigned* bar, unsigned& target, unsigned long long timeout_ticks, int* lost) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's sc1 stores are at their coherence point
    __syncthreads();
    target += PG_GROUPS;
    if (threadIdx.x == 0) {
        unsigned* grp = bar + 32 * (1 + (blockIdx.x & (PG_GROUPS - 1)));
        const unsigned old = __hip_atomic_fetch_add(grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (((old + 1u) & (PG_WG / PG_GROUPS - 1)) == 0u) __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long* word = reinterpret_cast<unsigned long long*>(bar);      // generation | error flag << 32: one poll sees both
        bool ok = timeout_ticks != 0;
        const unsigned long long t0 = wall_clock64();
        for (int spins = 0; ok; ++spins) {
            const unsigned long long w = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)(w >> 32)) { ok = false; break; }
            if ((int)((unsigned)w - target) >= 0) break;
            __builtin_amdgcn_s_sleep(1);
            if ((spins & 63) == 63 && wall_clock64() - t0 > timeout_ticks) ok = false;
        }
        if (!ok) __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *lost = ok ? 0 : 1;
    }
    __syncthreads();
    return *lost == 0;
}

// The stages of a GNN layer, ONE set for both persistent kernels: a stage works on the rows [r0, r0 + nR) and deals its items to the
// caller's workers (first item, stride).  gnn_persistent_kernel passes all rows and all 256 workgroups, gnn_rowpart_kernel the rows of
// its XCD and that XCD's 32 workgroups; an output element is computed by the same instructions either way: the kernels agree bit for bit.
// FAR: the output is read by workgroups behind ANOTHER L2 before the next device-wide barrier, so it is stored sc1 (written through to
// the coherence point); otherwise the readers share this XCD's L2, and a plain store, drained by the XCD-local barrier, is enough.
// Rows that were exchanged are always LOADED sc1 (past the non-coherent vector L1); the weights are read-only: plain, cached.
//
// Y[r0 .. r0 + nR, N] = act(X W[N, K]^T + b (+ res)); one 16x16 output block per workgroup and item (wi, then every nw-th), wave w
// takes k in [w K / 4, (w + 1) K / 4).  v_mfma_f32_16x16x4_f32: lane l carries A[row l % 16][k l / 16] and B[col l % 16][k l / 16];
// a lane's 16-byte load holds the k slots of four consecutive instructions (A and B permute k the same way).
// (One ascending-k chain per output on a single wave was tried as well: 386 us per launch instead of 250.)
template <int K, bool RELU, bool FAR>
__device__ void stage_gemm(const float* X, int lda, const float* W, const float* b, int r0, int nR, int N, const float* res,
                           float* Y, int ldc, float* red, int wave, int lane, int wi, int nw) {
    constexpr int KW = K / PG_NW, NL = KW / 16;            // k per wave, 16-byte loads per lane and operand
    const int RB = (nR + 15) >> 4, CB = N >> 4, rlim = r0 + nR;
    const int li = lane & 15, kq = lane >> 4;
    const __amdgpu_buffer_rsrc_t xb = coh_buf(X), yb = coh_buf(Y), rsb = coh_buf(res ? res : Y);
    for (int item = wi; item < RB * CB; item += nw) {
        const int rb = item / CB, cb = item - rb * CB;
        const int r = r0 + rb * 16 + li;
        const int xo = (r < rlim ? r : rlim - 1) * lda + wave * KW + 4 * kq;
        const float* wp = W + (size_t)(cb * 16 + li) * K + wave * KW + 4 * kq;
        float4 a[NL], w[NL];
#pragma unroll
        for (int t = 0; t < NL; t++) {
            a[t] = coh_ld4(xb, xo + 16 * t);
            w[t] = *reinterpret_cast<const float4*>(wp + 16 * t);
        }
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NL; t++) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, w[t].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, w[t].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, w[t].z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, w[t].w, acc1, 0, 0, 0);
        }
        const f32x4 part = acc0 + acc1;
        if (wave) *reinterpret_cast<f32x4*>(red + ((wave - 1) * 64 + lane) * 4) = part;
        __syncthreads();
        if (wave == 0) {
            f32x4 tot = part;
#pragma unroll
            for (int w2 = 0; w2 < PG_NW - 1; w2++) tot += *reinterpret_cast<const f32x4*>(red + (w2 * 64 + lane) * 4);
            const int col = cb * 16 + li;
            const float bias = b ? b[col] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) {      // accumulator register i of lane l: row 4 (l / 16) + i, column l % 16
                const int row = r0 + rb * 16 + 4 * kq + i;
                if (row < rlim) {
                    float v = tot[i] + bias;
                    if (res) v += coh_ld(rsb, row * ldc + col);
                    if (RELU) v = fmaxf(v, 0.0f);
                    if (FAR) coh_st(yb, row * ldc + col, v);
                    else Y[(size_t)row * ldc + col] = v;
                }
            }
        }
        __syncthreads();
    }
}

// softmax(Q K^T / 8) V per (query row, head) for the queries [r0, r0 + nR), head dimension 64 (associator.py:75-82); one wavefront
// per item (wave_x, then every n_waves-th): lane j scores key j, lane d accumulates output channel d, 64 source rows at a time (online
// softmax across chunks); the key rows and the value columns of a chunk are all in flight together.  Keys and values of every row
// come from kv (sc1 loads).  sc: this wave's LDS strip [64].
template <int ldatt, bool FAR>
__device__ void stage_attn(const float* kv, int T, int cross, float* att, float* sc, int r0, int nR, int wave_x, int n_waves, int lane) {
    const __amdgpu_buffer_rsrc_t kb = coh_buf(kv);
    for (int item = wave_x; item < nR * 4; item += n_waves) {
        const int q = r0 + (item >> 2), hd = item & 3;
        const bool is_track = q < T;
        const bool src_tracks = is_track != (cross != 0);
        const int src0 = src_tracks ? 0 : T, nsrc = src_tracks ? T : ND;
        const int qo = q * 768 + hd * 64;
        float4 qq[16];
#pragma unroll
        for (int d = 0; d < 16; d++) qq[d] = coh_ld4(kb, qo + 4 * d);
        float run_max = -INFINITY, run_sum = 0.0f, o = 0.0f;
        for (int j0 = 0; j0 < nsrc; j0 += 64) {
            const int j = j0 + lane, nj = nsrc - j0 < 64 ? nsrc - j0 : 64;
            const int ko = (src0 + (j < nsrc ? j : nsrc - 1)) * 768 + 256 + hd * 64;
            const int vo = (src0 + j0) * 768 + 512 + hd * 64 + lane;
            float4 kk[16];
            float vv[64];
#pragma unroll
            for (int d = 0; d < 16; d++) kk[d] = coh_ld4(kb, ko + 4 * d);
#pragma unroll
            for (int jj = 0; jj < 64; jj++) vv[jj] = coh_ld(kb, vo + (jj < nj ? jj : nj - 1) * 768);
            float acc = 0.0f;
#pragma unroll
            for (int d = 0; d < 16; d++) {
                acc += qq[d].x * kk[d].x; acc += qq[d].y * kk[d].y; acc += qq[d].z * kk[d].z; acc += qq[d].w * kk[d].w;
            }
            const float sdot = j < nsrc ? acc * 0.125f : -INFINITY;
            const float mx = fmaxf(run_max, wave_reduce(sdot, [](float a, float b) { return fmaxf(a, b); }));
            const float p = j < nsrc ? expf(sdot - mx) : 0.0f;
            const float corr = expf(run_max - mx);            // 0 on the first chunk (run_max = -inf)
            run_sum = run_sum * corr + wave_sum(p);
            run_max = mx;
            sc[lane] = p;
            __builtin_amdgcn_wave_barrier();
            o *= corr;
#pragma unroll
            for (int jj = 0; jj < 64; jj++) o += (jj < nj ? sc[jj] : 0.0f) * vv[jj];
            __builtin_amdgcn_wave_barrier();
        }
        if (FAR) coh_st(coh_buf(att), q * ldatt + hd * 64 + lane, o / run_sum);
        else att[(size_t)q * ldatt + hd * 64 + lane] = o / run_sum;
    }
}

// MERGED = odam_config assoc.merge: m0_w / m0_b hold [W0x | W0m Wm] / b0 + W0m bm, the attention writes into X[:, 256:], no merge stage
// (two instantiations: one kernel holding both forms went from 245 to 248 + 32 registers and 256 B of scratch)
template <bool MERGED>
__global__ __launch_bounds__(PG_NT) void gnn_persistent_kernel(GnnArgs a) {
    __shared__ float red[(PG_NW - 1) * 64 * 4];
    __shared__ float scs[PG_NW * 64];
    __shared__ int lost;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = blockIdx.x, nw = PG_WG;                 // every stage: all rows, dealt to all workgroups, stored FAR
    const int wave_g = wave * PG_WG + blockIdx.x, n_waves = PG_WG * PG_NW;      // consecutive attention items go to different workgroups
    unsigned target = 0;
    const int T = a.T, MX = T + ND;
    int n_stamp = 0;
    auto stamp = [&] { if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[n_stamp++] = wall_clock64(); };
#define PG_BARRIER() do { if (!grid_barrier(a.bar, target, a.timeout_ticks, &lost)) return; stamp(); } while (0)
    stamp();
    float* sc = scs + wave * 64;
    for (int l = 0; l < a.n_layers; l++) {
        const GnnLayerW& P = a.L[l];
        stage_gemm<D, false, true>(a.X, 512, P.qkv_w, P.qkv_b, 0, MX, 3 * D, nullptr, a.kv, 3 * D, red, wave, lane, wi, nw);
        PG_BARRIER();
        if constexpr (MERGED) {      // the attention's rows ARE the second half of the MLP's input (merge folded into m0_w)
            stage_attn<512, true>(a.kv, T, P.cross, a.X + D, sc, 0, MX, wave_g, n_waves, lane);
            PG_BARRIER();
        } else {
            stage_attn<256, true>(a.kv, T, P.cross, a.att, sc, 0, MX, wave_g, n_waves, lane);
            PG_BARRIER();
            stage_gemm<D, false, true>(a.att, D, P.mg_w, P.mg_b, 0, MX, D, nullptr, a.X + D, 512, red, wave, lane, wi, nw);
            PG_BARRIER();
        }
        stage_gemm<2 * D, true, true>(a.X, 512, P.m0_w, P.m0_b, 0, MX, 2 * D, nullptr, a.h, 2 * D, red, wave, lane, wi, nw);
        PG_BARRIER();
        stage_gemm<2 * D, false, true>(a.h, 2 * D, P.m2_w, P.m2_b, 0, MX, D, a.X, a.X, 512, red, wave, lane, wi, nw);
        PG_BARRIER();
    }
    stage_gemm<D, false, true>(a.X, 512, a.fin_w, a.fin_b, 0, MX, D, nullptr, a.mT, D, red, wave, lane, wi, nw);
    stamp();
}

// ---- the same network, ROWS DEALT TO THE XCDs: one device-wide barrier per layer instead of five -------------------------------------
// Of a layer's five stages only the attention needs rows of other workgroups' making in bulk -- keys and values of ALL rows; the
// projections and the MLP are row-wise.  Workgroup b of a plain launch always runs on XCD b mod 8 (tests/native/xcd_probe.hip), and an
// exchange among the 32 workgroups of one XCD -- plain stores, sc1 loads that hit that XCD's L2, a workgroup-scope counter executed
// in that L2 -- costs 1.1 us where the device-wide form costs 4.9 (tests/native/xcd_barrier_probe.hip).  So XCD x owns rows
// [x R, (x + 1) R), R = ceil(rows / 8): its workgroups project q | k | v of those rows (stored sc1: the one thing that crosses XCDs),
// all 256 workgroups meet ONCE, then attention, merge and the two MLP layers of those rows run behind XCD-local barriers.  Every
// output element is computed by the stage functions gnn_persistent_kernel calls (same 16x16 blocks, same K split over the four
// waves): the two kernels agree bit for bit.  k | v alternate between two buffers by layer: a fast XCD may project layer l + 1 while a slow one still
// reads layer l's keys (the device barrier of layer l + 1 is what frees buffer l & 1 again).
__device__ __forceinline__ bool xcd_barrier(unsigned* bar, unsigned* cnt, unsigned& target, unsigned long long timeout_ticks, int* lost) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's stores have reached the L2 the readers will hit
    __syncthreads();
    target += PG_WG / PG_GROUPS;
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        bool ok = timeout_ticks != 0;
        const unsigned long long t0 = wall_clock64();
        for (int spins = 0; ok; ++spins) {
            unsigned g, e;      // sc0 sc1: past the vector L1 (an sc0-only poll can spin on a stale line)
            asm volatile("global_load_dword %0, %2, off sc0 sc1\n\tglobal_load_dword %1, %3, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(g), "=&v"(e) : "v"(cnt), "v"(bar + 1) : "memory");
            if (e) { ok = false; break; }
            if ((int)(g - target) >= 0) break;
            __builtin_amdgcn_s_sleep(1);
            if ((spins & 63) == 63 && wall_clock64() - t0 > timeout_ticks) ok = false;
        }
        if (!ok) __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *lost = ok ? 0 : 1;
    }
    __syncthreads();
    return *lost == 0;
}

template <bool MERGED>
__global__ __launch_bounds__(PG_NT) void gnn_rowpart_kernel(GnnArgs a) {
    __shared__ float red[(PG_NW - 1) * 64 * 4];
    __shared__ float scs[PG_NW * 64];
    __shared__ int lost;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xcd = blockIdx.x & (PG_GROUPS - 1), wi = blockIdx.x >> 3, nw = PG_WG / PG_GROUPS;
    const int T = a.T, MX = T + ND;
    const int R = (MX + PG_GROUPS - 1) / PG_GROUPS;
    const int r0 = xcd * R, nR = MX - r0 < 0 ? 0 : (MX - r0 < R ? MX - r0 : R);      // the rows of this XCD (the last XCDs may have none)
    const int wave_x = wave * nw + wi, n_waves = nw * PG_NW;
    unsigned target = 0, target_x = 0;
    unsigned* cnt_x = a.bar + 32 * (1 + PG_GROUPS + xcd);
    int n_stamp = 0;
    auto stamp = [&] { if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[n_stamp++] = wall_clock64(); };
#define PX_BARRIER() do { if (!xcd_barrier(a.bar, cnt_x, target_x, a.timeout_ticks, &lost)) return; stamp(); } while (0)
    // Placement check.  The XCD-local stages below are exchanged with plain stores and a workgroup-scope counter, which is right only
    // if the 32 workgroups of a group (equal blockIdx mod 8) run behind ONE L2.  That is how the dispatcher has always placed a plain
    // launch here (tests/native/xcd_probe.hip), but HIP promises nothing: every workgroup reads the hardware's XCC id and the first of a
    // group to arrive records it; one that finds another id raises the launch's error flag -- every workgroup then returns at its
    // first barrier, the Sinkhorn kernel reports the launch as lost and the host re-runs the frame through the launch sequence
    // (and, after three such losses in a row, stays on it: associator.py).
    if (tid == 0) {
        const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) + 1u;       // HW_REG_XCC_ID [3:0], + 1: 0 = nobody yet
        unsigned seen = 0u;
        if (!__hip_atomic_compare_exchange_strong(a.bar + 32 * (1 + 2 * PG_GROUPS) + xcd, &seen, xcc, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &&
            (seen != xcc || a.fake_misplaced))
            __hip_atomic_store(a.bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    stamp();
    float* sc = scs + wave * 64;
    for (int l = 0; l < a.n_layers; l++) {
        const GnnLayerW& P = a.L[l];
        float* kv = (l & 1) ? a.kv2 : a.kv;
        stage_gemm<D, false, true>(a.X, 512, P.qkv_w, P.qkv_b, r0, nR, 3 * D, nullptr, kv, 3 * D, red, wave, lane, wi, nw);
        PG_BARRIER();
        if constexpr (MERGED) {
            stage_attn<512, false>(kv, T, P.cross, a.X + D, sc, r0, nR, wave_x, n_waves, lane);
            PX_BARRIER();
        } else {
            stage_attn<256, false>(kv, T, P.cross, a.att, sc, r0, nR, wave_x, n_waves, lane);
            PX_BARRIER();
            stage_gemm<D, false, false>(a.att, D, P.mg_w, P.mg_b, r0, nR, D, nullptr, a.X + D, 512, red, wave, lane, wi, nw);
            PX_BARRIER();
        }
        stage_gemm<2 * D, true, false>(a.X, 512, P.m0_w, P.m0_b, r0, nR, 2 * D, nullptr, a.h, 2 * D, red, wave, lane, wi, nw);
        PX_BARRIER();
        stage_gemm<2 * D, false, false>(a.h, 2 * D, P.m2_w, P.m2_b, r0, nR, D, a.X, a.X, 512, red, wave, lane, wi, nw);
        PX_BARRIER();
    }
#undef PG_BARRIER
#undef PX_BARRIER
    stage_gemm<D, false, false>(a.X, 512, a.fin_w, a.fin_b, r0, nR, D, nullptr, a.mT, D, red, wave, lane, wi, nw);
    stamp();
}

int lin(const Lin& L, const float* x, int lda, int M, const float* res, bool relu, float* y, int ldc, const float* scale,
        hipStream_t st) {
    ConvGemmArgs a{};
    a.A = x; a.Wt = L.w; a.scale = scale; a.bias = L.b; a.res = res; a.C = y;
    a.B = 1; a.H = 1; a.W = M; a.Cin = L.K; a.lda = lda;
    int lg = 0; while ((1 << lg) < L.K) lg++;
    a.log2Cin = lg;
    a.Ho = 1; a.Wo = M; a.Cout = L.N; a.KH = a.KW = 1; a.stride = 1; a.pad = 0; a.Kpad = L.K;
    a.relu = relu ? 1 : 0; a.M = M; a.ldc = ldc;
    a.no_pin = 1;      // replicated on every rank with identical rows: nothing to pin, and 4,000 rows want the small tiles
    return odam_cg::launch_conv_gemm(a, st);
}

#define RC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

}  // namespace

int odam_assoc_internal::assoc_lin(const Lin& L, const float* x, int lda, int M, const float* res, bool relu, float* y, int ldc,
                                   const float* scale, hipStream_t st) {
    return lin(L, x, lda, M, res, relu, y, ldc, scale, st);
}

namespace {

const HostT* findw(odam_assoc* m, const std::string& n) {
    auto it = m->host.find(n);
    return it == m->host.end() ? nullptr : &it->second;
}
#define NEEDW(var, name)                                                                                  \
    const HostT* var = findw(m, name);                                                                     \
    if (!var) {                                                                                            \
        std::snprintf(g_odam_err, sizeof(g_odam_err), "odam_assoc_finalize: missing weight %s", std::string(name).c_str()); \
        return 1;                                                                                          \
    }

// Conv1d(k=1) weight [N, K(,1)] + bias -> Lin with K padded to Kp; optional row/column permutations
int pack(odam_assoc* m, Lin& L, const HostT& w, const HostT* b, int Kp, const std::vector<int>* row_perm,
         const std::vector<int>* col_perm) {
    const int N = (int)w.shape[0], K = (int)w.shape[1];
    std::vector<float> p((size_t)N * Kp, 0.0f), bb(N, 0.0f);
    for (int r = 0; r < N; r++) {
        const int sr = row_perm ? (*row_perm)[r] : r;
        for (int c = 0; c < K; c++) {
            const int sc = col_perm ? (*col_perm)[c] : c;
            p[(size_t)r * Kp + c] = w.data[(size_t)sr * K + sc];
        }
        if (b) bb[r] = b->data[sr];
    }
    L.K = Kp; L.N = N;
    if (int rc = m->upload(&L.w, p)) return rc;
    return m->upload(&L.b, bb);
}

// the reference views the 256 projected channels as (dim 64, head 4): channel c = d*4 + h (associator.py:77-81);
// the attention kernel wants head-major channels c' = h*64 + d: perm[c'] = d*4 + h
std::vector<int> head_perm() {
    std::vector<int> p(D);
    for (int h = 0; h < 4; h++)
        for (int d = 0; d < 64; d++) p[h * 64 + d] = d * 4 + h;
    return p;
}

int pack_prop(odam_assoc* m, Prop& P, const std::string& pre) {
    const std::vector<int> hp = head_perm();
    NEEDW(w0, pre + "attn.proj.0.weight"); NEEDW(b0, pre + "attn.proj.0.bias");
    NEEDW(w1, pre + "attn.proj.1.weight"); NEEDW(b1, pre + "attn.proj.1.bias");
    NEEDW(w2, pre + "attn.proj.2.weight"); NEEDW(b2, pre + "attn.proj.2.bias");
    HostT wqkv, bqkv;        // query, key and value projections of one row block: one [768, 256] layer, rows head-major
    wqkv.shape = {3 * D, D};
    for (const HostT* w : {w0, w1, w2})
        for (int r = 0; r < D; r++)
            wqkv.data.insert(wqkv.data.end(), w->data.begin() + (size_t)hp[r] * D, w->data.begin() + (size_t)(hp[r] + 1) * D);
    for (const HostT* b : {b0, b1, b2})
        for (int r = 0; r < D; r++) bqkv.data.push_back(b->data[hp[r]]);
    bqkv.shape = {3 * D};
    RC(pack(m, P.qkv, wqkv, &bqkv, D, nullptr, nullptr));
    NEEDW(wm, pre + "attn.merge.weight"); NEEDW(bm, pre + "attn.merge.bias");
    RC(pack(m, P.merge, *wm, bm, D, nullptr, &hp));      // its input channels arrive head-major
    NEEDW(m0w, pre + "mlp.0.weight"); NEEDW(m0b, pre + "mlp.0.bias");
    NEEDW(m2w, pre + "mlp.2.weight"); NEEDW(m2b, pre + "mlp.2.bias");
    if (m->merged) {
        // message = Wm att + bm feeds only the first MLP layer, h = relu(W0x x + W0m message + b0) (associator.py:92-97): the same function of
        // [x | att] with W0' = [W0x | W0m Wm] and b0' = b0 + W0m bm -- products in binary64, rounded to float32 once.  att arrives head-major
        // (column c' of the attention's output is the reference's channel hp[c']), so the folded columns are taken in that order.
        HostT w0f, b0f;
        w0f.shape = {2 * D, 2 * D}; b0f.shape = {2 * D};
        w0f.data.resize((size_t)2 * D * 2 * D); b0f.data.resize(2 * D);
        for (int o = 0; o < 2 * D; o++) {
            const float* w0row = m0w->data.data() + (size_t)o * 2 * D;
            for (int c = 0; c < D; c++) w0f.data[(size_t)o * 2 * D + c] = w0row[c];
            for (int c = 0; c < D; c++) {
                double s_ = 0.0;
                for (int r = 0; r < D; r++) s_ += (double)w0row[D + r] * (double)wm->data[(size_t)r * D + hp[c]];
                w0f.data[(size_t)o * 2 * D + D + c] = (float)s_;
            }
            double sb = (double)m0b->data[o];
            for (int r = 0; r < D; r++) sb += (double)w0row[D + r] * (double)bm->data[r];
            b0f.data[o] = (float)sb;
        }
        RC(pack(m, P.m0, w0f, &b0f, 2 * D, nullptr, nullptr));
    } else {
        RC(pack(m, P.m0, *m0w, m0b, 2 * D, nullptr, nullptr));
    }
    RC(pack(m, P.m2, *m2w, m2b, 2 * D, nullptr, nullptr));
    return 0;
}

// self-attention layer over Bt sequences of L rows (the fuser): message into cat_x[:, 256:], delta added in place
int prop_forward_self(const Prop& P, float* cat_x, int Mx, int Bt, int L, float* qkvb, float* attb, float* hb, hipStream_t st, bool merged) {
    RC(lin(P.qkv, cat_x, 512, Mx, nullptr, false, qkvb, 3 * D, nullptr, st));
    if (merged) {      // the attention's rows are the second half of the MLP's input as they stand (merge folded into P.m0: pack_prop)
        RC(odam_dk::launch_attention_d64(qkvb, 3 * D, qkvb + D, 3 * D, qkvb + 2 * D, 3 * D, cat_x + D, 512, Bt, 4, L, L, st));
    } else {
        RC(odam_dk::launch_attention_d64(qkvb, 3 * D, qkvb + D, 3 * D, qkvb + 2 * D, 3 * D, attb, D, Bt, 4, L, L, st));
        RC(lin(P.merge, attb, D, Mx, nullptr, false, cat_x + D, 512, nullptr, st));
    }
    RC(lin(P.m0, cat_x, 512, Mx, nullptr, true, hb, 2 * D, nullptr, st));
    RC(lin(P.m2, hb, 2 * D, Mx, cat_x, false, cat_x, 512, nullptr, st));
    return 0;
}

}  // namespace

extern "C" int odam_assoc_create(int max_tracks, int n_self_layers, const int* gnn_is_cross, int n_gnn_layers,
                                 int sinkhorn_iters, odam_assoc** out) {
    if (!out || max_tracks < 1 || max_tracks > 1024 || n_self_layers < 0 || n_gnn_layers < 0 || !gnn_is_cross)
        return odam_fail(1, "odam_assoc_create: bad argument (1 <= max_tracks <= 1024)");
    odam_assoc* m = new odam_assoc();
    m->max_tracks = max_tracks; m->n_self = n_self_layers; m->n_gnn = n_gnn_layers; m->iters = sinkhorn_iters;
    m->gnn_cross.assign(gnn_is_cross, gnn_is_cross + n_gnn_layers);
    *out = m;
    return 0;
}

extern "C" int odam_assoc_destroy(odam_assoc* m) {
    if (!m) return 0;
    if (m->lost_count) (void)hipHostFree(m->lost_count);
    batch_release(m);
    if (m->init_stream) { (void)hipStreamSynchronize(m->init_stream); (void)hipStreamDestroy(m->init_stream); }
    for (void* p : m->allocs) (void)hipFree(p);
    delete m;
    return 0;
}

extern "C" int odam_assoc_set_weight(odam_assoc* m, const char* name, const float* data, const long long* shape, int ndim) {
    if (!m || !name || !data || ndim < 0 || ndim > 3 || m->finalized) return odam_fail(1, "odam_assoc_set_weight: bad argument");
    HostT t;
    size_t n = 1;
    for (int i = 0; i < ndim; i++) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    m->host[name] = std::move(t);
    return 0;
}

extern "C" int odam_assoc_finalize(odam_assoc* m) {
    if (!m) return odam_fail(1, "odam_assoc_finalize: null model");
    if (m->finalized) return 0;
    {
        NEEDW(w0, "encoder.0.weight"); NEEDW(b0, "encoder.0.bias");
        NEEDW(w2, "encoder.2.weight"); NEEDW(b2, "encoder.2.bias");
        RC(pack(m, m->enc0, *w0, b0, FPAD, nullptr, nullptr));
        RC(pack(m, m->enc2, *w2, b2, D, nullptr, nullptr));
        NEEDW(fw, "final_proj.weight"); NEEDW(fb, "final_proj.bias");
        RC(pack(m, m->final_proj, *fw, fb, D, nullptr, nullptr));
        NEEDW(bs, "bin_score");
        m->bin_score = bs->data[0];
        NEEDW(dv, "pe_div_term");
        if (dv->data.size() != D / 2) return odam_fail(1, "pe_div_term must have 128 entries");
        RC(m->upload(&m->div_term, dv->data));
        RC(m->upload(&m->sc16, std::vector<float>(ND, 1.0f / 16.0f)));   // scores / descriptor_dim ** 0.5
    }
    m->merged = odam_cfg::get(odam_cfg::ASSOC_MERGE) != 0;
    for (int i = 0; i < m->n_self; i++) {
        Prop P;
        RC(pack_prop(m, P, "fuser.layers." + std::to_string(i) + "."));
        m->fuser.push_back(P);
    }
    for (int i = 0; i < m->n_gnn; i++) {
        Prop P;
        RC(pack_prop(m, P, "gnn.layers." + std::to_string(i) + "."));
        m->gnn.push_back(P);
    }
    const size_t T = m->max_tracks, N = T * NT;
    // + the 30 detection rows behind the tracks', of every sample of a batched forward (assoc_batch.hip)
    constexpr size_t NDB = (size_t)ND * MAX_BATCH;
    RC(m->alloc(&m->feat, (N + NDB) * FPAD)); RC(m->alloc(&m->h256, (N + NDB) * D)); RC(m->alloc(&m->catT, (N + NDB) * 512));
    RC(m->alloc(&m->kv, N * 768)); RC(m->alloc(&m->att, N * D)); RC(m->alloc(&m->h512, N * 512));
    // fused tracks [T] and the 30 detection slots share one row block (detections start at row T of the frame) so the
    // shared-weight GNN layers see both sets as ONE matrix
    RC(m->alloc(&m->catTr, (T + ND) * 512));
    RC(m->alloc(&m->kvX, (T + ND) * 768)); RC(m->alloc(&m->kvX2, (T + ND) * 768)); RC(m->alloc(&m->attX, (T + ND) * D));
    RC(m->alloc(&m->hX, (T + ND) * 512));
    RC(m->alloc(&m->mT, (T + ND + 2) * D)); RC(m->alloc(&m->scores, T * 32));   // the score block reads 32 detection rows
    {
        float* b = nullptr;
        RC(m->alloc(&b, PG_BAR_WORDS));
        m->bar = reinterpret_cast<unsigned*>(b);
    }
    {
        float* b = nullptr;
        RC(m->alloc(&b, 256));
        m->stamps = reinterpret_cast<unsigned long long*>(b);
    }
    ODAM_HIP(hipHostMalloc((void**)&m->lost_count, 64, hipHostMallocDefault));
    *m->lost_count = 0u;
    // odam_config assoc.persist = 0 / odam_assoc_set_persistent(m, 0): the matching GNN as one launch per layer op (the
    // round-1 sequence; tests compare the two)
    m->persist = m->n_gnn <= PG_MAXL && odam_cfg::get(odam_cfg::ASSOC_PERSIST) != 0;
    {   // The persistent launch is a plain launch whose PG_WG workgroups wait for each other: all of them must be resident at
        // once.  How many fit is asked of the runtime for THIS kernel (246 VGPRs: two workgroups per CU), less one per CU
        // where it says more than one (MI355X_MICROARCH.md: the API reads one high for some SGPR counts), times the CUs;
        // a CU mask hides CUs from the launch without changing multiProcessorCount, so it turns the path off.
        int dev = 0, n_cu = 0, per_cu = 0;
        ODAM_HIP(hipGetDevice(&dev));
        ODAM_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        ODAM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)gnn_persistent_kernel<false>, PG_NT, 0));
        m->resident_capacity = (per_cu > 1 ? per_cu - 1 : per_cu) * n_cu;
        if (getenv("HSA_CU_MASK") != nullptr || getenv("ROC_GLOBAL_CU_MASK") != nullptr) m->resident_capacity = 0;
        if (m->resident_capacity < PG_WG) m->persist = false;
    }
    m->host.clear();
    // every buffer alloc() zeroed is zero from here on (see alloc)
    RC(m->init_done());
    m->finalized = true;
    return 0;
}

// encoder + frame-index encoding (associator.py:222-229) and the fuser, for one frame (n_det_rows = 30) or a batch of them
int odam_assoc_internal::encode_and_fuse(odam_assoc* m, const float* tracks, int T, const float* detections, int n_det_rows, hipStream_t st) {
    const int N = T * NT, NDR = n_det_rows;
    // The detections go through the encoder as 30 more rows of the tracks' matrix (rows N .. N + 29 of feat / catT: same weights, rows are
    // independent, and the same tile shape serves 30 and 100 T + 30 rows -- one launch per layer instead of two); time_mean_kernel moves
    // their encodings behind the track means afterwards.
    // (the same three launches on a second stream beside the tracks' branch, forked and joined by events: measured, no change; not kept)
    hipLaunchKernelGGL(prepare_kernel, dim3(N + NDR), dim3(256), 0, st, tracks, NT, N, m->div_term, m->feat, m->catT, detections, ND, NDR);
    ODAM_HIP(hipGetLastError());
    RC(lin(m->enc0, m->feat, FPAD, N + NDR, nullptr, true, m->h256, D, nullptr, st));
    RC(lin(m->enc2, m->h256, D, N + NDR, m->catT, false, m->catT, 512, nullptr, st));           // + pe, in place
    // fuser: self-attention over each track's 100 time steps (associator.py:143-160, 230)
    for (const Prop& P : m->fuser)
        RC(prop_forward_self(P, m->catT, N, T, NT, m->kv, m->att, m->h512, st, m->merged));
    return 0;
}

// the launch sequence of one forward: ~65 kernels, every one a memory round trip long at these sizes (<= 70 rows)
static int enqueue_forward(odam_assoc* m, const float* tracks, int T, const float* detections, int n_det, float* Z_out, hipStream_t st,
                           bool allow_persist = true) {
    float* X = m->catTr;                      // [T + 30][512]: fused tracks, then the detection slots (rows T ..)
    const int MX = T + ND;
    RC(encode_and_fuse(m, tracks, T, detections, ND, st));
    hipLaunchKernelGGL(time_mean_kernel, dim3(T + ND), dim3(256), 0, st, m->catT, NT, X, T);
    ODAM_HIP(hipGetLastError());
    // matching GNN between the fused tracks [T] and all 30 detection slots (associator.py:111-139, 240).  Both sets
    // go through the same weights, so every projection / MLP runs once on the [T + 30] row block; only the attention
    // differs per side (self: own set, cross: the other set).  All deltas come from the layer's inputs: the query,
    // key and value projections are taken before the residual update of either set.
    const bool persist = m->persist && allow_persist;
    if (persist) {
        GnnArgs g{};
        for (size_t i = 0; i < m->gnn.size(); i++) {
            const Prop& P = m->gnn[i];
            g.L[i] = GnnLayerW{P.qkv.w, P.qkv.b, P.merge.w, P.merge.b, P.m0.w, P.m0.b, P.m2.w, P.m2.b, m->gnn_cross[i] != 0 ? 1 : 0};
        }
        g.n_layers = (int)m->gnn.size();
        g.fin_w = m->final_proj.w; g.fin_b = m->final_proj.b;
        g.X = X; g.kv = m->kvX; g.kv2 = m->kvX2; g.att = m->attX; g.h = m->hX; g.mT = m->mT;
        g.T = T;
        g.bar = m->bar; g.timeout_ticks = m->timeout_ticks;
        g.stamps = m->want_stamps ? m->stamps : nullptr;
        g.fake_misplaced = m->fake_misplaced ? 1 : 0;
        // counters and the error flag start from zero every launch: zeroed here, unless the Sinkhorn kernel behind the previous launch did it
        if (!m->bar_clean) ODAM_HIP(hipMemsetAsync(m->bar, 0, sizeof(unsigned) * PG_BAR_WORDS, st));
        m->bar_clean = false;
        static void (*const kernels[2][2])(GnnArgs) = {{gnn_persistent_kernel<false>, gnn_rowpart_kernel<false>},      // [merged][rowpart]
                                                       {gnn_persistent_kernel<true>, gnn_rowpart_kernel<true>}};
        const bool rowpart = odam_cfg::get(odam_cfg::ASSOC_PERSIST) == 2;
        hipLaunchKernelGGL(kernels[m->merged][rowpart], dim3(PG_WG), dim3(PG_NT), 0, st, g);
        ODAM_HIP(hipGetLastError());
    } else {
        for (size_t i = 0; i < m->gnn.size(); i++) {
            const Prop& P = m->gnn[i];
            const bool cross = m->gnn_cross[i] != 0;
            RC(lin(P.qkv, X, 512, MX, nullptr, false, m->kvX, 3 * D, nullptr, st));     // rows: q | k | v
            const float* srcT = cross ? m->kvX + (size_t)T * 3 * D : m->kvX;     // source rows of the track queries
            const float* srcD = cross ? m->kvX : m->kvX + (size_t)T * 3 * D;     // ... of the detection queries
            const int nT = cross ? ND : T, nD = cross ? T : ND;
            float* attO = m->merged ? X + D : m->attX;
            const int ldO = m->merged ? 512 : D;
            RC(odam_dk::launch_attention_d64(m->kvX, 3 * D, srcT + D, 3 * D, srcT + 2 * D, 3 * D, attO, ldO, 1, 4, T, nT, st));
            RC(odam_dk::launch_attention_d64(m->kvX + (size_t)T * 3 * D, 3 * D, srcD + D, 3 * D, srcD + 2 * D, 3 * D,
                                             attO + (size_t)T * ldO, ldO, 1, 4, ND, nD, st));
            if (!m->merged) RC(lin(P.merge, m->attX, D, MX, nullptr, false, X + D, 512, nullptr, st));
            RC(lin(P.m0, X, 512, MX, nullptr, true, m->hX, 2 * D, nullptr, st));
            RC(lin(P.m2, m->hX, 2 * D, MX, X, false, X, 512, nullptr, st));
        }
        RC(lin(m->final_proj, X, 512, MX, nullptr, false, m->mT, D, nullptr, st));      // descriptors (associator.py:242-244)
    }
    // scores, optimal transport (associator.py:245-254).  Beside the persistent kernel too, the score matrix keeps its own launch on
    // the tiles of conv_gemm.hip: with saturated scores (the hand-built scene weights reach +-1000) the Sinkhorn loop shares a
    // detection's mass equally among several tracks and which of them the Hungarian step then picks hangs on the last bit of the
    // scores -- the reference-run fixtures (tests/test_e2e.py) hold for the summation order of that kernel, and a different order
    // moved 20 of 40 frames' tie-breaks.
    const float* mD = m->mT + (size_t)T * D;
    Lin sc; sc.w = const_cast<float*>(mD); sc.b = nullptr; sc.K = D; sc.N = ND;
    RC(lin(sc, m->mT, D, T, nullptr, false, m->scores, 32, m->sc16, st));
    if (!persist) return launch_sinkhorn(m->scores, 32, T, n_det, n_det, m->bin_score, m->iters, Z_out, nullptr, st);
    bool cleaned = false;      // the persistent launch's error flag goes along: a lost launch turns Z into NaN
    const int rc = launch_sinkhorn(m->scores, 32, T, n_det, n_det, m->bin_score, m->iters, Z_out, nullptr, st, m->bar + 1, m->lost_count, &cleaned);
    m->bar_clean = rc == 0 && cleaned;
    return rc;
}

// One frame (stream-ordered).  (Replaying the launch sequence from a hipGraph per track count was built in round 2 and measured
// no gain -- the sequence is bound by ~65 dependent kernels of ~10 us on the device, not by host launches -- and is gone.)
extern "C" int odam_assoc_forward(odam_assoc* m, const float* tracks, int T, const float* detections, int n_det,
                                  float* Z_out, void* stream) {
    if (!m || !tracks || !detections || !Z_out) return odam_fail(1, "odam_assoc_forward: null pointer");
    if (!m->finalized) return odam_fail(1, "odam_assoc_forward: call odam_assoc_finalize first");
    if (T < 1 || T > m->max_tracks || n_det < 1 || n_det > ND) return odam_fail(3, "odam_assoc_forward: T / n_det out of range");
    return enqueue_forward(m, tracks, T, detections, n_det, Z_out, (hipStream_t)stream);
}

// The same forward with the matching layers as separate launches (no device-wide barrier, no residency assumption): what
// the host re-runs a frame through when odam_assoc_lost_launches has moved.
extern "C" int odam_assoc_forward_sequence(odam_assoc* m, const float* tracks, int T, const float* detections, int n_det,
                                           float* Z_out, void* stream) {
    if (!m || !tracks || !detections || !Z_out) return odam_fail(1, "odam_assoc_forward_sequence: null pointer");
    if (!m->finalized) return odam_fail(1, "odam_assoc_forward_sequence: call odam_assoc_finalize first");
    if (T < 1 || T > m->max_tracks || n_det < 1 || n_det > ND) return odam_fail(3, "odam_assoc_forward_sequence: T / n_det out of range");
    return enqueue_forward(m, tracks, T, detections, n_det, Z_out, (hipStream_t)stream, false);
}

extern "C" int odam_assoc_lost_launches(odam_assoc* m, unsigned* count) {
    if (!m || !m->finalized || !count) return odam_fail(1, "odam_assoc_lost_launches: bad argument");
    *count = __atomic_load_n(m->lost_count, __ATOMIC_ACQUIRE);
    return 0;
}

extern "C" int odam_assoc_set_persistent(odam_assoc* m, int on) {
    if (!m || !m->finalized) return odam_fail(1, "odam_assoc_set_persistent: bad argument");
    m->persist = on != 0 && m->n_gnn <= PG_MAXL && m->resident_capacity >= PG_WG;
    return 0;
}

extern "C" int odam_assoc_info(odam_assoc* m, int* persistent, int* resident_capacity, int* workgroups) {
    if (!m || !m->finalized) return odam_fail(1, "odam_assoc_info: bad argument");
    if (persistent) *persistent = m->persist ? 1 : 0;
    if (resident_capacity) *resident_capacity = m->resident_capacity;
    if (workgroups) *workgroups = PG_WG;
    return 0;
}

extern "C" int odam_assoc_debug_misplace(odam_assoc* m, int on) {
    if (!m) return odam_fail(1, "odam_assoc_debug_misplace: null handle");
    m->fake_misplaced = on != 0;
    return 0;
}

extern "C" int odam_assoc_set_barrier_timeout_us(odam_assoc* m, long long us) {
    if (!m || us < 0) return odam_fail(1, "odam_assoc_set_barrier_timeout_us: bad argument");
    m->timeout_ticks = (unsigned long long)us * 100ull;
    return 0;
}

// One frame of OdamProcess.process_frame's device work behind ONE call (src/processor.py:320-337): the observations the previous frame
// attached (n_app <= 30 rows: odam_trackwin_append), this frame's track input for its camera (odam_trackwin_build_tracks) and the
// association forward on it (odam_assoc_forward) -- the same three entry points in the same order, so the results are theirs bit for
// bit; what goes is the host time between them (three binding calls, their argument marshalling and the interpreter in between, with the
// device idle).  tracks_out [dev][T][79][window] is the caller's buffer (it needs it again if the frame has to be re-run through
// odam_assoc_forward_sequence); detections / Z_out as in odam_assoc_forward (device or mapped pinned host memory).
extern "C" int odam_assoc_step(odam_assoc* m, odam_trackwin* w, struct odam_sq_ctx* sq, int n_app, const int* app_ids, const double* app_rows14,
                               int T, const double* T_cw12_K9, double cam_azi, double img_w, double img_h, const float* detections, int n_det,
                               float* tracks_out, float* Z_out, void* stream) {
    if (!m || !w || !sq || !tracks_out || !detections || !Z_out) return odam_fail(1, "odam_assoc_step: null pointer");
    if (n_app < 0 || n_app > 32) return odam_fail(1, "odam_assoc_step: at most 32 observations per frame");
    if (n_app) { if (int rc = odam_trackwin_append(w, n_app, app_ids, app_rows14, stream)) return rc; }
    if (int rc = odam_trackwin_build_tracks(w, sq, T, T_cw12_K9, cam_azi, img_w, img_h, tracks_out, stream)) return rc;
    return odam_assoc_forward(m, tracks_out, T, detections, n_det, Z_out, stream);
}

// diagnostics: run the next forwards with stage stamps (enable != 0), or read the stamps of the last one: out[0..n) =
// 100 MHz timer of workgroup 0 at kernel start and after every stage of the persistent matching kernel
extern "C" int odam_assoc_stage_stamps(odam_assoc* m, int enable, unsigned long long* out, int n) {
    if (!m || !m->finalized || n < 0 || n > 128) return odam_fail(1, "odam_assoc_stage_stamps: bad argument");
    m->want_stamps = enable != 0;
    if (out && n) {
        ODAM_HIP(hipDeviceSynchronize());
        ODAM_HIP(hipMemcpy(out, m->stamps, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return 0;
}

// diagnostics: a workspace buffer of the last forward ([host] out[n]): 0 = row block X [(T + 30), 512], 1 = descriptors mT
// [(T + 30), 256], 2 = scores [T, 32]; of the last BATCHED forward (assoc_batch.hip): 3 = the padded row block as assembled
// [(B Tmax + 30 B), 256], 4 = its descriptors [(B Tmax + 30 B), 256], 5 = its score blocks [sum T, 32]
extern "C" int odam_assoc_debug_read(odam_assoc* m, int which, float* out, long long n) {
    if (m && m->finalized && out && n > 0 && which >= 3 && which <= 5) return batch_debug_read(m, which, out, n);
    if (!m || !m->finalized || !out || n <= 0 || which < 0 || which > 2) return odam_fail(1, "odam_assoc_debug_read: bad argument");
    const float* src = which == 0 ? m->catTr : (which == 1 ? m->mT : m->scores);
    ODAM_HIP(hipDeviceSynchronize());
    ODAM_HIP(hipMemcpy(out, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
