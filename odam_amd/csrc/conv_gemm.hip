// conv_gemm.hip -- see conv_gemm.h
#include "conv_gemm.h"

#include "cg_common.hpp"
#include "cg_launch.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <mutex>

namespace odam_cg {

// ---- kernel-choice log ----------------------------------------------------------------------------------------------
static std::mutex g_path_mu;
static char g_path_ring[PATH_LOG_N][PATH_TOKEN_LEN];
static long long g_path_head = 0, g_path_base = 0;      // tokens noted since load / at the last reset

void note_path(const char* fmt, ...) {
    char tok[PATH_TOKEN_LEN];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tok, sizeof(tok), fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_path_mu);
    memcpy(g_path_ring[g_path_head % PATH_LOG_N], tok, sizeof(tok));
    g_path_head++;
}

long long read_paths(char* buf, int n, int reset) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    const long long noted = g_path_head - g_path_base;
    if (buf) {
        if (n <= 0) return -1;
        int used = 0;
        buf[0] = 0;
        for (long long i = std::max(g_path_base, g_path_head - PATH_LOG_N); i < g_path_head; i++) {
            const char* t = g_path_ring[i % PATH_LOG_N];
            const int len = (int)strlen(t);
            if (used + len + 2 > n) break;
            if (used) buf[used++] = '\n';
            memcpy(buf + used, t, len + 1);
            used += len;
        }
    }
    if (reset) g_path_base = g_path_head;
    return noted;
}

// NST: LDS stages.  2 = one tile in flight under the tile being multiplied (two workgroups per CU hide the rest).
// 4 (UT only; small, latency-bound problems that leave most CUs with one workgroup): three tiles in flight, retired
// with a counted s_waitcnt so the DMA queue stays full across the per-tile barrier.
template <int BM, int BN, int WM, int WN, bool BF16, bool UT, int NST = 2, bool X3 = false>
__global__ __launch_bounds__(64 * WM * WN) void conv_gemm_kernel(ConvGemmArgs a) {
    static_assert(NST == 2 || (UT && (NST & (NST - 1)) == 0), "deep pipelines are LDS-DMA only");
    static_assert(!X3 || (UT && !BF16), "split products: fp32 operands on the LDS-DMA path");
    using T = typename std::conditional<BF16, unsigned short, float>::type;
    constexpr int EPC = BF16 ? 8 : 4;   // elements per 16-byte chunk
    constexpr int BKE = 8 * EPC;        // elements per k-tile (32 fp32 / 64 bf16)
    constexpr int NTH = 64 * WM * WN;   // threads per workgroup
    constexpr int RPP = NTH / 8;        // tile rows staged per pass (8 chunks per row)
    constexpr int TM = BM / WM / 32;    // 32x32 MFMA tiles per wave along M
    constexpr int TN = BN / WN / 32;
    constexpr int A_LD = BM / RPP;      // 16-byte loads per thread for the A tile
    constexpr int B_LD = BN / RPP;
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows divide over the loader threads");

    // LDS tile image.  Register-staged path: rows padded to 36 floats.  UT path: the tiles are written by LDS-DMA
    // (buffer_load ... lds: one wave-instruction fills 8 rows x 128 B, lane-linear), so rows are unpadded and the
    // 16-byte chunk c of row r sits at position c ^ ((r >> 1) & 7) -- the DMA's *source* address carries the
    // permutation, ds_read_b128 applies it again; every 16-lane read group then covers 16 distinct slots.
    constexpr int LDS_LD = UT ? 32 : LDS_STRIDE;
    __shared__ __align__(16) float smem[NST * (BM + BN) * LDS_LD];   // static: 32 / 48 / 64 KiB (UT)
    float* As = smem;                        // [NST][BM][LDS_LD]
    float* Bs = smem + NST * BM * LDS_LD;    // [NST][BN][LDS_LD]

    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    const T* __restrict__ Ag = reinterpret_cast<const T*>(a.A);
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.Wt);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tiles_n = (a.Cout + BN - 1) / BN;
    // Workgroups are dealt round-robin over the 8 XCDs (each with its own L2): give every XCD a contiguous run
    // of tile ids, so the n-tiles that re-read one A row block (and neighbouring m-tiles that share filter
    // taps) meet in one L2.  Bijective for any grid size; placement only changes speed, never results.
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_m = bid / tiles_n;
    const int tile_n = bid - tile_m * tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---- per-thread gather bookkeeping (rows are fixed over the K loop) ---------------------
    const int c4 = tid & 7;    // which 16-byte chunk of the k slice
    const int r0 = tid >> 3;   // 0..RPP-1
    int a_base[A_LD], a_iy0[A_LD], a_ix0[A_LD];
    bool a_ok[A_LD];
    const int hw = a.Ho * a.Wo;
    const int lda = a.lda > 0 ? a.lda : a.Cin;   // elements between consecutive input pixels
    const bool plain = a.KH * a.KW == 1 && a.stride == 1 && a.pad == 0;
#pragma unroll
    for (int i = 0; i < A_LD; i++) {
        const int m = m0 + r0 + RPP * i;
        a_ok[i] = m < a.M;
        const int mm = a_ok[i] ? m : 0;
        if (plain) {   // 1x1, stride 1, no padding (a Linear layer, half of the detector's convolutions): pixel = row
            a_iy0[i] = 0; a_ix0[i] = 0;
            a_base[i] = mm * lda;
            continue;
        }
        const int b = mm / hw;
        const int rem = mm - b * hw;
        const int oy = rem / a.Wo;
        const int ox = rem - oy * a.Wo;
        a_iy0[i] = oy * a.stride - a.pad;
        a_ix0[i] = ox * a.stride - a.pad;
        a_base[i] = ((b * a.H + a_iy0[i]) * a.W + a_ix0[i]) * lda;
    }
    const T* w_ptr[B_LD];
    bool b_ok[B_LD];
#pragma unroll
    for (int i = 0; i < B_LD; i++) {
        const int n = n0 + r0 + RPP * i;
        b_ok[i] = n < a.Cout;
        w_ptr[i] = Wg + (size_t)(b_ok[i] ? n : 0) * a.Kpad + c4 * EPC;
    }
    const int ntaps = a.KH * a.KW;
    const int kw_inv = (65536 + a.KW - 1) / a.KW;  // tap / KW for tap < 64, KW <= 7
    const int nt_inv = (65536 + ntaps - 1) / ntaps; // kt / ntaps for kt < 2048, ntaps <= 32 (checked at launch)

    // UT bookkeeping: descriptors over the input (rebased to the first image this tile touches, minus the padding
    // margin so every row offset is non-negative) and the filters; per row a byte offset and a bit per filter tap.
    __amdgpu_buffer_rsrc_t a_rs, w_rs;
    u32x4 a_rs4, w_rs4;   // the same descriptors as four SGPR words, for the hand-written DMA
    const unsigned lds_base = (unsigned)(size_t)(lds_ptr_t)smem;
    unsigned a_voff[A_LD], a_mask[A_LD], w_voff[B_LD];
    if constexpr (UT) {
        const int b0 = m0 / hw;
        const int csrc = c4 ^ ((r0 >> 1) & 7);   // RPP % 16 == 0: the permutation key is the same for every i
        const int margin = (a.pad * a.W + a.pad) * lda;
        a_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(Ag + (size_t)b0 * a.H * a.W * lda - margin), 0, (int)OOB_VOFF, 0x00020000);
        w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)Wg, 0, (int)OOB_VOFF, 0x00020000);
        const unsigned long long pa = (unsigned long long)(Ag + (size_t)b0 * a.H * a.W * lda - margin), pw = (unsigned long long)Wg;
        a_rs4 = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, OOB_VOFF, 0x00020000u};
        w_rs4 = u32x4{(unsigned)pw, (unsigned)(pw >> 32) & 0xffffu, OOB_VOFF, 0x00020000u};
#pragma unroll
        for (int i = 0; i < A_LD; i++) {
            a_voff[i] = (unsigned)(a_base[i] - b0 * a.H * a.W * lda + margin + csrc * EPC) * (unsigned)sizeof(T);
            unsigned mk = plain ? 1u : 0u;
            for (int t = 0; t < (plain ? 0 : ntaps); t++) {
                const int ky = (t * kw_inv) >> 16, kx = t - ky * a.KW;
                if ((unsigned)(a_iy0[i] + ky * a.dil) < (unsigned)a.H && (unsigned)(a_ix0[i] + kx * a.dil) < (unsigned)a.W) mk |= 1u << t;
            }
            a_mask[i] = a_ok[i] ? mk : 0u;
        }
#pragma unroll
        for (int i = 0; i < B_LD; i++)
            w_voff[i] = b_ok[i] ? (unsigned)((n0 + r0 + RPP * i) * a.Kpad + csrc * EPC) * (unsigned)sizeof(T) : OOB_VOFF;
    }

    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    float4 ra[A_LD], rb[B_LD];
    auto load_tile = [&](int kt, int buf) {
        if constexpr (UT) {
            const int kb = kt * BKE;
            int tap, cbase;
            if (a.k_order) {   // chunk-major: kt = chunk * ntaps + tap
                const int chunk = (kt * nt_inv) >> 16;
                tap = kt - chunk * ntaps;
                cbase = chunk * BKE;
            } else {
                tap = kb >> a.log2Cin;
                cbase = kb & (a.Cin - 1);
            }
            const int ky = (tap * kw_inv) >> 16;
            const int kx = tap - ky * a.KW;
            const int soff = ((ky * a.W + kx) * a.dil * lda + cbase) * (int)sizeof(T);
#pragma unroll
            for (int i = 0; i < A_LD; i++) {
                const unsigned vo = ((a_mask[i] >> tap) & 1u) ? a_voff[i] : OOB_VOFF;
                if constexpr (NST > 2)
                    lds_dma16(a_rs4, lds_base + (unsigned)((buf * BM + wave_u * 8 + RPP * i) * LDS_LD * 4), vo, soff);
                else
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rs, (lds_ptr_t)(As + (buf * BM + wave_u * 8 + RPP * i) * LDS_LD),
                                                             16, (int)vo, soff, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < B_LD; i++) {
                if constexpr (NST > 2)
                    lds_dma16(w_rs4, lds_base + (unsigned)((NST * BM + buf * BN + wave_u * 8 + RPP * i) * LDS_LD * 4), w_voff[i],
                              kb * (int)sizeof(T));
                else
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_ptr_t)(Bs + (buf * BN + wave_u * 8 + RPP * i) * LDS_LD),
                                                             16, (int)w_voff[i], kb * (int)sizeof(T), 0, 0);
            }
            return;
        }
        const int k0 = kt * BKE + c4 * EPC;
        int tap = k0 >> a.log2Cin;
        int ci = k0 & (a.Cin - 1);
        if (a.k_order) {
            const int chunk = (kt * nt_inv) >> 16;
            tap = kt - chunk * ntaps;
            ci = chunk * BKE + c4 * EPC;
        }
        const int ky = (tap * kw_inv) >> 16;
        const int kx = tap - ky * a.KW;
        const bool tap_ok = tap < ntaps;
        const int koff = (ky * a.W + kx) * a.dil * lda + ci;
#pragma unroll
        for (int i = 0; i < A_LD; i++) {
            const int iy = a_iy0[i] + ky * a.dil, ix = a_ix0[i] + kx * a.dil;
            const bool ok = a_ok[i] && tap_ok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            ra[i] = ok ? *reinterpret_cast<const float4*>(Ag + (size_t)(a_base[i] + koff)) : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < B_LD; i++)
            rb[i] = b_ok[i] ? *reinterpret_cast<const float4*>(w_ptr[i] + kt * BKE) : float4{0.f, 0.f, 0.f, 0.f};
    };
    auto store_tile = [&](int buf) {
        if constexpr (UT) return;
#pragma unroll
        for (int i = 0; i < A_LD; i++)
            *reinterpret_cast<float4*>(&As[(buf * BM + r0 + RPP * i) * LDS_STRIDE + c4 * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LD; i++)
            *reinterpret_cast<float4*>(&Bs[(buf * BN + r0 + RPP * i) * LDS_STRIDE + c4 * 4]) = rb[i];
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    const int nk = a.Kpad / BKE;

    // Operand fragments: lane (row = lane & 31, half = lane >> 5) reads the 16-byte chunk 2 g + half of its row for
    // k-group g = 0..3.  fp32: 4 values = the k slots of four v_mfma_f32_32x32x2_f32 steps (A and B use the same
    // (step, half) -> k map, so the k order inside a group is free).  bf16: 8 values = exactly the operand of one
    // v_mfma_f32_32x32x16_bf16 (lane half h holds k = 8 h + j).
    const int frag_row = lane & 31;
    const int frag_k = UT ? 0 : (lane >> 5) * 4;
    int frag_q[4];   // float offset of k-group q's chunk inside the row
#pragma unroll
    for (int q = 0; q < 4; q++) frag_q[q] = UT ? ((2 * q + (lane >> 5)) ^ ((frag_row >> 1) & 7)) * 4 : q * 8;

    // one k-tile of MFMAs out of LDS stage `cur`; `issue_next` (the next tile's global loads) runs right after the
    // first fragment reads, under their LDS latency; every k-group's fragments are fetched one group ahead
    auto mma_tile = [&](int cur, auto&& issue_next) {
        const float* Ab = &As[(cur * BM + wm * (BM / WM) + frag_row) * LDS_LD + frag_k];
        const float* Bb = &Bs[(cur * BN + wn * (BN / WN) + frag_row) * LDS_LD + frag_k];
        if constexpr (X3) {
            // the exact three-way bf16 split of both operands (cg_common.hpp cg_split8), six products per 16 k on v_mfma_f32_32x32x16_bf16:
            // lane (row, half) takes its 8 consecutive k of step s from chunks 4 s + 2 half, + 1 of the row
            const int sw = (frag_row >> 1) & 7, hf = lane >> 5;
            float4 a0[TM], a1[TM], b0[TN], b1[TN];
#pragma unroll
            for (int i = 0; i < TM; i++) {
                a0[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + (((2 * hf) ^ sw) << 2));
                a1[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + (((2 * hf + 1) ^ sw) << 2));
            }
#pragma unroll
            for (int j = 0; j < TN; j++) {
                b0[j] = *reinterpret_cast<const float4*>(Bb + j * 32 * LDS_LD + (((2 * hf) ^ sw) << 2));
                b1[j] = *reinterpret_cast<const float4*>(Bb + j * 32 * LDS_LD + (((2 * hf + 1) ^ sw) << 2));
            }
            issue_next();
#pragma unroll
            for (int st = 0; st < 2; st++) {
                uint4 ah[TM], am[TM], al[TM], bh[TN], bm[TN], bl[TN];
#pragma unroll
                for (int i = 0; i < TM; i++) cg_split8(a0[i], a1[i], ah[i], am[i], al[i]);
#pragma unroll
                for (int j = 0; j < TN; j++) cg_split8(b0[j], b1[j], bh[j], bm[j], bl[j]);
                if (st == 0) {
#pragma unroll
                    for (int i = 0; i < TM; i++) {
                        a0[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + (((4 + 2 * hf) ^ sw) << 2));
                        a1[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + (((4 + 2 * hf + 1) ^ sw) << 2));
                    }
#pragma unroll
                    for (int j = 0; j < TN; j++) {
                        b0[j] = *reinterpret_cast<const float4*>(Bb + j * 32 * LDS_LD + (((4 + 2 * hf) ^ sw) << 2));
                        b1[j] = *reinterpret_cast<const float4*>(Bb + j * 32 * LDS_LD + (((4 + 2 * hf + 1) ^ sw) << 2));
                    }
                }
#define ODAM_MMS(x, y) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, y), acc[i][j], 0, 0, 0)
#pragma unroll
                for (int i = 0; i < TM; i++)
#pragma unroll
                    for (int j = 0; j < TN; j++) {      // smallest products first
                        ODAM_MMS(al[i], bh[j]); ODAM_MMS(am[i], bm[j]); ODAM_MMS(ah[i], bl[j]);
                        ODAM_MMS(am[i], bh[j]); ODAM_MMS(ah[i], bm[j]);
                        ODAM_MMS(ah[i], bh[j]);
                    }
#undef ODAM_MMS
            }
            return;
        }
        float4 af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; i++) af[0][i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + frag_q[0]);
#pragma unroll
        for (int j = 0; j < TN; j++) bf[0][j] = *reinterpret_cast<const float4*>(Bb + j * 32 * LDS_LD + frag_q[0]);
        issue_next();
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int pb = q & 1;
            if (q + 1 < 4) {
#pragma unroll
                for (int i = 0; i < TM; i++)
                    af[pb ^ 1][i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_LD + frag_q[(q + 1) & 3]);
#pragma unroll
                for (int j = 0; j < TN; j++)
                    bf[pb ^ 1][j] = *reinterpret_cast<const float4*>(Bb + j * 32 * LDS_LD + frag_q[(q + 1) & 3]);
            }
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++) {
                    if constexpr (BF16) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[pb][i]),
                                                                            __builtin_bit_cast(bf16x8, bf[pb][j]),
                                                                            acc[i][j], 0, 0, 0);
                    } else {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[pb][i].x, bf[pb][j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[pb][i].y, bf[pb][j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[pb][i].z, bf[pb][j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[pb][i].w, bf[pb][j].w, acc[i][j], 0, 0, 0);
                    }
                }
        }
    };

    if constexpr (NST == 2) {
        if (!(CG_ABLATE & 16)) load_tile(0, 0);   // 16: pretend the first tile is already there (cross-tile prefetch bound)
        store_tile(0);
        if constexpr (UT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            mma_tile(cur, [&] { if (!(CG_ABLATE & 1) && kt + 1 < nk) load_tile(kt + 1, cur ^ 1); });
            if (!(CG_ABLATE & 2) && kt + 1 < nk) store_tile(cur ^ 1);
            if constexpr (UT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA of tile kt + 1 has landed
            if (!(CG_ABLATE & 4)) __syncthreads();
        }
    } else {
        // Tiles kt .. kt + NST - 2 are in flight when tile kt is awaited: each thread's DMAs retire in order, so
        // "at most (NST - 2) tiles' worth of my loads outstanding" means my part of tile kt has landed; the barrier
        // extends that to every wave and also says stage (kt - 1) % NST has been read by all, so it can be refilled.
        constexpr int LPT = A_LD + B_LD;   // DMA instructions per thread per tile
#pragma unroll
        for (int s0 = 0; s0 < NST - 1; s0++)
            if (s0 < nk) load_tile(s0, s0);
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + NST - 1 <= nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPT) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            mma_tile(kt & (NST - 1), [&] { if (kt + NST - 1 < nk) load_tile(kt + NST - 1, (kt + NST - 1) & (NST - 1)); });
        }
        __syncthreads();   // the last stage is fully read before the epilogue reuses the tile buffers
    }

    static_assert(WM * WN * 32 * (BN / WN) <= NST * (BM + BN) * LDS_LD, "epilogue staging fits the tile buffers");
    if (epilogue2_ok<BM, BN, WM, WN, BF16>(a)) epilogue2<BM, BN, WM, WN, TM, TN, BF16>(a, acc, smem, m0, n0, wm, wn, wave, lane);      // (its own barrier: one more)
    else epilogue<BM, BN, WM, WN, TM, TN, BF16>(a, acc, smem, (int)sizeof(smem) / 4, m0, n0, wm, wn, wave, lane);
}

void split3_filters(const float* w, int Cout, int Kpad, unsigned short* out) {
    const int nk = Kpad / 16;
    for (int n = 0; n < Cout; n++)
        for (int kt = 0; kt < nk; kt++) {
            unsigned short* o = out + ((size_t)n * nk + kt) * 48;
            for (int e = 0; e < 16; e++) {
                const float v = w[(size_t)n * Kpad + kt * 16 + e];
                unsigned u;
                memcpy(&u, &v, 4);
                float fh; const unsigned uh = u & 0xffff0000u; memcpy(&fh, &uh, 4);
                const float r1 = v - fh;
                unsigned u1; memcpy(&u1, &r1, 4);
                float fm; const unsigned um = u1 & 0xffff0000u; memcpy(&fm, &um, 4);
                const float r2 = r1 - fm;
                unsigned u2; memcpy(&u2, &r2, 4);
                o[e] = (unsigned short)(u >> 16); o[16 + e] = (unsigned short)(u1 >> 16); o[32 + e] = (unsigned short)(u2 >> 16);
            }
        }
}

// the small tiles: gather and products (Choice::ut, x3) as chosen; NST_UT = LDS stages of the LDS-DMA gather
template <int BM, int BN, int WM, int WN, int NST_UT = 2>
static int launch_cfg(const ConvGemmArgs& a, const Choice& c, hipStream_t stream) {
    const dim3 g(((a.M + BM - 1) / BM) * ((a.Cout + BN - 1) / BN)), b(64 * WM * WN);
    if (c.bf16) {
        if (c.ut) hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, true, true, NST_UT>), g, b, 0, stream, a);
        else hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, true, false>), g, b, 0, stream, a);
    } else {
        if (c.x3) hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, false, true, NST_UT, true>), g, b, 0, stream, a);
        else if (c.ut) hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, false, true, NST_UT>), g, b, 0, stream, a);
        else hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, false, false>), g, b, 0, stream, a);
    }
    ODAM_HIP(hipGetLastError());
    return 0;
}

int launch_conv_gemm(const ConvGemmArgs& a, hipStream_t stream) {
    const Choice c = choose(a, current_switches());
    if (c.family == Family::Refused) return odam_fail(c.code, c.message);
    if (c.family == Family::Nothing) return 0;
    char tok[PATH_TOKEN_LEN];
    choice_token(c, tok);
    note_path("%s", tok);
    switch (c.family) {
    case Family::RingF32: return launch_big_f32(c.mode, c.bn, 64 * c.waves, a, stream);
    case Family::RingBF16: return launch_big_bf16(c.bn, 64 * c.waves, c.s1_window, a, stream);
    case Family::FusedF32: return launch_big_fused(c.mode, a, stream);
    case Family::FusedBF16: return launch_fused_bf16(c.s1_window, a, stream);
    default:      // Family::Small
        if (c.bm == 128 && c.bn == 64) return c.waves == 8 ? launch_cfg<128, 64, 4, 2>(a, c, stream) : launch_cfg<128, 64, 4, 1>(a, c, stream);
        if (c.bm == 64) return c.stages == 4 ? launch_cfg<64, 64, 2, 2, 4>(a, c, stream) : launch_cfg<64, 64, 2, 2>(a, c, stream);
        return c.waves == 8 ? launch_cfg<128, 128, 4, 2>(a, c, stream) : launch_cfg<128, 128, 2, 2>(a, c, stream);
    }
}

}  // namespace odam_cg
