// detr_kernels.hip -- see detr_kernels.h
#include "detr_kernels.h"

#include <cstdlib>

#include "odam_config.h"
#include "odam_err.h"
#include "stem_u8_fold.h"

namespace odam_dk {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned short bf16_t;   // raw bfloat16 bits (bf16 mode: activations in HBM are bf16, arithmetic stays fp32)

__device__ __forceinline__ float bf2f(bf16_t u) { return __builtin_bit_cast(float, (unsigned)u << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
// two floats -> one register of two bf16 (lo in the low half), round to nearest even: ONE v_cvt_pk_bf16_f32 (the scalar casts of
// f2bf(lo) | f2bf(hi) << 16 compile to two conversions, a shift and an or)
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t));
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const bf16_t* p) {
    const ushort4 u = *reinterpret_cast<const ushort4*>(p);
    return float4{bf2f(u.x), bf2f(u.y), bf2f(u.z), bf2f(u.w)};
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(bf16_t* p, float4 v) {
    *reinterpret_cast<uint2*>(p) = uint2{pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
}
#define ODAM_DISPATCH(dtype, KERNEL, ...)                                                  \
    do {                                                                                  \
        if ((dtype) == 1) { KERNEL(bf16_t, __VA_ARGS__); } else { KERNEL(float, __VA_ARGS__); } \
    } while (0)

// =================================================================================================
// Fused attention, d_head = 32, fp32 on v_mfma_f32_32x32x2_f32.
//
// Workgroup = 4 wavefronts, each owns 32 query rows of one (batch, head); the workgroup walks the
// keys in tiles of 32 staged once in LDS for all four wavefronts (double buffered).
//   S^T tile (keys x queries) = K_tile . Q^T        16 MFMA (K-dim = 32 head channels, 2 per MFMA)
//   online softmax over keys: the key index lives in the accumulator REGISTER (plus the lane
//     half), the query on the lane -> row max / row sum are 15 in-register ops + one lane^32 swap
//   O^T (channels x queries) += V_tile^T . P^T       16 MFMA; the S^T accumulator registers ARE the
//     B operand of this product (same lane <-> query, same register <-> key), so P never leaves
//     the register file and stays fp32.
// Reference semantics: torch.nn.functional.multi_head_attention_forward as called from
// src/models/transformer.py:154-167, 217-238 (q scaled by sqrt(1/32) before the product, softmax
// over keys, no dropout at inference, padding mask all-false for same-size frames).
// =================================================================================================
constexpr int ATT_KT = 32;          // keys per tile

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// D = head dimension: 32 (detector, 8 heads) or 64 (associator GNN, 4 heads)
template <typename T, int D>
__global__ __launch_bounds__(256) void attention_kernel(const T* __restrict__ Q, int ldq,
                                                        const T* __restrict__ K, int ldk,
                                                        const T* __restrict__ V, int ldv,
                                                        T* __restrict__ O, int ldo, int Lq, int Lk, float scale,
                                                        const unsigned char* __restrict__ key_mask) {
    // key_mask (nullable): [B][Lk], non-zero = padded key, excluded from the softmax (key_padding_mask of
    // nn.MultiheadAttention as src/models/transformer.py:157-160, 224-228 pass it)
    constexpr int LD = D + 4;        // LDS row stride (floats)
    constexpr int HD = D / 2;        // channels of the QK^T reduction held by one lane half
    constexpr int NO = D / 32;       // 32-channel output tiles
    constexpr int CPR = D / 4;       // 16-byte... 4-channel chunks per K/V row
    constexpr int RPP = 256 / CPR;   // K/V rows staged per pass
    __shared__ __align__(16) float Ks[2][ATT_KT][LD];
    __shared__ __align__(16) float Vs[2][ATT_KT][LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int h = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const T* Qb = Q + (size_t)b * Lq * ldq + h * D;
    const T* Kb = K + (size_t)b * Lk * ldk + h * D;
    const T* Vb = V + (size_t)b * Lk * ldv + h * D;

    // this lane's HD query channels d = HD*half + s, pre-scaled (a power-of-two scale commutes with the product)
    float qreg[HD];
    {
        const int q = q0 + col;
#pragma unroll
        for (int g = 0; g < HD / 4; g++) {
            float4 v = (q < Lq) ? ld4(Qb + (size_t)q * ldq + HD * half + 4 * g) : float4{0.f, 0.f, 0.f, 0.f};
            qreg[4 * g + 0] = v.x * scale; qreg[4 * g + 1] = v.y * scale;
            qreg[4 * g + 2] = v.z * scale; qreg[4 * g + 3] = v.w * scale;
        }
    }

    const int lr = tid / CPR, lc = (tid % CPR) * 4;  // tile loader: row, 4-channel column
    constexpr int NLD = ATT_KT / RPP;                // passes to stage one 32-key tile (1 for D = 32, 2 for D = 64)
    auto load_kv = [&](int kt, float4* kv, float4* vv) {
#pragma unroll
        for (int pss = 0; pss < NLD; pss++) {
            const int key = kt * ATT_KT + lr + pss * RPP;
            if (key < Lk) {
                kv[pss] = ld4(Kb + (size_t)key * ldk + lc);
                vv[pss] = ld4(Vb + (size_t)key * ldv + lc);
            } else {
                kv[pss] = float4{0.f, 0.f, 0.f, 0.f};
                vv[pss] = float4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    auto store_kv = [&](int buf, const float4* kv, const float4* vv) {
#pragma unroll
        for (int pss = 0; pss < NLD; pss++) {
            *reinterpret_cast<float4*>(&Ks[buf][lr + pss * RPP][lc]) = kv[pss];
            *reinterpret_cast<float4*>(&Vs[buf][lr + pss * RPP][lc]) = vv[pss];
        }
    };

    floatx16 oacc[NO];
#pragma unroll
    for (int o = 0; o < NO; o++)
#pragma unroll
        for (int r = 0; r < 16; r++) oacc[o][r] = 0.0f;
    float m_run = -1e30f, l_run = 0.0f;

    const int ntiles = (Lk + ATT_KT - 1) / ATT_KT;
    float4 kv[NLD], vv[NLD];
    load_kv(0, kv, vv);
    store_kv(0, kv, vv);
    __syncthreads();

    for (int kt = 0; kt < ntiles; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < ntiles) load_kv(kt + 1, kv, vv);

        // S^T = K . Q^T   (rows = keys, cols = queries)
        floatx16 s;
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] = 0.0f;
#pragma unroll
        for (int g = 0; g < HD / 4; g++) {
            const float4 kf = *reinterpret_cast<const float4*>(&Ks[cur][col][HD * half + 4 * g]);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qreg[4 * g + 0], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qreg[4 * g + 1], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qreg[4 * g + 2], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qreg[4 * g + 3], s, 0, 0, 0);
        }
        // mask keys beyond Lk (last tile only) and padded keys
        const int kbase = kt * ATT_KT;
        if (kbase + ATT_KT > Lk) {
#pragma unroll
            for (int r = 0; r < 16; r++)
                if (kbase + acc_row(r, half) >= Lk) s[r] = -1e30f;
        }
        if (key_mask) {
            const unsigned char* mk = key_mask + (size_t)b * Lk + kbase;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int k = acc_row(r, half);
                if (kbase + k < Lk && mk[k]) s[r] = -1e30f;
            }
        }
        // online softmax over the key axis (registers + the other lane half)
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; r++) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            s[r] = __expf(s[r] - m_new);
            psum += s[r];
        }
        psum += __shfl_xor(psum, 32);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int r = 0; r < 16; r++) oacc[o][r] *= alpha;
        // O^T += V^T . P^T : k-slot (step r, lane half) <-> key acc_row(r, half) on both operands
#pragma unroll
        for (int r = 0; r < 16; r++) {
#pragma unroll
            for (int o = 0; o < NO; o++) {
                const float vf = Vs[cur][acc_row(r, half)][o * 32 + col];
                oacc[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf, s[r], oacc[o], 0, 0, 0);
            }
        }
        if (kt + 1 < ntiles) store_kv(cur ^ 1, kv, vv);
        __syncthreads();
    }

    const int q = q0 + col;
    if (q < Lq) {
        const float inv = 1.0f / l_run;
        T* Ob = O + ((size_t)b * Lq + q) * ldo + h * D;
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                float4 v = {oacc[o][4 * g + 0] * inv, oacc[o][4 * g + 1] * inv, oacc[o][4 * g + 2] * inv,
                            oacc[o][4 * g + 3] * inv};
                st4(Ob + o * 32 + 8 * g + 4 * half, v);  // channels o*32 + acc_row(4g..4g+3, half)
            }
    }
}

// =================================================================================================
// Attention on v_mfma_f32_32x32x16_bf16: what attention_bf16_kernel<D> and attention_x3_kernel<D> below share.  D = head dim, 32
// or 64; workgroup, query ownership and the online softmax's shape are attention_kernel's.
//
// LDS image of a key tile: one row of 2 D bytes per key, NC = D / 8 chunks of 16 bytes (8 bf16 channels) per row.
//   K: chunk c of key r sits at c ^ ((r >> 2) & 3) at D = 32 (64-byte rows, as in conv_gemm's bf16 kernel) and at
//      c ^ ((r >> 1) & 7) at D = 64 (128-byte rows, two keys per 256-byte bank row): the ds_read_b128 lane groups of the QK^T
//      step are conflict-free at both.
//   V: row-major as it comes from HBM (one 16-byte store per chunk) and read through ds_read_b64_tr_b16, the hardware
//      transpose: a 16-lane group reads a block of 4 keys x 16 channels and lane i receives channel i of the four keys --
//      the PV product's A operand (V^T: channel on the lane, four consecutive keys in the register pair).  Lane 4 q + p of
//      16-lane group g supplies the address of key row q, channels 4 p .. 4 p + 3 of the group's channel block (g & 1); the
//      group's half (g >> 1) selects keys 4 half .. of an 8-key step, as the P operand's k order wants them.  At D = 32 the
//      32 lanes of a half read 4 keys x 64 bytes = 256 contiguous bytes: conflict-free without a swizzle.  At D = 64 a row keeps
//      its two 64-byte halves swapped where bit 1 of the key is set (the four keys of a transposed read then cover all 64
//      banks), so the half holding output tile o is o ^ (bit 1 of the lane's key row q).
// =================================================================================================
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short tr4_t __attribute__((ext_vector_type(4)));
typedef tr4_t __attribute__((address_space(3))) * lds_tr_ptr;

template <int D> __device__ __forceinline__ int att_kswz(int r, int c) {      // index of 16-byte chunk c of key r in a K tile
    if constexpr (D == 32) return r * 4 + (c ^ ((r >> 2) & 3));
    else return r * 8 + (c ^ ((r >> 1) & 7));
}
template <int D> __device__ __forceinline__ int att_vswz(int r, int c) {      // the same in a V tile
    if constexpr (D == 32) return r * 4 + c;
    else return r * 8 + (c ^ (((r >> 1) & 1) << 2));
}
// byte offset inside a V tile of this lane's transposed read for the 32-channel output tile o
template <int D> __device__ __forceinline__ int att_tr_off(int lane, int o) {
    const int blk = D == 32 ? 0 : o ^ ((lane >> 3) & 1);
    return (((lane >> 5) * 4 + ((lane & 15) >> 2)) * 2 * D) + ((blk * 32 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2);
}
// V^T fragment of one 16-key step: keys 4 half .. + 3 and 8 + 4 half .. + 3 of the step that starts at vb
template <int D> __device__ __forceinline__ uint4 att_read_vt(const char* vb) {
    const uint2 lo = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vb)));
    const uint2 hi = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vb + 8 * 2 * D)));
    return uint4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ void att_mma(floatx16& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}
// (The epilogue, eight lines, is written out in both kernels: behind a helper it costs attention_x3_kernel<32> two more s_waitcnt
// vmcnt(0), one of them in the key loop -- profiles/attention_template.txt.)
// exact three-way bf16 split of eight fp32 values (a = hi + mid + lo by truncation), as conv_gemm.hip's: one uint4 of bf16 per plane
__device__ __forceinline__ void att_split8(const float4& c0, const float4& c1, uint4& hi, uint4& mid, uint4& lo) {
    const float v[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    unsigned uh[8], um[8], ul[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        uh[e] = __builtin_bit_cast(unsigned, v[e]);
        const float r1 = v[e] - __builtin_bit_cast(float, uh[e] & 0xffff0000u);
        um[e] = __builtin_bit_cast(unsigned, r1);
        ul[e] = __builtin_bit_cast(unsigned, r1 - __builtin_bit_cast(float, um[e] & 0xffff0000u));
    }
    auto pk = [](unsigned lo_, unsigned hi_) { return __builtin_amdgcn_perm(hi_, lo_, 0x07060302u); };   // two top halves
    hi = uint4{pk(uh[0], uh[1]), pk(uh[2], uh[3]), pk(uh[4], uh[5]), pk(uh[6], uh[7])};
    mid = uint4{pk(um[0], um[1]), pk(um[2], um[3]), pk(um[4], um[5]), pk(um[6], um[7])};
    lo = uint4{pk(ul[0], ul[1]), pk(ul[2], ul[3]), pk(ul[4], ul[5]), pk(ul[6], ul[7])};
}

// =================================================================================================
// Fused attention on the bf16 matrix instruction (bf16 and mxfp8 modes), head dim D = 32 or 64.
// The dataflow of attention_kernel with v_mfma_f32_32x32x16_bf16: per 64-key tile 2 NS MFMAs give S^T = K . Q^T (two 32-key
// blocks x NS = D / 16 k-steps of 16 channels) and 4 NO more O^T += V^T . P^T (NO = D / 32 output tiles of 32 channels) -- at
// D = 32, 8 x 32 cycles instead of 64 x 64.  P stays in registers: the S^T accumulator (query on the lane, key in the
// register) converted pairwise to bf16 IS the B operand of the PV product; its k order inside a 16-key step is
// 16 s + 8 (j >> 2) + 4 half + (j & 3), so the A operand (V^T) is read as two 4-key groups per step (att_read_vt).  Softmax in
// fp32 with exp2 (scale * log2 e folded in).  D changes the row width of the LDS images (att_kswz / att_vswz / att_tr_off),
// the loader passes per tile (one chunk per thread and pass: 1 at D = 32, 2 at D = 64), NS, NO and the score of a dead key; at
// twice the head width a score tile feeds twice the matrix work per exponential.
// =================================================================================================
// score of a key outside the softmax (beyond Lk, or padded) in attention_bf16_kernel.  D = 64: -2^100, below the running max's
// start, -1e30.  The exponent is fma(s, c, -m c) with c = scale * log2 e: for s = m = -1e30 that is the rounding error of the
// product, about 1e22 -- exp2 of it is inf where it is positive, and a leading tile with every key padded would poison the row.
// At D = 64 (c = 0.125 log2 e) s c is exact at a power of two, so a padded key gives fma(s, c, -m c) <= -0.27e30 c: p = 0.
// D = 32 keeps -1e30, the value its outputs have always been computed with (tests/width_ref.py restates both constants), so
// there a leading 64-key tile that is all padding is not covered by this argument.
template <int D> constexpr float ATT_DEAD_BF16 = D == 32 ? -1e30f : -1267650600228229401496703205376.0f;

template <int D>
__global__ __launch_bounds__(256) void attention_bf16_kernel(const bf16_t* __restrict__ Q, int ldq,
                                                             const bf16_t* __restrict__ K, int ldk,
                                                             const bf16_t* __restrict__ V, int ldv,
                                                             bf16_t* __restrict__ O, int ldo, int Lq, int Lk, float c_log2,
                                                             const unsigned char* __restrict__ key_mask) {
    static_assert(D == 32 || D == 64, "head dim 32 or 64");
    constexpr int KT = 64;
    constexpr int NC = D / 8;            // 16-byte chunks per K / V row
    constexpr int NS = D / 16;           // 16-channel k-steps of S^T = K . Q^T
    constexpr int NO = D / 32;           // 32-channel output tiles
    constexpr int RPP = 256 / NC;        // key rows staged per loader pass
    constexpr int NLD = KT / RPP;        // loader passes per tile
    __shared__ __align__(16) uint4 Ks[2][KT * NC];
    __shared__ __align__(16) uint4 Vs[2][KT * NC];     // row-major as att_vswz places the chunks, read transposed (att_read_vt)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int h = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const bf16_t* Qb = Q + (size_t)b * Lq * ldq + h * D;
    const bf16_t* Kb = K + (size_t)b * Lk * ldk + h * D;
    const bf16_t* Vb = V + (size_t)b * Lk * ldv + h * D;

    uint4 qf[NS];    // B operand of S^T = K . Q^T: lane (query col, half) holds Q[q][16 s + 8 half .. + 7]
    {
        const int q = q0 + col;
#pragma unroll
        for (int st = 0; st < NS; st++)
            qf[st] = (q < Lq) ? *reinterpret_cast<const uint4*>(Qb + (size_t)q * ldq + 16 * st + 8 * half) : uint4{0u, 0u, 0u, 0u};
    }
    const int lk = tid / NC, lc = tid % NC;        // loader: key row of the tile, 8-channel chunk
    auto load_kv = [&](int kt, uint4 (&kr)[NLD], uint4 (&vr)[NLD]) {
#pragma unroll
        for (int pss = 0; pss < NLD; pss++) {
            const int key = kt * KT + lk + pss * RPP;
            if (key < Lk) {
                kr[pss] = *reinterpret_cast<const uint4*>(Kb + (size_t)key * ldk + lc * 8);
                vr[pss] = *reinterpret_cast<const uint4*>(Vb + (size_t)key * ldv + lc * 8);
            } else {
                kr[pss] = uint4{0u, 0u, 0u, 0u}; vr[pss] = uint4{0u, 0u, 0u, 0u};
            }
        }
    };
    auto store_kv = [&](int buf, const uint4 (&kr)[NLD], const uint4 (&vr)[NLD]) {
#pragma unroll
        for (int pss = 0; pss < NLD; pss++) {
            const int r = lk + pss * RPP;
            Ks[buf][att_kswz<D>(r, lc)] = kr[pss];
            Vs[buf][att_vswz<D>(r, lc)] = vr[pss];
        }
    };
    int tr_off[NO];
#pragma unroll
    for (int o = 0; o < NO; o++) tr_off[o] = att_tr_off<D>(lane, o);

    floatx16 oacc[NO];
#pragma unroll
    for (int o = 0; o < NO; o++)
#pragma unroll
        for (int r = 0; r < 16; r++) oacc[o][r] = 0.0f;
    float m_run = -1e30f, l_run = 0.0f;
    const int ntiles = (Lk + KT - 1) / KT;
    uint4 kr[NLD], vr[NLD];
    load_kv(0, kr, vr);
    store_kv(0, kr, vr);
    __syncthreads();
    for (int kt = 0; kt < ntiles; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < ntiles) load_kv(kt + 1, kr, vr);
        floatx16 s[2];
#pragma unroll
        for (int jh = 0; jh < 2; jh++) {
#pragma unroll
            for (int r = 0; r < 16; r++) s[jh][r] = 0.0f;
            const int key = jh * 32 + col;
#pragma unroll
            for (int st = 0; st < NS; st++) att_mma(s[jh], Ks[cur][att_kswz<D>(key, 2 * st + half)], qf[st]);
        }
        const int kbase = kt * KT;
        if (kbase + KT > Lk || key_mask) {
            const unsigned char* mk = key_mask ? key_mask + (size_t)b * Lk + kbase : nullptr;
#pragma unroll
            for (int jh = 0; jh < 2; jh++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int k = jh * 32 + acc_row(r, half);
                    if (kbase + k >= Lk || (mk && mk[k])) s[jh][r] = ATT_DEAD_BF16<D>;
                }
        }
        float mx = s[0][0];
#pragma unroll
        for (int jh = 0; jh < 2; jh++)
#pragma unroll
            for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[jh][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c_log2);
        const float mc = m_new * c_log2;
        float psum = 0.0f;
#pragma unroll
        for (int jh = 0; jh < 2; jh++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[jh][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[jh][r], c_log2, -mc));
                psum += s[jh][r];
            }
        psum += __shfl_xor(psum, 32);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int r = 0; r < 16; r++) oacc[o][r] *= alpha;
#pragma unroll
        for (int jh = 0; jh < 2; jh++)
#pragma unroll
            for (int st = 0; st < 2; st++) {
                unsigned pw[4];
#pragma unroll
                for (int e = 0; e < 4; e++)
                    pw[e] = pack_bf16x2(s[jh][8 * st + 2 * e], s[jh][8 * st + 2 * e + 1]);
#pragma unroll
                for (int o = 0; o < NO; o++)
                    att_mma(oacc[o], att_read_vt<D>(reinterpret_cast<const char*>(&Vs[cur][0]) + (jh * 32 + 16 * st) * 2 * D + tr_off[o]),
                            uint4{pw[0], pw[1], pw[2], pw[3]});
            }
        if (kt + 1 < ntiles) store_kv(cur ^ 1, kr, vr);
        __syncthreads();
    }
    const int q = q0 + col;
    if (q < Lq) {
        const float inv = 1.0f / l_run;
        auto* Ob = O + ((size_t)b * Lq + q) * ldo + h * D;
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                st4(Ob + o * 32 + 8 * g + 4 * half,      // channels o * 32 + acc_row(4 g .. 4 g + 3, half)
                    float4{oacc[o][4 * g + 0] * inv, oacc[o][4 * g + 1] * inv, oacc[o][4 * g + 2] * inv, oacc[o][4 * g + 3] * inv});
    }
}

// =================================================================================================
// Fused attention for fp32 operands on the bf16 matrix instruction (the fp32 detector), head dim D = 32 or 64: the dataflow of
// attention_bf16_kernel with every product taken through the exact three-way bf16 split of conv_gemm.hip (a = hi + mid + lo
// by truncation, six bf16 x bf16 products per fp32 product, fp32 accumulate; max error vs float64 0.8-1.4e-7 of sum |a b|,
// the fp32 matrix instruction's own chain 1.1-1.9e-7).  K and V tiles are split once when they are staged (three bf16 planes
// each in LDS, laid out as the bf16 kernel's), the pre-scaled query fragment is split once per workgroup, the probabilities
// -- fp32 in the S^T accumulators -- are split in registers and are the B operand of the PV product as they stand.  At
// D = 32, per 64-key tile and wave 48 matrix instructions of 32 cycles against 64 of 64 on v_mfma_f32_32x32x2_f32.  Softmax
// as in the fp32 kernel (q pre-scaled, __expf).  D changes the LDS rows, NS, NO and the key tile: KT = 2048 / D keys, 64 at
// D = 32 and 32 at D = 64, so that the K / V images (three planes each, double buffered) stay at 48 KiB and three workgroups
// share a CU; that is 256 chunks of 8 values per tile, one per thread.  With the key tile goes the form of the key mask
// (see there).
// =================================================================================================
template <int D>
__global__ __launch_bounds__(256) void attention_x3_kernel(const float* __restrict__ Q, int ldq,
                                                           const float* __restrict__ K, int ldk,
                                                           const float* __restrict__ V, int ldv,
                                                           float* __restrict__ O, int ldo, int Lq, int Lk, float scale,
                                                           const unsigned char* __restrict__ key_mask) {
    static_assert(D == 32 || D == 64, "head dim 32 or 64");
    constexpr int KT = 2048 / D;
    constexpr int NJ = KT / 32;          // 32-key blocks per tile
    constexpr int NC = D / 8;            // 16-byte (bf16) chunks per K / V row
    static_assert(KT * NC == 256, "one 8-value chunk per thread and tile");
    constexpr int NS = D / 16;           // 16-channel k-steps of S^T = K . Q^T
    constexpr int NO = D / 32;           // 32-channel output tiles
    __shared__ __align__(16) uint4 Ks[2][3][KT * NC];
    __shared__ __align__(16) uint4 Vs[2][3][KT * NC];     // V's three planes, each as attention_bf16_kernel's V tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int h = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const float* Qb = Q + (size_t)b * Lq * ldq + h * D;
    const float* Kb = K + (size_t)b * Lk * ldk + h * D;
    const float* Vb = V + (size_t)b * Lk * ldv + h * D;

    uint4 qh[NS], qm[NS], ql[NS];     // B operand of S^T = K . Q^T: lane (query col, half) holds Q[q][16 s + 8 half .. + 7], pre-scaled
    {
        const int q = q0 + col;
#pragma unroll
        for (int st = 0; st < NS; st++) {
            float4 a = float4{0.f, 0.f, 0.f, 0.f}, c = a;
            if (q < Lq) {
                a = ld4(Qb + (size_t)q * ldq + 16 * st + 8 * half);
                c = ld4(Qb + (size_t)q * ldq + 16 * st + 8 * half + 4);
            }
            a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
            c.x *= scale; c.y *= scale; c.z *= scale; c.w *= scale;
            att_split8(a, c, qh[st], qm[st], ql[st]);
        }
    }
    const int lk = tid / NC, lc = tid % NC;        // loader: key row of the tile, 8-channel chunk
    auto load_kv = [&](int kt, float4 (&kr)[2], float4 (&vr)[2]) {
        const int key = kt * KT + lk;
        if (key < Lk) {
            kr[0] = ld4(Kb + (size_t)key * ldk + lc * 8); kr[1] = ld4(Kb + (size_t)key * ldk + lc * 8 + 4);
            vr[0] = ld4(Vb + (size_t)key * ldv + lc * 8); vr[1] = ld4(Vb + (size_t)key * ldv + lc * 8 + 4);
        } else {
            kr[0] = kr[1] = vr[0] = vr[1] = float4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_kv = [&](int buf, const float4 (&kr)[2], const float4 (&vr)[2]) {
        uint4 p[3];
        att_split8(kr[0], kr[1], p[0], p[1], p[2]);
#pragma unroll
        for (int pl = 0; pl < 3; pl++) Ks[buf][pl][att_kswz<D>(lk, lc)] = p[pl];
        att_split8(vr[0], vr[1], p[0], p[1], p[2]);
#pragma unroll
        for (int pl = 0; pl < 3; pl++) Vs[buf][pl][att_vswz<D>(lk, lc)] = p[pl];
    };
    int tr_off[NO];
#pragma unroll
    for (int o = 0; o < NO; o++) tr_off[o] = att_tr_off<D>(lane, o);

    floatx16 oacc[NO];
#pragma unroll
    for (int o = 0; o < NO; o++)
#pragma unroll
        for (int r = 0; r < 16; r++) oacc[o][r] = 0.0f;
    float m_run = -1e30f, l_run = 0.0f;
    const int ntiles = (Lk + KT - 1) / KT;
    float4 kr[2], vr[2];
    load_kv(0, kr, vr);
    store_kv(0, kr, vr);
    __syncthreads();
    for (int kt = 0; kt < ntiles; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < ntiles) load_kv(kt + 1, kr, vr);
        floatx16 s[NJ];
#pragma unroll
        for (int jh = 0; jh < NJ; jh++) {
#pragma unroll
            for (int r = 0; r < 16; r++) s[jh][r] = 0.0f;
            const int key = jh * 32 + col;
#pragma unroll
            for (int st = 0; st < NS; st++) {
                const int idx = att_kswz<D>(key, 2 * st + half);
                const uint4 kh = Ks[cur][0][idx], km = Ks[cur][1][idx], kl = Ks[cur][2][idx];
                att_mma(s[jh], kl, qh[st]); att_mma(s[jh], km, qm[st]); att_mma(s[jh], kh, ql[st]);     // smallest products first
                att_mma(s[jh], km, qh[st]); att_mma(s[jh], kh, qm[st]);
                att_mma(s[jh], kh, qh[st]);
            }
        }
        const int kbase = kt * KT;
        // keys beyond Lk and padded keys, in one form per tile size, and both are needed.  One 32-key block per tile: one bit per
        // accumulator register, gathered first and applied by selects -- written inside the branch, the stores to the accumulator
        // were lost in code generation at this tile size ("Kernels (detr_kernels.hip)").  Two blocks: written inside
        // the branch, which costs nothing on an interior tile without a mask; the selects always execute, about 125 vector
        // instructions per key tile at this size.
        if constexpr (NJ == 1) {
            unsigned dead = 0u;
            if (kbase + KT > Lk || key_mask) {
                const unsigned char* mk = key_mask ? key_mask + (size_t)b * Lk + kbase : nullptr;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int k = acc_row(r, half);
                    if (kbase + k >= Lk || (mk && mk[k])) dead |= 1u << r;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r++) s[0][r] = ((dead >> r) & 1u) ? -1e30f : s[0][r];
        } else if (kbase + KT > Lk || key_mask) {
            const unsigned char* mk = key_mask ? key_mask + (size_t)b * Lk + kbase : nullptr;
#pragma unroll
            for (int jh = 0; jh < NJ; jh++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int k = jh * 32 + acc_row(r, half);
                    if (kbase + k >= Lk || (mk && mk[k])) s[jh][r] = -1e30f;
                }
        }
        float mx = s[0][0];
#pragma unroll
        for (int jh = 0; jh < NJ; jh++)
#pragma unroll
            for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[jh][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int jh = 0; jh < NJ; jh++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[jh][r] = __expf(s[jh][r] - m_new);
                psum += s[jh][r];
            }
        psum += __shfl_xor(psum, 32);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int r = 0; r < 16; r++) oacc[o][r] *= alpha;
        // O^T += V^T . P^T: the accumulator registers 8 st .. 8 st + 7 of s[jh], split, are the B operand of k-step (jh, st)
#pragma unroll
        for (int jh = 0; jh < NJ; jh++)
#pragma unroll
            for (int st = 0; st < 2; st++) {
                uint4 ph, pm, pl_;
                att_split8(float4{s[jh][8 * st + 0], s[jh][8 * st + 1], s[jh][8 * st + 2], s[jh][8 * st + 3]},
                           float4{s[jh][8 * st + 4], s[jh][8 * st + 5], s[jh][8 * st + 6], s[jh][8 * st + 7]}, ph, pm, pl_);
#pragma unroll
                for (int o = 0; o < NO; o++) {
                    uint4 vf[3];
#pragma unroll
                    for (int pl = 0; pl < 3; pl++)
                        vf[pl] = att_read_vt<D>(reinterpret_cast<const char*>(&Vs[cur][pl][0]) + (jh * 32 + 16 * st) * 2 * D + tr_off[o]);
                    att_mma(oacc[o], vf[2], ph); att_mma(oacc[o], vf[1], pm); att_mma(oacc[o], vf[0], pl_);
                    att_mma(oacc[o], vf[1], ph); att_mma(oacc[o], vf[0], pm);
                    att_mma(oacc[o], vf[0], ph);
                }
            }
        if (kt + 1 < ntiles) store_kv(cur ^ 1, kr, vr);
        __syncthreads();
    }
    const int q = q0 + col;
    if (q < Lq) {
        const float inv = 1.0f / l_run;
        auto* Ob = O + ((size_t)b * Lq + q) * ldo + h * D;
#pragma unroll
        for (int o = 0; o < NO; o++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                st4(Ob + o * 32 + 8 * g + 4 * half,      // channels o * 32 + acc_row(4 g .. 4 g + 3, half)
                    float4{oacc[o][4 * g + 0] * inv, oacc[o][4 * g + 1] * inv, oacc[o][4 * g + 2] * inv, oacc[o][4 * g + 3] * inv});
    }
}

template <int D>
static int launch_attention_hd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                               dim3 grid, int Lq, int Lk, int dtype, hipStream_t stream, const unsigned char* key_mask) {
    // sqrt(1/D) as torch computes it in float64, then float32 (F.multi_head_attention_forward: q * float(head_dim) ** -0.5)
    const float scale = D == 32 ? (float)0.1767766952966369 : 0.125f;
    const bool bf16_mfma = odam_cfg::get(odam_cfg::ATT_BF16_MFMA) != 0;   // 0: keep bf16 mode on the fp32-instruction kernel
    // fp32: products through the exact three-way bf16 split (ODAM_ATT_X3=0 keeps the fp32 matrix instruction)
    const bool x3 = odam_cfg::get(odam_cfg::ATT_X3) != 0;
    if (dtype == 1 && bf16_mfma && (ldq % 8) == 0 && (ldk % 8) == 0 && (ldv % 8) == 0 && (ldo % 4) == 0) {
        hipLaunchKernelGGL(attention_bf16_kernel<D>, grid, dim3(256), 0, stream, (const bf16_t*)Q, ldq, (const bf16_t*)K, ldk,
                           (const bf16_t*)V, ldv, (bf16_t*)O, ldo, Lq, Lk, scale * 1.44269504088896341f, key_mask);
    } else if (dtype == 0 && x3 && (ldq % 4) == 0 && (ldk % 4) == 0 && (ldv % 4) == 0 && (ldo % 4) == 0) {
        hipLaunchKernelGGL(attention_x3_kernel<D>, grid, dim3(256), 0, stream, (const float*)Q, ldq, (const float*)K, ldk,
                           (const float*)V, ldv, (float*)O, ldo, Lq, Lk, scale, key_mask);
    } else {
#define ODAM_K(T, ...) hipLaunchKernelGGL((attention_kernel<T, D>), grid, dim3(256), 0, stream, (const T*)Q, ldq, (const T*)K, ldk, (const T*)V, ldv, (T*)O, ldo, Lq, Lk, scale, key_mask)
        ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    }
    ODAM_HIP(hipGetLastError());
    return 0;
}

int launch_attention(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                     int B, int H, int Lq, int Lk, int dtype, hipStream_t stream, const unsigned char* key_mask, int head_dim) {
    if (Lq <= 0 || Lk <= 0 || B <= 0) return 0;
    if (head_dim != 32 && head_dim != 64) return odam_fail(1, "launch_attention: head dim 32 or 64 only");
    const dim3 grid((Lq + 127) / 128, H, B);
    return head_dim == 32 ? launch_attention_hd<32>(Q, ldq, K, ldk, V, ldv, O, ldo, grid, Lq, Lk, dtype, stream, key_mask)
                          : launch_attention_hd<64>(Q, ldq, K, ldk, V, ldv, O, ldo, grid, Lq, Lk, dtype, stream, key_mask);
}

// head dimension 64, fp32 (associator GNN: scores / 64**0.5, src/models/associator.py:47-56)
int launch_attention_d64(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                         int B, int H, int Lq, int Lk, hipStream_t stream) {
    if (Lq <= 0 || Lk <= 0 || B <= 0) return 0;
    dim3 grid((Lq + 127) / 128, H, B);
    hipLaunchKernelGGL((attention_kernel<float, 64>), grid, dim3(256), 0, stream, Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk,
                       0.125f, (const unsigned char*)nullptr);
    ODAM_HIP(hipGetLastError());
    return 0;
}

// =================================================================================================
// residual add + LayerNorm over 256 channels: one wavefront per row, 4 channels per lane
// (nn.LayerNorm(256), eps 1e-5, biased variance; transformer.py:147-148, 160-166)
// =================================================================================================
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void add_layernorm_kernel(const T* __restrict__ x, const T* __restrict__ r,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ y,
                                                            const float* __restrict__ pos, int L,
                                                            T* __restrict__ y_pos, int M) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    float4 v = ld4(x + (size_t)row * 256 + lane * 4);
    if (r) {
        const float4 t = ld4(r + (size_t)row * 256 + lane * 4);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / 256.0f);
    const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
    const float var = wave_sum((dx * dx + dy * dy) + (dz * dz + dw * dw)) * (1.0f / 256.0f);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    const float4 g = *reinterpret_cast<const float4*>(gamma + lane * 4);
    const float4 be = *reinterpret_cast<const float4*>(beta + lane * 4);
    float4 o = {dx * rstd * g.x + be.x, dy * rstd * g.y + be.y, dz * rstd * g.z + be.z, dw * rstd * g.w + be.w};
    st4(y + (size_t)row * 256 + lane * 4, o);
    if (y_pos) {
        const float4 p = *reinterpret_cast<const float4*>(pos + (size_t)(row % L) * 256 + lane * 4);
        float4 o2 = {o.x + p.x, o.y + p.y, o.z + p.z, o.w + p.w};
        st4(y_pos + (size_t)row * 256 + lane * 4, o2);
    }
}

// the same over any C = 64 n, n = 2 .. 16 (transformer widths other than 256): one wavefront per row, channel 64 j + lane in
// register j (coalesced 64-element rows), two-pass statistics of the row shifted by its first value
constexpr int LN_MAXJ = 16;

template <typename T>
__global__ __launch_bounds__(256) void add_layernorm_c_kernel(const T* __restrict__ x, const T* __restrict__ r,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, T* __restrict__ y,
                                                              const float* __restrict__ pos, int L,
                                                              T* __restrict__ y_pos, int M, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const int nj = C >> 6;
    const size_t base = (size_t)row * C + lane;
    auto ld1 = [](const T* p) -> float {
        if constexpr (sizeof(T) == 2) return bf2f(*p);
        else return *p;
    };
    auto st1 = [](T* p, float v) {
        if constexpr (sizeof(T) == 2) *p = f2bf(v);
        else *p = v;
    };
    float v[LN_MAXJ];
#pragma unroll
    for (int j = 0; j < LN_MAXJ; j++) {
        v[j] = 0.0f;
        if (j < nj) {
            v[j] = ld1(x + base + 64 * j);
            if (r) v[j] += ld1(r + base + 64 * j);
        }
    }
    // statistics of v - v0 (v0 = the row's channel 0): C need not be a power of two, so a constant row summed as it stands would
    // not return its value as the mean; shifted, it sums to exactly 0 and the output is beta, as the C = 256 kernel gives it
    const float v0 = __shfl(v[0], 0);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; j++) {
        v[j] -= v0;
        if (j < nj) s += v[j];
    }
    const float inv_c = 1.0f / (float)C;
    const float mean = wave_sum(s) * inv_c;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; j++) {
        v[j] -= mean;
        if (j < nj) q += v[j] * v[j];
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_c + 1e-5f);
    const float* pr = y_pos ? pos + (size_t)(row % L) * C + lane : nullptr;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; j++) {
        if (j < nj) {
            const int c = 64 * j + lane;
            const float o = v[j] * rstd * gamma[c] + beta[c];
            st1(y + base + 64 * j, o);
            if (y_pos) st1(y_pos + base + 64 * j, o + pr[64 * j]);
        }
    }
}

int launch_add_layernorm(const void* x, const void* r, const float* gamma, const float* beta, void* y,
                         const float* pos, int L, void* y_pos, int M, int dtype, hipStream_t stream, int C) {
    if (M <= 0) return 0;
    if (C == 256) {
#define ODAM_K(T, ...) hipLaunchKernelGGL(add_layernorm_kernel<T>, dim3((M + 3) / 4), dim3(256), 0, stream, (const T*)x, (const T*)r, gamma, beta, (T*)y, pos, L, (T*)y_pos, M)
        ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    } else {
        if (C % 64 || C < 128 || C > 64 * LN_MAXJ) return odam_fail(1, "launch_add_layernorm: C must be a multiple of 64 in 128 .. 1024");
#define ODAM_K(T, ...) hipLaunchKernelGGL(add_layernorm_c_kernel<T>, dim3((M + 3) / 4), dim3(256), 0, stream, (const T*)x, (const T*)r, gamma, beta, (T*)y, pos, L, (T*)y_pos, M, C)
        ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    }
    ODAM_HIP(hipGetLastError());
    return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void add_pos_kernel(const T* __restrict__ x, const float* __restrict__ pos,
                                                      int L, T* __restrict__ out, int M) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // float4 index
    if (i >= (size_t)M * 64) return;
    const int row = (int)(i >> 6), c4 = (int)(i & 63);
    float4 p = *reinterpret_cast<const float4*>(pos + (size_t)(row % L) * 256 + c4 * 4);
    if (x) {
        const float4 v = ld4(x + i * 4);
        p.x += v.x; p.y += v.y; p.z += v.z; p.w += v.w;
    }
    st4(out + i * 4, p);
}

// rows of C4 = C / 4 four-channel groups (any C % 4 == 0)
template <typename T>
__global__ __launch_bounds__(256) void add_pos_c_kernel(const T* __restrict__ x, const float* __restrict__ pos,
                                                        int L, T* __restrict__ out, int M, int C4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // float4 index
    if (i >= (size_t)M * C4) return;
    const int row = (int)(i / C4), c4 = (int)(i - (size_t)row * C4);
    float4 p = *reinterpret_cast<const float4*>(pos + ((size_t)(row % L) * C4 + c4) * 4);
    if (x) {
        const float4 v = ld4(x + i * 4);
        p.x += v.x; p.y += v.y; p.z += v.z; p.w += v.w;
    }
    st4(out + i * 4, p);
}

int launch_add_pos(const void* x, const float* pos, int L, void* out, int M, int dtype, hipStream_t stream, int C) {
    if (M <= 0) return 0;
    if (C == 256) {
        const size_t n4 = (size_t)M * 64;
#define ODAM_K(T, ...) hipLaunchKernelGGL(add_pos_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const T*)x, pos, L, (T*)out, M)
        ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    } else {
        if (C <= 0 || C % 4) return odam_fail(1, "launch_add_pos: C must be a positive multiple of 4");
        const size_t n4 = (size_t)M * (C / 4);
#define ODAM_K(T, ...) hipLaunchKernelGGL(add_pos_c_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const T*)x, pos, L, (T*)out, M, C / 4)
        ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    }
    ODAM_HIP(hipGetLastError());
    return 0;
}

// =================================================================================================
// layout / pooling
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc4_kernel(const float* __restrict__ in, T* __restrict__ out,
                                                            int HW, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // pixel index over B*H*W
    if (i >= total) return;
    const size_t b = i / HW, p = i - b * HW;
    const float* s = in + b * 3 * (size_t)HW + p;
    float4 v = {s[0], s[HW], s[2 * (size_t)HW], 0.0f};
    if constexpr (sizeof(T) == 2) {      // bf16: one 16-byte chunk = 8 channels per pixel (3 real + 5 zero)
        st4(out + i * 8, v);
        st4(out + i * 8 + 4, float4{0.f, 0.f, 0.f, 0.f});
    } else {
        st4(out + i * 4, v);
    }
}

// fp32 NCHW -> NHWC4 with a zero frame: out [B][H + 6][W + 8][4], the image at rows 3 .. H + 2, columns 3 .. W + 2.
// What the stem-as-rows convolution reads (detr_model.hip, stem_rows): 8 consecutive pixels = 32 floats per filter row.
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc4_framed_kernel(const float* __restrict__ in, T* __restrict__ out,
                                                                   int H, int W, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // pixel index over B*(H+6)*(W+8)
    if (i >= total) return;
    const int Wp = W + 8, Hp = H + 6;
    const int xp = (int)(i % Wp);
    const size_t r = i / Wp;
    const int yp = (int)(r % Hp);
    const size_t b = r / Hp;
    const int x = xp - 3, y = yp - 3;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
        const size_t HW = (size_t)H * W;
        const float* sp = in + b * 3 * HW + (size_t)y * W + x;
        v = float4{sp[0], sp[HW], sp[2 * HW], 0.0f};
    }
    st4(out + i * 4, v);
}

int launch_nchw_to_nhwc4_framed(const float* in, void* out, int B, int H, int W, int dtype, hipStream_t stream) {
    const size_t total = (size_t)B * (H + 6) * (W + 8);
    if (!total) return 0;
#define ODAM_K(T, ...) hipLaunchKernelGGL(nchw_to_nhwc4_framed_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, (T*)out, H, W, total)
    ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    ODAM_HIP(hipGetLastError());
    return 0;
}

int launch_nchw_to_nhwc4(const float* in, void* out, int B, int H, int W, int dtype, hipStream_t stream) {
    const size_t total = (size_t)B * H * W;
    if (!total) return 0;
#define ODAM_K(T, ...) hipLaunchKernelGGL(nchw_to_nhwc4_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, (T*)out, H * W, total)
    ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    ODAM_HIP(hipGetLastError());
    return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ in, T* __restrict__ out, int H,
                                                      int W, int C4, int Ho, int Wo, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // over B*Ho*Wo*C4
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    size_t p = i / C4;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const size_t b = p / Ho;
    float4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = 0; dy < 3; dy++) {
        const int iy = oy * 2 - 1 + dy;
        if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const int ix = ox * 2 - 1 + dx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const float4 v = ld4(in + (((b * H + iy) * W + ix) * (size_t)C4 + c4) * 4);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    st4(out + i * 4, m);
}

int launch_maxpool3x3s2(const void* in, void* out, int B, int H, int W, int C, int Ho, int Wo, int dtype,
                        hipStream_t stream) {
    const size_t total = (size_t)B * Ho * Wo * (C / 4);
    if (!total) return 0;
#define ODAM_K(T, ...) hipLaunchKernelGGL(maxpool_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const T*)in, (T*)out, H, W, C / 4, Ho, Wo, total)
    ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    ODAM_HIP(hipGetLastError());
    return 0;
}


template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* __restrict__ in, float* __restrict__ out,
                                                           int HW, int C, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // output index over B*C*HW
    if (i >= total) return;
    const size_t p = i % HW;
    const size_t c = (i / HW) % C;
    const size_t b = i / ((size_t)HW * C);
    if constexpr (sizeof(T) == 2) out[i] = bf2f(in[(b * HW + p) * C + c]);
    else out[i] = in[(b * HW + p) * C + c];
}

int launch_nhwc_to_nchw(const void* in, float* out, int B, int H, int W, int C, int dtype, hipStream_t stream) {
    const size_t total = (size_t)B * H * W * C;
    if (!total) return 0;
#define ODAM_K(T, ...) hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const T*)in, out, H * W, C, total)
    ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    ODAM_HIP(hipGetLastError());
    return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void to_f32_kernel(const T* __restrict__ in, float* __restrict__ out, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) *reinterpret_cast<float4*>(out + i * 4) = ld4(in + i * 4);
}

int launch_to_f32(const void* in, float* out, size_t n, int dtype, hipStream_t stream) {
    if (n % 4) return odam_fail(1, "launch_to_f32: n must be a multiple of 4");      // whole float4 groups: no tail is dropped
    const size_t n4 = n / 4;
    if (!n4) return 0;
#define ODAM_K(T, ...) hipLaunchKernelGGL(to_f32_kernel<T>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const T*)in, out, n4)
    ODAM_DISPATCH(dtype, ODAM_K, 0);
#undef ODAM_K
    ODAM_HIP(hipGetLastError());
    return 0;
}

__global__ void sigmoid_kernel(float* x, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = 1.0f / (1.0f + expf(-x[i]));
}

int launch_sigmoid(float* x, int n, hipStream_t stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sigmoid_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, x, n);
    ODAM_HIP(hipGetLastError());
    return 0;
}

// =================================================================================================
// DETR.postprocess arithmetic per query (detr.py:111-140); thresholding + greedy NMS stay on the host
// =================================================================================================
__global__ void postprocess_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                   const float* __restrict__ angle, const float* __restrict__ offset,
                                   const float* __restrict__ size, const float* __restrict__ depth, int n, int n_cls1,
                                   int n_bins, float img_w, float img_h, float fx, float fy, float cx, float cy,
                                   float* __restrict__ rows) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* lg = logits + (size_t)i * n_cls1;
    float mx = lg[0];
    for (int c = 1; c < n_cls1; c++) mx = fmaxf(mx, lg[c]);
    float den = 0.0f;
    for (int c = 0; c < n_cls1; c++) den += expf(lg[c] - mx);
    float best = -1.0f;
    int cls = 0;
    for (int c = 0; c < n_cls1 - 1; c++) {  // softmax(-1)[..., :-1].max(-1): first maximum wins
        const float p = expf(lg[c] - mx) / den;
        if (p > best) { best = p; cls = c; }
    }
    const float* bx = boxes + (size_t)i * 4;
    const float x0 = (bx[0] - 0.5f * bx[2]) * img_w, y0 = (bx[1] - 0.5f * bx[3]) * img_h;
    const float x1 = (bx[0] + 0.5f * bx[2]) * img_w, y1 = (bx[1] + 0.5f * bx[3]) * img_h;
    const float d = depth[i];
    const float scx = offset[(size_t)i * 2 + 0] * img_w + (x0 + x1) / 2.0f;
    const float scy = offset[(size_t)i * 2 + 1] * img_h + (y0 + y1) / 2.0f;
    const float c3x = ((scx - cx) / fx) * d;
    const float c3y = ((scy - cy) / fy) * d;
    const float* an = angle + (size_t)i * n_bins;
    int ab = 0;
    float am = an[0];
    for (int k = 1; k < n_bins; k++)
        if (an[k] > am) { am = an[k]; ab = k; }
    float* o = rows + (size_t)i * 16;
    o[0] = best; o[1] = (float)cls;
    o[2] = x0; o[3] = y0; o[4] = x1; o[5] = y1;
    o[6] = c3x; o[7] = c3y; o[8] = d;
    o[9] = (float)ab;
    o[10] = size[(size_t)i * 3 + 0]; o[11] = size[(size_t)i * 3 + 1]; o[12] = size[(size_t)i * 3 + 2];
    o[13] = 0.0f; o[14] = 0.0f; o[15] = 0.0f;
}

int launch_postprocess(const float* logits, const float* boxes, const float* angle, const float* offset,
                       const float* size, const float* depth, int B, int Q, int n_cls1, int n_bins, float img_w,
                       float img_h, float fx, float fy, float cx, float cy, float* rows, hipStream_t stream) {
    const int n = B * Q;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(postprocess_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, logits, boxes, angle, offset,
                       size, depth, n, n_cls1, n_bins, img_w, img_h, fx, fy, cx, cy, rows);
    ODAM_HIP(hipGetLastError());
    return 0;
}

// ---- input transform: PIL bilinear resize of the uint8 frame + ToTensor + Normalize ------------
// Pillow's 8-bit resampling is two passes of integer arithmetic (src/libImaging/Resample.c): each pass rounds to a
// byte, clip8((2^21 + sum_k px[k] * K[k]) >> 22).  One thread owns one output pixel: it recomputes the (<= ksize)
// horizontally resampled bytes of the rows its vertical taps need, so no intermediate image exists.
struct ResampleTable {   // device pointers
    const int* xmin;     // [out] first source index
    const int* cnt;      // [out] taps
    const int* K;        // [out][ksize] fixed-point weights (22 fractional bits)
    int ksize;
};

__device__ __forceinline__ int clip8_22(int v) {
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the resized frame's three bytes at output pixel (X, Y) of image `img` [h][w][3]: both integer passes, as Pillow rounds them
__device__ __forceinline__ void resample_u8_pixel(const unsigned char* __restrict__ img, int w, const ResampleTable& tx, const ResampleTable& ty,
                                                  int need_x, int need_y, int X, int Y, int& u0, int& u1, int& u2) {
    const int x0 = need_x ? tx.xmin[X] : X, nx = need_x ? tx.cnt[X] : 1;
    const int y0 = need_y ? ty.xmin[Y] : Y, ny = need_y ? ty.cnt[Y] : 1;
    const int* kx = tx.K + (size_t)X * tx.ksize;
    const int* ky = ty.K + (size_t)Y * ty.ksize;
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    int last[3] = {0, 0, 0};
    for (int j = 0; j < ny; j++) {
        const unsigned char* row = img + ((size_t)(y0 + j) * w + x0) * 3;
        int hv[3];
        if (need_x) {
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int k = 0; k < nx; k++) {
                const int kk = kx[k];
                a0 += row[k * 3 + 0] * kk; a1 += row[k * 3 + 1] * kk; a2 += row[k * 3 + 2] * kk;
            }
            hv[0] = clip8_22(a0); hv[1] = clip8_22(a1); hv[2] = clip8_22(a2);
        } else {
            hv[0] = row[0]; hv[1] = row[1]; hv[2] = row[2];
        }
        if (need_y) {
            const int kk = ky[j];
            acc[0] += hv[0] * kk; acc[1] += hv[1] * kk; acc[2] += hv[2] * kk;
        }
        last[0] = hv[0]; last[1] = hv[1]; last[2] = hv[2];
    }
    u0 = need_y ? clip8_22(acc[0]) : last[0];
    u1 = need_y ? clip8_22(acc[1]) : last[1];
    u2 = need_y ? clip8_22(acc[2]) : last[2];
}

__global__ __launch_bounds__(256) void preprocess_u8_kernel(const unsigned char* __restrict__ rgb, int h, int w,
                                                            ResampleTable tx, ResampleTable ty, int need_x, int need_y,
                                                            float* __restrict__ out, int H, int W, float3 mean,
                                                            float3 stdv) {
    const int X = blockIdx.x * 256 + threadIdx.x;
    const int Y = blockIdx.y;
    const size_t b = blockIdx.z;
    if (X >= W) return;
    int u0, u1, u2;
    resample_u8_pixel(rgb + b * (size_t)h * w * 3, w, tx, ty, need_x, need_y, X, Y, u0, u1, u2);
    // ToTensor: float32(u8) / 255; Normalize: (x - mean) / std, float32 (transforms.py:222-243)
    const size_t plane = (size_t)H * W, o = (b * 3 * H + Y) * (size_t)W + X;
    out[o] = ((float)u0 / 255.0f - mean.x) / stdv.x;
    out[o + plane] = ((float)u1 / 255.0f - mean.y) / stdv.y;
    out[o + 2 * plane] = ((float)u2 / 255.0f - mean.z) / stdv.z;
}

int launch_preprocess_u8(const unsigned char* rgb, int B, int h, int w, const int* tx_xmin, const int* tx_cnt,
                         const int* tx_K, int tx_ksize, const int* ty_xmin, const int* ty_cnt, const int* ty_K,
                         int ty_ksize, float* out, int H, int W, const float mean[3], const float stdv[3],
                         hipStream_t stream) {
    if (B <= 0) return 0;
    ResampleTable tx{tx_xmin, tx_cnt, tx_K, tx_ksize}, ty{ty_xmin, ty_cnt, ty_K, ty_ksize};
    hipLaunchKernelGGL(preprocess_u8_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, stream, rgb, h, w, tx, ty,
                       (int)(W != w), (int)(H != h), out, H, W, float3{mean[0], mean[1], mean[2]},
                       float3{stdv[0], stdv[1], stdv[2]});
    ODAM_HIP(hipGetLastError());
    return 0;
}

// The same resize, written as what the stem's bf16-plane contraction reads (detr_forward.hip stem_u8): the framed NHWC4 image
// [B][H + 6][W + 8] of four bf16 per pixel, (u0 - c0, u1 - c1, u2 - c2, 1) inside the image and four zeros in the frame.  The
// differences are integers in [-255, 255], exact in bf16 (top 16 bits of their fp32 form); the fourth channel tells conv1's folded
// filters that the pixel exists (detr_weights.hip stem_u8_filters).  One thread per framed pixel, one 8-byte store: the grid covers
// the frame, so nothing needs clearing and nothing stale is read.
__global__ __launch_bounds__(256) void preprocess_u8_bf16x4_framed_kernel(const unsigned char* __restrict__ rgb, int h, int w,
                                                                          ResampleTable tx, ResampleTable ty, int need_x, int need_y,
                                                                          uint2* __restrict__ out, int H, int W, int c0, int c1, int c2) {
    const int Xp = blockIdx.x * 256 + threadIdx.x;
    const int Yp = blockIdx.y;
    const size_t b = blockIdx.z;
    if (Xp >= W + 8) return;
    int X, Y;
    uint2 v = uint2{0u, 0u};
    if (odam_dm::stem_u8_inside(Xp, Yp, H, W, X, Y)) {
        int u0, u1, u2;
        resample_u8_pixel(rgb + b * (size_t)h * w * 3, w, tx, ty, need_x, need_y, X, Y, u0, u1, u2);
        odam_dm::stem_u8_pixel(u0, u1, u2, c0, c1, c2, v.x, v.y);
    }
    out[(b * (H + 6) + Yp) * (size_t)(W + 8) + Xp] = v;
}

int launch_preprocess_u8_bf16x4_framed(const unsigned char* rgb, int B, int h, int w, const int* tx_xmin, const int* tx_cnt,
                                       const int* tx_K, int tx_ksize, const int* ty_xmin, const int* ty_cnt, const int* ty_K,
                                       int ty_ksize, void* out, int H, int W, const int centre[3], hipStream_t stream) {
    if (B <= 0) return 0;
    ResampleTable tx{tx_xmin, tx_cnt, tx_K, tx_ksize}, ty{ty_xmin, ty_cnt, ty_K, ty_ksize};
    hipLaunchKernelGGL(preprocess_u8_bf16x4_framed_kernel, dim3((W + 8 + 255) / 256, H + 6, B), dim3(256), 0, stream, rgb, h, w, tx, ty,
                       (int)(W != w), (int)(H != h), (uint2*)out, H, W, centre[0], centre[1], centre[2]);
    ODAM_HIP(hipGetLastError());
    return 0;
}

}  // namespace odam_dk
