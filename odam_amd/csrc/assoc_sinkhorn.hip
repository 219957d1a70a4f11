// assoc_sinkhorn.hip -- log_optimal_transport (likojack/ODAM src/models/associator.py:283-312): the whole loop as ONE single-workgroup
// launch.  Three kernels behind launch_sinkhorn, which the association forward (assoc.hip) and odam_assoc_sinkhorn call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/odam_assoc.h"
#include "assoc_internal.h"
#include "odam_config.h"
#include "odam_err.h"
#include "sk_wave.h"

using odam_assoc_internal::PG_GROUPS;

namespace {

// log_optimal_transport + log_sinkhorn_iterations (associator.py:283-312), one 1024-thread workgroup:
//   couplings Z[(m+1) x (n+1)] = [[scores, alpha], [alpha, alpha]] in LDS; u, v in LDS;
//   iters x { u = log_mu - logsumexp_j(Z + v);  v = log_nu - logsumexp_i(Z + u) };  out = Z + u + v - norm
// A row (or column) is reduced by a group of 8 lanes (xor butterflies inside the group), 128 groups at a time.
constexpr int SK_NT = 1024, SK_G = 8;

__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 4));
    return v;
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    return v;
}

__global__ __launch_bounds__(SK_NT) void sinkhorn_kernel(const float* __restrict__ scores, int lds, int m, int n,
                                                         float alpha, int iters, float* __restrict__ out,
                                                         const int* __restrict__ n_dev, const unsigned* __restrict__ err, unsigned* lost_count) {
    extern __shared__ float sm[];
    if (n_dev) n = *n_dev;      // replayed from a captured graph: the number of detections of THIS frame lives in memory
    const int M1 = m + 1, N1 = n + 1;
    float* Z = sm;                 // [M1][N1]
    float* u = Z + M1 * N1;        // [M1]
    float* v = u + M1;             // [N1]
    const int tid = threadIdx.x;
    for (int i = tid; i < M1 * N1; i += SK_NT) {
        const int r = i / N1, c = i - r * N1;
        Z[i] = (r < m && c < n) ? scores[(size_t)r * lds + c] : alpha;
    }
    for (int i = tid; i < M1; i += SK_NT) u[i] = 0.0f;
    for (int i = tid; i < N1; i += SK_NT) v[i] = 0.0f;
    const float norm = -logf((float)m + (float)n);
    const float log_mu_last = logf((float)n) + norm, log_nu_last = logf((float)m) + norm;
    __syncthreads();
    const int grp = tid / SK_G, gl = tid % SK_G;
    constexpr int NG = SK_NT / SK_G;
    for (int it = 0; it < iters; ++it) {
        for (int r0 = 0; r0 < M1; r0 += NG) {            // u: one group per row
            const int r = r0 + grp;
            float mx = -INFINITY;
            if (r < M1) for (int c = gl; c < N1; c += SK_G) mx = fmaxf(mx, Z[r * N1 + c] + v[c]);
            mx = group_max(mx);
            float sum = 0.0f;
            if (r < M1) for (int c = gl; c < N1; c += SK_G) sum += expf(Z[r * N1 + c] + v[c] - mx);
            sum = group_sum(sum);
            if (r < M1 && gl == 0) u[r] = ((r < m) ? norm : log_mu_last) - (logf(sum) + mx);
        }
        __syncthreads();
        for (int c0 = 0; c0 < N1; c0 += NG) {            // v: one group per column
            const int c = c0 + grp;
            float mx = -INFINITY;
            if (c < N1) for (int r = gl; r < M1; r += SK_G) mx = fmaxf(mx, Z[r * N1 + c] + u[r]);
            mx = group_max(mx);
            float sum = 0.0f;
            if (c < N1) for (int r = gl; r < M1; r += SK_G) sum += expf(Z[r * N1 + c] + u[r] - mx);
            sum = group_sum(sum);
            if (c < N1 && gl == 0) v[c] = ((c < n) ? norm : log_nu_last) - (logf(sum) + mx);
        }
        __syncthreads();
    }
    for (int i = tid; i < M1 * N1; i += SK_NT) {
        const int r = i / N1, c = i - r * N1;
        out[i] = (err && *err) ? NAN : Z[i] + u[r] + v[c] - norm;     // the matching kernel's launch was lost (grid_barrier): fail loudly downstream
    }
    if (tid == 0 && err && *err && lost_count) __hip_atomic_fetch_add(lost_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- Sinkhorn for at most 31 columns (the associator's case: <= 30 detections + dustbin) ----------------------------------
// Same iteration as sinkhorn_kernel; what differs is who reduces what.  A row (<= 32 entries) is one 16-lane DPP row of a
// wavefront, two columns per lane: four rows per wavefront, 64 rows per sweep of the 16 waves, reduced by quad permutes and
// half-row / row mirrors alone (register-file speed).  A wavefront takes two columns at once, lane = row; its 64-lane
// reductions finish through v_readlane.  No ds_bpermute is left on the dependent path of an iteration, and Z is stored with
// an odd row stride so that a column walks all LDS banks.  Measured per 100 iterations: DESIGN.md section 4.
__device__ __forceinline__ float dpp_f(float v, int ctrl_sel) {
    const int x = __builtin_bit_cast(int, v);
    int r;
    switch (ctrl_sel) {
        case 0: r = __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false); break;     // quad_perm [1,0,3,2]
        case 1: r = __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false); break;     // quad_perm [2,3,0,1]
        case 2: r = __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false); break;    // row_half_mirror
        default: r = __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false); break;   // row_mirror
    }
    return __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float max16(float v) {
    v = fmaxf(v, dpp_f(v, 0)); v = fmaxf(v, dpp_f(v, 1)); v = fmaxf(v, dpp_f(v, 2)); v = fmaxf(v, dpp_f(v, 3));
    return v;
}
__device__ __forceinline__ float sum16(float v) {
    v += dpp_f(v, 0); v += dpp_f(v, 1); v += dpp_f(v, 2); v += dpp_f(v, 3);
    return v;
}

// exp / log of the iteration: the hardware's v_exp_f32 / v_log_f32 (through exp2 / log2).  The library functions are a
// range reduction and a polynomial each -- four of them sit on the dependent path of every iteration and were most of its
// 1.9 us; arguments here are (x - max) <= 0 and sums in [1, 64], where the hardware forms are good to ~1e-6 relative.
#define SK_EXP(x) __expf(x)
#define SK_LOG(x) __logf(x)
__global__ __launch_bounds__(SK_NT) void sinkhorn32_kernel(const float* __restrict__ scores, int lds, int m, int n,
                                                           float alpha, int iters, float* __restrict__ out,
                                                           const int* __restrict__ n_dev, const unsigned* __restrict__ err, unsigned* lost_count) {
    extern __shared__ float sm[];
    if (n_dev) n = *n_dev;
    const int M1 = m + 1, N1 = n + 1;       // N1 <= 32
    constexpr int ZS = 33;
    float* Z = sm;                          // [M1][33]
    float* u = Z + (size_t)M1 * ZS;         // [M1]
    float* v = u + M1;                      // [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NWV = SK_NT / 64;
    for (int i = tid; i < M1 * N1; i += SK_NT) {
        const int r = i / N1, c = i - r * N1;
        Z[r * ZS + c] = (r < m && c < n) ? scores[(size_t)r * lds + c] : alpha;
    }
    for (int i = tid; i < M1; i += SK_NT) u[i] = 0.0f;
    if (tid < 32) v[tid] = 0.0f;
    const float norm = -logf((float)m + (float)n);
    const float log_mu_last = logf((float)n) + norm, log_nu_last = logf((float)m) + norm;
    __syncthreads();
    const int q4 = lane >> 4, l16 = lane & 15;
    // 64-lane reductions: DPP inside the four 16-lane rows, then the four row results through SGPRs (v_readlane) --
    // no ds_bpermute on the dependent path
    auto max64 = [](float x) {
        x = max16(x);
        const float a0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 0));
        const float a1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 16));
        const float a2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 32));
        const float a3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 48));
        return fmaxf(fmaxf(a0, a1), fmaxf(a2, a3));
    };
    auto sum64 = [](float x) {
        x = sum16(x);
        const float a0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 0));
        const float a1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 16));
        const float a2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 32));
        const float a3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 48));
        return (a0 + a1) + (a2 + a3);
    };
    for (int it = 0; it < iters; ++it) {
        // u: four rows per wavefront, one per 16-lane DPP row; a lane holds columns l16 and l16 + 16 of its row
        for (int r0 = 4 * wave; r0 < M1; r0 += 4 * NWV) {
            const int r = r0 + q4;
            const bool ok0 = r < M1 && l16 < N1, ok1 = r < M1 && l16 + 16 < N1;
            const float x0 = ok0 ? Z[r * ZS + l16] + v[l16] : -INFINITY;
            const float x1 = ok1 ? Z[r * ZS + l16 + 16] + v[l16 + 16] : -INFINITY;
            const float mx = max16(fmaxf(x0, x1));
            const float e = sum16((ok0 ? SK_EXP(x0 - mx) : 0.0f) + (ok1 ? SK_EXP(x1 - mx) : 0.0f));
            if (r < M1 && l16 == 0) u[r] = ((r < m) ? norm : log_mu_last) - (SK_LOG(e) + mx);
        }
        __syncthreads();
        // v: columns wave and wave + 16 on this wavefront (two independent chains), lane = row
        {
            const int c0 = wave, c1 = wave + NWV;
            const bool h0 = c0 < N1, h1 = c1 < N1;
            float m0 = -INFINITY, m1 = -INFINITY;
            for (int r = lane; r < M1; r += 64) {
                const float ur = u[r];
                if (h0) m0 = fmaxf(m0, Z[r * ZS + c0] + ur);
                if (h1) m1 = fmaxf(m1, Z[r * ZS + c1] + ur);
            }
            m0 = max64(m0); m1 = max64(m1);
            float e0 = 0.0f, e1 = 0.0f;
            for (int r = lane; r < M1; r += 64) {
                const float ur = u[r];
                if (h0) e0 += SK_EXP(Z[r * ZS + c0] + ur - m0);
                if (h1) e1 += SK_EXP(Z[r * ZS + c1] + ur - m1);
            }
            e0 = sum64(e0); e1 = sum64(e1);
            if (lane == 0) {
                if (h0) v[c0] = ((c0 < n) ? norm : log_nu_last) - (SK_LOG(e0) + m0);
                if (h1) v[c1] = ((c1 < n) ? norm : log_nu_last) - (SK_LOG(e1) + m1);
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < M1 * N1; i += SK_NT) {
        const int r = i / N1, c = i - r * N1;
        out[i] = (err && *err) ? NAN : Z[r * ZS + c] + u[r] + v[c] - norm;
    }
    // ... and tell the host (pinned counter, read after the stream has been synchronised: odam_assoc_lost_launches)
    if (tid == 0 && err && *err && lost_count) __hip_atomic_fetch_add(lost_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- Sinkhorn on ONE wavefront: <= 128 rows, <= 32 columns -----------------------------------------------------------------------
// The iteration of log_sinkhorn_iterations (associator.py:283-312) on scaling factors instead of potentials.  With
// K_rc = exp(Z_rc + u_r + v_c) (the coupling at the potentials reached so far), a_r, b_c the factors since then, an iteration is
//     a_r = mu_r / sum_c K_rc b_c        b_c = nu_c / sum_r K_rc a_r
// -- multiply-adds and two reciprocals; no exp / log / max, no LDS and no barrier.  Every J iterations the factors are ABSORBED:
// u += log a, v += log b, K recomputed from Z, u, v, a = b = 1.  In exact arithmetic this is the log-space iteration; in float32
// it stays so as long as the factors of J iterations stay far inside the float range (they are checked at every absorption:
// 1e-18 .. 1e18) -- an entry of K that underflows is one whose mass is below e^-87 of a unit AT the current potentials, which the
// log-space sum drops in the same way; and it is recomputed at the next absorption.  The potentials start at u = -(row maximum),
// v = 0, so that no entry of K overflows whatever the size of the scores (the hand-built scene weights reach +-1000).  A failed
// check restarts the whole loop with J = 1 (absorb after every iteration), then in log space -- same launch, wave-uniform decision.
// Layout: lane = row (RB rows per lane), its K row in NC registers.  The column sums are one TRANSPOSING reduction (sk_wave.h): a
// level combines two registers into one -- the lanes whose level bit is clear keep the first column and receive the partner
// lane's share of it, the others the second -- so 32 columns cost 16 + 8 + 4 + 2 + 1 exchanges, not 32 x 6, and end with column
// c's total in lane sk_lane(c): b is ONE register (lane = column), one reciprocal per iteration; the row sums read it back
// through v_readlane.
template <int RB, int NC>
__global__ __launch_bounds__(64) void sinkhorn_wave_kernel(const float* __restrict__ scores, int lds, int m, int n, float alpha, int iters,
                                                           float* __restrict__ out, const int* __restrict__ n_dev,
                                                           const unsigned* __restrict__ err, unsigned* lost_count, int first_mode) {
    constexpr int P = NC <= 8 ? 8 : NC <= 16 ? 16 : 32;
    if (n_dev) n = *n_dev;
    const int lane = threadIdx.x, M1 = m + 1, N1 = n + 1;
    const float inv = 1.0f / ((float)m + (float)n);          // exp(norm)
    const float norm = -logf((float)m + (float)n);
    float z[RB][NC], rho[RB], mu[RB], u[RB], vc[NC];
#pragma unroll
    for (int j = 0; j < RB; j++) {
        const int r = lane + 64 * j;
        const bool valid = r < M1;
        rho[j] = -INFINITY;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            z[j][c] = (valid && c < N1) ? ((r < m && c < n) ? scores[(size_t)r * lds + c] : alpha) : -INFINITY;
            rho[j] = fmaxf(rho[j], z[j][c]);
        }
        mu[j] = valid ? (r < m ? inv : (float)n * inv) : 0.0f;
    }
    const int cl = sk_lane(lane & 31) & (P - 1);             // the column whose total this lane receives
    const float nu = cl < n ? inv : (cl == n ? (float)m * inv : 0.0f);
    auto bcast = [&](float x, float (&o)[NC]) {             // lane = column -> every lane holds all columns
#pragma unroll
        for (int c = 0; c < NC; c++) o[c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), sk_lane(c)));
    };
    bool done = false;
    for (int mode = first_mode; mode < 2 && !done; mode++) {
        const int J = mode == 0 ? 10 : 1;
        float K[RB][NC], a[RB], vl = 0.0f, b = nu != 0.0f ? 1.0f : 0.0f;
        bool good = true;
#pragma unroll
        for (int j = 0; j < RB; j++) {
            u[j] = (mu[j] != 0.0f && iters > 0) ? -rho[j] : 0.0f;      // no iteration, no absorption: the result is Z - norm, as from every other kernel
            a[j] = 0.0f;
#pragma unroll
            for (int c = 0; c < NC; c++) K[j][c] = expf(z[j][c] + u[j]);          // exp(-inf) = 0 outside the matrix
        }
        for (int it0 = 0; it0 < iters; it0 += J) {
            const int ne = iters - it0 < J ? iters - it0 : J;
            for (int e = 0; e < ne; e++) {
                float bc[NC];
                bcast(b, bc);
#pragma unroll
                for (int j = 0; j < RB; j++) {
                    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
                    for (int c = 0; c < NC; c += 2) { s0 = fmaf(K[j][c], bc[c], s0); s1 = fmaf(K[j][c + 1], bc[c + 1], s1); }
                    a[j] = mu[j] != 0.0f ? mu[j] * __builtin_amdgcn_rcpf(s0 + s1) : 0.0f;
                }
                float t[32];
#pragma unroll
                for (int c = 0; c < 32; c++) {
                    if (c < NC) {
                        t[c] = K[0][c] * a[0];
#pragma unroll
                        for (int j = 1; j < RB; j++) t[c] = fmaf(K[j][c], a[j], t[c]);
                    } else t[c] = 0.0f;
                }
                const float tot = sk_colsum<P>(t, lane);
                b = nu != 0.0f ? nu * __builtin_amdgcn_rcpf(tot) : 0.0f;
            }
            // absorb the factors into the potentials
            good = good && (nu == 0.0f || (b > 1e-18f && b < 1e18f));
            vl += nu != 0.0f ? logf(b) : 0.0f;
#pragma unroll
            for (int j = 0; j < RB; j++) {
                good = good && (mu[j] == 0.0f || (a[j] > 1e-18f && a[j] < 1e18f));
                u[j] += mu[j] != 0.0f ? logf(a[j]) : 0.0f;
            }
            if (it0 + J < iters) {
                bcast(vl, vc);
#pragma unroll
                for (int j = 0; j < RB; j++)
#pragma unroll
                    for (int c = 0; c < NC; c++) K[j][c] = expf(z[j][c] + u[j] + vc[c]);
                b = nu != 0.0f ? 1.0f : 0.0f;
            }
        }
        bcast(vl, vc);
        done = __all(good);
    }
    if (!done) {
        // log space with the same layout: a row's logsumexp is per lane, a column's a 64-lane reduction
        const float log_mu_last = logf((float)n) + norm, log_nu_last = logf((float)m) + norm;
#pragma unroll
        for (int c = 0; c < NC; c++) vc[c] = 0.0f;
#pragma unroll
        for (int j = 0; j < RB; j++) u[j] = 0.0f;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int j = 0; j < RB; j++) {
                const int r = lane + 64 * j;
                float mx = -INFINITY, sum = 0.0f;
#pragma unroll
                for (int c = 0; c < NC; c++) mx = fmaxf(mx, z[j][c] + vc[c]);
#pragma unroll
                for (int c = 0; c < NC; c++) sum += expf(z[j][c] + vc[c] - mx);          // exp(-inf) = 0 outside the matrix
                u[j] = r < M1 ? ((r < m) ? norm : log_mu_last) - (logf(sum) + mx) : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < RB; j++) mx = fmaxf(mx, z[j][c] + u[j]);
                mx = sk_wave_max(mx);
                float sum = 0.0f;
#pragma unroll
                for (int j = 0; j < RB; j++) sum += expf(z[j][c] + u[j] - mx);
                sum = sk_wave_sum(sum);
                vc[c] = c < N1 ? ((c < n) ? norm : log_nu_last) - (logf(sum) + mx) : 0.0f;
            }
        }
    }
    const bool lost = err && *err;
#pragma unroll
    for (int j = 0; j < RB; j++) {
        const int r = lane + 64 * j;
        if (r < M1) {
#pragma unroll
            for (int c = 0; c < NC; c++)
                if (c < N1) out[(size_t)r * N1 + c] = lost ? NAN : z[j][c] + u[j] + vc[c] - norm;
        }
    }
    if (lane == 0 && lost && lost_count) __hip_atomic_fetch_add(lost_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // err = the persistent matching kernel's flag word (bar + 1): that launch is over (stream order) and its flag has been read
    // above -- leave generation, flag, the group counters and the per-XCD counters at zero for the next launch (saves a memset per frame)
    if (err && lane <= 2 * PG_GROUPS + PG_GROUPS) {
        unsigned* bar = const_cast<unsigned*>(err) - 1;
        if (lane == 0) { bar[0] = 0u; bar[1] = 0u; }
        else if (lane <= 2 * PG_GROUPS) bar[32 * lane] = 0u;
        else bar[32 * (1 + 2 * PG_GROUPS) + (lane - 2 * PG_GROUPS - 1)] = 0u;      // the placement words of gnn_rowpart_kernel
    }
}

// The two LDS-resident kernels hold up to 150 KB of dynamic LDS (the default bound is 64 KB): allowed here, once per device, before
// their first launch from either entry point
constexpr size_t SK_LDS_MAX = 150 * 1024;
int allow_big_lds() {
    static bool done[64] = {};
    int dev = 0;
    ODAM_HIP(hipGetDevice(&dev));
    if (done[dev & 63]) return 0;
    ODAM_HIP(hipFuncSetAttribute((const void*)sinkhorn32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SK_LDS_MAX));
    ODAM_HIP(hipFuncSetAttribute((const void*)sinkhorn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SK_LDS_MAX));
    done[dev & 63] = true;
    return 0;
}

// which of the three kernels launch_sinkhorn takes for m rows and room for n_cap columns (dustbins not counted), and the dynamic LDS it asks for
enum SkKernel { SK_WAVE, SK_COLS32, SK_GENERAL };
SkKernel sinkhorn_choice(size_t m, size_t n_cap, size_t* lds_bytes) {
    if (n_cap + 1 <= 32 && m + 1 <= 128 && odam_cfg::get(odam_cfg::ASSOC_SK_FAST) != 0) { *lds_bytes = 0; return SK_WAVE; }      // one wavefront, registers only
    if (n_cap + 1 <= 32 && m + 1 <= 1100) { *lds_bytes = ((m + 1) * 33 + (m + 1) + 32) * sizeof(float); return SK_COLS32; }      // 1100 rows of 33 floats + u + v fit the 150 KB
    *lds_bytes = ((m + 1) * (n_cap + 1) + (m + 1) + (n_cap + 1)) * sizeof(float);
    return SK_GENERAL;
}

}  // namespace

int odam_assoc_internal::launch_sinkhorn(const float* scores, int lds_, int m_, int n_, int n_cap, float alpha, int iters, float* Z_out,
                                         const int* n_dev, hipStream_t st, const unsigned* err, unsigned* lost_count, bool* cleans_bar) {
    size_t lds = 0;
    const SkKernel which = sinkhorn_choice((size_t)m_, (size_t)n_cap, &lds);
    if (lds > SK_LDS_MAX) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "launch_sinkhorn: %d x %d needs %zu bytes of LDS, the limit is %zu (the (m+1) x (n+1) matrix, u and v)", m_, n_cap, lds, SK_LDS_MAX);
        return odam_fail(1, msg);
    }
    if (which == SK_WAVE) {
        const int nc = (n_cap + 1 + 7) >> 3;
#define ODAM_SKW(RB, NC) hipLaunchKernelGGL((sinkhorn_wave_kernel<RB, NC>), dim3(1), dim3(64), 0, st, scores, lds_, m_, n_, alpha, iters, Z_out, n_dev, err, lost_count, odam_cfg::get(odam_cfg::ASSOC_SK_FAST) - 1)
        if (m_ + 1 <= 64) { if (nc == 1) ODAM_SKW(1, 8); else if (nc == 2) ODAM_SKW(1, 16); else if (nc == 3) ODAM_SKW(1, 24); else ODAM_SKW(1, 32); }
        else { if (nc == 1) ODAM_SKW(2, 8); else if (nc == 2) ODAM_SKW(2, 16); else if (nc == 3) ODAM_SKW(2, 24); else ODAM_SKW(2, 32); }
#undef ODAM_SKW
        if (cleans_bar) *cleans_bar = err != nullptr;
    } else if (which == SK_COLS32) {
        if (int rc = allow_big_lds()) return rc;
        hipLaunchKernelGGL(sinkhorn32_kernel, dim3(1), dim3(SK_NT), lds, st, scores, lds_, m_, n_, alpha, iters, Z_out, n_dev, err, lost_count);
    } else {
        if (int rc = allow_big_lds()) return rc;
        hipLaunchKernelGGL(sinkhorn_kernel, dim3(1), dim3(SK_NT), lds, st, scores, lds_, m_, n_, alpha, iters, Z_out, n_dev, err, lost_count);
    }
    ODAM_HIP(hipGetLastError());
    return 0;
}

extern "C" int odam_assoc_sinkhorn(const float* scores, int lds_, int m_, int n_, float alpha, int iters, float* Z_out,
                                   void* stream) {
    if (!scores || !Z_out || m_ < 1 || n_ < 1) return odam_fail(1, "odam_assoc_sinkhorn: bad argument");
    if (lds_ < n_) return odam_fail(1, "odam_assoc_sinkhorn: row stride lds must be at least n");
    if (iters < 0) return odam_fail(1, "odam_assoc_sinkhorn: iters must be at least 0");
    // the whole matrix lives in one workgroup's LDS (or one wavefront's registers): what the kernel launch_sinkhorn would take needs
    size_t need = ~(size_t)0;
    if ((size_t)m_ <= SK_LDS_MAX && (size_t)n_ <= SK_LDS_MAX) (void)sinkhorn_choice((size_t)m_, (size_t)n_, &need);      // (beyond that u or v alone do not fit; no overflow below it)
    if (need > SK_LDS_MAX) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "odam_assoc_sinkhorn: %d x %d needs %zu bytes of LDS, the limit is %zu (the (m+1) x (n+1) matrix, u and v)", m_, n_, need, SK_LDS_MAX);
        return odam_fail(1, msg);
    }
    return odam_assoc_internal::launch_sinkhorn(scores, lds_, m_, n_, n_, alpha, iters, Z_out, nullptr, (hipStream_t)stream);
}
