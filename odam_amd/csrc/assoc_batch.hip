// assoc_batch.hip -- the association network's BATCHED forward with the validation loss (likojack/ODAM src/models/associator.py:202-268,
// eval_only = False): b samples with their own track and detection counts, the tracks of all samples through the encoder and the fuser as
// one row set, the fused tracks padded with -1 to the batch's largest track count (_reshape_tracks, :184-200), the matching layers over
// the padded block -- the padding rows are keys and queries like any other (AttentionalGNN.forward passes no mask), so a sample's
// assignment depends on the batch it sits in --, the score blocks, and log_optimal_transport plus the loss gather
// sum_pairs -Z[gt_track, gt_det] (:256-258) of all samples in ONE launch (odam_assoc_ot_batch).
//
// The matching layers are the launch sequence of assoc.hip's enqueue_forward over [B Tmax track rows | 30 B detection rows]: one lin per
// projection and MLP over the whole block, two batched attention launches per layer (launch_attention_d64's batch argument strides the
// queries by Lq ld and the keys by Lk ld: exactly this layout).  No persistent kernel: with B times the rows the sequence is not
// latency-bound in the way the single frame is, and a device-wide barrier would bring a residency assumption along.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "../../include/odam_assoc.h"
#include "assoc_internal.h"
#include "detr_kernels.h"
#include "odam_err.h"

using namespace odam_assoc_internal;

namespace {

constexpr int D = 256, NT = 100, ND = 30;
constexpr int MAX_SUM_T = 1024, MAX_GT = 4096;      // tracks of a batch; ground-truth pairs of a batch

#define RC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// ---- log_optimal_transport + loss gather, one workgroup per sample -----------------------------------------------------------------
// The iteration of sinkhorn32_kernel (assoc_sinkhorn.hip): couplings [(m+1) x (n+1)] in LDS with an odd row stride, a row reduced by one
// 16-lane DPP row (two columns per lane), a column by one wavefront (lane = row, 64 rows at a time), exp / log through the hardware's
// v_exp_f32 / v_log_f32.  What a row's or a column's reduction adds in which order does not depend on the number of wavefronts (a
// wavefront only takes MORE rows and columns in turn when there are fewer of them), so the 256-thread form, taken when every sample of
// the launch has at most 127 rows, and the 1024-thread form give the same bits: a sample's Z does not depend on what else is in the batch.
constexpr int OT_ZS = 33;
constexpr size_t OT_LDS_MAX = 150 * 1024;
__host__ __device__ constexpr size_t ot_lds_bytes(int max_m) { return ((size_t)(max_m + 1) * (OT_ZS + 1) + 32) * sizeof(float); }

__device__ __forceinline__ float ot_dpp(float v, int sel) {
    const int x = __builtin_bit_cast(int, v);
    int r;
    switch (sel) {
        case 0: r = __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false); break;     // quad_perm [1,0,3,2]
        case 1: r = __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false); break;     // quad_perm [2,3,0,1]
        case 2: r = __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false); break;    // row_half_mirror
        default: r = __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false); break;   // row_mirror
    }
    return __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float ot_max16(float v) {
    v = fmaxf(v, ot_dpp(v, 0)); v = fmaxf(v, ot_dpp(v, 1)); v = fmaxf(v, ot_dpp(v, 2)); v = fmaxf(v, ot_dpp(v, 3));
    return v;
}
__device__ __forceinline__ float ot_sum16(float v) {
    v += ot_dpp(v, 0); v += ot_dpp(v, 1); v += ot_dpp(v, 2); v += ot_dpp(v, 3);
    return v;
}
__device__ __forceinline__ float ot_row(float x, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); }
__device__ __forceinline__ float ot_max64(float x) {
    x = ot_max16(x);
    return fmaxf(fmaxf(ot_row(x, 0), ot_row(x, 16)), fmaxf(ot_row(x, 32), ot_row(x, 48)));
}
__device__ __forceinline__ float ot_sum64(float x) {
    x = ot_sum16(x);
    return (ot_row(x, 0) + ot_row(x, 16)) + (ot_row(x, 32) + ot_row(x, 48));
}

// status bits: 1 = Z holds a NaN (the loss term is 0: associator.py:254-255), 2 = the sample's shape is outside the launch's limits
// (nothing written but status and a zero loss term), 4 = a ground-truth index outside [-1, m] x [-1, n] (that pair is left out)
template <int NTH>
__global__ __launch_bounds__(NTH) void ot_batch_kernel(const float* __restrict__ scores, const long long* __restrict__ score_off,
                                                       const int* __restrict__ lds_, const int* __restrict__ m_, const int* __restrict__ n_,
                                                       int max_m, float alpha, int iters, const int* __restrict__ gt,
                                                       const int* __restrict__ gt_off, float* __restrict__ Z_out,
                                                       const long long* __restrict__ Z_off, double* __restrict__ loss_terms,
                                                       int* __restrict__ status) {
    extern __shared__ float sm[];
    __shared__ int has_nan;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = m_[b], n = n_[b], lds = lds_[b];
    if (m < 1 || m > max_m || n < 1 || n > ND || lds < n) {      // (uniform over the workgroup) the LDS of this launch holds max_m + 1 rows of 31 columns
        if (tid == 0) { status[b] = 2; loss_terms[b] = 0.0; }
        return;
    }
    constexpr int NWV = NTH / 64, ZS = OT_ZS;
    const int M1 = m + 1, N1 = n + 1;
    float* Z = sm;                          // [M1][33]
    float* u = Z + (size_t)M1 * ZS;         // [M1]
    float* v = u + M1;                      // [32]
    const float* sc = scores + score_off[b];
    for (int i = tid; i < M1 * N1; i += NTH) {
        const int r = i / N1, c = i - r * N1;
        Z[r * ZS + c] = (r < m && c < n) ? sc[(size_t)r * lds + c] : alpha;
    }
    for (int i = tid; i < M1; i += NTH) u[i] = 0.0f;
    if (tid < 32) v[tid] = 0.0f;
    if (tid == 0) has_nan = 0;
    const float norm = -logf((float)m + (float)n);
    const float log_mu_last = logf((float)n) + norm, log_nu_last = logf((float)m) + norm;
    __syncthreads();
    const int q4 = lane >> 4, l16 = lane & 15;
    for (int it = 0; it < iters; ++it) {
        // u: four rows per wavefront, one per 16-lane DPP row; a lane holds columns l16 and l16 + 16 of its row
        for (int r0 = 4 * wave; r0 < M1; r0 += 4 * NWV) {
            const int r = r0 + q4;
            const bool ok0 = r < M1 && l16 < N1, ok1 = r < M1 && l16 + 16 < N1;
            const float x0 = ok0 ? Z[r * ZS + l16] + v[l16] : -INFINITY;
            const float x1 = ok1 ? Z[r * ZS + l16 + 16] + v[l16 + 16] : -INFINITY;
            const float mx = ot_max16(fmaxf(x0, x1));
            const float e = ot_sum16((ok0 ? __expf(x0 - mx) : 0.0f) + (ok1 ? __expf(x1 - mx) : 0.0f));
            if (r < M1 && l16 == 0) u[r] = ((r < m) ? norm : log_mu_last) - (__logf(e) + mx);
        }
        __syncthreads();
        // v: two columns at a time per wavefront (two independent chains), lane = row
        for (int c0 = wave; c0 < N1; c0 += 2 * NWV) {
            const int c1 = c0 + NWV;
            const bool h1 = c1 < N1;
            float m0 = -INFINITY, m1 = -INFINITY;
            for (int r = lane; r < M1; r += 64) {
                const float ur = u[r];
                m0 = fmaxf(m0, Z[r * ZS + c0] + ur);
                if (h1) m1 = fmaxf(m1, Z[r * ZS + c1] + ur);
            }
            m0 = ot_max64(m0); m1 = ot_max64(m1);
            float e0 = 0.0f, e1 = 0.0f;
            for (int r = lane; r < M1; r += 64) {
                const float ur = u[r];
                e0 += __expf(Z[r * ZS + c0] + ur - m0);
                if (h1) e1 += __expf(Z[r * ZS + c1] + ur - m1);
            }
            e0 = ot_sum64(e0); e1 = ot_sum64(e1);
            if (lane == 0) {
                v[c0] = ((c0 < n) ? norm : log_nu_last) - (__logf(e0) + m0);
                if (h1) v[c1] = ((c1 < n) ? norm : log_nu_last) - (__logf(e1) + m1);
            }
        }
        __syncthreads();
    }
    float* out = Z_out + Z_off[b];
    bool nan = false;
    for (int i = tid; i < M1 * N1; i += NTH) {      // every element is read and rewritten by ONE thread; u and v are only read
        const int r = i / N1, c = i - r * N1;
        const float z = Z[r * ZS + c] + u[r] + v[c] - norm;
        Z[r * ZS + c] = z;
        out[i] = z;
        nan = nan || z != z;
    }
    if (nan) has_nan = 1;
    __syncthreads();
    if (tid == 0) {
        int st = has_nan ? 1 : 0;
        double s = 0.0;      // in pair order, binary64: the same bits on every call, whatever else the launch holds
        const int k0 = gt_off ? gt_off[b] : 0, k1 = gt_off ? gt_off[b + 1] : 0;
        for (int k = k0; k < k1; k++) {
            const int g0 = gt[2 * k], g1 = gt[2 * k + 1];
            if (g0 < -1 || g0 > m || g1 < -1 || g1 > n) { st |= 4; continue; }
            s += -(double)Z[(g0 < 0 ? m : g0) * ZS + (g1 < 0 ? n : g1)];      // -1: the dustbin, as the reference's negative index
        }
        loss_terms[b] = (st & 1) ? 0.0 : s;
        status[b] = st;
    }
}

int launch_ot_batch(const float* scores, const long long* score_off, const int* lds, const int* m, const int* n, int B, int max_m, float alpha,
                    int iters, const int* gt, const int* gt_off, float* Z_out, const long long* Z_off, double* loss_terms, int* status,
                    hipStream_t st) {
    const size_t bytes = ot_lds_bytes(max_m);
    if (max_m + 1 <= 128) {
        hipLaunchKernelGGL(ot_batch_kernel<256>, dim3(B), dim3(256), bytes, st, scores, score_off, lds, m, n, max_m, alpha, iters, gt, gt_off,
                           Z_out, Z_off, loss_terms, status);
    } else {
        static bool allowed[64] = {};      // up to 150 KB of dynamic LDS (the default bound is 64 KB): once per device
        int dev = 0;
        ODAM_HIP(hipGetDevice(&dev));
        if (!allowed[dev & 63]) {
            ODAM_HIP(hipFuncSetAttribute((const void*)ot_batch_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OT_LDS_MAX));
            allowed[dev & 63] = true;
        }
        hipLaunchKernelGGL(ot_batch_kernel<1024>, dim3(B), dim3(1024), bytes, st, scores, score_off, lds, m, n, max_m, alpha, iters, gt, gt_off,
                           Z_out, Z_off, loss_terms, status);
    }
    ODAM_HIP(hipGetLastError());
    return 0;
}

// ---- the padded row block ----------------------------------------------------------------------------------------------------------
// Row r < B Tmax: sample r / Tmax, track t = r % Tmax -- the mean over the 100 time steps of the fuser's output (F.avg_pool1d; the sum
// runs in time order, as time_mean_kernel's in assoc.hip) or, for t >= T_b, the padding -1 (_reshape_tracks).  Rows B Tmax ..: the
// encoded detection slots of all samples, which went through the encoder behind the tracks' rows.  Columns 256 .. 511 of X receive the
// attention message of every layer before anything reads them.  Xpad keeps the block as assembled (odam_assoc_debug_read, which = 3).
__global__ __launch_bounds__(256) void batch_assemble_kernel(const float* __restrict__ cat, const int* __restrict__ T_, const int* __restrict__ Toff,
                                                             int Tmax, int RT, int sumT, float* __restrict__ X, float* __restrict__ Xpad) {
    const int r = blockIdx.x, c = threadIdx.x;
    float val;
    if (r >= RT) {
        val = cat[((size_t)sumT * NT + (r - RT)) * 512 + c];
    } else {
        const int b = r / Tmax, t = r - b * Tmax;
        if (t >= T_[b]) {
            val = -1.0f;
        } else {
            const float* p = cat + (size_t)(Toff[b] + t) * NT * 512 + c;
            float acc = 0.0f;
            for (int l = 0; l < NT; l += 10) {          // ten rows in flight, added in order
                float x[10];
#pragma unroll
                for (int i = 0; i < 10; i++) x[i] = p[(size_t)(l + i) * 512];
#pragma unroll
                for (int i = 0; i < 10; i++) acc += x[i];
            }
            val = acc / (float)NT;
        }
    }
    X[(size_t)r * 512 + c] = val;
    Xpad[(size_t)r * D + c] = val;
}

// scores[Toff_b + t][j] = <desc track (b, t), desc detection (b, j)> / 16 for all 30 detection slots (associator.py:242-243): eight
// track rows and the sample's 30 detection rows in LDS, one ascending-k fma chain per output.  Row stride 32, as the single frame's.
__global__ __launch_bounds__(256) void batch_scores_kernel(const float* __restrict__ mT, const int* __restrict__ T_, const int* __restrict__ Toff,
                                                           int Tmax, int RT, float* __restrict__ scores) {
    __shared__ float dd[ND][D + 1];
    __shared__ float tt[8][D];
    const int b = blockIdx.y, t0 = blockIdx.x * 8, tid = threadIdx.x;
    const int T = T_[b];
    if (t0 >= T) return;
    for (int j = 0; j < ND; j++) dd[j][tid] = mT[((size_t)RT + (size_t)b * ND + j) * D + tid];
    for (int i = 0; i < 8; i++) tt[i][tid] = t0 + i < T ? mT[((size_t)b * Tmax + t0 + i) * D + tid] : 0.0f;
    __syncthreads();
    const int i = tid >> 5, j = tid & 31;
    if (j >= ND || t0 + i >= T) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int k = 0; k < D; k++) acc = fmaf(tt[i][k], dd[j][k], acc);
    scores[(size_t)(Toff[b] + t0 + i) * 32 + j] = acc * 0.0625f;
}

// ---- per-sample descriptors: one pinned slot of a ring, one device mirror -------------------------------------------------------------
struct Desc {
    int T[MAX_BATCH], n[MAX_BATCH], lds[MAX_BATCH], Toff[MAX_BATCH + 1], gt_off[MAX_BATCH + 1], pad_[2];
    long long score_off[MAX_BATCH], Z_off[MAX_BATCH];
    int gt[2 * MAX_GT];
};
constexpr int RING = 4;

}  // namespace

struct odam_assoc_internal::BatchState {
    size_t rows = 0;                 // the padded block's reservation: B (Tmax + 30) rows
    float *X = nullptr, *Xpad = nullptr, *kv = nullptr, *att = nullptr, *h = nullptr, *mT = nullptr, *scores = nullptr;
    Desc* dev = nullptr;
    Desc* pin[RING] = {};
    hipEvent_t ev[RING] = {};
    bool used[RING] = {};
    int slot = 0;
    void release() {
        for (float* p : {X, Xpad, kv, att, h, mT, scores}) if (p) (void)hipFree(p);
        if (dev) (void)hipFree(dev);
        for (int i = 0; i < RING; i++) {
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};

void odam_assoc_internal::batch_release(odam_assoc* m) {
    if (!m || !m->batch) return;
    m->batch->release();
    delete m->batch;
    m->batch = nullptr;
}

int odam_assoc_internal::batch_debug_read(odam_assoc* m, int which, float* out, long long n) {
    if (!m->batch) return odam_fail(1, "odam_assoc_debug_read: no batched forward has run on this handle");
    if ((size_t)n > (which == 5 ? (size_t)MAX_SUM_T * 32 : m->batch->rows * D)) return odam_fail(1, "odam_assoc_debug_read: more than the reserved block");
    ODAM_HIP(hipDeviceSynchronize());
    const float* src = which == 3 ? m->batch->Xpad : (which == 4 ? m->batch->mT : m->batch->scores);
    ODAM_HIP(hipMemcpy(out, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int odam_assoc_reserve_batch(odam_assoc* m, int max_batch, int max_tracks_per_sample) {
    if (!m) return odam_fail(1, "odam_assoc_reserve_batch: null handle");
    if (max_batch < 1 || max_batch > MAX_BATCH || max_tracks_per_sample < 1 || max_tracks_per_sample > MAX_SUM_T)
        return odam_fail(3, "odam_assoc_reserve_batch: 1 <= max_batch <= 64 and 1 <= max_tracks_per_sample <= 1024");
    if (!m->finalized) return odam_fail(1, "odam_assoc_reserve_batch: call odam_assoc_finalize first");
    const size_t rows = (size_t)max_batch * (size_t)(max_tracks_per_sample + ND);
    if (m->batch && m->batch->rows >= rows) return 0;
    ODAM_HIP(hipDeviceSynchronize());      // a forward may still read the block that goes
    batch_release(m);
    BatchState* s = new BatchState();
    m->batch = s;      // (a failure below leaves a partial state that odam_assoc_destroy releases; rows stays 0, so no forward accepts it)
    ODAM_HIP(hipMalloc((void**)&s->X, rows * 512 * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->Xpad, rows * D * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->kv, rows * 768 * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->att, rows * D * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->h, rows * 512 * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->mT, rows * D * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->scores, (size_t)MAX_SUM_T * 32 * sizeof(float)));
    ODAM_HIP(hipMalloc((void**)&s->dev, sizeof(Desc)));
    for (int i = 0; i < RING; i++) {
        ODAM_HIP(hipHostMalloc((void**)&s->pin[i], sizeof(Desc), hipHostMallocDefault));
        ODAM_HIP(hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming));
    }
    s->rows = rows;
    return 0;
}

extern "C" int odam_assoc_ot_batch(const float* scores, const long long* score_off, const int* lds, const int* m, const int* n, int B, int max_m,
                                   float alpha, int iters, const int* gt, const int* gt_off, float* Z_out, const long long* Z_off,
                                   double* loss_terms, int* status, void* stream) {
    if (!scores || !score_off || !lds || !m || !n || !Z_out || !Z_off || !loss_terms || !status)
        return odam_fail(1, "odam_assoc_ot_batch: null pointer");
    if ((gt == nullptr) != (gt_off == nullptr)) return odam_fail(1, "odam_assoc_ot_batch: gt and gt_off go together (both null: no pairs)");
    if (iters < 0) return odam_fail(1, "odam_assoc_ot_batch: iters must be at least 0");
    if (B < 1 || B > MAX_BATCH) return odam_fail(3, "odam_assoc_ot_batch: 1 <= B <= 64");
    if (max_m < 1 || max_m > MAX_SUM_T) return odam_fail(3, "odam_assoc_ot_batch: 1 <= max_m <= 1024");
    return launch_ot_batch(scores, score_off, lds, m, n, B, max_m, alpha, iters, gt, gt_off, Z_out, Z_off, loss_terms, status, (hipStream_t)stream);
}

extern "C" int odam_assoc_forward_batch(odam_assoc* m, const float* tracks, const int* T, const float* detections, const int* n_det, int B,
                                        const int* gt, const int* gt_off, float* Z_out, const long long* Z_off, double* loss_terms, int* status,
                                        void* stream) {
    char msg[200];
    if (!m || !tracks || !T || !detections || !n_det || !Z_out || !Z_off || !loss_terms || !status)
        return odam_fail(1, "odam_assoc_forward_batch: null pointer");
    if ((gt == nullptr) != (gt_off == nullptr)) return odam_fail(1, "odam_assoc_forward_batch: gt and gt_off go together (both null: no pairs)");
    if (B < 1 || B > MAX_BATCH) return odam_fail(3, "odam_assoc_forward_batch: 1 <= B <= 64");
    long long sumT = 0;
    int Tmax = 0;
    for (int b = 0; b < B; b++) {
        if (T[b] < 1 || n_det[b] < 1 || n_det[b] > ND) {
            std::snprintf(msg, sizeof(msg), "odam_assoc_forward_batch: sample %d has T = %d, n_det = %d (T >= 1, 1 <= n_det <= 30)", b, T[b], n_det[b]);
            return odam_fail(3, msg);
        }
        sumT += T[b];
        Tmax = T[b] > Tmax ? T[b] : Tmax;
    }
    if (sumT > MAX_SUM_T) {
        std::snprintf(msg, sizeof(msg), "odam_assoc_forward_batch: %lld tracks in the batch, the limit is %d", sumT, MAX_SUM_T);
        return odam_fail(3, msg);
    }
    int n_gt = 0;
    if (gt_off) {
        if (gt_off[0] != 0) return odam_fail(1, "odam_assoc_forward_batch: gt_off must start at 0");
        for (int b = 0; b < B; b++) {
            if (gt_off[b + 1] < gt_off[b]) return odam_fail(1, "odam_assoc_forward_batch: gt_off must not decrease");
            if (gt_off[b + 1] > MAX_GT) return odam_fail(3, "odam_assoc_forward_batch: more than 4096 ground-truth pairs in the batch");
            for (int k = gt_off[b]; k < gt_off[b + 1]; k++) {
                if (gt[2 * k] < -1 || gt[2 * k] > T[b] || gt[2 * k + 1] < -1 || gt[2 * k + 1] > n_det[b]) {
                    std::snprintf(msg, sizeof(msg), "odam_assoc_forward_batch: ground-truth pair %d of sample %d is (%d, %d), outside [-1, %d] x [-1, %d]",
                                  k - gt_off[b], b, gt[2 * k], gt[2 * k + 1], T[b], n_det[b]);
                    return odam_fail(1, msg);
                }
            }
        }
        n_gt = gt_off[B];
    }
    if (sumT > m->max_tracks) {
        std::snprintf(msg, sizeof(msg), "odam_assoc_forward_batch: %lld tracks in the batch exceed the handle's max_tracks %d", sumT, m->max_tracks);
        return odam_fail(3, msg);
    }
    const size_t rows = (size_t)B * (size_t)(Tmax + ND);
    if (!m->batch || rows > m->batch->rows) {
        std::snprintf(msg, sizeof(msg), "odam_assoc_forward_batch: the padded block of %zu rows is larger than the reservation of %zu (odam_assoc_reserve_batch)",
                      rows, m->batch ? m->batch->rows : (size_t)0);
        return odam_fail(3, msg);
    }
    if (!m->finalized) return odam_fail(1, "odam_assoc_forward_batch: call odam_assoc_finalize first");
    // ---- the device is touched from here on ----
    BatchState* s = m->batch;
    hipStream_t st = (hipStream_t)stream;
    const int slot = s->slot;
    s->slot = (slot + 1) % RING;
    if (s->used[slot]) ODAM_HIP(hipEventSynchronize(s->ev[slot]));      // waits only if the stream is RING calls behind (as odam_trackwin_append's ring)
    Desc* d = s->pin[slot];
    d->Toff[0] = 0; d->gt_off[0] = 0;
    for (int b = 0; b < B; b++) {
        d->T[b] = T[b]; d->n[b] = n_det[b]; d->lds[b] = 32;
        d->Toff[b + 1] = d->Toff[b] + T[b];
        d->gt_off[b + 1] = gt_off ? gt_off[b + 1] : 0;
        d->score_off[b] = (long long)d->Toff[b] * 32;
        d->Z_off[b] = Z_off[b];
    }
    if (n_gt) std::memcpy(d->gt, gt, sizeof(int) * 2 * (size_t)n_gt);
    ODAM_HIP(hipMemcpyAsync(s->dev, d, offsetof(Desc, gt) + sizeof(int) * 2 * (size_t)n_gt, hipMemcpyHostToDevice, st));
    ODAM_HIP(hipEventRecord(s->ev[slot], st));
    s->used[slot] = true;
    const Desc* dd = s->dev;

    const int ST = (int)sumT, RT = B * Tmax, R = RT + B * ND;
    RC(encode_and_fuse(m, tracks, ST, detections, B * ND, st));
    float* X = s->X;
    hipLaunchKernelGGL(batch_assemble_kernel, dim3(R), dim3(256), 0, st, m->catT, dd->T, dd->Toff, Tmax, RT, ST, X, s->Xpad);
    ODAM_HIP(hipGetLastError());
    // matching layers (associator.py:111-139): every projection / MLP once over the whole block; the attention per side, batched over the samples
    float* kvT = s->kv;                                    // rows: q | k | v
    float* kvD = s->kv + (size_t)RT * 3 * D;
    for (size_t i = 0; i < m->gnn.size(); i++) {
        const Prop& P = m->gnn[i];
        const bool cross = m->gnn_cross[i] != 0;
        RC(assoc_lin(P.qkv, X, 512, R, nullptr, false, s->kv, 3 * D, nullptr, st));
        const float* srcT = cross ? kvD : kvT;             // source rows of the track queries
        const float* srcD = cross ? kvT : kvD;             // ... of the detection queries
        const int nT = cross ? ND : Tmax, nD = cross ? Tmax : ND;
        float* attO = m->merged ? X + D : s->att;
        const int ldO = m->merged ? 512 : D;
        RC(odam_dk::launch_attention_d64(kvT, 3 * D, srcT + D, 3 * D, srcT + 2 * D, 3 * D, attO, ldO, B, 4, Tmax, nT, st));
        RC(odam_dk::launch_attention_d64(kvD, 3 * D, srcD + D, 3 * D, srcD + 2 * D, 3 * D, attO + (size_t)RT * ldO, ldO, B, 4, ND, nD, st));
        if (!m->merged) RC(assoc_lin(P.merge, s->att, D, R, nullptr, false, X + D, 512, nullptr, st));
        RC(assoc_lin(P.m0, X, 512, R, nullptr, true, s->h, 2 * D, nullptr, st));
        RC(assoc_lin(P.m2, s->h, 2 * D, R, X, false, X, 512, nullptr, st));
    }
    RC(assoc_lin(m->final_proj, X, 512, R, nullptr, false, s->mT, D, nullptr, st));      // descriptors (associator.py:239)
    hipLaunchKernelGGL(batch_scores_kernel, dim3((Tmax + 7) / 8, B), dim3(256), 0, st, s->mT, dd->T, dd->Toff, Tmax, RT, s->scores);
    ODAM_HIP(hipGetLastError());
    return launch_ot_batch(s->scores, dd->score_off, dd->lds, dd->T, dd->n, B, Tmax, m->bin_score, m->iters, gt_off ? dd->gt : nullptr,
                           gt_off ? dd->gt_off : nullptr, Z_out, dd->Z_off, loss_terms, status, st);
}
