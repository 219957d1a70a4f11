// dq_fit.hip -- the reference's second object model on the device: QuadricOptimizer.run (likojack/ODAM
// src/super_quadric/sq_libs.py:194-241), the ellipsoid (dual quadric) fit of the ODAM paper's comparison.
//
// One launch fits every object through all its Adam steps.  No surface sampler is involved: the projected box of a dual
// quadric is a closed form of C = M Q M^T, so an object is ONE wavefront -- views strided over the 64 lanes -- and a workgroup
// is a handful of independent wavefronts (no LDS, no barrier).  Five parameters per object (translate[3], angle,
// scale_factor); every lane keeps them, their Adam moments and the derived Q redundantly, so nothing is broadcast.
//
// Summation order (part of the contract with tests/dq_ref.py), for each of the nine per-view sums -- the four masked L1 terms
// (x_min, x_max, y_min, y_max) and the five gradient components:
//   1. lane l adds the views l, l + 64, l + 128, ... in ascending order to a partial that starts at +0;
//   2. the 64 partials go through a butterfly of six rounds, partner = lane XOR 32, 16, 8, 4, 2, 1 in this order, each round
//      partial <- partial + partner's partial (addition commutes, so all lanes end with the same bits).
// Then loss = ((s0 / F + s1 / F) + s2 / F) + s3 / F, and torch.optim.Adam's single-tensor step (sq_core.h adam_scalar) with
// lr 0.01 for all five parameters.  The gradient components already carry the 1 / F of the mean.
//
// Discriminant rule: the reference asserts that no view's sqrt argument is negative (sq_libs.py:129,136).  Here the object's
// status becomes 1, the step at which it happened is recorded, and the object keeps the parameters it had BEFORE that step
// (the reference raises before optimizer.step()); the other objects of the launch are not affected.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/odam_sq.h"
#include "dq_core.h"
#include "dq_ctx.h"
#include "odam_err.h"
#include "wave_ops.h"

namespace {

using namespace odam_dq;

struct DqArgs {
    const float* init5;
    const float* half_dims;
    const int* view_offsets;
    const float* P;
    const float* tgt;
    const float* mask;
    const float* adam;      // [n_iters][2]
    int n_obj, n_iters, max_views;
    float* out5;
    float* out_Q;
    float* loss_log;
    float* traj;
    int* status;            // [n_obj][2]: code, first step
};

// NV = 1, 2: a lane keeps its (at most NV) views in registers for the whole fit; NV == 0: it reads them every step (four views per
// lane in registers need more than the 256 registers of an eight-wave workgroup and spill).  Same arithmetic in every form.
template <int NV>
__global__ __launch_bounds__(512) void dq_fit_kernel(DqArgs A) {
    const int lane = threadIdx.x & 63;
    const int obj = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (obj >= A.n_obj) return;
    const int v0 = A.view_offsets[obj];
    const int F = A.view_offsets[obj + 1] - v0;
    float p[5], m1[5], m2[5], h[3];
    for (int k = 0; k < 5; k++) { p[k] = A.init5[5 * obj + k]; m1[k] = 0.0f; m2[k] = 0.0f; }
    for (int k = 0; k < 3; k++) h[k] = A.half_dims[3 * obj + k];
    const float qnan = __builtin_nanf("");
    int code = 0, first = -1;
    if (F < 1 || F > A.max_views) { code = 2; first = 0; }

    constexpr int NR = NV > 0 ? NV : 1;
    float Mr[NR][12], tr[NR][4], mr[NR][4];
    if (NV > 0 && code == 0) {
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const int v = lane + 64 * j;
            if (v < F) {
                for (int k = 0; k < 12; k++) Mr[j][k] = A.P[(size_t)(v0 + v) * 12 + k];
                for (int k = 0; k < 4; k++) { tr[j][k] = A.tgt[(size_t)(v0 + v) * 4 + k]; mr[j][k] = A.mask[(size_t)(v0 + v) * 4 + k]; }
            } else {
                for (int k = 0; k < 12; k++) Mr[j][k] = 0.0f;
                for (int k = 0; k < 4; k++) { tr[j][k] = 0.0f; mr[j][k] = 0.0f; }
            }
        }
    }
    const float Ff = (float)F;
    const float invF = 1.0f / Ff;
    int it = 0;
    for (; it < A.n_iters && code == 0; it++) {
        const Obj o = make_obj(p, h);
        float acc[9];
        for (int k = 0; k < 9; k++) acc[k] = 0.0f;
        bool bad = false;
        if (NV > 0) {
#pragma unroll
            for (int j = 0; j < NR; j++) {
                if (lane + 64 * j < F) {
                    const ViewOut w = view_terms(o, p, h, Mr[j], tr[j], mr[j], invF);
                    bad = bad || w.bad;
                    for (int k = 0; k < 4; k++) acc[k] = acc[k] + w.l[k];
                    for (int k = 0; k < 5; k++) acc[4 + k] = acc[4 + k] + w.g[k];
                }
            }
        } else {
            for (int v = lane; v < F; v += 64) {
                float M[12], t[4], m[4];
                for (int k = 0; k < 12; k++) M[k] = A.P[(size_t)(v0 + v) * 12 + k];
                for (int k = 0; k < 4; k++) { t[k] = A.tgt[(size_t)(v0 + v) * 4 + k]; m[k] = A.mask[(size_t)(v0 + v) * 4 + k]; }
                const ViewOut w = view_terms(o, p, h, M, t, m, invF);
                bad = bad || w.bad;
                for (int k = 0; k < 4; k++) acc[k] = acc[k] + w.l[k];
                for (int k = 0; k < 5; k++) acc[4 + k] = acc[4 + k] + w.g[k];
            }
        }
        if (__ballot(bad) != 0ull) {      // wave-uniform: every lane of the object leaves the loop together
            code = 1;
            first = it;
            break;
        }
        for (int k = 0; k < 9; k++) acc[k] = wave_sum(acc[k]);
        const float loss = ((acc[0] / Ff + acc[1] / Ff) + acc[2] / Ff) + acc[3] / Ff;
        const float neg_step = A.adam[2 * it], bc2_sqrt = A.adam[2 * it + 1];
        for (int k = 0; k < 5; k++) odam_sq::adam_scalar(p[k], m1[k], m2[k], acc[4 + k], neg_step, bc2_sqrt);
        if (lane == 0) {
            if (A.loss_log) A.loss_log[(size_t)obj * A.n_iters + it] = loss;
            if (A.traj)
                for (int k = 0; k < 5; k++) A.traj[((size_t)obj * A.n_iters + it) * 5 + k] = p[k];
        }
    }
    // an object that stopped: the remaining rows say so (loss NaN, parameters as they stay)
    for (int r = it + lane; r < A.n_iters; r += 64) {
        if (A.loss_log) A.loss_log[(size_t)obj * A.n_iters + r] = qnan;
        if (A.traj)
            for (int k = 0; k < 5; k++) A.traj[((size_t)obj * A.n_iters + r) * 5 + k] = p[k];
    }
    const Obj o = make_obj(p, h);
    if (lane < 16) {      // Q entry k from lane k, without a dynamically indexed register array
        float q = o.Q[0];
#pragma unroll
        for (int k = 1; k < 16; k++) q = (lane == k) ? o.Q[k] : q;
        A.out_Q[(size_t)obj * 16 + lane] = q;
    }
    if (lane == 0) {
        for (int k = 0; k < 5; k++) A.out5[5 * obj + k] = p[k];
        A.status[2 * obj] = code;
        A.status[2 * obj + 1] = first;
    }
}

int ensure_adam(odam_dq_state* st, int n_iters, hipStream_t stream) {
    if (n_iters <= st->adam_iters) return ODAM_OK;
    std::vector<float> tab((size_t)2 * n_iters);
    for (int t = 1; t <= n_iters; t++) {      // torch/optim/adam.py _single_tensor_adam: Python floats (binary64), cast at use
        const double bc1 = 1.0 - std::pow(0.9, (double)t);
        const double bc2 = 1.0 - std::pow(0.999, (double)t);
        tab[2 * (t - 1) + 0] = (float)(-(0.01 / bc1));
        tab[2 * (t - 1) + 1] = (float)std::pow(bc2, 0.5);
    }
    if (st->d_adam) {      // an earlier launch on this stream may still read the smaller table
        ODAM_HIP(hipStreamSynchronize(stream));
        (void)hipFree(st->d_adam);
        st->d_adam = nullptr;
        st->adam_iters = 0;
    }
    ODAM_HIP(hipMalloc(&st->d_adam, sizeof(float) * tab.size()));
    ODAM_HIP(hipMemcpy(st->d_adam, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    st->adam_iters = n_iters;
    return ODAM_OK;
}

}  // namespace

extern "C" int odam_dq_set_group_waves(odam_sq_ctx* ctx, int waves) {
    if (!ctx || (waves != 1 && waves != 2 && waves != 4 && waves != 8))
        return odam_fail(ODAM_E_INVALID, "odam_dq_set_group_waves: waves must be 1, 2, 4 or 8");
    odam_sq_ctx_dq(ctx)->group_waves = waves;
    return ODAM_OK;
}

extern "C" int odam_dq_fit_batch(odam_sq_ctx* ctx, int n_obj, const float* init5, const float* half_dims, const int* view_offsets,
                                 const float* P, const float* tgt, const float* mask, int n_iters, int max_views, float* out5,
                                 float* out_Q, float* loss_log, float* traj, int* status, void* stream) {
    if (!ctx || !init5 || !half_dims || !view_offsets || !P || !tgt || !mask || !out5 || !out_Q || !status)
        return odam_fail(ODAM_E_INVALID, "odam_dq_fit_batch: null pointer");
    if (n_obj < 0 || n_iters < 0) return odam_fail(ODAM_E_INVALID, "odam_dq_fit_batch: bad size");
    if (max_views < 1 || max_views > 16 * ODAM_SQ_MAX_VIEWS)
        return odam_fail(ODAM_E_LIMIT, "odam_dq_fit_batch: max_views outside 1..16 * ODAM_SQ_MAX_VIEWS");
    if (n_obj == 0) return ODAM_OK;
    odam_dq_state* st = odam_sq_ctx_dq(ctx);
    const int rc = ensure_adam(st, n_iters, (hipStream_t)stream);
    if (rc != ODAM_OK) return rc;
    DqArgs A{};
    A.init5 = init5; A.half_dims = half_dims; A.view_offsets = view_offsets; A.P = P; A.tgt = tgt; A.mask = mask;
    A.adam = st->d_adam; A.n_obj = n_obj; A.n_iters = n_iters; A.max_views = max_views;
    A.out5 = out5; A.out_Q = out_Q; A.loss_log = loss_log; A.traj = traj; A.status = status;
    const int waves = st->group_waves;
    const dim3 grid((unsigned)((n_obj + waves - 1) / waves)), block((unsigned)(64 * waves));
    hipStream_t s = (hipStream_t)stream;
    if (max_views <= 64) hipLaunchKernelGGL(dq_fit_kernel<1>, grid, block, 0, s, A);
    else if (max_views <= 128) hipLaunchKernelGGL(dq_fit_kernel<2>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dq_fit_kernel<0>, grid, block, 0, s, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
