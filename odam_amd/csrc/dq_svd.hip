// dq_svd.hip -- the reference's closed-form dual quadric on the device: compute_quadric_svd (likojack/ODAM
// src/super_quadric/sq_libs.py:30-36) over the plane vectors load_pred_object builds (src/utils/tracking_gt_utils.py:198-205)
// and quadric_2mat (src/super_quadric/quadric_helper.py:16-36).  No 3D guess is involved: 2D box edges and projections only.
//
// One launch, one wavefront per object, views strided over the 64 lanes, a workgroup of 1, 2, 4 or 8 independent wavefronts
// (odam_dq_set_group_waves, the switch of dq_fit.hip; no workgroup barrier anywhere).  Everything is float64.
//
// Rows.  View v, edge e in the order x_min, x_max, y_min, y_max, if mask[v][e] != 0:
//   pi_k = P_v[0][k] - x * P_v[2][k]  (x edges)  or  P_v[1][k] - y * P_v[2][k]  (y edges), k = 0..3      (the line [1, 0, -x] @ P)
//   pi  <- pi / sqrt((pi_0^2 + pi_1^2) + pi_2^2)                                                         (normalize_plane)
//   s   = (pi_0^2, 2 pi_0 pi_1, 2 pi_0 pi_2, 2 pi_0 pi_3, pi_1^2, 2 pi_1 pi_2, 2 pi_1 pi_3, pi_2^2, 2 pi_2 pi_3, pi_3^2)   (plane_2vect)
// with every product and sum rounded on its own (the unit is compiled with -ffp-contract=off).
//
// Summation order (part of the contract with tests/quadric_svd_ref.py) of the 55 sums A_ij = sum s_i s_j, i <= j:
//   1. lane l takes the views l, l + 64, l + 128, ... in ascending order and, inside a view, the unmasked edges in the order
//      above; each row adds the rounded product s_i * s_j to a partial that starts at +0;
//   2. the 64 partials go through a butterfly of six rounds, partner = lane XOR 32, 16, 8, 4, 2, 1 in this order, each round
//      partial <- partial + partner's partial (addition commutes, so all lanes end with the same bits).
// Nothing depends on which wavefront of a workgroup an object is, so results are bit-identical for every group size.
//
// Eigen step.  Cyclic Jacobi on the symmetric 10 x 10 matrix, kept with the accumulated rotations V in the wavefront's own
// slice of LDS; lane k < 10 owns index k of a rotation.  Pivot order (0,1), (0,2), ..., (0,9), (1,2), ..., (8,9) in every
// sweep; a pivot that is exactly zero is passed over.  Before every sweep: off = sqrt(sum_{i != j} a_ij^2) and
// tr = sum |a_ii| (the trace: A is positive semi-definite); stop when off <= 2^-52 * tr, or after JACOBI_MAX_SWEEPS sweeps
// (status 1).  All control flow is wave-uniform: every lane reads the same pivot from LDS.  The answer is the column of V of
// the smallest diagonal entry (the first one if two are equal), unpacked by quadric_2mat and normalised Q <- -Q / Q[3][3].
// The ellipsoid test of DualQuadric.get_srt (sq_libs.py:257-280) is the same iteration on the 3 x 3 matrix
// Q[:3,:3] + t t^T, t = -Q[:3,3], in registers: an ellipsoid has three eigenvalues > 0.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/odam_sq.h"
#include "dq_ctx.h"
#include "odam_err.h"
#include "wave_ops.h"

namespace {

constexpr int N = 10;                    // entries of the vectorised quadric
constexpr int NT = 55;                   // upper triangle of A
constexpr int LD = N + 1;                // padded row of the LDS matrices
constexpr int MAX_WAVES = 8;             // largest group (odam_dq_set_group_waves)
constexpr int JACOBI_MAX_SWEEPS = 30;    // 10 x 10 needs 6 - 9 on the fixture; the limit only ends a matrix with NaN / Inf in it
constexpr int MIN_EDGES = 9;             // a dual quadric has 9 degrees of freedom up to scale

struct SvdArgs {
    const int* view_offsets;
    const double* P;
    const double* edges;
    const float* mask;
    int n_obj, max_views;
    double* out_Q;
    double* out_eig;
    int* status;
};

// the rotation that annihilates a_pq: tangent, cosine, sine (Rutishauser's form; theta = +-Inf gives t = 0)
__device__ inline void jacobi_cs(double app, double aqq, double apq, double& t, double& c, double& s) {
    const double theta = (aqq - app) / (2.0 * apq);
    t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

// one rotation of the 3 x 3 problem in registers: pivot (p, q), k the third index
__device__ inline void rot3(double& app, double& aqq, double& apq, double& akp, double& akq) {
    if (apq == 0.0) return;
    double t, c, s;
    jacobi_cs(app, aqq, apq, t, c, s);
    const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    akp = np_;
    akq = nq_;
}

__global__ __launch_bounds__(512) void dq_svd_kernel(SvdArgs A) {
    __shared__ double sA[MAX_WAVES][N][LD];
    __shared__ double sV[MAX_WAVES][N][LD];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int obj = blockIdx.x * (blockDim.x >> 6) + w;
    if (obj >= A.n_obj) return;
    const int v0 = A.view_offsets[obj];
    const int F = A.view_offsets[obj + 1] - v0;
    const double qnan = __builtin_nan("");
    const bool views_ok = F >= 1 && F <= A.max_views;

    double acc[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) acc[k] = 0.0;
    int cnt = 0;
    if (views_ok) {
        for (int v = lane; v < F; v += 64) {
            const size_t row = (size_t)(v0 + v);
            double M[12];
#pragma unroll
            for (int k = 0; k < 12; k++) M[k] = A.P[row * 12 + k];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (A.mask[row * 4 + e] != 0.0f) {
                    const double val = A.edges[row * 4 + e];
                    double pi[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) pi[k] = M[4 * (e >> 1) + k] - val * M[8 + k];
                    const double nrm = sqrt((pi[0] * pi[0] + pi[1] * pi[1]) + pi[2] * pi[2]);
#pragma unroll
                    for (int k = 0; k < 4; k++) pi[k] = pi[k] / nrm;
                    const double s[N] = {pi[0] * pi[0], 2.0 * pi[0] * pi[1], 2.0 * pi[0] * pi[2], 2.0 * pi[0] * pi[3],
                                         pi[1] * pi[1], 2.0 * pi[1] * pi[2], 2.0 * pi[1] * pi[3],
                                         pi[2] * pi[2], 2.0 * pi[2] * pi[3], pi[3] * pi[3]};
                    int idx = 0;
#pragma unroll
                    for (int i = 0; i < N; i++)
#pragma unroll
                        for (int j = i; j < N; j++, idx++) acc[idx] = acc[idx] + s[i] * s[j];
                    cnt++;
                }
            }
        }
    }
    const int n_edges = wave_sum(cnt);
    if (!views_ok || n_edges < MIN_EDGES) {      // wave-uniform: nothing computed
        if (lane < 16) A.out_Q[(size_t)obj * 16 + lane] = qnan;
        if (lane < 3) A.out_eig[(size_t)obj * 3 + lane] = qnan;
        if (lane == 0) A.status[obj] = 2;
        return;
    }
#pragma unroll
    for (int k = 0; k < NT; k++) acc[k] = wave_sum(acc[k]);

    double (*a)[LD] = sA[w];
    double (*vv)[LD] = sV[w];
    if (lane == 0) {
        int idx = 0;
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = i; j < N; j++, idx++) { a[i][j] = acc[idx]; a[j][i] = acc[idx]; }
    }
    if (lane < N)
        for (int j = 0; j < N; j++) vv[lane][j] = (j == lane) ? 1.0 : 0.0;

    bool converged = false;
    for (int sweep = 0;; sweep++) {
        wave_lds_sync();
        double off = 0.0, tr = 0.0;
        if (lane < N)
            for (int j = 0; j < N; j++) {
                const double x = a[lane][j];
                if (j != lane) off = off + x * x;
                else tr = fabs(x);
            }
        off = wave_sum(off);
        tr = wave_sum(tr);
        if (sqrt(off) <= 0x1p-52 * tr) { converged = true; break; }
        if (sweep == JACOBI_MAX_SWEEPS) break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                wave_lds_sync();
                const double apq = a[p][q];      // the same address in every lane: the branch is wave-uniform
                if (apq == 0.0) continue;
                const double app = a[p][p], aqq = a[q][q];
                double t, c, s;
                jacobi_cs(app, aqq, apq, t, c, s);
                if (lane < N) {
                    const int k = lane;
                    if (k == p) {
                        a[p][p] = app - t * apq;
                        a[p][q] = 0.0;
                        a[q][p] = 0.0;
                    } else if (k == q) {
                        a[q][q] = aqq + t * apq;
                    } else {
                        const double akp = a[k][p], akq = a[k][q];
                        const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                        a[k][p] = np_; a[p][k] = np_;
                        a[k][q] = nq_; a[q][k] = nq_;
                    }
                    const double vkp = vv[k][p], vkq = vv[k][q];
                    vv[k][p] = c * vkp - s * vkq;
                    vv[k][q] = s * vkp + c * vkq;
                }
            }
    }

    // eigenvalues: the smallest (its index), the second smallest, the largest -- every lane, from the same LDS words
    int imin = 0;
    double l1 = a[0][0], l2 = HUGE_VAL, l10 = a[0][0];
    for (int k = 1; k < N; k++) {
        const double d = a[k][k];
        if (d < l1) { l2 = l1; l1 = d; imin = k; }
        else if (d < l2) l2 = d;
        if (d > l10) l10 = d;
    }
    double qv[N];
#pragma unroll
    for (int k = 0; k < N; k++) qv[k] = vv[k][imin];
    // quadric_2mat
    double Q[16] = {qv[0], qv[1], qv[2], qv[3], qv[1], qv[4], qv[5], qv[6], qv[2], qv[5], qv[7], qv[8], qv[3], qv[6], qv[8], qv[9]};
    int code = converged ? 0 : 1;
    if (qv[9] == 0.0) {
        code = 1;      // no affine normalisation exists: Q stays the unit eigenvector's matrix
    } else {
        const double q33 = qv[9];
#pragma unroll
        for (int k = 0; k < 16; k++) Q[k] = -(Q[k] / q33);
        // get_srt's test: eigenvalues of Q[:3,:3] + t t^T, t = -Q[:3,3]
        const double t0 = -Q[3], t1 = -Q[7], t2 = -Q[11];
        double b00 = Q[0] + t0 * t0, b01 = Q[1] + t0 * t1, b02 = Q[2] + t0 * t2;
        double b11 = Q[5] + t1 * t1, b12 = Q[6] + t1 * t2, b22 = Q[10] + t2 * t2;
        bool conv3 = false;
        for (int sweep = 0;; sweep++) {
            const double off3 = sqrt(2.0 * ((b01 * b01 + b02 * b02) + b12 * b12));
            if (off3 <= 0x1p-52 * ((fabs(b00) + fabs(b11)) + fabs(b22))) { conv3 = true; break; }
            if (sweep == JACOBI_MAX_SWEEPS) break;
            rot3(b00, b11, b01, b02, b12);
            rot3(b00, b22, b02, b01, b12);
            rot3(b11, b22, b12, b01, b02);
        }
        if (!(conv3 && b00 > 0.0 && b11 > 0.0 && b22 > 0.0)) code = 1;
    }
    if (lane < 16) {      // Q entry k from lane k, without a dynamically indexed register array
        double q = Q[0];
#pragma unroll
        for (int k = 1; k < 16; k++) q = (lane == k) ? Q[k] : q;
        A.out_Q[(size_t)obj * 16 + lane] = q;
    }
    if (lane == 0) {
        A.out_eig[(size_t)obj * 3 + 0] = l1;
        A.out_eig[(size_t)obj * 3 + 1] = l2;
        A.out_eig[(size_t)obj * 3 + 2] = l10;
        A.status[obj] = code;
    }
}

}  // namespace

extern "C" int odam_dq_svd_batch(odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const double* P, const double* edges,
                                 const float* mask, int max_views, double* out_Q, double* out_eig, int* status, void* stream) {
    if (!ctx || !view_offsets || !P || !edges || !mask || !out_Q || !out_eig || !status)
        return odam_fail(ODAM_E_INVALID, "odam_dq_svd_batch: null pointer");
    if (n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_dq_svd_batch: bad size");
    if (max_views < 1 || max_views > 16 * ODAM_SQ_MAX_VIEWS)
        return odam_fail(ODAM_E_LIMIT, "odam_dq_svd_batch: max_views outside 1..16 * ODAM_SQ_MAX_VIEWS");
    if (n_obj == 0) return ODAM_OK;
    SvdArgs A{};
    A.view_offsets = view_offsets; A.P = P; A.edges = edges; A.mask = mask; A.n_obj = n_obj; A.max_views = max_views;
    A.out_Q = out_Q; A.out_eig = out_eig; A.status = status;
    const int waves = odam_sq_ctx_dq(ctx)->group_waves;
    const dim3 grid((unsigned)((n_obj + waves - 1) / waves)), block((unsigned)(64 * waves));
    hipLaunchKernelGGL(dq_svd_kernel, grid, block, 0, (hipStream_t)stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
