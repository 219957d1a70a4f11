// reproject.hip -- how well a fitted object explains the 2D detections it was fitted to, view by view: the forward half of the
// reference's two box predictions (likojack/ODAM src/super_quadric/sq_libs.py) for all objects and all views in one launch each,
// and the scores on top.  Arithmetic in reproject_core.h; restated in numpy by tests/reproject_ref.py.
//
//   reproject_sq_kernel     :395-413  constraint_2d: the object's surface points through every view, min / max of the valid ones.
//                           binary32.  Grid (objects, slices of 64 views): a workgroup of four wavefronts copies the object's points
//                           into LDS (n_pts x 12 bytes) and each wavefront takes every fourth view of the slice -- its 64 lanes
//                           stride over the points, the 12 values of M are wave-uniform, and a six-round XOR butterfly merges the
//                           lanes.  Min and max are exact and NaN-propagating (torch.min / torch.max), so the order is free.
//   reproject_dq_kernel     :289-314  get_bbox: the box of the conic C = (P Q) P^T.  binary64.  One wavefront per object, views strided
//                           over the lanes, Q in registers; per-view status 1 (four NaN) where the reference's sqrt would see a
//                           negative number, or c22 == 0.
//   reproject_score_kernel  per view the four residuals |ext - box| (mask, NaN -> 0, as :423-428) and the IoU of the detected box with
//                           the predicted box clipped to the image; per object their sums.  One wavefront per object.
//
// Summation order of the score kernel (wave_sum of wave_ops.h; tests/dq_ref.wave_sums): lane l adds the views l, l + 64, ... in
// ascending order to a partial that starts at +0; the 64 partials go through the butterfly partner = lane XOR 32, 16, 8, 4, 2, 1.
// The smallest IoU is merged as the pair (value, view) -- the smaller value, of equal values the smaller view -- so worst_view is
// the first view with the smallest IoU whatever the order.
//
// An object whose view count is outside 1 .. max_views owns no view: the reprojection kernels write nothing for it, the score
// kernel writes its row as NaN / -1 / 0.  No kernel writes a word that no view or object owns.  The wavefronts of a workgroup of
// the last two kernels are independent (odam_dq_set_group_waves objects per workgroup: scheduling only).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "../../include/odam_sq.h"
#include "dq_ctx.h"
#include "odam_err.h"
#include "reproject_core.h"
#include "wave_ops.h"

namespace {

using namespace odam_rp;

constexpr int SLICE = 64;          // views one workgroup of reproject_sq_kernel takes
constexpr int SQ_WAVES = 4;        // its wavefronts
constexpr int MAX_PTS = 4096;      // 48 KiB of LDS

struct SqArgs {
    const float* points;
    const int* view_offsets;
    const float* P;
    int n_pts, max_views;
    float* out_ext;
    int* out_nvalid;
};

__global__ __launch_bounds__(64 * SQ_WAVES) void reproject_sq_kernel(SqArgs A) {
    extern __shared__ float s_pts[];      // [n_pts][3]
    const int obj = blockIdx.x;
    const int v0 = A.view_offsets[obj];
    const int F = A.view_offsets[obj + 1] - v0;
    const int first = blockIdx.y * SLICE;
    if (F < 1 || F > A.max_views || first >= F) return;      // the same for the whole workgroup, and before its barrier
    const int n3 = 3 * A.n_pts;
    const float* src = A.points + (size_t)obj * n3;
    for (int i = threadIdx.x; i < n3; i += 64 * SQ_WAVES) s_pts[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int last = (first + SLICE < F) ? first + SLICE : F;
    for (int v = first + w; v < last; v += SQ_WAVES) {
        const size_t row = (size_t)(v0 + v);
        float M[12];
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = A.P[row * 12 + k];
        float e0 = FILL, e1 = -FILL, e2 = FILL, e3 = -FILL;
        int cnt = 0;
        for (int i = lane; i < A.n_pts; i += 64) {
            float u, t;
            if (sq_pixel(s_pts[3 * i], s_pts[3 * i + 1], s_pts[3 * i + 2], M, u, t)) {
                e0 = min_nan(e0, u);
                e1 = max_nan(e1, u);
                e2 = min_nan(e2, t);
                e3 = max_nan(e3, t);
                cnt++;
            }
        }
        e0 = wave_reduce(e0, min_nan<float>);
        e1 = wave_reduce(e1, max_nan<float>);
        e2 = wave_reduce(e2, min_nan<float>);
        e3 = wave_reduce(e3, max_nan<float>);
        cnt = wave_sum(cnt);
        if (lane < 4) {
            const float e = (lane == 0) ? e0 : (lane == 1) ? e1 : (lane == 2) ? e2 : e3;
            A.out_ext[row * 4 + lane] = store_ext(e);
        }
        if (lane == 0) A.out_nvalid[row] = cnt;
    }
}

struct DqArgs {
    const double* Q;
    const int* view_offsets;
    const double* P;
    int n_obj, max_views;
    double* out_ext;
    int* out_status;
};

__global__ __launch_bounds__(512) void reproject_dq_kernel(DqArgs A) {
    const int lane = threadIdx.x & 63;
    const int obj = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (obj >= A.n_obj) return;
    const int v0 = A.view_offsets[obj];
    const int F = A.view_offsets[obj + 1] - v0;
    if (F < 1 || F > A.max_views) return;
    double Q[16];
#pragma unroll
    for (int k = 0; k < 16; k++) Q[k] = A.Q[(size_t)obj * 16 + k];
    for (int v = lane; v < F; v += 64) {
        const size_t row = (size_t)(v0 + v);
        double M[12], ext[4];
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = A.P[row * 12 + k];
        const int st = dq_box(M, Q, ext);
#pragma unroll
        for (int d = 0; d < 4; d++) A.out_ext[row * 4 + d] = ext[d];
        A.out_status[row] = st;
    }
}

template <typename T>
struct ScoreArgs {
    const int* view_offsets;
    const T* ext;
    const int* bad;
    const T* boxes;
    const float* mask;
    T img_w, img_h;
    int n_obj, max_views;
    T* out_res;
    T* out_iou;
    T* out_obj;
    int* out_obj_i;
};

template <typename T>
__global__ __launch_bounds__(512) void reproject_score_kernel(ScoreArgs<T> A) {
    const int lane = threadIdx.x & 63;
    const int obj = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (obj >= A.n_obj) return;
    const int v0 = A.view_offsets[obj];
    const int F = A.view_offsets[obj + 1] - v0;
    const T qnan = (T)__builtin_nanf("");
    if (F < 1 || F > A.max_views) {      // wave-uniform: the row of an object without views
        if (lane < 4) A.out_obj[(size_t)obj * 4 + lane] = qnan;
        if (lane < 3) A.out_obj_i[(size_t)obj * 3 + lane] = (lane == 0) ? -1 : 0;
        return;
    }
    T s0 = 0, s1 = 0, s2 = 0, s3 = 0, si = 0;
    T mn = (T)HUGE_VALF;
    int mi = INT_MAX, ne = 0, nb = 0;
    for (int v = lane; v < F; v += 64) {
        const size_t row = (size_t)(v0 + v);
        const bool bad = A.bad ? (A.bad[row] != 0) : false;
        T e[4], b[4], r[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            e[d] = A.ext[row * 4 + d];
            b[d] = A.boxes[row * 4 + d];
            const float m = A.mask[row * 4 + d];
            r[d] = edge_residual(e[d], b[d], m);
            A.out_res[row * 4 + d] = r[d];
            ne += (m != 0.0f) ? 1 : 0;
        }
        s0 = s0 + r[0]; s1 = s1 + r[1]; s2 = s2 + r[2]; s3 = s3 + r[3];
        const T iou = box_iou(e, b, A.img_w, A.img_h, bad);
        A.out_iou[row] = iou;
        si = si + iou;
        if (iou < mn) { mn = iou; mi = v; }
        nb += bad ? 1 : 0;
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); si = wave_sum(si); ne = wave_sum(ne); nb = wave_sum(nb);
    wave_reduce_pair(mn, mi, [](T omn, int omi, T mn, int mi) { return omn < mn || (omn == mn && omi < mi); });
    const T Ff = (T)F;
    const T loss = ((s0 / Ff + s1 / Ff) + s2 / Ff) + s3 / Ff;
    const T mean_abs = (ne > 0) ? (((s0 + s1) + s2) + s3) / (T)ne : qnan;
    const T mean_iou = si / Ff;
    if (lane < 4) {
        const T o = (lane == 0) ? loss : (lane == 1) ? mean_abs : (lane == 2) ? mean_iou : mn;
        A.out_obj[(size_t)obj * 4 + lane] = o;
    }
    if (lane < 3) {
        const int o = (lane == 0) ? mi : (lane == 1) ? ne : nb;
        A.out_obj_i[(size_t)obj * 3 + lane] = o;
    }
}

bool views_in_limit(int max_views) { return max_views >= 1 && max_views <= 16 * ODAM_SQ_MAX_VIEWS; }

template <typename T>
int score(const char* name, odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const T* ext, const int* bad, const T* boxes,
          const float* mask, T img_w, T img_h, int max_views, T* out_res, T* out_iou, T* out_obj, int* out_obj_i, void* stream) {
    char msg[96];
    if (!ctx || !view_offsets || !ext || !boxes || !mask || !out_res || !out_iou || !out_obj || !out_obj_i) {
        std::snprintf(msg, sizeof(msg), "%s: null pointer", name);
        return odam_fail(ODAM_E_INVALID, msg);
    }
    if (n_obj < 0 || !(img_w > (T)0) || !(img_h > (T)0)) {
        std::snprintf(msg, sizeof(msg), "%s: bad size", name);
        return odam_fail(ODAM_E_INVALID, msg);
    }
    if (!views_in_limit(max_views)) {
        std::snprintf(msg, sizeof(msg), "%s: max_views outside 1..16 * ODAM_SQ_MAX_VIEWS", name);
        return odam_fail(ODAM_E_LIMIT, msg);
    }
    if (n_obj == 0) return ODAM_OK;
    ScoreArgs<T> A{};
    A.view_offsets = view_offsets; A.ext = ext; A.bad = bad; A.boxes = boxes; A.mask = mask; A.img_w = img_w; A.img_h = img_h;
    A.n_obj = n_obj; A.max_views = max_views; A.out_res = out_res; A.out_iou = out_iou; A.out_obj = out_obj; A.out_obj_i = out_obj_i;
    const int waves = odam_sq_ctx_dq(ctx)->group_waves;
    const dim3 grid((unsigned)((n_obj + waves - 1) / waves)), block((unsigned)(64 * waves));
    hipLaunchKernelGGL(reproject_score_kernel<T>, grid, block, 0, (hipStream_t)stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

}  // namespace

extern "C" int odam_sq_reproject_batch(odam_sq_ctx* ctx, int n_obj, const float* points, int n_pts, const int* view_offsets,
                                       const float* P, int max_views, float* out_ext, int* out_nvalid, void* stream) {
    if (!ctx || !points || !view_offsets || !P || !out_ext || !out_nvalid)
        return odam_fail(ODAM_E_INVALID, "odam_sq_reproject_batch: null pointer");
    if (n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_sq_reproject_batch: bad size");
    if (n_pts < 1 || n_pts > MAX_PTS) return odam_fail(ODAM_E_LIMIT, "odam_sq_reproject_batch: n_pts outside 1..4096");
    if (!views_in_limit(max_views))
        return odam_fail(ODAM_E_LIMIT, "odam_sq_reproject_batch: max_views outside 1..16 * ODAM_SQ_MAX_VIEWS");
    if (n_obj == 0) return ODAM_OK;
    SqArgs A{};
    A.points = points; A.view_offsets = view_offsets; A.P = P; A.n_pts = n_pts; A.max_views = max_views;
    A.out_ext = out_ext; A.out_nvalid = out_nvalid;
    const dim3 grid((unsigned)n_obj, (unsigned)((max_views + SLICE - 1) / SLICE)), block(64 * SQ_WAVES);
    hipLaunchKernelGGL(reproject_sq_kernel, grid, block, (size_t)n_pts * 3 * sizeof(float), (hipStream_t)stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_dq_reproject_batch(odam_sq_ctx* ctx, int n_obj, const double* Q, const int* view_offsets, const double* P,
                                       int max_views, double* out_ext, int* out_status, void* stream) {
    if (!ctx || !Q || !view_offsets || !P || !out_ext || !out_status)
        return odam_fail(ODAM_E_INVALID, "odam_dq_reproject_batch: null pointer");
    if (n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_dq_reproject_batch: bad size");
    if (!views_in_limit(max_views))
        return odam_fail(ODAM_E_LIMIT, "odam_dq_reproject_batch: max_views outside 1..16 * ODAM_SQ_MAX_VIEWS");
    if (n_obj == 0) return ODAM_OK;
    DqArgs A{};
    A.Q = Q; A.view_offsets = view_offsets; A.P = P; A.n_obj = n_obj; A.max_views = max_views; A.out_ext = out_ext;
    A.out_status = out_status;
    const int waves = odam_sq_ctx_dq(ctx)->group_waves;
    const dim3 grid((unsigned)((n_obj + waves - 1) / waves)), block((unsigned)(64 * waves));
    hipLaunchKernelGGL(reproject_dq_kernel, grid, block, 0, (hipStream_t)stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_reproject_score_f32(odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const float* ext, const int* bad,
                                        const float* boxes, const float* mask, float img_w, float img_h, int max_views,
                                        float* out_res, float* out_iou, float* out_obj, int* out_obj_i, void* stream) {
    return score<float>("odam_reproject_score_f32", ctx, n_obj, view_offsets, ext, bad, boxes, mask, img_w, img_h, max_views, out_res,
                        out_iou, out_obj, out_obj_i, stream);
}

extern "C" int odam_reproject_score_f64(odam_sq_ctx* ctx, int n_obj, const int* view_offsets, const double* ext, const int* bad,
                                        const double* boxes, const float* mask, double img_w, double img_h, int max_views,
                                        double* out_res, double* out_iou, double* out_obj, int* out_obj_i, void* stream) {
    return score<double>("odam_reproject_score_f64", ctx, n_obj, view_offsets, ext, bad, boxes, mask, img_w, img_h, max_views, out_res,
                         out_iou, out_obj, out_obj_i, stream);
}
