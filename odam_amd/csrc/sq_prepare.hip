// sq_prepare.hip -- the prelude of a fit pass on the device (include/odam_sq.h, odam_sq_prepare_batch): the views, constraint rows and
// initial shape of every track in one launch.  Restates, for sequences whose frame ids are all different (likojack/ODAM):
//   src/utils/tracking_gt_utils.py:145-211, 59-66   load_pred_object, averaging_T_wos
//   src/super_quadric/quadric_helper.py:69-109      bbox_to_lines
//   src/scripts/run_multi_view.py:44-62             the views with a constrained edge, get_3d_box of the detector's pose
//   src/super_quadric/sq_libs.py:353-371, 41-58     the initial parameters of both optimisers
//
// One workgroup per track, no device-wide barrier, no persistent loop.  Row i of the track becomes the 64-bit key
// (image index << 32 | i), or all ones when its frame id names no image (view_keys.h); the LDS sort of wave_ops.h, sized to the track's own
// power of two, puts the rows in image order with the lowest row of a frame id first, so a sorted entry is a view exactly when it is
// not all ones and its image differs from its left neighbour's.  A block scan of those flags gives every view its place, and the
// thread that owns a view writes its per-view outputs.
//
// Sums whose bits are part of the contract are taken by single lanes in the stated order (lanes 0..2 of wave 0: columns 9..11 over all
// rows in row order; lanes 3..5: columns 6..8 over the views in view order; the loads are issued eight ahead of the additions).  The
// sums of sin / cos that decide the yaw are a per-thread, per-wave (XOR butterfly), per-workgroup (wave order) reduction: fixed, so
// results repeat from launch to launch, but not the order of a host sum.  The class is a median over integers 0..63: a histogram.
// Compiled with -ffp-contract=off: every product and sum is rounded on its own.
//
// odam_sq_prepare_scenes is the same kernel instantiated with SCENES: the tracks of many scenes in one launch, every workgroup on its
// own scene's image tables and image size.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/odam_sq.h"
#include "odam_err.h"
#include "view_keys.h"
#include "wave_ops.h"

namespace {

constexpr int MAX_WAVES = 16;
constexpr int N_CLASS = 64;

struct PrepArgs {
    const int* row_off;
    const double* rows;
    const long long* img_ids;
    const int* img_order;
    const double* P_cws;
    int n_obj, n_img, cap, representation;      // cap: keys the launch's LDS holds
    double img_w, img_h, thr;
    // odam_sq_prepare_scenes only: the tracks of n_scene scenes, every scene with its own slice of the image tables and its own image size
    int n_scene;
    const int* trk_off;
    const int* img_off;
    const double* img_wh;
    const int* scene_rows;      // nullable: per scene, the max_rows a launch for that scene alone would have been given
    int *cls, *n_obs, *n_valid;
    float *init, *half_dims;
    double *pose, *bboxes_dl;
    int* status;
    int *view_img, *view_row;
    float *tgt, *mask, *P;
    int* valid;
};

// SCENES: the workgroup first finds the scene its track belongs to (trk_off, a wave-uniform binary search: blockIdx only) and takes that
// scene's slice of img_ids / img_order / P_cws and its image size; everything after that is the single-scene kernel on that slice, so
// every word is the word odam_sq_prepare_batch writes for the scene alone.  Without SCENES the slice is the whole table.
// The order of the sin / cos sums follows from how the sorted entries are dealt to the threads, and that from the size the launch was
// given (threads = cap / 2).  With scene_rows the workgroup deals them as the launch for its scene alone would -- to the first `own`
// threads, the others hold no entry and add zeros -- so the yaw too has that launch's bits, whatever size this launch has.
template <bool SCENES>
__global__ __launch_bounds__(1024) void sq_prepare_kernel(PrepArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    __shared__ int s_hist[N_CLASS];
    __shared__ int s_bad;
    __shared__ int s_wcnt[MAX_WAVES], s_wvalid[MAX_WAVES];
    __shared__ double s_wsin[MAX_WAVES], s_wcos[MAX_WAVES];
    __shared__ double s_mean[6];      // translation[3], scales[3]
    __shared__ double s_yaw;

    const int obj = blockIdx.x;
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = T >> 6;
    int i0 = 0, n_img = A.n_img;      // the scene's slice of the image tables
    double img_w = A.img_w, img_h = A.img_h;
    int cap = A.cap, own = T;         // rows a track may have; threads that are dealt sorted entries
    if constexpr (SCENES) {
        int lo = 0, hi = A.n_scene;      // first scene whose tracks end behind obj (an empty scene never is)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (A.trk_off[mid + 1] <= obj) lo = mid + 1; else hi = mid;
        }
        i0 = 0; n_img = 0;               // a track no scene owns, or a slice outside the tables: no image, so no view
        if (lo < A.n_scene) {
            const int a = A.img_off[lo], b = A.img_off[lo + 1];
            if (a >= 0 && b >= a && b <= A.n_img) { i0 = a; n_img = b - a; }
            img_w = A.img_wh[2 * lo]; img_h = A.img_wh[2 * lo + 1];
            if (A.scene_rows) {      // the launch shape of odam_sq_prepare_batch(max_rows = scene_rows[lo]), never beyond this launch's
                const int m = A.scene_rows[lo];
                int c = 1;
                while (c < m && c < cap) c <<= 1;
                cap = c;
                own = c / 2;
                own = own < 64 ? 64 : (own > T ? T : own);
            }
        }
    }
    const long long* img_ids = A.img_ids + i0;
    const int* img_order = A.img_order + i0;
    const double* P_cws = A.P_cws + (size_t)i0 * 12;
    const int r0 = A.row_off[obj];
    const int n = A.row_off[obj + 1] - r0;
    // both refusals are workgroup-uniform and come before any row is read
    if (n > cap || n <= 0) {
        if (tid == 0) {
            A.cls[obj] = -1;
            A.n_obs[obj] = 0;
            A.n_valid[obj] = 0;
            A.status[obj] = n > cap ? ODAM_SQ_PREPARE_TOO_MANY_ROWS : ODAM_SQ_PREPARE_NO_VIEW;
        }
        return;
    }
    int n2 = 1;
    while (n2 < n) n2 <<= 1;      // <= cap: cap is a power of two
    const double* rows = A.rows + (size_t)r0 * 14;

    if (tid < N_CLASS) s_hist[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();

    // keys and the class histogram
    for (int i = tid; i < n2; i += T) {
        unsigned long long key = VIEW_NONE;
        if (i < n) {
            const double f = rows[(size_t)i * 14 + 0];
            if (f > -2147483649.0 && f < 2147483648.0) {      // truncates into int32 (NaN fails both)
                const long long id = (long long)(int)f;
                int lo = 0, hi = n_img;                        // first entry >= id
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (img_ids[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (lo < n_img && img_ids[lo] == id) {
                    const int img = img_order[lo];
                    if (img >= 0 && img < n_img) key = view_key(img, i);
                }
            }
            const double c = rows[(size_t)i * 14 + 1];
            if (c >= 0.0 && c <= (double)(N_CLASS - 1) && c == floor(c)) atomicAdd(&s_hist[(int)c], 1);
            else atomicOr(&s_bad, 1);
        }
        keys[i] = key;
    }
    __syncthreads();

    lds_bitonic_sort(keys, n2, tid, T);

    // every thread owns a run of L sorted entries; views in front of it = where its own views go
    const int L = n2 > own ? n2 / own : 1;      // (threads from `own` on start at or behind n2: they own nothing)
    const int j0 = tid * L;
    const int j1 = j0 < n ? (j0 + L < n ? j0 + L : n) : j0;      // entries past n are all ones
    int cnt = 0;
    for (int j = j0; j < j1; j++) cnt += first_of_image(keys, j) ? 1 : 0;
    // (wg_exclusive_scan of wave_ops.h, written out: called as a function it makes the compiler put the additions of the ordered sums
    //  below under exec masks instead of selects, 16 x 8192 rows then take 2.79 ms instead of 2.65: profiles/wave_ops_timing.txt)
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) s_wcnt[wave] = incl;
    __syncthreads();
    int base = incl - cnt, n_obs = 0;
    for (int w = 0; w < n_waves; w++) {
        if (w < wave) base += s_wcnt[w];
        n_obs += s_wcnt[w];
    }

    // per-view outputs
    const double lim[4] = {img_w, img_w, img_h, img_h};
    const int col[4] = {2, 4, 3, 5};      // x_min, x_max, y_min, y_max
    int my_valid = 0;
    double my_sin = 0.0, my_cos = 0.0;
    int p = base;
    for (int j = j0; j < j1; j++) {
        if (!first_of_image(keys, j)) continue;
        const unsigned long long key = keys[j];
        const int img = view_image(key), i = view_index(key);
        const size_t g = (size_t)r0 + (size_t)p;
        const double* row = rows + (size_t)i * 14;
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double v = row[col[e]];
            const bool m = v > A.thr && v < lim[e] - A.thr;
            A.mask[g * 4 + e] = m ? 1.0f : 0.0f;
            A.tgt[g * 4 + e] = m ? (float)v : 0.0f;
            any = any || m;
        }
#pragma unroll
        for (int k = 0; k < 12; k++) A.P[g * 12 + k] = (float)P_cws[(size_t)img * 12 + k];
        A.view_img[g] = img;
        A.view_row[g] = i;
        A.valid[g] = any ? 1 : 0;
        my_valid += any ? 1 : 0;
        const double a = row[12];
        my_sin = my_sin + sin(a);
        my_cos = my_cos + cos(a);
        p++;
    }
    const int wv = wave_sum(my_valid);
    const double ws = wave_sum(my_sin), wc = wave_sum(my_cos);
    if (lane == 0) { s_wvalid[wave] = wv; s_wsin[wave] = ws; s_wcos[wave] = wc; }

    // the sums in stated order: wave 0, lanes 0..2 all rows (columns 9..11), lanes 3..5 the views (columns 6..8)
    if (wave == 0) {
        const bool all_rows = lane < 3;
        const int c = all_rows ? 9 + lane : 3 + lane;
        double s = 0.0;
        bool have = false;
        if (lane < 6) {
            for (int jb = 0; jb < n; jb += 8) {
                double v[8];
                bool use[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int j = jb + k;
                    use[k] = false;
                    v[k] = 0.0;
                    if (j < n) {
                        int i = j;
                        if (all_rows) use[k] = true;
                        else if (first_of_image(keys, j)) { use[k] = true; i = view_index(keys[j]); }
                        if (use[k]) v[k] = rows[(size_t)i * 14 + c];
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (use[k]) { s = have ? s + v[k] : v[k]; have = true; }      // a sum starts with its first term, as np.add.reduce
            }
            if (all_rows) {
                const double t_wo = s / (double)n;
                if (n_obs > 0) {      // the mean of n_obs equal vectors, added one after the other
                    double acc = t_wo;
                    for (int k = 1; k < n_obs; k++) acc = acc + t_wo;
                    s_mean[lane] = acc / (double)n_obs;
                }
            } else if (n_obs > 0) {
                s_mean[lane] = s / (double)n_obs;
            }
        }
    }
    __syncthreads();

    if (tid == 0) {
        // class: median over the histogram
        int cls = -1;
        if (!s_bad) {
            const int ra = (n - 1) >> 1, rb = n >> 1;      // ranks of the two middle values (equal for an odd count)
            int seen = 0, va = -1, vb = -1;
            for (int c = 0; c < N_CLASS; c++) {
                seen += s_hist[c];
                if (va < 0 && seen > ra) va = c;
                if (vb < 0 && seen > rb) vb = c;
            }
            cls = (va + vb) >> 1;      // int((a + b) / 2) of non-negative integers
        }
        int nv = 0;
        double S = 0.0, C = 0.0;
        for (int w = 0; w < n_waves; w++) { nv += s_wvalid[w]; S = S + s_wsin[w]; C = C + s_wcos[w]; }
        A.cls[obj] = cls;
        A.n_obs[obj] = n_obs;
        A.n_valid[obj] = nv;
        A.status[obj] = n_obs == 0 ? ODAM_SQ_PREPARE_NO_VIEW : (s_bad ? ODAM_SQ_PREPARE_BAD_CLASS : 0);
        if (n_obs > 0) {
            const double yaw = atan2(S, C);
            s_yaw = yaw;
            double* pose = A.pose + (size_t)obj * 7;
            pose[0] = s_mean[0]; pose[1] = s_mean[1]; pose[2] = s_mean[2];
            pose[3] = yaw;
            pose[4] = s_mean[3]; pose[5] = s_mean[4]; pose[6] = s_mean[5];
            if (A.representation == ODAM_SQ_DUAL_QUADRIC) {
                float* o = A.init + (size_t)obj * 5;
                o[0] = (float)s_mean[0]; o[1] = (float)s_mean[1]; o[2] = (float)s_mean[2];
                o[3] = (float)yaw;
                o[4] = 1.0f;
                float* h = A.half_dims + (size_t)obj * 3;
                h[0] = (float)(s_mean[3] / 2.0); h[1] = (float)(s_mean[4] / 2.0); h[2] = (float)(s_mean[5] / 2.0);
            } else {
                float* o = A.init + (size_t)obj * 9;
                o[0] = (float)s_mean[0]; o[1] = (float)s_mean[1]; o[2] = (float)s_mean[2];
                o[3] = (float)yaw;
                o[4] = (float)sqrt(s_mean[3] / 2.0); o[5] = (float)sqrt(s_mean[4] / 2.0); o[6] = (float)sqrt(s_mean[5] / 2.0);
                const float shape = A.representation == ODAM_SQ_CUBE ? -10000.0f : -0.0f;
                o[7] = shape; o[8] = shape;
            }
        }
    }
    __syncthreads();

    // get_3d_box: corner k from thread k
    if (tid < 8 && n_obs > 0) {
        const double yaw = s_yaw;
        const double c = cos(yaw), s = sin(yaw);
        const double hl = s_mean[3] / 2.0, hw = s_mean[4] / 2.0, hh = s_mean[5] / 2.0;
        const int k = tid;
        const double x = (k & 2) ? -hl : hl;                       // l/2, l/2, -l/2, -l/2, ...
        const double y = (((k + 1) & 2) ? -hw : hw);               // w/2, -w/2, -w/2, w/2, ...
        const double z = (k & 4) ? -hh : hh;
        double* o = A.bboxes_dl + ((size_t)obj * 8 + k) * 3;
        o[0] = ((c * x + (-s) * y) + 0.0 * z) + s_mean[0];
        o[1] = ((s * x + c * y) + 0.0 * z) + s_mean[1];
        o[2] = ((0.0 * x + 0.0 * y) + 1.0 * z) + s_mean[2];
    }
}

// sizes the workgroup and its LDS from max_rows and launches one workgroup per track
template <bool SCENES>
int launch_prepare(PrepArgs& A, int max_rows, hipStream_t stream) {
    int cap = 1;
    while (cap < max_rows && cap < ODAM_SQ_PREPARE_MAX_ROWS) cap <<= 1;
    int threads = cap / 2;
    threads = threads < 64 ? 64 : (threads > 1024 ? 1024 : threads);
    const size_t lds = sizeof(unsigned long long) * (size_t)cap;
    if (lds > 48 * 1024)
        ODAM_HIP(hipFuncSetAttribute((const void*)sq_prepare_kernel<SCENES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    A.cap = cap;
    hipLaunchKernelGGL(sq_prepare_kernel<SCENES>, dim3((unsigned)A.n_obj), dim3((unsigned)threads), lds, stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

}  // namespace

extern "C" int odam_sq_prepare_batch(odam_sq_ctx* ctx, int n_obj, const int* row_off, const double* rows, int max_rows, int n_img,
                                     const long long* img_ids, const int* img_order, const double* P_cws, double img_w, double img_h,
                                     double thr, int representation, int* cls, int* n_obs, int* n_valid, float* init, float* half_dims,
                                     double* pose, double* bboxes_dl, int* status, int* view_img, int* view_row, float* tgt, float* mask,
                                     float* P, int* valid, void* stream) {
    if (!ctx || !row_off || !rows || !img_ids || !img_order || !P_cws || !cls || !n_obs || !n_valid || !init || !pose || !bboxes_dl ||
        !status || !view_img || !view_row || !tgt || !mask || !P || !valid)
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_batch: null pointer");
    if (representation < 0 || representation > ODAM_SQ_DUAL_QUADRIC)
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_batch: representation outside 0..3");
    if (representation == ODAM_SQ_DUAL_QUADRIC && !half_dims)
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_batch: half_dims is null for the dual quadric");
    if (n_obj < 0 || n_img < 0 || max_rows < 1) return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_batch: bad size");
    if (n_obj == 0) return ODAM_OK;
    PrepArgs A{};
    A.row_off = row_off; A.rows = rows; A.img_ids = img_ids; A.img_order = img_order; A.P_cws = P_cws;
    A.n_obj = n_obj; A.n_img = n_img; A.representation = representation;
    A.img_w = img_w; A.img_h = img_h; A.thr = thr;
    A.cls = cls; A.n_obs = n_obs; A.n_valid = n_valid; A.init = init; A.half_dims = half_dims; A.pose = pose; A.bboxes_dl = bboxes_dl;
    A.status = status; A.view_img = view_img; A.view_row = view_row; A.tgt = tgt; A.mask = mask; A.P = P; A.valid = valid;
    return launch_prepare<false>(A, max_rows, (hipStream_t)stream);
}

extern "C" int odam_sq_prepare_scenes(odam_sq_ctx* ctx, int n_obj, const int* row_off, const double* rows, int max_rows, int n_scene,
                                      const int* trk_off, const int* img_off, int n_img, const long long* img_ids, const int* img_order,
                                      const double* P_cws, const double* img_wh, const int* scene_rows, double thr, int representation, int* cls, int* n_obs,
                                      int* n_valid, float* init, float* half_dims, double* pose, double* bboxes_dl, int* status,
                                      int* view_img, int* view_row, float* tgt, float* mask, float* P, int* valid, void* stream) {
    if (!ctx || !row_off || !rows || !trk_off || !img_off || !img_ids || !img_order || !P_cws || !img_wh || !cls || !n_obs || !n_valid ||
        !init || !pose || !bboxes_dl || !status || !view_img || !view_row || !tgt || !mask || !P || !valid)
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_scenes: null pointer");
    if (representation < 0 || representation > ODAM_SQ_DUAL_QUADRIC)
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_scenes: representation outside 0..3");
    if (representation == ODAM_SQ_DUAL_QUADRIC && !half_dims)
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_scenes: half_dims is null for the dual quadric");
    if (n_obj < 0 || n_scene < 0 || n_img < 0 || max_rows < 1 || (n_obj > 0 && n_scene < 1))
        return odam_fail(ODAM_E_INVALID, "odam_sq_prepare_scenes: bad size");
    if (n_obj == 0) return ODAM_OK;
    PrepArgs A{};
    A.row_off = row_off; A.rows = rows; A.img_ids = img_ids; A.img_order = img_order; A.P_cws = P_cws;
    A.n_obj = n_obj; A.n_img = n_img; A.representation = representation;
    A.thr = thr;
    A.n_scene = n_scene; A.trk_off = trk_off; A.img_off = img_off; A.img_wh = img_wh; A.scene_rows = scene_rows;
    A.cls = cls; A.n_obs = n_obs; A.n_valid = n_valid; A.init = init; A.half_dims = half_dims; A.pose = pose; A.bboxes_dl = bboxes_dl;
    A.status = status; A.view_img = view_img; A.view_row = view_row; A.tgt = tgt; A.mask = mask; A.P = P; A.valid = valid;
    return launch_prepare<true>(A, max_rows, (hipStream_t)stream);
}
