// box_iou.hip -- evaluation of a finished map: oriented-box 3D IoU of every pair of a scene and the reference's greedy matching
// of predictions to ground truth (likojack/ODAM src/scripts/eval_scan2cad.py:249-267 match_sequence over src/utils/box_utils.py:98-120
// box3d_iou), all scenes in one launch each.  Arithmetic in box_iou_core.h; restated in numpy by tests/box_iou_ref.py.
//
//   box3d_iou_kernel    one lane per pair, binary64.  The pairs of all scenes are one row-major array ([n_s][m_s] blocks at pair_off[s]);
//                       lane p finds its scene by bisection of pair_off and its (a, b) by one division, so the 64 lanes of a wavefront
//                       write 64 consecutive words and, within a row, share `a` and walk `b`.  Every lane does the same 32 edge / plane
//                       tests with selects; the only branch is the gate (a gated-off pair is stored as 0 without the arithmetic).
//   box3d_match_kernel  one wavefront per scene.  Predictions are taken in their given order (the reference's loop is sequential); for
//                       each, the lanes stride over the scene's ground-truth boxes.  Lane l owns the boxes l, l + 64, ... and keeps
//                       their "used" flags as 64 bits in a register -- hence at most 4096 boxes per scene.  There is no `break` in the
//                       reference: a prediction claims EVERY free box of its class above the threshold, and each claim is a true
//                       positive.  Class counts are integer LDS adds (order-free).
//
// Neither kernel writes a word that no pair, box or scene owns.  A scene whose offsets are inconsistent with what the caller
// promised (n_pairs, max_gt) is not trusted: the IoU kernel skips the words outside n_s x m_s, the match kernel writes that scene's
// count row as -1 and nothing else.
#include <hip/hip_runtime.h>

#include "../../include/odam_eval.h"
#include "box_iou_core.h"
#include "odam_err.h"
#include "wave_ops.h"

namespace {

using namespace odam_biou;

constexpr int IOU_BLOCK = 256;
constexpr int MAX_CLASS = 64;
constexpr int MAX_GT = 4096;      // 64 lanes x 64 flag bits

struct IouArgs {
    const int* a_off;
    const int* b_off;
    const long long* pair_off;
    const double* A;
    const double* B;
    const int* cls_a;
    const int* cls_b;
    long long n_pairs;
    int n_scene, gate;
    double* out_iou3d;
    double* out_bev;
};

__global__ __launch_bounds__(IOU_BLOCK) void box3d_iou_kernel(IouArgs K) {
    const long long p = (long long)blockIdx.x * IOU_BLOCK + threadIdx.x;
    if (p >= K.n_pairs) return;
    int lo = 0, hi = K.n_scene;      // the last scene whose block starts at or before p (empty scenes before it start there too)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (K.pair_off[mid] <= p) lo = mid; else hi = mid;
    }
    const long long local = p - K.pair_off[lo];
    const int a0 = K.a_off[lo], n = K.a_off[lo + 1] - a0;
    const int b0 = K.b_off[lo], m = K.b_off[lo + 1] - b0;
    if (local < 0 || p >= K.pair_off[lo + 1] || n <= 0 || m <= 0 || local >= (long long)n * m) return;
    const size_t ia = (size_t)a0 + (size_t)(local / m), ib = (size_t)b0 + (size_t)(local % m);
    double iou = 0.0, bev = 0.0;
    if (gate_open(K.gate, K.gate ? K.cls_a[ia] : 0, K.gate ? K.cls_b[ib] : 0)) {
        double c1[24], c2[24];
#pragma unroll
        for (int k = 0; k < 24; k++) {
            c1[k] = K.A[ia * 24 + k];
            c2[k] = K.B[ib * 24 + k];
        }
        iou = box3d_iou(c1, c2, bev);
    }
    K.out_iou3d[p] = iou;
    if (K.out_bev) K.out_bev[p] = bev;
}

struct MatchArgs {
    const int* a_off;
    const int* b_off;
    const long long* pair_off;
    const double* iou;
    const int* cls_pred;
    const int* cls_gt;
    double threshold;
    int n_class, max_gt;
    int* out_counts;
    int* out_claimed;
    int* out_gt_match;
};

__global__ __launch_bounds__(64) void box3d_match_kernel(MatchArgs M) {
    __shared__ int s_cnt[3 * MAX_CLASS];      // gts, preds, tps per class
    const int s = blockIdx.x, lane = threadIdx.x;
    const int a0 = M.a_off[s], n = M.a_off[s + 1] - a0;
    const int b0 = M.b_off[s], m = M.b_off[s + 1] - b0;
    int* cnt = M.out_counts + (size_t)s * 3 * M.n_class;
    if (n < 0 || m < 0 || m > M.max_gt) {      // block-uniform, before the barriers: not what the caller promised
        for (int k = lane; k < 3 * M.n_class; k += 64) cnt[k] = -1;
        return;
    }
    for (int k = lane; k < 3 * MAX_CLASS; k += 64) s_cnt[k] = 0;
    __syncthreads();
    for (int i = lane; i < m; i += 64) {
        const int c = M.cls_gt[b0 + i];
        if ((unsigned)c < (unsigned)M.n_class) atomicAdd(&s_cnt[c], 1);
        M.out_gt_match[b0 + i] = -1;
    }
    for (int p = lane; p < n; p += 64) {
        const int c = M.cls_pred[a0 + p];
        if ((unsigned)c < (unsigned)M.n_class) atomicAdd(&s_cnt[MAX_CLASS + c], 1);
    }
    __syncthreads();
    const double* iou = M.iou + M.pair_off[s];
    unsigned long long used = 0;      // bit k: ground-truth box lane + 64 k is taken
    for (int p = 0; p < n; p++) {
        const int cp = M.cls_pred[a0 + p];      // wave-uniform
        const bool valid = (unsigned)cp < (unsigned)M.n_class;
        int mine = 0;
        if (valid) {
            int k = 0;
            for (int i = lane; i < m; i += 64, k++) {
                const bool hit = (M.cls_gt[b0 + i] == cp) && (iou[(size_t)p * m + i] > M.threshold) && !((used >> k) & 1ull);
                if (hit) {
                    used |= 1ull << k;
                    M.out_gt_match[b0 + i] = p;
                    mine++;
                }
            }
        }
        mine = wave_sum(mine);
        if (lane == 0) {
            M.out_claimed[a0 + p] = mine;
            if (valid) s_cnt[2 * MAX_CLASS + cp] += mine;
        }
    }
    __syncthreads();
    for (int k = lane; k < 3 * M.n_class; k += 64) cnt[k] = s_cnt[(k / M.n_class) * MAX_CLASS + k % M.n_class];
}

}  // namespace

extern "C" int odam_box3d_iou_batch(odam_sq_ctx* ctx, int n_scene, const int* a_off, const int* b_off, const long long* pair_off,
                                    long long n_pairs, const double* A, const double* B, const int* cls_a, const int* cls_b, int gate,
                                    double* out_iou3d, double* out_bev, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_box3d_iou_batch: null context");
    if (n_scene < 0 || n_pairs < 0) return odam_fail(ODAM_E_INVALID, "odam_box3d_iou_batch: bad size");
    if (gate < 0 || gate > 2) return odam_fail(ODAM_E_INVALID, "odam_box3d_iou_batch: gate outside 0..2");
    if (gate != 0 && (!cls_a || !cls_b)) return odam_fail(ODAM_E_INVALID, "odam_box3d_iou_batch: gate != 0 needs cls_a and cls_b");
    if (n_scene == 0 || n_pairs == 0) return ODAM_OK;
    if (!a_off || !b_off || !pair_off || !A || !B || !out_iou3d) return odam_fail(ODAM_E_INVALID, "odam_box3d_iou_batch: null pointer");
    const long long blocks = (n_pairs + IOU_BLOCK - 1) / IOU_BLOCK;
    if (blocks > 0x7fffffffLL) return odam_fail(ODAM_E_LIMIT, "odam_box3d_iou_batch: more than 2^31 workgroups of pairs");
    IouArgs K{};
    K.a_off = a_off; K.b_off = b_off; K.pair_off = pair_off; K.A = A; K.B = B; K.cls_a = cls_a; K.cls_b = cls_b; K.n_pairs = n_pairs;
    K.n_scene = n_scene; K.gate = gate; K.out_iou3d = out_iou3d; K.out_bev = out_bev;
    hipLaunchKernelGGL(box3d_iou_kernel, dim3((unsigned)blocks), dim3(IOU_BLOCK), 0, (hipStream_t)stream, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_box3d_match_batch(odam_sq_ctx* ctx, int n_scene, const int* a_off, const int* b_off, const long long* pair_off,
                                      const double* iou3d, const int* cls_pred, const int* cls_gt, double threshold, int n_class,
                                      int max_gt, int* out_counts, int* out_claimed, int* out_gt_match, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_box3d_match_batch: null context");
    if (n_scene < 0 || max_gt < 0) return odam_fail(ODAM_E_INVALID, "odam_box3d_match_batch: bad size");
    if (n_class < 1 || n_class > MAX_CLASS) return odam_fail(ODAM_E_INVALID, "odam_box3d_match_batch: n_class outside 1..64");
    if (max_gt > MAX_GT) return odam_fail(ODAM_E_LIMIT, "odam_box3d_match_batch: more than 4096 ground-truth boxes in a scene");
    if (n_scene == 0) return ODAM_OK;
    if (!a_off || !b_off || !pair_off || !iou3d || !cls_pred || !cls_gt || !out_counts || !out_claimed || !out_gt_match)
        return odam_fail(ODAM_E_INVALID, "odam_box3d_match_batch: null pointer");
    MatchArgs M{};
    M.a_off = a_off; M.b_off = b_off; M.pair_off = pair_off; M.iou = iou3d; M.cls_pred = cls_pred; M.cls_gt = cls_gt;
    M.threshold = threshold; M.n_class = n_class; M.max_gt = max_gt; M.out_counts = out_counts; M.out_claimed = out_claimed;
    M.out_gt_match = out_gt_match;
    hipLaunchKernelGGL(box3d_match_kernel, dim3((unsigned)n_scene), dim3(64), 0, (hipStream_t)stream, M);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
