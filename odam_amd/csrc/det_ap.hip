// det_ap.hip -- average precision of score-ranked predictions against ground truth, all classes and all images at once: the
// reference's eval_det_cls / voc_ap (likojack/ODAM src/utils/eval_utils.py:43-176) without its three nested Python loops.
// Arithmetic in det_ap_core.h; restated in numpy by tests/det_ap_ref.py.  An "image" is a scene (a finished map against its
// ground truth) or a frame (one detector run against another).
//
// odam_det_ap is SIX launches, whatever the sizes; each kernel runs to completion on its own and they meet only in memory:
//   ap_overlap_kernel  one lane per prediction slot and per ground-truth slot.  A lane finds its image (bisection of the offsets, or
//                      slot / 30 for detection rows), decides the class it counts under (-1: none) and, for a prediction, walks the
//                      ground truth of its image: ovmax / jmax by `iou > ovmax`, the first of equal maxima wins, a NaN never.  The
//                      prediction's box stays in registers; every test is a select.  Fills the claim words with their sentinel.
//   ap_count_kernel    one workgroup: predictions and ground-truth boxes per class (integer LDS adds, order-free), class offsets.
//   ap_rank_kernel     one lane per prediction; scores and classes of all predictions pass through LDS in tiles of 256.
//                      rank = number of predictions of the class that rank before it (det_ap_core.h::ranks_before, a strict total
//                      order): exact, no order dependence, O(n^2) -- hence RANK_CAP.  A sort would lift the cap with far more code;
//                      at the cap the counting takes well under the time of one host-side evaluation.
//   ap_claim_kernel    one lane per prediction above the threshold: integer atomicMin of its rank on its box's claim word.  The
//                      minimum does not depend on the order of the atomics.
//   ap_flag_kernel     a prediction is a true positive when the claim word of its box holds its own rank; a box names the prediction
//                      of that rank.
//   ap_curve_kernel    one workgroup per class, chunks of 256 in rank order with a carry: integer inclusive scans of tp / fp,
//                      rec / prec and each chunk's largest prec; then the 11-point maxima or the reverse running maximum of prec
//                      (a suffix maximum inside the chunk, against the largest prec of the later chunks) and the sum of
//                      (rec[r] - rec[r-1]) * envelope[r], one term after the other in rank order.
//
// No kernel writes a word that no prediction, box, class or image owns; scratch is written inside [0, 2 n_pred + 2 n_gt) only.
// Offsets and counts on the device that contradict the sizes of the call are not trusted: the predictions and boxes of such an
// image count under no class (include/odam_eval.h says what is written for them).  Every index is checked against the sizes.
#include <hip/hip_runtime.h>

#include "../../include/odam_eval.h"
#include "det_ap_core.h"
#include "odam_err.h"
#include "wave_ops.h"

namespace {

using namespace odam_ap;

constexpr int BLOCK = 256;          // lanes per workgroup, and the chunk of the rank tiles and of the curve scans
constexpr int MAX_CLASS = 64;
constexpr int RANK_CAP = 32768;     // prediction slots per call (ODAM_AP_MAX_PRED)
constexpr int FREE = 0x7fffffff;    // claim word of a box no prediction reached
constexpr int NO_CLASS = -1;        // an owned prediction / box that counts nowhere
constexpr int NOT_OWNED = -2;       // a slot past its frame's count: nothing is written for it

static_assert(RANK_CAP == ODAM_AP_MAX_PRED && ROW_SLOTS == ODAM_AP_ROW_SLOTS, "include/odam_eval.h");

struct ApArgs {
    int kind, n_image, n_pred, n_gt, n_class, use_07;
    const int* pred_off;
    const int* gt_off;
    const void* pred_box;
    const void* gt_box;
    const int* cls_pred;
    const int* cls_gt;
    const double* score;
    const long long* pair_off;
    const double* iou;
    long long n_pairs;
    double ovthresh;
    int* s_pcls;       // scratch [n_pred]  class a prediction counts under, NO_CLASS or NOT_OWNED
    int* s_jglob;      // scratch [n_pred]  index of its best box among all ground truth, or -1
    int* s_gcls;       // scratch [n_gt]
    int* s_claim;      // scratch [n_gt]    smallest rank of a prediction that reaches the box, or FREE
    double* ovmax;
    int* jmax;
    int* rank;
    int* is_tp;
    int* gt_claim;
    int* order;
    int* npos;
    int* npred;
    int* cls_off;
    double* ap;
    int* tp;
    int* fp;
    double* rec;
    double* prec;
};

// the class word of a detection row: a whole number 0 .. 63, else none (a NaN, a negative or a huge word is never converted)
__device__ __forceinline__ int row_class(float v) { return (v >= 0.0f && v < (float)MAX_CLASS) ? (int)v : NO_CLASS; }

// image of slot `idx` of one side (predictions or ground truth), -1 when no trusted image owns it.  Offsets: the last image whose
// range starts at or before idx, and the range must hold idx and lie inside [0, n_total].  Rows: frame idx / 30, slot below its count.
__device__ __forceinline__ int image_of(const ApArgs& K, const int* off, int idx, int n_total) {
    if (K.n_image <= 0) return -1;
    if (K.kind >= 2) {
        const int img = idx / ROW_SLOTS, cnt = off[img];
        return (cnt >= 0 && cnt <= ROW_SLOTS && idx - img * ROW_SLOTS < cnt) ? img : -1;
    }
    const int lo = last_le(off, K.n_image, idx);
    const int a = off[lo], b = off[lo + 1];
    return (a >= 0 && a <= idx && idx < b && b <= n_total) ? lo : -1;
}

__global__ __launch_bounds__(BLOCK) void ap_overlap_kernel(ApArgs K) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < K.n_gt) {      // ---- a ground-truth slot
        const int img = image_of(K, K.gt_off, t, K.n_gt);
        int c = NOT_OWNED;
        if (img >= 0) {
            c = (K.kind >= 2) ? row_class(((const float*)K.gt_box)[(size_t)t * ROW_WORDS + 1]) : K.cls_gt[t];
            if ((unsigned)c >= (unsigned)K.n_class) c = NO_CLASS;
        } else if (K.kind < 2) {
            c = NO_CLASS;      // offsets: every one of the n_gt boxes is the caller's, whatever the offsets say
        }
        K.s_gcls[t] = c;
        K.s_claim[t] = FREE;
    }
    if (t >= K.n_pred) return;
    // ---- a prediction slot
    const int img = image_of(K, K.pred_off, t, K.n_pred);
    int c = (K.kind < 2) ? NO_CLASS : NOT_OWNED;
    int g0 = 0, m = 0;
    long long p0 = 0;
    if (img >= 0) {
        c = (K.kind >= 2) ? row_class(((const float*)K.pred_box)[(size_t)t * ROW_WORDS + 1]) : K.cls_pred[t];
        if ((unsigned)c >= (unsigned)K.n_class) c = NO_CLASS;
        bool ok;
        if (K.kind >= 2) {
            g0 = img * ROW_SLOTS; m = K.gt_off[img];
            ok = m >= 0 && m <= ROW_SLOTS;
        } else {
            g0 = K.gt_off[img]; m = K.gt_off[img + 1] - g0;
            ok = g0 >= 0 && m >= 0 && m <= K.n_gt - g0;
            if (ok && K.kind == 1) {      // its row of the image's [n][m] pair block must lie inside [0, n_pairs)
                const long long n = (long long)K.pred_off[img + 1] - K.pred_off[img];
                p0 = K.pair_off[img];
                ok = p0 >= 0 && p0 <= K.n_pairs && n * m <= K.n_pairs - p0;
                p0 += (long long)(t - K.pred_off[img]) * m;
            }
        }
        if (!ok) c = NO_CLASS;
    }
    K.s_pcls[t] = c;
    int jm = -1;
    if (c >= 0) {
        double ov = -__builtin_inf();
        double alo[3], ahi[3];
        const float* prow = (const float*)K.pred_box + (size_t)t * ROW_WORDS;
        if (K.kind == 0) {
            double cn[24];
#pragma unroll
            for (int k = 0; k < 24; k++) cn[k] = ((const double*)K.pred_box)[(size_t)t * 24 + k];
            aabb_of_corners(cn, alo, ahi);
        } else if (K.kind == 2) {
            aabb_of_row(prow, alo, ahi);
        }
        for (int j = 0; j < m; j++) {
            const size_t g = (size_t)g0 + j;
            const int cg = (K.kind >= 2) ? row_class(((const float*)K.gt_box)[g * ROW_WORDS + 1]) : K.cls_gt[g];
            if (cg != c) continue;
            double iou;
            if (K.kind == 0) {
                double cn[24], blo[3], bhi[3];
#pragma unroll
                for (int k = 0; k < 24; k++) cn[k] = ((const double*)K.gt_box)[g * 24 + k];
                aabb_of_corners(cn, blo, bhi);
                iou = iou_3d(alo, ahi, blo, bhi);
            } else if (K.kind == 1) {
                iou = K.iou[p0 + j];
            } else if (K.kind == 2) {
                double blo[3], bhi[3];
                aabb_of_row((const float*)K.gt_box + g * ROW_WORDS, blo, bhi);
                iou = iou_3d(alo, ahi, blo, bhi);
            } else {
                iou = iou_2d_rows(prow, (const float*)K.gt_box + g * ROW_WORDS);
            }
            if (iou > ov) { ov = iou; jm = j; }
        }
        K.ovmax[t] = ov;
        K.jmax[t] = jm;
    } else if (c == NO_CLASS) {
        K.ovmax[t] = __builtin_nan("");
        K.jmax[t] = -1;
    }
    K.s_jglob[t] = (jm >= 0) ? g0 + jm : -1;
}

__global__ __launch_bounds__(BLOCK) void ap_count_kernel(ApArgs K) {
    __shared__ int s_n[2 * MAX_CLASS];      // predictions, ground truth per class
    const int tid = threadIdx.x;
    for (int k = tid; k < 2 * MAX_CLASS; k += BLOCK) s_n[k] = 0;
    __syncthreads();
    for (int d = tid; d < K.n_pred; d += BLOCK) {
        const int c = K.s_pcls[d];
        if (c >= 0) atomicAdd(&s_n[c], 1);
    }
    for (int g = tid; g < K.n_gt; g += BLOCK) {
        const int c = K.s_gcls[g];
        if (c >= 0) atomicAdd(&s_n[MAX_CLASS + c], 1);
    }
    __syncthreads();
    if (tid < K.n_class) {
        K.npred[tid] = s_n[tid];
        K.npos[tid] = s_n[MAX_CLASS + tid];
    }
    if (tid == 0) {
        int off = 0;
        for (int c = 0; c < K.n_class; c++) {
            K.cls_off[c] = off;
            off += s_n[c];
        }
        K.cls_off[K.n_class] = off;
    }
}

__global__ __launch_bounds__(BLOCK) void ap_rank_kernel(ApArgs K) {
    __shared__ double s_sc[BLOCK];
    __shared__ int s_cl[BLOCK];
    const int tid = threadIdx.x, d = blockIdx.x * BLOCK + tid;
    auto score_of = [&](int e, int c) -> double {
        if (c < 0) return 0.0;      // never compared; a slot that is not owned is not read
        return (K.kind >= 2) ? (double)((const float*)K.pred_box)[(size_t)e * ROW_WORDS + 14] : K.score[e];
    };
    const int c = (d < K.n_pred) ? K.s_pcls[d] : NOT_OWNED;
    const double sd = (d < K.n_pred) ? score_of(d, c) : 0.0;
    int before = 0;
    for (int base = 0; base < K.n_pred; base += BLOCK) {
        const int e = base + tid;
        const int ce = (e < K.n_pred) ? K.s_pcls[e] : NOT_OWNED;
        s_cl[tid] = ce;
        s_sc[tid] = (e < K.n_pred) ? score_of(e, ce) : 0.0;
        __syncthreads();
        if (c >= 0) {
            const int lim = min(BLOCK, K.n_pred - base);
            for (int k = 0; k < lim; k++)
                before += (s_cl[k] == c && ranks_before(s_sc[k], base + k, sd, d)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (c >= 0) {
        K.rank[d] = before;
        const int at = K.cls_off[c] + before;
        if (before < K.npred[c] && at >= 0 && at < K.n_pred) K.order[at] = d;      // (always: the order is total)
    } else if (c == NO_CLASS) {
        K.rank[d] = -1;
    }
}

__global__ __launch_bounds__(BLOCK) void ap_claim_kernel(ApArgs K) {
    const int d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= K.n_pred || K.s_pcls[d] < 0) return;
    const int jg = K.s_jglob[d];
    if (jg >= 0 && jg < K.n_gt && K.ovmax[d] > K.ovthresh) atomicMin(&K.s_claim[jg], K.rank[d]);
}

__global__ __launch_bounds__(BLOCK) void ap_flag_kernel(ApArgs K) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < K.n_pred) {
        const int c = K.s_pcls[t];
        if (c >= 0) {
            const int jg = K.s_jglob[t];
            K.is_tp[t] = (jg >= 0 && jg < K.n_gt && K.ovmax[t] > K.ovthresh && K.s_claim[jg] == K.rank[t]) ? 1 : 0;
        } else if (c == NO_CLASS) {
            K.is_tp[t] = -1;
        }
    }
    if (t < K.n_gt) {
        const int c = K.s_gcls[t];
        if (c >= 0) {
            const int r = K.s_claim[t];
            int who = -1;
            if (r != FREE && r >= 0 && r < K.npred[c]) {
                const int at = K.cls_off[c] + r;
                if (at >= 0 && at < K.n_pred) who = K.order[at];
            }
            K.gt_claim[t] = who;
        } else if (c == NO_CLASS) {
            K.gt_claim[t] = -1;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void ap_curve_kernel(ApArgs K) {
    __shared__ int s_tp[BLOCK], s_fp[BLOCK];
    __shared__ double s_d[BLOCK];
    __shared__ double s_cmax[RANK_CAP / BLOCK];      // largest prec of each chunk
    const int c = blockIdx.x, tid = threadIdx.x;
    const int off = K.cls_off[c], npos = K.npos[c];
    int n = K.npred[c];
    if (off < 0 || off > K.n_pred) n = 0;
    n = max(0, min(n, K.n_pred - max(off, 0)));      // (always npred[c]: the count kernel wrote both)
    const double ninf = -__builtin_inf();
    double pmax[11];
#pragma unroll
    for (int i = 0; i < 11; i++) pmax[i] = ninf;
    // ---- forward: tp / fp prefix sums in rank order, rec, prec
    int carry_tp = 0, carry_fp = 0;
    for (int base = 0; base < n; base += BLOCK) {
        const int r = base + tid;
        int vt = 0, vf = 0;
        if (r < n) {
            const int d = K.order[off + r];
            vt = (d >= 0 && d < K.n_pred && K.is_tp[d] == 1) ? 1 : 0;
            vf = 1 - vt;
        }
        s_tp[tid] = vt; s_fp[tid] = vf;
        __syncthreads();
        for (int s = 1; s < BLOCK; s <<= 1) {
            const int at = (tid >= s) ? s_tp[tid - s] : 0, af = (tid >= s) ? s_fp[tid - s] : 0;
            __syncthreads();
            s_tp[tid] += at; s_fp[tid] += af;
            __syncthreads();
        }
        double prec = 0.0;
        if (r < n) {
            const int tp = carry_tp + s_tp[tid], fp = carry_fp + s_fp[tid];
            const double rec = curve_rec(tp, npos);
            prec = curve_prec(tp, fp);
            K.tp[off + r] = tp; K.fp[off + r] = fp; K.rec[off + r] = rec; K.prec[off + r] = prec;
#pragma unroll
            for (int i = 0; i < 11; i++)
                if (rec >= ap11_threshold(i) && prec > pmax[i]) pmax[i] = prec;
        }
        carry_tp += s_tp[BLOCK - 1]; carry_fp += s_fp[BLOCK - 1];
        s_d[tid] = prec;
        __syncthreads();
        for (int s = BLOCK / 2; s >= 1; s >>= 1) {
            if (tid < s && s_d[tid + s] > s_d[tid]) s_d[tid] = s_d[tid + s];
            __syncthreads();
        }
        if (tid == 0) s_cmax[base / BLOCK] = s_d[0];
        __syncthreads();
    }
    // ---- average precision
    double ap = 0.0;
    if (npos <= 0) {
        ap = __builtin_nan("");      // no ground truth of the class: left out of the mean
    } else if (n > 0 && K.use_07) {
#pragma unroll
        for (int i = 0; i < 11; i++) {      // voc_ap :52-57
            s_d[tid] = pmax[i];
            __syncthreads();
            for (int s = BLOCK / 2; s >= 1; s >>= 1) {
                if (tid < s && s_d[tid + s] > s_d[tid]) s_d[tid] = s_d[tid + s];
                __syncthreads();
            }
            const double p = (s_d[0] == ninf) ? 0.0 : s_d[0];
            ap = ap + p / 11.0;
            __syncthreads();
        }
    } else if (n > 0) {      // voc_ap :59-73
        if (tid == 0) {      // largest prec of every later chunk (mpre's closing sentinel is 0)
            double later = 0.0;
            for (int ch = (n - 1) / BLOCK; ch >= 0; ch--) {
                const double m = s_cmax[ch];
                s_cmax[ch] = later;
                if (m > later) later = m;
            }
        }
        __threadfence_block();
        __syncthreads();
        for (int base = 0; base < n; base += BLOCK) {
            const int r = base + tid;
            s_d[tid] = (r < n) ? K.prec[off + r] : 0.0;
            __syncthreads();
            for (int s = 1; s < BLOCK; s <<= 1) {      // suffix maximum inside the chunk
                const double o = (tid + s < BLOCK) ? s_d[tid + s] : 0.0;
                __syncthreads();
                if (o > s_d[tid]) s_d[tid] = o;
                __syncthreads();
            }
            const double later = s_cmax[base / BLOCK];
            const double env = (later > s_d[tid]) ? later : s_d[tid];
            __syncthreads();
            double term = 0.0;
            if (r < n) {
                const double rec = K.rec[off + r], prev = (r > 0) ? K.rec[off + r - 1] : 0.0;
                if (rec != prev) term = (rec - prev) * env;
            }
            s_d[tid] = term;
            __syncthreads();
            if (tid == 0) {      // in rank order, one term after the other: with every prediction a true positive the partial sums
                const int lim = min(BLOCK, n - base);      // are rec[r] itself, and the AP is exactly 1
                for (int k = 0; k < lim; k++) ap = ap + s_d[k];
            }
            __syncthreads();
        }
    }
    if (tid == 0) K.ap[c] = ap;
}

}  // namespace

extern "C" int odam_det_ap(odam_sq_ctx* ctx, int kind, int n_image, int n_pred, int n_gt, int n_class, const int* pred_off,
                           const int* gt_off, const void* pred_box, const void* gt_box, const int* cls_pred, const int* cls_gt,
                           const double* score, const long long* pair_off, const double* iou, long long n_pairs, double ovthresh,
                           int use_07_metric, int* scratch, double* out_ovmax, int* out_jmax, int* out_rank, int* out_is_tp,
                           int* out_gt_claim, int* out_order, int* out_npos, int* out_npred, int* out_cls_off, double* out_ap,
                           int* out_tp, int* out_fp, double* out_rec, double* out_prec, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_det_ap: null context");
    if (kind < 0 || kind > 3) return odam_fail(ODAM_E_INVALID, "odam_det_ap: box kind outside 0..3");
    if (n_image < 0 || n_pred < 0 || n_gt < 0 || n_pairs < 0) return odam_fail(ODAM_E_INVALID, "odam_det_ap: bad size");
    if (n_class < 1 || n_class > MAX_CLASS) return odam_fail(ODAM_E_INVALID, "odam_det_ap: n_class outside 1..64");
    if (kind >= 2 && (n_image > 0x7fffffff / ROW_SLOTS || n_pred != n_image * ROW_SLOTS || n_gt != n_image * ROW_SLOTS))
        return odam_fail(ODAM_E_INVALID, "odam_det_ap: detection rows need n_pred == n_gt == 30 n_image");
    if (!pred_off || !gt_off || !scratch || !out_ovmax || !out_jmax || !out_rank || !out_is_tp || !out_gt_claim || !out_order ||
        !out_npos || !out_npred || !out_cls_off || !out_ap || !out_tp || !out_fp || !out_rec || !out_prec)
        return odam_fail(ODAM_E_INVALID, "odam_det_ap: null pointer");
    if (kind != 1 && (!pred_box || !gt_box)) return odam_fail(ODAM_E_INVALID, "odam_det_ap: null boxes");
    if (kind < 2 && (!cls_pred || !cls_gt || !score)) return odam_fail(ODAM_E_INVALID, "odam_det_ap: null classes or scores");
    if (kind == 1 && (!pair_off || !iou)) return odam_fail(ODAM_E_INVALID, "odam_det_ap: kind 1 needs pair_off and iou");
    if (n_pred > RANK_CAP) return odam_fail(ODAM_E_LIMIT, "odam_det_ap: more than 32768 prediction slots (the ranking counts pairs)");
    ApArgs K{};
    K.kind = kind; K.n_image = n_image; K.n_pred = n_pred; K.n_gt = n_gt; K.n_class = n_class; K.use_07 = use_07_metric ? 1 : 0;
    K.pred_off = pred_off; K.gt_off = gt_off; K.pred_box = pred_box; K.gt_box = gt_box; K.cls_pred = cls_pred; K.cls_gt = cls_gt;
    K.score = score; K.pair_off = pair_off; K.iou = iou; K.n_pairs = n_pairs; K.ovthresh = ovthresh;
    K.s_pcls = scratch; K.s_jglob = scratch + n_pred; K.s_gcls = scratch + 2 * (size_t)n_pred; K.s_claim = K.s_gcls + n_gt;
    K.ovmax = out_ovmax; K.jmax = out_jmax; K.rank = out_rank; K.is_tp = out_is_tp; K.gt_claim = out_gt_claim; K.order = out_order;
    K.npos = out_npos; K.npred = out_npred; K.cls_off = out_cls_off; K.ap = out_ap; K.tp = out_tp; K.fp = out_fp; K.rec = out_rec;
    K.prec = out_prec;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gp = (unsigned)((n_pred + BLOCK - 1) / BLOCK), gg = (unsigned)(((long long)n_gt + BLOCK - 1) / BLOCK);
    const unsigned g_both = gp > gg ? gp : gg;
    hipLaunchKernelGGL(ap_overlap_kernel, dim3(g_both ? g_both : 1), dim3(BLOCK), 0, st, K);
    hipLaunchKernelGGL(ap_count_kernel, dim3(1), dim3(BLOCK), 0, st, K);
    hipLaunchKernelGGL(ap_rank_kernel, dim3(gp ? gp : 1), dim3(BLOCK), 0, st, K);
    hipLaunchKernelGGL(ap_claim_kernel, dim3(gp ? gp : 1), dim3(BLOCK), 0, st, K);
    hipLaunchKernelGGL(ap_flag_kernel, dim3(g_both ? g_both : 1), dim3(BLOCK), 0, st, K);
    hipLaunchKernelGGL(ap_curve_kernel, dim3((unsigned)n_class), dim3(BLOCK), 0, st, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
