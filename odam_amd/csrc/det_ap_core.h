// det_ap_core.h -- leaf arithmetic of the average-precision kernels (det_ap.hip), written so that a host restatement
// (tests/det_ap_ref.py) reproduces it operation for operation, and includable from a plain host program
// (tests/native/det_ap_check.cpp).
//
// Restates, of the reference (likojack/ODAM):
//   src/utils/eval_utils.py:147-152   the axis-aligned box of 8 corners (np.min / np.max per axis: a NaN corner gives NaN)
//   src/utils/box_utils.py:424-447    iou_3d      x_min = max(a, b) ... with PYTHON's max / min: max(a, b) is `b > a ? b : a`,
//   src/utils/box_utils.py:123-144    iou_2d      min(a, b) is `b < a ? b : a`, max(0, d) is `d > 0 ? d : 0` -- a NaN never wins
//   src/models/detr.py:176-183        the box of a detection row: t_co -+ dims / 2, in binary64 from the float32 words
//   src/utils/eval_utils.py:126       the order of np.argsort(-confidence), made total: equal scores keep their input order, a NaN
//                                     score ranks after every number
//   src/utils/eval_utils.py:169-173   rec = tp / npos, prec = tp / max(tp + fp, eps)
// The reference's `assert 0 <= IoU <= 1` is not restated: 0 / 0 is NaN, and a NaN is never `> ovmax`.
//
// Operation order is part of the contract: binary64, no implicit contraction (-ffp-contract=off), products and sums left to right.
#pragma once
#include "sq_math.h"

namespace odam_ap {

constexpr int ROW_SLOTS = 30;      // detection rows per frame of a [F, 30, 15] block (odam_detr_select_pack)
constexpr int ROW_WORDS = 15;

ODAM_HD double py_max(double a, double b) { return b > a ? b : a; }      // Python's max(a, b)
ODAM_HD double py_min(double a, double b) { return b < a ? b : a; }      // Python's min(a, b)
ODAM_HD double py_max0(double d) { return d > 0.0 ? d : 0.0; }           // max(0, d)
ODAM_HD double np_amin(double m, double x) { return (m <= x || m != m) ? m : x; }      // np.min step: NaN if either is NaN
ODAM_HD double np_amax(double m, double x) { return (m >= x || m != m) ? m : x; }      // np.max step

// lo[3], hi[3] of 8 corners c[8][3] (eval_utils.py:148-151)
ODAM_HD void aabb_of_corners(const double* c, double* lo, double* hi) {
    for (int a = 0; a < 3; a++) {
        double mn = c[a], mx = c[a];
        for (int k = 1; k < 8; k++) {
            mn = np_amin(mn, c[3 * k + a]);
            mx = np_amax(mx, c[3 * k + a]);
        }
        lo[a] = mn;
        hi[a] = mx;
    }
}

// lo[3], hi[3] of a detection row (detr.py:176-183): (-dims) / 2 + t_co and dims / 2 + t_co
ODAM_HD void aabb_of_row(const float* row, double* lo, double* hi) {
    for (int a = 0; a < 3; a++) {
        const double h = (double)row[6 + a] / 2.0, t = (double)row[9 + a];
        lo[a] = t - h;
        hi[a] = t + h;
    }
}

// box_utils.iou_3d on two [2][3] boxes
ODAM_HD double iou_3d(const double* alo, const double* ahi, const double* blo, const double* bhi) {
    const double dx = py_min(ahi[0], bhi[0]) - py_max(alo[0], blo[0]);
    const double dy = py_min(ahi[1], bhi[1]) - py_max(alo[1], blo[1]);
    const double dz = py_min(ahi[2], bhi[2]) - py_max(alo[2], blo[2]);
    const double inter = (py_max0(dx) * py_max0(dy)) * py_max0(dz);
    const double va = ((ahi[0] - alo[0]) * (ahi[1] - alo[1])) * (ahi[2] - alo[2]);
    const double vb = ((bhi[0] - blo[0]) * (bhi[1] - blo[1])) * (bhi[2] - blo[2]);
    return inter / ((va + vb) - inter);
}

// box_utils.iou_2d on the columns 2-5 (x0, y0, x1, y1) of two detection rows
ODAM_HD double iou_2d_rows(const float* ra, const float* rb) {
    const double ax0 = ra[2], ay0 = ra[3], ax1 = ra[4], ay1 = ra[5];
    const double bx0 = rb[2], by0 = rb[3], bx1 = rb[4], by1 = rb[5];
    const double dx = py_min(ax1, bx1) - py_max(ax0, bx0);
    const double dy = py_min(ay1, by1) - py_max(ay0, by0);
    const double inter = py_max0(dx) * py_max0(dy);
    const double aa = (ax1 - ax0) * (ay1 - ay0);
    const double ab = (bx1 - bx0) * (by1 - by0);
    return inter / ((aa + ab) - inter);
}

// does prediction e (score se, input index e) rank before prediction d (score sd) of the same class?  Descending score; equal
// scores (and two NaN) by input index; a NaN after every number.  A strict total order: the rank is a count of `before`.
ODAM_HD bool ranks_before(double se, int e, double sd, int d) {
    const bool ne = se != se, nd = sd != sd;
    if (ne | nd) return (ne & nd) ? (e < d) : nd;
    return (se > sd) | ((se == sd) & (e < d));
}

ODAM_HD double curve_rec(int tp, int npos) { return (double)tp / (double)npos; }
ODAM_HD double curve_prec(int tp, int fp) {
    const double eps = 2.220446049250313e-16;      // np.finfo(np.float64).eps
    const double den = (double)(tp + fp);
    return (double)tp / (den >= eps ? den : eps);      // np.maximum(tp + fp, eps); the sum is a whole number, never NaN
}

// the thresholds of the 11-point form: np.arange(0., 1.1, 0.1)[i], which numpy fills as 0.0 + i * 0.1
ODAM_HD double ap11_threshold(int i) { return 0.0 + (double)i * 0.1; }

}  // namespace odam_ap
