// box_iou_core.h -- leaf arithmetic of the oriented-box IoU kernel (box_iou.hip), written so that a host restatement
// (tests/box_iou_ref.py) reproduces it operation for operation, and includable from a plain host program.
//
// Restates odam_amd/merge.py::box3d_iou_pairs, the closed form that stands for the reference's box3d_iou (likojack/ODAM
// src/utils/box_utils.py:98-120: polygon_clip of the two footprints, qhull's area, the z overlap, box3d_vol):
//   footprints        R[k] = C[3 - k][:2], k = 0..3                                        (merge.py: C[:, 3::-1, :2])
//   signed area       0.5 * (((t0 + t1) + t2) + t3), t_k = x_k y_{k+1} - y_k x_{k+1}
//   orientation flip  a footprint of negative area is walked backwards; a clipper (box 2) that is not counter-clockwise gives 0
//   boundary pieces   every edge of one quadrilateral cut parametrically against the four half-planes of the other
//                     (merge.py::_boundary_inside: `closed` true for box 1's edges, false for box 2's), Green's theorem in edge order
//   z overlap         from corners 0 and 4; volumes from the three edge norms |c0 - c1| |c1 - c2| |c0 - c4|
//
// Operation order is part of the contract: binary64, no implicit contraction (-ffp-contract=off), IEEE sqrt and division, sums in
// index order.  Minimum and maximum are numpy's: a NaN operand gives NaN.  No branch on data: every lane does the same 32 tests.
#pragma once
#include "sq_math.h"

namespace odam_biou {

ODAM_HD double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }      // np.maximum: NaN if either is NaN
ODAM_HD double np_min(double a, double b) { return (a <= b || a != a) ? a : b; }      // np.minimum
ODAM_HD double clip01(double x) { return np_min(np_max(x, 0.0), 1.0); }               // np.clip(x, 0, 1)

// merge.py::_signed_area of the quadrilateral (x[k], y[k])
ODAM_HD double signed_area(const double* x, const double* y) {
    double s = 0.0;
    for (int k = 0; k < 4; k++) {
        const int k1 = (k + 1) & 3;
        const double t = x[k] * y[k1] - y[k] * x[k1];
        s = (k == 0) ? t : s + t;
    }
    return 0.5 * s;
}

// merge.py::_boundary_inside for one pair: the Green's-theorem sum over the parts of P's edges inside the convex quadrilateral Q
ODAM_HD double boundary_inside(const double* px, const double* py, const double* qx, const double* qy, bool closed) {
    const double inf = __builtin_inf();
    double sum = 0.0;
    for (int j = 0; j < 4; j++) {
        const int j1 = (j + 1) & 3;
        const double dx = px[j1] - px[j], dy = py[j1] - py[j];
        double enter = -inf, leave = inf;
        bool out_par = false;
        for (int k = 0; k < 4; k++) {
            const int k1 = (k + 1) & 3;
            const double ex = qx[k1] - qx[k], ey = qy[k1] - qy[k];
            const double dist = ex * (py[j] - qy[k]) - ey * (px[j] - qx[k]);
            const double rate = ex * dy - ey * dx;
            const double t = -dist / rate;
            const bool par = rate == 0.0;
            out_par = out_par | (par & (closed ? (dist < 0.0) : (dist <= 0.0)));
            enter = np_max(enter, (rate > 0.0) ? t : -inf);
            leave = np_min(leave, (rate < 0.0) ? t : inf);
        }
        const double t0 = clip01(enter), t1 = clip01(leave);
        const bool ok = (t1 > t0) & !out_par;
        const double sx = px[j] + t0 * dx, sy = py[j] + t0 * dy;
        const double ex = px[j] + t1 * dx, ey = py[j] + t1 * dy;
        const double c = ok ? (sx * ey - sy * ex) : 0.0;
        sum = (j == 0) ? c : sum + c;
    }
    return sum * 0.5;
}

// |a - b| of two corners (np.linalg.norm: the squares added in index order, IEEE sqrt)
ODAM_HD double edge_norm(const double* a, const double* b) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

ODAM_HD double box_volume(const double* c) { return (edge_norm(c, c + 3) * edge_norm(c + 3, c + 6)) * edge_norm(c, c + 12); }

// c1[24], c2[24]: the eight corners of box 1 (clipped) and box 2 (clipper), row-major [8][3].  Returns the 3D IoU, bev = the IoU of
// the footprints.
ODAM_HD double box3d_iou(const double* c1, const double* c2, double& bev) {
    double x1[4], y1[4], x2[4], y2[4];
    for (int k = 0; k < 4; k++) {
        x1[k] = c1[3 * (3 - k)]; y1[k] = c1[3 * (3 - k) + 1];
        x2[k] = c2[3 * (3 - k)]; y2[k] = c2[3 * (3 - k) + 1];
    }
    const double s1 = signed_area(x1, y1), s2 = signed_area(x2, y2);
    const double a1 = __builtin_fabs(s1), a2 = __builtin_fabs(s2);
    const bool f1 = s1 < 0.0, f2 = s2 < 0.0;
    double ax[4], ay[4], bx[4], by[4];
    for (int k = 0; k < 4; k++) {
        ax[k] = f1 ? x1[3 - k] : x1[k]; ay[k] = f1 ? y1[3 - k] : y1[k];
        bx[k] = f2 ? x2[3 - k] : x2[k]; by[k] = f2 ? y2[3 - k] : y2[k];
    }
    const double raw = np_max(boundary_inside(ax, ay, bx, by, true) + boundary_inside(bx, by, ax, ay, false), 0.0);
    const double inter = (s2 > 0.0) ? raw : 0.0;
    bev = inter / ((a1 + a2) - inter);
    const double dz = np_max(0.0, np_min(c1[2], c2[2]) - np_max(c1[14], c2[14]));
    const double iv = inter * dz;
    return iv / ((box_volume(c1) + box_volume(c2)) - iv);
}

// the pairs a launch evaluates: 0 = all, 1 = equal class, 2 = the merge rule (run_merge.py:105-110): equal class, or both in {4, 5}
ODAM_HD bool gate_open(int gate, int ca, int cb) {
    const bool same = ca == cb;
    const bool sofa_chair = ((ca == 4) | (ca == 5)) & ((cb == 4) | (cb == 5));
    return (gate == 0) | same | ((gate == 2) & sofa_chair);
}

}  // namespace odam_biou
