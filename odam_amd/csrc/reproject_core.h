// reproject_core.h -- leaf arithmetic of the reprojection kernels (reproject.hip), written so that a host restatement
// (tests/reproject_ref.py) reproduces it operation for operation.
//
// Restates, forward only (likojack/ODAM src/super_quadric/sq_libs.py):
//   :395-413  SuperQuadricOptimizer.constraint_2d   surface points through every view, the four extents of the valid ones
//   :289-314  DualQuadric.get_bbox                  the box of the projected conic C = P Q P^T
//   :420-429  the L1 terms against the detected edges (NaN -> 0, mask), here kept per view and summed per object
// and adds the 2D IoU of the detected box with the predicted one.
//
// Operation order is part of the contract: binary32 / binary64 as the signatures say, no implicit contraction
// (-ffp-contract=off), fmaf only inside odam_sq::proj_row, IEEE sqrt and division.
#pragma once
#include "sq_core.h"

namespace odam_rp {

constexpr float FILL = 1000000.0f;      // sq_libs.py:403-412

// ---- super-quadric path, binary32 -----------------------------------------------------------------------------------------------
// one surface point in one view (sq_libs.py:398-400): the projection rows are the fit's own odam_sq::proj_row
ODAM_HD bool sq_pixel(float w0, float w1, float w2, const float* M, float& u, float& v) {
    const float qx = odam_sq::proj_row(w0, w1, w2, M[0], M[1], M[2], M[3]);
    const float qy = odam_sq::proj_row(w0, w1, w2, M[4], M[5], M[6], M[7]);
    const float qz = odam_sq::proj_row(w0, w1, w2, M[8], M[9], M[10], M[11]);
    const float den = odam_sq::absf(qz) + 1e-6f;
    u = qx / den;
    v = qy / den;
    return qz > 0.5f;
}

// torch.min / torch.max of two values: NaN if either is NaN (not fminf / fmaxf).  Exact, so any merge order gives the same
// value; the sign of a zero is the one thing an order could change, and store_ext takes it away.
template <typename T>
ODAM_HD T min_nan(T a, T b) { return (a != a || b != b) ? (T)__builtin_nanf("") : ((b < a) ? b : a); }
template <typename T>
ODAM_HD T max_nan(T a, T b) { return (a != a || b != b) ? (T)__builtin_nanf("") : ((b > a) ? b : a); }

// what is stored for an extent: -0 becomes +0 (x + 0 in round-to-nearest), every NaN the default quiet NaN
ODAM_HD float store_ext(float x) { return (x != x) ? __builtin_nanf("") : (x + 0.0f); }

// ---- dual-quadric path, binary64 ------------------------------------------------------------------------------------------------
ODAM_HD double dot4d(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

// the five entries of C = (P Q) P^T the box reads: c00, c02, c11, c12, c22.  P[12], Q[16] row-major.
ODAM_HD void conic5(const double* P, const double* Q, double c[5]) {
    double PQ[12];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 4; k++)
            PQ[4 * i + k] = dot4d(P[4 * i], P[4 * i + 1], P[4 * i + 2], P[4 * i + 3], Q[k], Q[4 + k], Q[8 + k], Q[12 + k]);
    c[0] = dot4d(PQ[0], PQ[1], PQ[2], PQ[3], P[0], P[1], P[2], P[3]);
    c[1] = dot4d(PQ[0], PQ[1], PQ[2], PQ[3], P[8], P[9], P[10], P[11]);
    c[2] = dot4d(PQ[4], PQ[5], PQ[6], PQ[7], P[4], P[5], P[6], P[7]);
    c[3] = dot4d(PQ[4], PQ[5], PQ[6], PQ[7], P[8], P[9], P[10], P[11]);
    c[4] = dot4d(PQ[8], PQ[9], PQ[10], PQ[11], P[8], P[9], P[10], P[11]);
}

// one axis of get_bbox (sq_libs.py:294-298 / :300-304); false when the discriminant is negative or NaN
ODAM_HD bool dq_axis(double cii, double ci2, double c22, double& lo, double& hi) {
    const double D = 4.0 * (ci2 * ci2) - (4.0 * cii) * c22;
    if (!(D >= 0.0)) return false;
    const double b = __builtin_sqrt(D);
    const double r = 0.5 / c22;
    const double s2 = 2.0 * ci2;
    const double x0 = r * (s2 + b), x1 = r * (s2 - b);
    lo = (x1 < x0) ? x1 : x0;      // Python's min(x_0, x_1) / max(x_0, x_1)
    hi = (x1 > x0) ? x1 : x0;
    return true;
}

// ext[4] = x_min, x_max, y_min, y_max of the conic of Q in view P; status 1 and four NaN when a discriminant is negative or NaN,
// or c22 == 0
ODAM_HD int dq_box(const double* P, const double* Q, double ext[4]) {
    double c[5];
    conic5(P, Q, c);
    const bool okx = dq_axis(c[0], c[1], c[4], ext[0], ext[1]);
    const bool oky = dq_axis(c[2], c[3], c[4], ext[2], ext[3]);
    if (okx && oky && c[4] != 0.0) return 0;
    for (int d = 0; d < 4; d++) ext[d] = __builtin_nan("");
    return 1;
}

// ---- scores, T = float or double ------------------------------------------------------------------------------------------------
// the residual of one edge (sq_libs.py:423-428): |ext - box| where the edge is a constraint, NaN -> 0
template <typename T>
ODAM_HD T edge_residual(T ext, T box, float mask) {
    const T d = ext - box;
    const T a = (d < (T)0) ? -d : d;
    return (mask != 0.0f && a == a) ? a : (T)0;
}

template <typename T>
ODAM_HD T clip(T x, T lo, T hi) { return (x < lo) ? lo : ((x > hi) ? hi : x); }      // a NaN passes
template <typename T>
ODAM_HD T pos(T x) { return (x > (T)0) ? x : (T)0; }                                 // a NaN gives 0

// 2D IoU of the detected box with the predicted one, both x_min, x_max, y_min, y_max.  The prediction is clipped to the image
// first (the detector clips its boxes, nothing clips a prediction); a union that is <= 0 or NaN gives 0, a bad view gives 0.
template <typename T>
ODAM_HD T box_iou(const T* ext, const T* box, T img_w, T img_h, bool bad) {
    const T px0 = clip(ext[0], (T)0, img_w), px1 = clip(ext[1], (T)0, img_w);
    const T py0 = clip(ext[2], (T)0, img_h), py1 = clip(ext[3], (T)0, img_h);
    const T area_p = pos(px1 - px0) * pos(py1 - py0);
    const T area_d = pos(box[1] - box[0]) * pos(box[3] - box[2]);
    const T ix0 = (box[0] > px0) ? box[0] : px0, ix1 = (box[1] < px1) ? box[1] : px1;
    const T iy0 = (box[2] > py0) ? box[2] : py0, iy1 = (box[3] < py1) ? box[3] : py1;
    const T inter = pos(ix1 - ix0) * pos(iy1 - iy0);
    const T uni = (area_p + area_d) - inter;
    if (bad || !(uni > (T)0)) return (T)0;
    const T q = inter / uni;
    return (q == q) ? q : (T)0;      // Inf / Inf of a box with an infinite edge
}

}  // namespace odam_rp
