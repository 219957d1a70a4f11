// dq_core.h -- leaf arithmetic of the dual-quadric multi-view fit (dq_fit.hip), written so that a host restatement
// (tests/dq_ref.py) reproduces it bit for bit.
//
// Restates the reference's QuadricOptimizer (likojack/ODAM src/super_quadric/sq_libs.py:39-241):
//   :68-78    params2mat                Q = T diag(a, -1) T^T,  T = [rotz(angle) | translate]
//   :123-147  compute_projected_lines   the four box edges of the conic C = M Q M^T
//   :149-168  constraint_2d             L1 against the stored lines, NaN -> 0, mask, mean per direction, sum of the four
// and takes the gradient autograd computes through them in closed form.
//
// Operation order is part of the contract: binary32, no implicit contraction (-ffp-contract=off), fmaf exactly where
// written, IEEE sqrt and division.
#pragma once
#include "sq_core.h"

namespace odam_dq {

using odam_sq::absf;
using odam_sq::sgnf;

ODAM_HD float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// state: p[0..2] translate, p[3] angle, p[4] scale_factor;  h[3] = dims / 2 (constant)
struct Obj {
    float c, s;       // cos / sin(angle)            sq_libs.py:112-113
    float sc[3];      // scale_factor * h            sq_libs.py:229
    float a[3];       // (scale_factor * h)^2
    float Q[16];      // row-major dual quadric      sq_libs.py:78
};

// sq_libs.py:229-230, :68-78.  (T @ diag) first, then @ T^T, each entry as an fmaf chain over the inner index; the products
// with the structural zeros of T are left out.  Q is NOT symmetrised: Q[0][1] and Q[1][0] are rounded separately, as in the
// reference's matrix product.
ODAM_HD Obj make_obj(const float* p, const float* h) {
    Obj o;
    o.c = odam_math::cosf_(p[3]);
    o.s = odam_math::sinf_(p[3]);
    for (int k = 0; k < 3; k++) {
        o.sc[k] = p[4] * h[k];
        o.a[k] = o.sc[k] * o.sc[k];
    }
    const float tx = p[0], ty = p[1], tz = p[2];
    const float t00 = o.c * o.a[0], t01 = (-o.s) * o.a[1], t10 = o.s * o.a[0], t11 = o.c * o.a[1];
    float* Q = o.Q;
    Q[0] = fma_(-tx, tx, fma_(t01, -o.s, t00 * o.c));
    Q[1] = fma_(-tx, ty, fma_(t01, o.c, t00 * o.s));
    Q[2] = (-tx) * tz;
    Q[3] = -tx;
    Q[4] = fma_(-ty, tx, fma_(t11, -o.s, t10 * o.c));
    Q[5] = fma_(-ty, ty, fma_(t11, o.c, t10 * o.s));
    Q[6] = (-ty) * tz;
    Q[7] = -ty;
    Q[8] = (-tz) * tx;
    Q[9] = (-tz) * ty;
    Q[10] = fma_(-tz, tz, o.a[2]);
    Q[11] = -tz;
    Q[12] = -tx;
    Q[13] = -ty;
    Q[14] = -tz;
    Q[15] = -1.0f;
    return o;
}

ODAM_HD float dot4(float a0, float a1, float a2, float a3, float b0, float b1, float b2, float b3) {
    return fma_(a3, b3, fma_(a2, b2, fma_(a1, b1, a0 * b0)));
}

// what one view adds: loss terms per direction (x_min, x_max, y_min, y_max; already masked) and the five gradient components
struct ViewOut {
    float l[4];
    float g[5];
    bool bad;         // a negative (or NaN) discriminant: sq_libs.py:129,136 would assert
};

// one axis of compute_projected_lines (sq_libs.py:128-133 / :135-140) and its backward.
//   cii = C[i][i], ci2 = C[i][2], c22 = C[2][2];  t_lo / t_hi, m_lo / m_hi: pixel targets and masks of the min / max edge
// Adds to gii, gi2, g22 (gradients w.r.t. the three conic entries); returns false when the discriminant is negative.
ODAM_HD bool axis_terms(float cii, float ci2, float c22, float t_lo, float t_hi, float m_lo, float m_hi, float invF,
                        float& l_lo, float& l_hi, float& gii, float& gi2, float& g22) {
    const float D = 4.0f * (ci2 * ci2) - (4.0f * cii) * c22;
    l_lo = 0.0f; l_hi = 0.0f; gii = 0.0f; gi2 = 0.0f;
    if (!(D >= 0.0f)) return false;
    const float b = __builtin_sqrtf(D);
    const float r = 0.5f / c22;
    const float s2 = 2.0f * ci2;
    const float u0 = s2 + b, u1 = s2 - b;
    const float x0 = r * u0, x1 = r * u1;
    const bool min0 = !(x1 < x0), max0 = !(x1 > x0);      // torch.min / max over the stacked pair: the first of equal values
    const float lo = min0 ? x0 : x1, hi = max0 ? x0 : x1;
    // the reference compares -lo with gt = -pixel: |(-lo) - (-t)| = |lo - t| exactly, d/d lo = sign(lo - t)
    const float d_lo = lo - t_lo, d_hi = hi - t_hi;
    float a_lo = absf(d_lo), a_hi = absf(d_hi);
    float g_lo = (sgnf(d_lo) * m_lo) * invF, g_hi = (sgnf(d_hi) * m_hi) * invF;
    if (d_lo != d_lo) { a_lo = 0.0f; g_lo = 0.0f; }       // NaN -> 0   sq_libs.py:164-165
    if (d_hi != d_hi) { a_hi = 0.0f; g_hi = 0.0f; }
    l_lo = a_lo * m_lo;
    l_hi = a_hi * m_hi;
    if (g_lo == 0.0f && g_hi == 0.0f) return true;          // both edges masked or on target: nothing flows back
    const float gx0 = (min0 ? g_lo : 0.0f) + (max0 ? g_hi : 0.0f);
    const float gx1 = (min0 ? 0.0f : g_lo) + (max0 ? 0.0f : g_hi);
    const float g_r = gx0 * u0 + gx1 * u1;
    const float g_b = r * (gx0 - gx1);
    const float g_D = (0.5f * g_b) / b;
    gi2 = (2.0f * r) * (gx0 + gx1) + g_D * (8.0f * ci2);
    gii = -((4.0f * c22) * g_D);
    g22 += -(g_r * (r / c22)) - (4.0f * cii) * g_D;
    return true;
}

// M[12]: row-major 3x4 projection;  t[4], m[4]: pixel targets / masks in the order x_min, x_max, y_min, y_max
ODAM_HD ViewOut view_terms(const Obj& o, const float* p, const float* h, const float* M, const float* t, const float* m, float invF) {
    ViewOut out;
    const float* Q = o.Q;
    // C = (M Q) M^T  (sq_libs.py:156): rows of M Q, then the five entries the lines read
    float MQ[12];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 4; k++)
            MQ[4 * i + k] = dot4(M[4 * i], M[4 * i + 1], M[4 * i + 2], M[4 * i + 3], Q[k], Q[4 + k], Q[8 + k], Q[12 + k]);
    const float c00 = dot4(MQ[0], MQ[1], MQ[2], MQ[3], M[0], M[1], M[2], M[3]);
    const float c02 = dot4(MQ[0], MQ[1], MQ[2], MQ[3], M[8], M[9], M[10], M[11]);
    const float c11 = dot4(MQ[4], MQ[5], MQ[6], MQ[7], M[4], M[5], M[6], M[7]);
    const float c12 = dot4(MQ[4], MQ[5], MQ[6], MQ[7], M[8], M[9], M[10], M[11]);
    const float c22 = dot4(MQ[8], MQ[9], MQ[10], MQ[11], M[8], M[9], M[10], M[11]);
    float g00, g02, g11, g12, g22 = 0.0f;
    const bool okx = axis_terms(c00, c02, c22, t[0], t[1], m[0], m[1], invF, out.l[0], out.l[1], g00, g02, g22);
    const bool oky = axis_terms(c11, c12, c22, t[2], t[3], m[2], m[3], invF, out.l[2], out.l[3], g11, g12, g22);
    out.bad = !(okx && oky);
    // backward through C_ij = sum_k a_k q_ik q_jk - z_i z_j  with  q_i = R^T M_i[:3],  z_i = M_i[:3] . translate + M_i[3]
    float z[3], q[3][3];
    for (int i = 0; i < 3; i++) {
        const float* r = M + 4 * i;
        z[i] = fma_(r[2], p[2], fma_(r[1], p[1], r[0] * p[0])) + r[3];
        q[i][0] = fma_(r[1], o.s, r[0] * o.c);
        q[i][1] = fma_(r[1], o.c, r[0] * (-o.s));
        q[i][2] = r[2];
    }
    const float e0 = (2.0f * g00) * z[0] + g02 * z[2];
    const float e1 = (2.0f * g11) * z[1] + g12 * z[2];
    const float e2 = (g02 * z[0] + g12 * z[1]) + (2.0f * g22) * z[2];
    for (int k = 0; k < 3; k++) out.g[k] = -((M[k] * e0 + M[4 + k] * e1) + M[8 + k] * e2);
    float S[3];
    for (int k = 0; k < 3; k++)
        S[k] = (((g00 * q[0][k]) * q[0][k] + (g02 * q[0][k]) * q[2][k]) + (g22 * q[2][k]) * q[2][k]) +
               ((g11 * q[1][k]) * q[1][k] + (g12 * q[1][k]) * q[2][k]);
    const float X = (((2.0f * g00) * (q[0][0] * q[0][1]) + g02 * (q[0][0] * q[2][1] + q[0][1] * q[2][0])) +
                     (2.0f * g22) * (q[2][0] * q[2][1])) +
                    ((2.0f * g11) * (q[1][0] * q[1][1]) + g12 * (q[1][0] * q[2][1] + q[1][1] * q[2][0]));
    out.g[3] = (o.a[0] - o.a[1]) * X;
    out.g[4] = (((2.0f * o.sc[0]) * h[0]) * S[0] + ((2.0f * o.sc[1]) * h[1]) * S[1]) + ((2.0f * o.sc[2]) * h[2]) * S[2];
    return out;
}

}  // namespace odam_dq
