// det_loss_core.h -- leaf arithmetic of the matching cost and the losses (det_loss.hip), usable from host and device and written
// so that the numpy restatement (tests/criterion_ref.py) follows it operation for operation.
//
// Restates, of the reference (likojack/ODAM):
//   src/utils/box_utils.py:490-494   box_cxcywh_to_xyxy_pytorch: (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h)
//   src/utils/box_utils.py:8-21      box_iou: inter / (area1 + area2 - inter), no epsilon
//   src/utils/box_utils.py:147-166   generalized_box_iou: iou - (area - union) / area, after `x1 >= x0, y1 >= y0` on both sides
//   src/models/matcher.py:51, 61     softmax of a query row, read at the target's label
//   src/models/detr.py:299, 370      cross entropy of a row: logsumexp - logit[target]
//
// float32 per element, as the reference computes on float32 tensors; no implicit contraction (-ffp-contract=off); sums and
// products left to right.
#pragma once
#include <math.h>

#include "sq_math.h"

namespace odam_loss {

// (x0, y0, x1, y1) of (cx, cy, w, h)
ODAM_HD void xyxy_of(const float* b, float* o) {
    o[0] = b[0] - 0.5f * b[2];
    o[1] = b[1] - 0.5f * b[3];
    o[2] = b[0] + 0.5f * b[2];
    o[3] = b[1] + 0.5f * b[3];
}

// what generalized_box_iou asserts of every box: a NaN fails it, as it fails the reference's `>=`
ODAM_HD bool xyxy_ok(const float* o) { return o[2] >= o[0] && o[3] >= o[1]; }

ODAM_HD float t_max(float a, float b) { return (a != a || a > b) ? a : b; }      // torch.max / torch.min of two: a NaN wins
ODAM_HD float t_min(float a, float b) { return (a != a || a < b) ? a : b; }
ODAM_HD float clamp0(float d) { return d < 0.0f ? 0.0f : d; }                    // clamp(min=0): a NaN stays

// generalized IoU of two xyxy boxes
ODAM_HD float giou_xyxy(const float* a, const float* b) {
    const float area1 = (a[2] - a[0]) * (a[3] - a[1]);
    const float area2 = (b[2] - b[0]) * (b[3] - b[1]);
    const float iw = clamp0(t_min(a[2], b[2]) - t_max(a[0], b[0]));
    const float ih = clamp0(t_min(a[3], b[3]) - t_max(a[1], b[1]));
    const float inter = iw * ih;
    const float uni = (area1 + area2) - inter;
    const float iou = inter / uni;
    const float cw = clamp0(t_max(a[2], b[2]) - t_min(a[0], b[0]));
    const float ch = clamp0(t_max(a[3], b[3]) - t_min(a[1], b[1]));
    const float area = cw * ch;
    return iou - (area - uni) / area;
}

// sum over n of |a - b|, left to right, in float32 (the matcher's cdist)
ODAM_HD float l1_f32(const float* a, const float* b, int n) {
    float s = 0.0f;
    for (int k = 0; k < n; k++) s = s + fabsf(a[k] - b[k]);
    return s;
}

// the same terms widened one by one and added in binary64 (the criterion's sums)
ODAM_HD double l1_f64(const float* a, const float* b, int n) {
    double s = 0.0;
    for (int k = 0; k < n; k++) s = s + (double)fabsf(a[k] - b[k]);
    return s;
}

// largest entry of a row and its first position; a NaN entry wins, as it does in torch
ODAM_HD float row_max(const float* x, int n, int* arg) {
    float m = x[0];
    int am = 0;
    for (int k = 1; k < n; k++)
        if (!(m != m) && (x[k] != x[k] || x[k] > m)) { m = x[k]; am = k; }
    *arg = am;
    return m;
}

// sum over the row of exp(x - m), left to right
ODAM_HD float row_sumexp(const float* x, int n, float m) {
    float s = 0.0f;
    for (int k = 0; k < n; k++) s = s + expf(x[k] - m);
    return s;
}

// softmax(x)[k] from the row's maximum and sum
ODAM_HD float softmax_at(float xk, float m, float s) { return expf(xk - m) / s; }

// cross entropy of a row at class k: log(sum exp(x - m)) - (x[k] - m)
ODAM_HD float nll_at(float xk, float m, float s) { return logf(s) - (xk - m); }

// a float32 word that holds a class: truncated as .long() truncates; a NaN or a huge word is no class
ODAM_HD int class_of(float v, int n) {
    if (!(v > -1.0f && v < (float)n)) return -1;
    return (int)v;
}

}  // namespace odam_loss
