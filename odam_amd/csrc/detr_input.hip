// detr_input.hip -- the two ends of the detector outside the network: the input transform's resampling tables (the resize
// itself runs on the device, detr_kernels.hip) and the host selection of detections (threshold + greedy NMS).
#include <hip/hip_runtime.h>

#include <cmath>

#include "detr_kernels.h"
#include "detr_model.h"

using namespace odam_dm;

// ---- resampling tables of the input transform, built once per (source length, output length) and kept on the device --
// Pillow src/libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle, support 1)
// filter over the whole image: what PIL's Image.resize(BILINEAR) -- torchvision F.resize on a PIL image, the
// reference's transforms.py:105 -- builds before its two integer passes.  Double arithmetic, C truncating casts.
static int resample_table(odam_detr* m, int in_size, int out_size, odam_detr::Resample* r) {
    auto it = m->resample.find({in_size, out_size});
    if (it != m->resample.end()) { *r = it->second; return 0; }
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    std::vector<int> xmin(out_size), cnt(out_size), K((size_t)out_size * ksize, 0);
    std::vector<double> w(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; xx++) {
        const double center = (xx + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double ww = 0.0;
        for (int x = 0; x < ksize; x++) w[x] = 0.0;
        for (int x = 0; x < n; x++) {
            double t = (x + lo - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            w[x] = t < 1.0 ? 1.0 - t : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < n; x++)
            if (ww != 0.0) w[x] /= ww;
        for (int x = 0; x < ksize; x++)
            K[(size_t)xx * ksize + x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << 22)) : (int)(0.5 + w[x] * (1 << 22));
        xmin[xx] = lo; cnt[xx] = n;
    }
    odam_detr::Resample t{};
    t.ksize = ksize;
    if (int rc = m->dev_alloc(&t.xmin, xmin.size())) return rc;
    if (int rc = m->dev_alloc(&t.cnt, cnt.size())) return rc;
    if (int rc = m->dev_alloc(&t.K, K.size())) return rc;
    ODAM_HIP(hipMemcpy(t.xmin, xmin.data(), xmin.size() * sizeof(int), hipMemcpyHostToDevice));
    ODAM_HIP(hipMemcpy(t.cnt, cnt.data(), cnt.size() * sizeof(int), hipMemcpyHostToDevice));
    ODAM_HIP(hipMemcpy(t.K, K.data(), K.size() * sizeof(int), hipMemcpyHostToDevice));
    m->resample[{in_size, out_size}] = t;
    *r = t;
    return 0;
}

int odam_dm::resample_tables(odam_detr* m, int h, int w, odam_detr::Resample* tx, odam_detr::Resample* ty) {
    RC(resample_table(m, w, m->cfg.img_w, tx));
    return resample_table(m, h, m->cfg.img_h, ty);
}

// transforms.py:281-290 on the device: resize to the model's (img_h, img_w) + ToTensor + Normalize
extern "C" int odam_detr_preprocess_u8(odam_detr* m, const unsigned char* rgb, int B, int h, int w, const float* mean,
                                       const float* stdv, float* out, void* stream) {
    if (!m || !rgb || !mean || !stdv || !out) return odam_fail(1, "odam_detr_preprocess_u8: null pointer");
    if (B < 0 || h < 1 || w < 1) return odam_fail(1, "odam_detr_preprocess_u8: bad size");
    odam_detr::Resample tx{}, ty{};
    RC(resample_table(m, w, m->cfg.img_w, &tx));
    RC(resample_table(m, h, m->cfg.img_h, &ty));
    return odam_dk::launch_preprocess_u8(rgb, B, h, w, tx.xmin, tx.cnt, tx.K, tx.ksize, ty.xmin, ty.cnt, ty.K, ty.ksize,
                                         out, m->cfg.img_h, m->cfg.img_w, mean, stdv, (hipStream_t)stream);
}

// ---- threshold + greedy 3D/2D NMS on one frame's post-processed rows (host, float32 as the reference's numpy) --
// detr.py:124-125 (keep = score > threshold, in query order) and :161-205 (nms_3d):
// candidates sorted by descending score; a later candidate is suppressed by a kept one when
// (same class and 3D-AABB IoU > 0.25) or (nms_2d and 2D IoU > 0.5).  keep_idx receives query indices in kept order.
extern "C" int odam_detr_select(const float* rows, int Q, float threshold, int nms_2d, int* keep_idx, int* n_keep) {
    if (!rows || !keep_idx || !n_keep || Q < 0) return odam_fail(1, "odam_detr_select: bad argument");
    std::vector<int> cand;
    for (int q = 0; q < Q; q++)
        if (rows[(size_t)q * 16] > threshold) cand.push_back(q);
    std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return rows[(size_t)a * 16] < rows[(size_t)b * 16]; });
    std::reverse(cand.begin(), cand.end());
    const int n = (int)cand.size();
    std::vector<char> sup(n, 0);
    auto box3 = [&](int q, float lo[3], float hi[3]) {
        const float* r = rows + (size_t)q * 16;
        for (int k = 0; k < 3; k++) {
            lo[k] = (-r[10 + k]) / 2.0f + r[6 + k];
            hi[k] = r[10 + k] / 2.0f + r[6 + k];
        }
    };
    int nk = 0;
    for (int i = 0; i < n; i++) {
        if (sup[i]) continue;
        const int s = cand[i];
        keep_idx[nk++] = s;
        float slo[3], shi[3];
        box3(s, slo, shi);
        const float* rs = rows + (size_t)s * 16;
        for (int j = i + 1; j < n; j++) {
            if (sup[j]) continue;
            const int t = cand[j];
            const float* rt = rows + (size_t)t * 16;
            float tlo[3], thi[3];
            box3(t, tlo, thi);
            float inter = 1.0f, va = 1.0f, vb = 1.0f;
            {
                const float dx = std::max(0.0f, std::min(shi[0], thi[0]) - std::max(slo[0], tlo[0]));
                const float dy = std::max(0.0f, std::min(shi[1], thi[1]) - std::max(slo[1], tlo[1]));
                const float dz = std::max(0.0f, std::min(shi[2], thi[2]) - std::max(slo[2], tlo[2]));
                inter = dx * dy * dz;
                va = (shi[0] - slo[0]) * (shi[1] - slo[1]) * (shi[2] - slo[2]);
                vb = (thi[0] - tlo[0]) * (thi[1] - tlo[1]) * (thi[2] - tlo[2]);
            }
            const float iou3 = inter / (va + vb - inter);
            if (rt[1] == rs[1] && iou3 > 0.25f) { sup[j] = 1; continue; }
            if (nms_2d) {
                const float ix = std::max(0.0f, std::min(rs[4], rt[4]) - std::max(rs[2], rt[2]));
                const float iy = std::max(0.0f, std::min(rs[5], rt[5]) - std::max(rs[3], rt[3]));
                const float ia = ix * iy;
                const float aa = (rs[4] - rs[2]) * (rs[5] - rs[3]);
                const float ab = (rt[4] - rt[2]) * (rt[5] - rt[3]);
                if (ia / (aa + ab - ia) > 0.5f) sup[j] = 1;
            }
        }
    }
    *n_keep = nk;
    return 0;
}
