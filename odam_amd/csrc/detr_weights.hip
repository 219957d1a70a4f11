// detr_weights.hip -- the detector's model handle: creation, weight intake under the reference's state_dict names, packing for
// the kernels (k-major NHWC filters, FrozenBN folded to scale / bias, fused attention projections) and the workspace.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "detr_model.h"
#include "stem_u8_fold.h"

using namespace odam_dm;

namespace {

const HostTensor* find(odam_detr* m, const std::string& name) {
    auto it = m->host.find(name);
    return it == m->host.end() ? nullptr : &it->second;
}

#define NEED(var, name)                                                                    \
    const HostTensor* var = find(m, name);                                                 \
    if (!var) {                                                                            \
        std::snprintf(g_odam_err, sizeof(g_odam_err), "odam_detr_finalize: missing weight %s", std::string(name).c_str()); \
        return 1;                                                                          \
    }

int upload(odam_detr* m, float** p, const std::vector<float>& v) {
    if (int rc = m->dev_alloc(p, v.size())) return rc;
    ODAM_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
int upload_u16(odam_detr* m, void** p, const std::vector<unsigned short>& h) {
    unsigned short* d = nullptr;
    if (int rc = m->dev_alloc(&d, h.size())) return rc;
    ODAM_HIP(hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    *p = d;
    return 0;
}
// fp32 models: the exact three-way bf16 split of a packed filter [Cout][Kpad] for the split contraction mode
int upload_w3(odam_detr* m, void** p, const std::vector<float>& v, int Cout, int Kpad) {
    *p = nullptr;
    if (m->dt != 0 || Kpad % 16 != 0 || (long)Cout * Kpad * 6 >= 0x7fffffffL) return 0;
    std::vector<unsigned short> h((size_t)Cout * Kpad * 3);
    odam_cg::split3_filters(v.data(), Cout, Kpad, h.data());
    return upload_u16(m, p, h);
}
// weights in the model's element type: fp32 as is, bf16 rounded to nearest even on the host
int upload_w(odam_detr* m, void** p, const std::vector<float>& v) {
    if (m->dt == 0) return upload(m, (float**)p, v);
    std::vector<unsigned short> h(v.size());
    for (size_t i = 0; i < v.size(); i++) {
        unsigned u;
        std::memcpy(&u, &v[i], 4);
        if ((u & 0x7fffffffu) > 0x7f800000u) h[i] = (unsigned short)((u >> 16) | 0x40);  // NaN stays NaN
        else h[i] = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    return upload_u16(m, p, h);
}

// [Cout, Cin, KH, KW] (PyTorch) -> [Cout][Kpad], k = (ky*KW + kx)*CinP + ci, CinP = Cin rounded up to 4
int pack_conv(odam_detr* m, Conv& c, const HostTensor& w, int stride, int pad, int dil = 1) {
    const int Cout = (int)w.shape[0], Cin = (int)w.shape[1];
    const int KH = w.shape.size() > 2 ? (int)w.shape[2] : 1, KW = w.shape.size() > 3 ? (int)w.shape[3] : 1;
    const int epc = m->dt ? 8 : 4;             // elements per 16-byte chunk
    const int CinP = (Cin + epc - 1) / epc * epc;
    const int K = KH * KW * CinP;
    const int Kpad = (K + 8 * epc - 1) / (8 * epc) * (8 * epc);
    std::vector<float> p((size_t)Cout * Kpad, 0.0f);
    const int kt = 8 * epc, ntaps = KH * KW;
    const int k_order = (ntaps > 1 && ntaps <= 32 && CinP % kt == 0) ? 1 : 0;
    for (int o = 0; o < Cout; o++)
        for (int ci = 0; ci < Cin; ci++)
            for (int ky = 0; ky < KH; ky++)
                for (int kx = 0; kx < KW; kx++) {
                    const int tap = ky * KW + kx;
                    const int k = k_order ? ((ci / kt) * ntaps + tap) * kt + ci % kt : tap * CinP + ci;
                    p[(size_t)o * Kpad + k] = w.data[(((size_t)o * Cin + ci) * KH + ky) * KW + kx];
                }
    c.k_order = k_order;
    c.Cin = CinP; c.Cout = Cout; c.KH = KH; c.KW = KW; c.stride = stride; c.pad = pad; c.Kpad = Kpad; c.dil = dil;
    if (int rc = upload_w3(m, &c.w3, p, Cout, Kpad)) return rc;
    return upload_w(m, &c.w, p);
}

// mxfp8 body layer: [Cout, Cin, KH, KW] -> MXFP8 [Cout][Kpad = KH KW Cin], k = (ky KW + kx) Cin + ci, scales per 32 k (cg_mx8.h)
int pack_conv_mx(odam_detr* m, Conv& c, const HostTensor& w, int stride, int pad) {
    const int Cout = (int)w.shape[0], Cin = (int)w.shape[1];
    const int KH = w.shape.size() > 2 ? (int)w.shape[2] : 1, KW = w.shape.size() > 3 ? (int)w.shape[3] : 1;
    if (Cin % 64 || Cout % 32) return odam_fail(1, "odam_detr_finalize: mxfp8 body layers need Cin % 64 == 0 and Cout % 32 == 0");
    const int Kpad = KH * KW * Cin;
    std::vector<float> p((size_t)Cout * Kpad);
    for (int o = 0; o < Cout; o++)
        for (int ci = 0; ci < Cin; ci++)
            for (int ky = 0; ky < KH; ky++)
                for (int kx = 0; kx < KW; kx++)
                    p[(size_t)o * Kpad + (ky * KW + kx) * Cin + ci] = w.data[(((size_t)o * Cin + ci) * KH + ky) * KW + kx];
    std::vector<unsigned char> q(p.size()), qs(p.size() / 32);
    odam_mx::quantize_host(p.data(), p.size(), q.data(), qs.data());
    c.Cin = Cin; c.Cout = Cout; c.KH = KH; c.KW = KW; c.stride = stride; c.pad = pad; c.Kpad = Kpad; c.dil = 1; c.k_order = 0;
    RC(m->dev_alloc(&c.wq, q.size()));
    RC(m->dev_alloc(&c.wqs, qs.size()));
    ODAM_HIP(hipMemcpy(c.wq, q.data(), q.size(), hipMemcpyHostToDevice));
    ODAM_HIP(hipMemcpy(c.wqs, qs.data(), qs.size(), hipMemcpyHostToDevice));
    return 0;
}

// a body layer in the form the model's mode multiplies (mxfp8 models have no dilation: refused at create)
int pack_body(odam_detr* m, Conv& c, const HostTensor& w, int stride, int pad, int dil = 1) {
    return m->mx ? pack_conv_mx(m, c, w, stride, pad) : pack_conv(m, c, w, stride, pad, dil);
}

// rows [r0, r1) of a [N, K] Linear weight (+ bias) as a 1x1 layer
int pack_linear(odam_detr* m, Conv& c, const HostTensor& w, const HostTensor* b, int r0, int r1) {
    const int K = (int)w.shape[1];
    std::vector<float> p(w.data.begin() + (size_t)r0 * K, w.data.begin() + (size_t)r1 * K);
    c.Cin = K; c.Cout = r1 - r0; c.KH = c.KW = 1; c.stride = 1; c.pad = 0; c.Kpad = K;
    if (int rc = upload_w3(m, &c.w3, p, r1 - r0, K)) return rc;
    if (int rc = upload_w(m, &c.w, p)) return rc;
    if (b) {
        std::vector<float> bb(b->data.begin() + r0, b->data.begin() + r1);
        if (int rc = upload(m, &c.bias, bb)) return rc;
    }
    return 0;
}

// FrozenBatchNorm2d.forward (backbone.py:46-56): scale = w * rsqrt(rv + 1e-5); bias = b - rm * scale, in float32
int fold_bn(odam_detr* m, Conv& c, const std::string& prefix) {
    NEED(w, prefix + ".weight"); NEED(b, prefix + ".bias");
    NEED(rm, prefix + ".running_mean"); NEED(rv, prefix + ".running_var");
    const size_t n = w->data.size();
    std::vector<float> sc(n), bi(n);
    for (size_t i = 0; i < n; i++) {
        const float s = w->data[i] * (1.0f / std::sqrt(rv->data[i] + 1e-5f));
        sc[i] = s;
        bi[i] = b->data[i] - rm->data[i] * s;
    }
    if (int rc = upload(m, &c.scale, sc)) return rc;
    return upload(m, &c.bias, bi);
}

int pack_ln(odam_detr* m, LN& ln, const std::string& prefix) {
    NEED(w, prefix + ".weight"); NEED(b, prefix + ".bias");
    if (w->data.size() != (size_t)m->cfg.hidden_dim || b->data.size() != (size_t)m->cfg.hidden_dim) {
        std::snprintf(g_odam_err, sizeof(g_odam_err), "odam_detr_finalize: %s must have hidden_dim = %d entries", prefix.c_str(),
                      m->cfg.hidden_dim);
        return 1;
    }
    if (int rc = upload(m, &ln.g, w->data)) return rc;
    return upload(m, &ln.b, b->data);
}

// nn.MultiheadAttention's packed projection of a hidden_dim-wide model: weight [3 E, E], bias [3 E]
int check_in_proj(const HostTensor& w, const HostTensor& b, int E, const std::string& name) {
    if (w.shape.size() == 2 && w.shape[0] == 3LL * E && w.shape[1] == E && b.data.size() == 3 * (size_t)E) return 0;
    std::snprintf(g_odam_err, sizeof(g_odam_err), "odam_detr_finalize: %s.in_proj_weight must be [%d, %d] (hidden_dim %d)", name.c_str(),
                  3 * E, E, E);
    return 1;
}

// a filter of the BasicBlock plan has the shape that plan reads ([Cout, Cin, k, k]): a Bottleneck checkpoint under a BasicBlock
// configuration fails here, by name, instead of being read out of bounds
int check_shape(const HostTensor& w, int cout, int cin, int k, const std::string& name) {
    if (w.shape.size() == 4 && w.shape[0] == cout && w.shape[1] == cin && w.shape[2] == k && w.shape[3] == k) return 0;
    std::snprintf(g_odam_err, sizeof(g_odam_err), "odam_detr_finalize: %s must be [%d, %d, %d, %d] for this backbone", name.c_str(),
                  cout, cin, k, k);
    return 1;
}

}  // namespace

namespace odam_dm {

// conv1 as KH = 7, KW = 1, Cin = 32: filter row ky of output channel o is the 28 values w[o][c][ky][kx] at position 4 kx + c (what 7
// consecutive NHWC4 pixels hold), then 4 zeros; K = 7 * 32 = 224.  fp32: k_order 1 (one 32-channel chunk); bf16: the k-tile is 32
// elements = one filter row, tap-major (k_order 0).  Keeps w for the filters of the uint8 stem (stem_u8_filters)
int pack_stem_rows(odam_detr* m, const float* w, int Cout, float* scale, float* bias) {
    const int Kp = m->dt ? 256 : 224;          // bf16: the dispatcher's k-tile is 64 elements (an eighth, all-zero filter row)
    std::vector<float> pr((size_t)Cout * Kp, 0.0f);
    for (int o = 0; o < Cout; o++)
        for (int ci = 0; ci < 3; ci++)
            for (int ky = 0; ky < 7; ky++)
                for (int kx = 0; kx < 7; kx++)
                    pr[(size_t)o * Kp + ky * 32 + kx * 4 + ci] = w[(((size_t)o * 3 + ci) * 7 + ky) * 7 + kx];
    Conv& r = m->stem_rows;
    r.Cin = 32; r.Cout = Cout; r.KH = 7; r.KW = 1; r.stride = 2; r.pad = 0; r.Kpad = Kp; r.k_order = m->dt ? 0 : 1;
    RC(upload_w3(m, &r.w3, pr, Cout, Kp));
    RC(upload_w(m, &r.w, pr));
    r.scale = scale; r.bias = bias;
    if (m->dt == 0) m->conv1_w.assign(w, w + (size_t)Cout * 147);
    return 0;
}

// conv1's filters for the centred uint8 frame (stem_u8_fold.h), split into the three bf16 planes of the split contraction mode:
// built on first use for a (mean, std) pair and kept on the model, as the resampling tables are
int stem_u8_filters(odam_detr* m, const float* mean, const float* stdv, const odam_detr::StemU8** out) {
    for (const odam_detr::StemU8& f : m->stem_u8)
        if (std::memcmp(f.mean, mean, 12) == 0 && std::memcmp(f.stdv, stdv, 12) == 0) { *out = &f; return 0; }
    const int Cout = m->stem_rows.Cout;
    if (m->conv1_w.size() != (size_t)Cout * 147 || m->stem_rows.Kpad != 224) return odam_fail(1, "stem_u8_filters: no fp32 conv1 filters on this model");
    odam_detr::StemU8 f{};
    std::memcpy(f.mean, mean, 12); std::memcpy(f.stdv, stdv, 12);
    stem_u8_centres(mean, f.centre);
    std::vector<float> rows((size_t)Cout * 224);
    stem_u8_fold(m->conv1_w.data(), Cout, mean, stdv, rows.data());
    RC(upload_w3(m, &f.w3, rows, Cout, 224));
    if (!f.w3) return odam_fail(1, "stem_u8_filters: the split filters could not be built");
    m->stem_u8.push_back(f);      // (the pointer handed out serves the one call that asked: a later pair may move the entries)
    *out = &m->stem_u8.back();
    return 0;
}

}  // namespace odam_dm

extern "C" int odam_detr_create(const odam_detr_cfg* cfg, odam_detr** out) {
    if (!cfg || !out) return odam_fail(1, "odam_detr_create: null argument");
    // transformer widths: the attention kernels take head dim 32 or 64, the LayerNorm kernels 64 n channels, n = 2 .. 16
    if (cfg->hidden_dim % 64 || cfg->hidden_dim < 128 || cfg->hidden_dim > 1024)
        return odam_fail(3, "odam_detr_create: hidden_dim must be a multiple of 64 in 128 .. 1024");
    if (cfg->nheads < 1 || cfg->hidden_dim % cfg->nheads)
        return odam_fail(3, "odam_detr_create: hidden_dim must be a multiple of nheads");
    if (cfg->hidden_dim / cfg->nheads != 32 && cfg->hidden_dim / cfg->nheads != 64)
        return odam_fail(3, "odam_detr_create: head dim hidden_dim / nheads must be 32 or 64 (16 and 128 are not built)");
    if (cfg->max_batch < 1 || cfg->img_h < 32 || cfg->img_w < 32) return odam_fail(1, "odam_detr_create: bad sizes");
    if (cfg->dtype < 0 || cfg->dtype > 2) return odam_fail(1, "odam_detr_create: dtype must be 0 (fp32), 1 (bf16) or 2 (mxfp8)");
    if (cfg->dtype == 2 && cfg->dilation)
        return odam_fail(3, "odam_detr_create: dilation (DC5) is not supported in the mxfp8 mode (dtype 2)");
    if (cfg->basic_block != 0 && cfg->basic_block != 1) return odam_fail(1, "odam_detr_create: basic_block must be 0 (Bottleneck) or 1 (BasicBlock)");
    if (cfg->basic_block && cfg->dilation)      // torchvision BasicBlock: "Dilation > 1 not supported in BasicBlock"
        return odam_fail(3, "odam_detr_create: dilation (DC5) is not supported with BasicBlock backbones (resnet18 / resnet34)");
    for (int l = 0; l < 4; l++)
        if (cfg->resnet_blocks[l] < 1) return odam_fail(1, "odam_detr_create: every ResNet stage needs at least one block");
    odam_detr* m = new odam_detr();
    m->cfg = *cfg;
    m->basic = cfg->basic_block != 0;
    m->mx = cfg->dtype == 2;
    m->dt = cfg->dtype ? 1 : 0;
    m->es = cfg->dtype ? 2 : 4;
    m->H1 = conv_out(cfg->img_h, 7, 2, 3); m->W1 = conv_out(cfg->img_w, 7, 2, 3);
    m->H2 = conv_out(m->H1, 3, 2, 1); m->W2 = conv_out(m->W1, 3, 2, 1);
    int h = m->H2, w = m->W2;
    for (int l = 1; l < (cfg->dilation ? 3 : 4); l++) { h = conv_out(h, 3, 2, 1); w = conv_out(w, 3, 2, 1); }      // dilation: layer4 keeps layer3's resolution
    m->fh = h; m->fw = w; m->L = h * w;
    *out = m;
    return 0;
}

extern "C" int odam_detr_destroy(odam_detr* m) {
    if (!m) return 0;
    for (void* p : m->allocs) (void)hipFree(p);
    for (hipEvent_t e : m->conv_ev.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : m->att_ev.ev) (void)hipEventDestroy(e);
    delete m;
    return 0;
}

extern "C" int odam_detr_feature_hw(const odam_detr* m, int* h, int* w) {
    if (!m || !h || !w) return odam_fail(1, "odam_detr_feature_hw: null argument");
    *h = m->fh; *w = m->fw;
    return 0;
}

extern "C" int odam_detr_set_weight(odam_detr* m, const char* name, const float* data, const long long* shape,
                                    int ndim) {
    if (!m || !name || !data || (!shape && ndim > 0) || ndim < 0 || ndim > 4)
        return odam_fail(1, "odam_detr_set_weight: bad argument");
    if (m->finalized) return odam_fail(1, "odam_detr_set_weight: model already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; i++) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    m->host[name] = std::move(t);
    return 0;
}

extern "C" int odam_detr_finalize(odam_detr* m) {
    if (!m) return odam_fail(1, "odam_detr_finalize: null model");
    if (m->finalized) return 0;
    const odam_detr_cfg& c = m->cfg;
    const std::string bb = "backbone.0.body.";
    {   // stem
        NEED(w, bb + "conv1.weight");
        RC(pack_conv(m, m->stem, *w, 2, 3));
        RC(fold_bn(m, m->stem, bb + "bn1"));
        if (w->shape.size() != 4 || w->shape[1] != 3 || w->shape[2] != 7 || w->shape[3] != 7)
            return odam_fail(1, "odam_detr_finalize: backbone.0.body.conv1.weight must be [Cout, 3, 7, 7]");
        RC(pack_stem_rows(m, w->data.data(), (int)w->shape[0], m->stem.scale, m->stem.bias));
    }
    int inplanes = 64;
    for (int l = 0; l < 4; l++) {
        for (int i = 0; i < c.resnet_blocks[l]; i++) {
            const std::string p = bb + "layer" + std::to_string(l + 1) + "." + std::to_string(i) + ".";
            if (m->basic) {
                // torchvision BasicBlock (expansion 1): conv1 3x3 / stride, pad 1 -> bn1 -> ReLU; conv2 3x3, pad 1 -> bn2 -> + identity
                // (or the 1x1 / stride downsample where the stride or the width changes: layer2.0, layer3.0, layer4.0) -> ReLU
                const int planes = 64 << l, stride = (i == 0 && l > 0) ? 2 : 1;
                const bool ds = stride != 1 || inplanes != planes;
                Bottleneck b;
                NEED(w1, p + "conv1.weight"); NEED(w2, p + "conv2.weight");
                RC(check_shape(*w1, planes, inplanes, 3, p + "conv1.weight"));
                RC(check_shape(*w2, planes, planes, 3, p + "conv2.weight"));
                RC(pack_body(m, b.c1, *w1, stride, 1)); RC(fold_bn(m, b.c1, p + "bn1"));
                RC(pack_body(m, b.c2, *w2, 1, 1)); RC(fold_bn(m, b.c2, p + "bn2"));
                if (ds) {
                    NEED(wd, p + "downsample.0.weight");
                    RC(check_shape(*wd, planes, inplanes, 1, p + "downsample.0.weight"));
                    RC(pack_body(m, b.ds, *wd, stride, 0)); RC(fold_bn(m, b.ds, p + "downsample.1"));
                    b.has_ds = true;
                }
                m->blocks.push_back(b);
                m->block_stride.push_back(stride);
                inplanes = planes;
                continue;
            }
            // `dilation` (backbone.py:89-91 -> torchvision replace_stride_with_dilation = [False, False, True]): layer4's stride
            // becomes a dilation -- its first block runs with stride 1 and the PREVIOUS dilation (1), the others with dilation 2
            // and padding 2 (torchvision ResNet._make_layer: previous_dilation for block 0, self.dilation *= stride after it)
            const bool dc5 = c.dilation && l == 3;
            const int stride = (i == 0 && l > 0 && !dc5) ? 2 : 1;
            const int dil = (dc5 && i > 0) ? 2 : 1;
            Bottleneck b;
            NEED(w1, p + "conv1.weight"); NEED(w2, p + "conv2.weight"); NEED(w3, p + "conv3.weight");
            RC(pack_body(m, b.c1, *w1, 1, 0));
            RC(pack_body(m, b.c2, *w2, stride, dil, dil));    // v1.5: stride on the 3x3
            RC(pack_body(m, b.c3, *w3, 1, 0));
            RC(fold_bn(m, b.c1, p + "bn1")); RC(fold_bn(m, b.c2, p + "bn2")); RC(fold_bn(m, b.c3, p + "bn3"));
            if (i == 0) {
                NEED(wd, p + "downsample.0.weight");
                RC(pack_body(m, b.ds, *wd, stride, 0)); RC(fold_bn(m, b.ds, p + "downsample.1"));
                b.has_ds = true;
            }
            m->blocks.push_back(b);
            m->block_stride.push_back(stride);
        }
    }
    m->l4_ch = m->basic ? m->blocks.back().c2.Cout : m->blocks.back().c3.Cout;
    {
        NEED(w, "input_proj.weight"); NEED(b, "input_proj.bias");
        if (w->shape.size() != 4 || (int)w->shape[1] != m->l4_ch) {
            std::snprintf(g_odam_err, sizeof(g_odam_err), "odam_detr_finalize: input_proj.weight must read the layer4 map (%d channels for "
                          "this backbone)", m->l4_ch);
            return 1;
        }
        RC(pack_conv(m, m->input_proj, *w, 1, 0));
        RC(upload(m, &m->input_proj.bias, b->data));
    }
    const int E = c.hidden_dim;
    for (int i = 0; i < c.enc_layers; i++) {
        const std::string p = "transformer.encoder.layers." + std::to_string(i) + ".";
        EncLayer e;
        NEED(ipw, p + "self_attn.in_proj_weight"); NEED(ipb, p + "self_attn.in_proj_bias");
        RC(check_in_proj(*ipw, *ipb, E, p + "self_attn"));
        RC(pack_linear(m, e.qk, *ipw, ipb, 0, 2 * E));
        RC(pack_linear(m, e.v, *ipw, ipb, 2 * E, 3 * E));
        NEED(ow, p + "self_attn.out_proj.weight"); NEED(ob, p + "self_attn.out_proj.bias");
        RC(pack_linear(m, e.out, *ow, ob, 0, E));
        NEED(w1, p + "linear1.weight"); NEED(b1, p + "linear1.bias");
        NEED(w2, p + "linear2.weight"); NEED(b2, p + "linear2.bias");
        RC(pack_linear(m, e.l1, *w1, b1, 0, c.dim_feedforward));
        RC(pack_linear(m, e.l2, *w2, b2, 0, E));
        RC(pack_ln(m, e.n1, p + "norm1")); RC(pack_ln(m, e.n2, p + "norm2"));
        m->enc.push_back(e);
    }
    // decoder; the cross-attention key/value projections of all layers read the same (memory + pos) / memory,
    // so their weights are stacked into two [dec_layers*E, E] layers evaluated once per forward
    HostTensor kall, vall, kball, vball;
    kall.shape = {(long long)c.dec_layers * E, E}; vall.shape = kall.shape;
    for (int i = 0; i < c.dec_layers; i++) {
        const std::string p = "transformer.decoder.layers." + std::to_string(i) + ".";
        DecLayer d;
        NEED(ipw, p + "self_attn.in_proj_weight"); NEED(ipb, p + "self_attn.in_proj_bias");
        RC(check_in_proj(*ipw, *ipb, E, p + "self_attn"));
        RC(pack_linear(m, d.qk, *ipw, ipb, 0, 2 * E));
        RC(pack_linear(m, d.v, *ipw, ipb, 2 * E, 3 * E));
        NEED(ow, p + "self_attn.out_proj.weight"); NEED(ob, p + "self_attn.out_proj.bias");
        RC(pack_linear(m, d.out, *ow, ob, 0, E));
        NEED(cw, p + "multihead_attn.in_proj_weight"); NEED(cb, p + "multihead_attn.in_proj_bias");
        RC(check_in_proj(*cw, *cb, E, p + "multihead_attn"));
        RC(pack_linear(m, d.cq, *cw, cb, 0, E));
        kall.data.insert(kall.data.end(), cw->data.begin() + (size_t)E * E, cw->data.begin() + (size_t)2 * E * E);
        vall.data.insert(vall.data.end(), cw->data.begin() + (size_t)2 * E * E, cw->data.begin() + (size_t)3 * E * E);
        kball.data.insert(kball.data.end(), cb->data.begin() + E, cb->data.begin() + 2 * E);
        vball.data.insert(vball.data.end(), cb->data.begin() + 2 * E, cb->data.begin() + 3 * E);
        NEED(cow, p + "multihead_attn.out_proj.weight"); NEED(cob, p + "multihead_attn.out_proj.bias");
        RC(pack_linear(m, d.cout, *cow, cob, 0, E));
        NEED(w1, p + "linear1.weight"); NEED(b1, p + "linear1.bias");
        NEED(w2, p + "linear2.weight"); NEED(b2, p + "linear2.bias");
        RC(pack_linear(m, d.l1, *w1, b1, 0, c.dim_feedforward));
        RC(pack_linear(m, d.l2, *w2, b2, 0, E));
        RC(pack_ln(m, d.n1, p + "norm1")); RC(pack_ln(m, d.n2, p + "norm2")); RC(pack_ln(m, d.n3, p + "norm3"));
        m->dec.push_back(d);
    }
    kball.shape = {(long long)c.dec_layers * E}; vball.shape = kball.shape;
    RC(pack_linear(m, m->cross_k_all, kall, &kball, 0, c.dec_layers * E));
    RC(pack_linear(m, m->cross_v_all, vall, &vball, 0, c.dec_layers * E));
    RC(pack_ln(m, m->dec_norm, "transformer.decoder.norm"));
    if (c.pre_norm) RC(pack_ln(m, m->enc_norm, "transformer.encoder.norm"));
    {
        NEED(w, "class_embed.weight"); NEED(b, "class_embed.bias");
        RC(pack_linear(m, m->class_embed, *w, b, 0, (int)w->shape[0]));
        const char* names[5] = {"bbox_embed", "offset_embed", "angle_embed", "size_embed", "depth_embed"};
        for (int k = 0; k < 5; k++)
            for (int j = 0; j < 3; j++) {
                const std::string p = std::string(names[k]) + ".layers." + std::to_string(j);
                NEED(lw, p + ".weight"); NEED(lb, p + ".bias");
                RC(pack_linear(m, m->mlp[k][j], *lw, lb, 0, (int)lw->shape[0]));
            }
        NEED(q, "query_embed.weight");
        if (q->data.size() != (size_t)c.num_queries * E) return odam_fail(1, "query_embed.weight must be [num_queries, hidden_dim]");
        RC(upload(m, &m->query_pos, q->data));
        NEED(pe, "pos_embed");
        if ((int)pe->shape[0] != m->L || (int)pe->shape[1] != E) return odam_fail(1, "pos_embed must be [h*w, hidden_dim]");
        RC(upload(m, &m->pos, pe->data));
    }
    // workspace (bytes = elements * es)
    const size_t B = c.max_batch, es = m->es;
    size_t big = B * m->H2 * m->W2 * 256 * es, tsz = big / 2;
    if (m->basic) {
        // BasicBlock: every tensor of a stage (block output, conv1 output, downsample) has that stage's width at its resolution;
        // the largest over the stages (and the pooled stem, 64 channels = layer1's) sizes all of them
        size_t mx = B * m->H2 * m->W2 * 64;
        int h = m->H2, w = m->W2;
        for (int l = 1; l < 4; l++) {
            h = conv_out(h, 3, 2, 1); w = conv_out(w, 3, 2, 1);
            mx = std::max(mx, B * h * w * (size_t)(64 << l));
        }
        big = tsz = mx * es;
    }
    RC(m->dev_alloc(&m->x4, B * (c.img_h + 6) * (c.img_w + 8) * (m->dt ? 8 : 4) * es));     // room for the framed fp32 image
    RC(m->dev_alloc(&m->stem_out, B * m->H1 * m->W1 * 64 * es));
    RC(m->dev_alloc(&m->bufA, big)); RC(m->dev_alloc(&m->bufB, big)); RC(m->dev_alloc(&m->dsb, big));
    RC(m->dev_alloc(&m->t1, tsz)); RC(m->dev_alloc(&m->t2, tsz));
    if (m->mx) {        // element counts: big / es (block inputs / outputs), tsz / es (reduce / 3x3 outputs); one scale per 32
        RC(m->dev_alloc(&m->qa, big / es)); RC(m->dev_alloc(&m->qb, big / es));
        RC(m->dev_alloc(&m->qas, big / es / 32)); RC(m->dev_alloc(&m->qbs, big / es / 32));
        RC(m->dev_alloc(&m->qt1, tsz / es)); RC(m->dev_alloc(&m->qt2, tsz / es));
        RC(m->dev_alloc(&m->qt1s, tsz / es / 32)); RC(m->dev_alloc(&m->qt2s, tsz / es / 32));
    }
    const size_t M = B * m->L, Mq = B * c.num_queries, F = c.dim_feedforward;
    RC(m->dev_alloc(&m->src, M * E * es)); RC(m->dev_alloc(&m->srcpos, M * E * es)); RC(m->dev_alloc(&m->qk, M * 2 * E * es));
    RC(m->dev_alloc(&m->v, M * E * es)); RC(m->dev_alloc(&m->att, M * E * es)); RC(m->dev_alloc(&m->tmp, M * E * es));
    RC(m->dev_alloc(&m->ffn, M * F * es));
    RC(m->dev_alloc(&m->kc, M * c.dec_layers * E * es)); RC(m->dev_alloc(&m->vc, M * c.dec_layers * E * es));
    RC(m->dev_alloc(&m->tgt, Mq * E * es)); RC(m->dev_alloc(&m->tgtpos, Mq * E * es)); RC(m->dev_alloc(&m->dqk, Mq * 2 * E * es));
    RC(m->dev_alloc(&m->dv, Mq * E * es)); RC(m->dev_alloc(&m->datt, Mq * E * es)); RC(m->dev_alloc(&m->dq, Mq * E * es));
    RC(m->dev_alloc(&m->dtmp, Mq * E * es)); RC(m->dev_alloc(&m->dffn, Mq * F * es)); RC(m->dev_alloc(&m->hs, Mq * E * es));
    RC(m->dev_alloc(&m->h1, Mq * E * es)); RC(m->dev_alloc(&m->h2, Mq * E * es));
    m->host.clear();
    m->finalized = true;
    return 0;
}
