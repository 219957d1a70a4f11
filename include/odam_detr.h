/*
 * odam_detr.h -- C ABI of the MI355X (gfx950) DETR-style monocular 3D detector forward pass.
 *
 * Drop-in boundary for the reference's (likojack/ODAM) detector as OdamProcess.run_detector uses it
 * (src/processor.py:259-289):
 *   src/models/detr.py:49-94      DETR.forward        -> odam_detr_forward
 *   src/models/detr.py:96-140     DETR.postprocess    -> odam_detr_postprocess (arithmetic per query;
 *                                 thresholding + greedy nms_3d :161-205 stay on the host: odam_detr_select -- or run on
 *                                 the device with the rows of run_detector behind them: odam_detr_select_pack)
 *   src/models/backbone.py:21-94  FrozenBatchNorm2d + torchvision ResNet-50/101 body
 *   src/models/transformer.py     6+6 post-norm encoder/decoder, nn.MultiheadAttention(256, 8)
 *   run_processor.py:32-33        load_state_dict      -> odam_detr_set_weight per state_dict entry,
 *                                 with the reference's key names
 *
 * Conventions as in odam_sq.h: int return codes (0 = OK), odam_last_error(), [dev]/[host] pointers,
 * caller's hipStream_t passed as void*, no allocation or synchronisation inside forward/postprocess
 * (the workspace is allocated by odam_detr_create for max_batch frames of img_h x img_w).
 */
#ifndef ODAM_DETR_H
#define ODAM_DETR_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct odam_detr odam_detr;

typedef struct {
    int resnet_blocks[4];  /* blocks per stage (backbone.py:90): Bottleneck {3,4,6,3} = resnet50, {3,4,23,3} = resnet101,
                              {3,8,36,3} = resnet152; BasicBlock (basic_block = 1) {2,2,2,2} = resnet18, {3,4,6,3} = resnet34 */
    int hidden_dim;        /* 256  (configs/detr_scan_net.yaml); a multiple of 64 in 128 .. 1024 */
    int nheads;            /* 8    hidden_dim % nheads == 0 and head dim hidden_dim / nheads 32 or 64 (else
                              odam_detr_create returns 3) */
    int dim_feedforward;   /* 2048 */
    int enc_layers;        /* 6 */
    int dec_layers;        /* 6 */
    int num_queries;       /* 100 */
    int num_classes1;      /* 18 + 1 "no object" (detr.py:531-532) */
    int angle_bins;        /* 30 */
    int max_batch;         /* frames per forward call */
    int img_h, img_w;      /* network input size, e.g. 800 x 1066 for a 640x480 frame (transforms.py:78-96) */
    int dtype;             /* 0: fp32 everywhere (parity mode).  1: bf16 weights + activations in memory, bf16 MFMA
                              with fp32 accumulation, fp32 softmax / LayerNorm / head outputs (BASELINE config 4).
                              2: mxfp8 -- every convolution of the ResNet body on MXFP8 operands (below) with fp32 accumulation
                              on v_mfma_scale_f32_32x32x64_f8f6f4; the stem, input_proj, the transformer and the heads exactly as
                              in 1.  Refused together with `dilation` */
    int pre_norm;          /* 0: post-norm layers (the shipped configuration).  1: `normalize_before` -- every encoder / decoder
                              sub-block normalises its input and adds its output to the stream, the encoder ends in its own
                              LayerNorm "transformer.encoder.norm.*" (src/models/transformer.py:169-188, 240-262, 26-28) */
    int dilation;          /* 1: the DC5 backbone (src/models/backbone.py:89-91): layer4 keeps layer3's resolution -- stride 1, its
                              3x3 filters dilated by 2 from the second block on -- so the token grid is ceil(H/16) x ceil(W/16) */
    int basic_block;       /* 0: torchvision Bottleneck (1x1 reduce, 3x3, 1x1 expand; layer4 has 2048 channels).  1: torchvision
                              BasicBlock (resnet18 / resnet34: 3x3 with the stage's stride, 3x3 + identity or 1x1 downsample; layer4
                              has 512 channels).  BasicBlock with `dilation` is refused, as torchvision refuses it */
} odam_detr_cfg;

int odam_detr_create(const odam_detr_cfg* cfg, odam_detr** out);
int odam_detr_destroy(odam_detr* m);

/* One call per state_dict entry, `name` = the reference's key (e.g.
 * "backbone.0.body.layer1.0.conv1.weight", "transformer.encoder.layers.0.self_attn.in_proj_weight",
 * "class_embed.bias"); data [host] float32, contiguous, PyTorch layout.  Unknown names are ignored
 * (e.g. "...num_batches_tracked", as FrozenBatchNorm2d._load_from_state_dict does, backbone.py:36-44).
 * The sine position embedding of the token grid is passed under the name "pos_embed"
 * ([h*w, hidden_dim], position_encoding.py:26-46 -- a constant of the input size). */
int odam_detr_set_weight(odam_detr* m, const char* name, const float* data, const long long* shape, int ndim);

/* Packs weights for the kernels (NHWC k-major filters, FrozenBN folded to scale/bias exactly as
 * backbone.py:46-56 computes them, fused attention projections); fails if any tensor is missing. */
int odam_detr_finalize(odam_detr* m);

/* token grid of the configured input: h = ceil(img_h/32), w = ceil(img_w/32) */
int odam_detr_feature_hw(const odam_detr* m, int* h, int* w);

/*
 * img [dev] [B,3,img_h,img_w] float32 (normalised, as get_transforms() produces).
 * Outputs [dev], the last decoder layer's predictions (detr.py:80-88):
 *   logits [B,Q,num_classes1], boxes [B,Q,4] (sigmoid applied), angle [B,Q,angle_bins], offset [B,Q,2],
 *   size [B,Q,3], depth [B,Q,1], obj_features [B,Q,hidden] (nullable).
 */
int odam_detr_forward(odam_detr* m, const float* img, int B, float* logits, float* boxes, float* angle,
                      float* offset, float* size, float* depth, float* obj_features, void* stream);

/*
 * The same forward over a batch of images of DIFFERENT sizes, zero-padded to the handle's img_h x img_w at the top-left
 * as nested_tensor_from_tensor_list does (src/utils/misc.py:303-320):
 *   key_mask [dev] [B][h*w] bytes, 1 = token lies in the padding (the image mask reduced to the feature grid by nearest
 *            interpolation, backbone.py:79) -- such keys are excluded in encoder self-attention and decoder
 *            cross-attention (key_padding_mask, transformer.py:157-160, 224-228);
 *   pos      [dev] [B][h*w][hidden] float32: each image's own sine embedding (position_encoding.py:26-46 depends on the
 *            mask through the cumulative sums and their normalisation).
 * odam_amd/detector.py::Detector.forward_nested builds both exactly as the reference does.
 */
int odam_detr_forward_masked(odam_detr* m, const float* img, int B, const unsigned char* key_mask, const float* pos,
                             float* logits, float* boxes, float* angle, float* offset, float* size, float* depth,
                             float* obj_features, void* stream);

/*
 * The forward with the predictions of EVERY decoder layer (DETR.forward with aux_loss, detr.py:70-93, 238-253): after each
 * decoder layer the decoder's final norm (transformer.py:117-127, in both pre_norm settings) and the six heads, on the same
 * B * Q rows and with the same launches as the plain forward.  L = cfg.dec_layers.
 *   key_mask, pos      as odam_detr_forward_masked, or both null for a same-size batch (odam_detr_forward)
 *   frames_per_layer   >= B: every output pointer (obj_features nullable) addresses a block [L][frames_per_layer][Q][.], and
 *                      layer l of frame b is written at (l * frames_per_layer + b) * Q * n -- a caller that splits a batch over
 *                      max_batch passes the block's address advanced by its first frame and the frames of the whole block
 *   Slot L-1 is the last layer: the bits odam_detr_forward / odam_detr_forward_masked write for the same input, in every dtype
 *   mode.  Slots 0 .. L-2 are the reference's aux_outputs[0 .. L-2].
 * A null pointer, a mask without a position table (or the reverse), a handle that is not finalised and frames_per_layer < B
 * return 1 before anything is launched.  No workspace beyond the plain forward's.
 */
int odam_detr_forward_aux(odam_detr* m, const float* img, int B, const unsigned char* key_mask, const float* pos,
                          float* logits, float* boxes, float* angle, float* offset, float* size, float* depth,
                          float* obj_features, int frames_per_layer, void* stream);

/* optional taps for parity tests: layer4 feature map as NCHW [B,C4,h,w] (C4 = 2048 Bottleneck, 512 BasicBlock) and encoder memory [B,h*w,hidden]
 * of the most recent forward (either may be null) */
int odam_detr_debug_read(odam_detr* m, int B, float* layer4_nchw, float* memory, void* stream);

/*
 * Per-query post-processing arithmetic (detr.py:111-140) on device:
 * rows [dev] [B,Q,16] = score, class, x0,y0,x1,y1 (pixels of img_w x img_h), cx3d, cy3d, depth,
 *                       angle_bin, d0,d1,d2, 0,0,0.   K9 [host] row-major 3x3 intrinsics.
 */
int odam_detr_postprocess(odam_detr* m, const float* logits, const float* boxes, const float* angle,
                          const float* offset, const float* size, const float* depth, int B, const float* K9,
                          float img_w, float img_h, float* rows, void* stream);

/* Threshold + greedy nms_3d (detr.py:124-125, 161-205) on ONE frame's rows [host][Q,16] as written by
 * odam_detr_postprocess; keep_idx [host][Q] receives the kept query indices in descending-score order. */
int odam_detr_select(const float* rows, int Q, float threshold, int nms_2d, int* keep_idx, int* n_keep);

/*
 * The same step for B frames on the device, with the rows of run_detector behind it (detr.py:124-125, 161-205;
 * src/processor.py:269-288, 318-319): what odam_detr_select, then odam_amd/processor.py::detection_array, then
 * odam_amd/parallel.py::pack_detections compute on the host, bit for bit, in one launch of one wavefront per frame
 * (odam_amd/csrc/det_select.hip).  Stream-ordered; allocates nothing, synchronises nothing.
 *   rows16     [dev][B][Q][16] as written by odam_detr_postprocess, 16-byte aligned; Q <= 256, else ODAM_E_LIMIT (3)
 *   frame_ids  [dev][B] the frame ids as float32 (column 0 of the rows)
 *   seq_w/h    the sequence's image size: columns 2-5 are the pixel box divided by it in float32
 *   sincos     [dev][n_bins][2] float32 sine and cosine of each angle bin, computed by the caller the way the host path
 *              computes them (odam_amd/detector.py::sincos_table); a bin outside 0 .. n_bins-1 (odam_detr_postprocess
 *              writes none) gives NaN in columns 12, 13
 *   det_block  [dev][B][30][15] float32: frame id, class, box / (seq_w, seq_h), dimensions, translate, sin, cos, score of
 *              the first 30 kept detections in kept order; unused slots hold -1
 *   det_count  [dev][B] detections kept (<= 30)
 *   keep_idx   [dev][B][30] their query indices, -1 in unused slots (nullable)
 */
int odam_detr_select_pack(const float* rows16, int B, int Q, float threshold, int nms_2d, const float* frame_ids,
                          float seq_w, float seq_h, const float* sincos, int n_bins, float* det_block, int* det_count,
                          int* keep_idx, void* stream);

/* The detector's input transform on the device (reference: src/datasets/transforms.py:281-290 = resize :75-105 via
 * torchvision F.resize -> PIL Image.resize(BILINEAR), ToTensor :222-224, Normalize :236-243; called per frame from
 * src/processor.py:263): rgb [dev][B,h,w,3] uint8 -> out [dev][B,3,img_h,img_w] float32 at the handle's size,
 * bit-identical to the host transform (Pillow's two-pass 22-bit fixed-point resampling, then float32 /255, -mean, /std).
 * mean, std: host float[3].  The resampling tables of each (h, w) are built and uploaded at first use (synchronous). */
int odam_detr_preprocess_u8(odam_detr* m, const unsigned char* rgb, int B, int h, int w, const float* mean,
                            const float* std_dev, float* out, void* stream);

/* Input transform + odam_detr_forward in one call: rgb [dev][B,h,w,3] uint8 as odam_detr_preprocess_u8 takes it, the outputs as
 * odam_detr_forward writes them.  For an fp32 model in split mode whose conv1 runs as the row convolution (odam_config stem.rows) and whose
 * framed row pitch img_w + 8 is even, with odam_config stem.u8 = 1 (default): the resize writes the frame as centred integers in one bf16
 * plane and conv1 reads that with the normalisation folded into its filters -- no fp32 image, no layout pass, three products per block
 * instead of six with none dropped; the result differs from the two-call path in the last bits.  Everywhere else (bf16 / mxfp8
 * models, cg.f32 = 0, stem.rows = 0, stem.u8 = 0, an odd pitch) the normalised image goes to a scratch of the handle's and the forward runs on
 * it: the bits of odam_detr_preprocess_u8 + odam_detr_forward.  A caller never has to know which ran. */
int odam_detr_forward_u8(odam_detr* m, const unsigned char* rgb, int B, int h, int w, const float* mean, const float* std_dev,
                         float* logits, float* boxes, float* angle, float* offset, float* size, float* depth, float* obj_features,
                         void* stream);

/* Per-launch timing of the contraction kernel (all conv / linear launches of a forward are bracketed by
 * event pairs while enabled); read returns the totals of the most recent forward. */
int odam_detr_profile_enable(odam_detr* m, int on);
int odam_detr_profile_read(odam_detr* m, int* n_launches, double* total_ms, double* total_flops);
int odam_detr_profile_read_attention(odam_detr* m, int* n_launches, double* total_ms, double* total_flops);

/*
 * MXFP8 (dtype 2): OCP MX v1.0 with these choices fixed --
 *   elements  e4m3fn (the OCP encoding, not MI300's fnuz), converted round-to-nearest-even with subnormals kept;
 *   scales    one E8M0 byte (2^(s - 127)) per block of 32 values: 32 consecutive channels of one NHWC pixel for activations,
 *             32 consecutive k of one output channel for filters (k = (ky KW + kx) Cin + ci).  A tensor [rows][C] is elements
 *             [rows][C] + scales [rows][C / 32]: the scale of element i is scale[i / 32];
 *   rule      e = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127]; an all-zero block gets -127.  Elements are
 *             x * 2^-e (exact) rounded to e4m3fn, so none saturates (the OCP default floor(log2 amax) - 8 would clip up to one
 *             binade of the block maximum).  A block holding a NaN or an Inf is outside the contract: its scale byte is 0xFF
 *             (the E8M0 NaN), so it dequantizes -- and multiplies -- to NaN; its element bytes are not specified.
 * Storage in the mxfp8 forward: a tensor a convolution reads is MXFP8; the downsample output (read only as a residual) is bf16;
 * block outputs are written in both forms; the residual add and the FrozenBN scale / bias run in fp32 in the epilogue.  The
 * pooled stem is bf16 and quantized once; layer4's last output is bf16 only (input_proj reads it, odam_detr_debug_read returns it).
 */

/* per-stage totals of the contraction launches of the most recent profiled forward (odam_detr_profile_enable): n >= 6 entries,
 * [0] stem, [1..4] layer1 .. layer4, [5] input_proj, transformer projections / FFN and heads.  A fused bf16 launch that also
 * computes the next stage's first reduce counts in the stage it starts in. */
int odam_detr_profile_read_stages(odam_detr* m, int n, int* launches, double* ms, double* flops);

/* ---- single-operator entry points (the same kernels the forward uses; for parity tests and reuse) ---- */
/* NHWC convolution / linear:  x [dev][B,H,W,Cin] (Cin power of two >= 4), w_packed [dev][Cout][Kpad], zero padded
 * to a multiple of the k-tile (32 fp32 / 64 bf16), scale/bias/residual nullable, y [dev][B,Ho,Wo,Cout].
 * k_order 0: k = (ky*KW+kx)*Cin + ci.  k_order 1 (Cin % k-tile == 0, KH*KW <= 32; what the detector uses for its 3x3
 * layers): k = ((ci / kt)*KH*KW + ky*KW+kx)*kt + ci % kt -- all taps of one channel chunk in consecutive k-tiles. */
int odam_op_conv2d_nhwc(const float* x, const float* w_packed, const float* scale, const float* bias,
                        const float* residual, float* y, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                        int stride, int pad, int Kpad, int relu, int k_order, void* stream);
/* same kernel in bf16 mode: x, w_packed, residual, y are raw bfloat16 (Cin a power of two >= 8, Kpad % 64 == 0);
 * out_f32 != 0 writes y as fp32 */
int odam_op_conv2d_nhwc_bf16(const void* x, const void* w_packed, const float* scale, const float* bias,
                             const void* residual, void* y, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                             int stride, int pad, int Kpad, int relu, int out_f32, int k_order, void* stream);
/* the same entry with dilation (dil >= 1: tap (ky, kx) reads input pixel (oy stride - pad + ky dil, ox stride - pad + kx dil)) for both
 * operand types: dtype 0 = fp32 (x, w_packed, residual, y float32; out_f32 must be 0), 1 = bf16 as odam_op_conv2d_nhwc_bf16 */
int odam_op_conv2d_nhwc_ex(const void* x, const void* w_packed, const float* scale, const float* bias, const void* residual,
                           void* y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                           int Kpad, int relu, int k_order, int dtype, int out_f32, void* stream);
/* bf16 bottleneck tail as one launch (BASELINE config 4; replaces what torchvision's Bottleneck.forward runs after conv1 --
 * conv2, bn2, relu, conv3, bn3, += identity, relu -- as instantiated at src/models/backbone.py:90-92, plus optionally the next
 * block's conv1 / bn1 / relu): x [dev][B,H,W,P] bf16 (P = 64 / 128 / 256), w2 [P][9 P] packed k_order 1, w3 [4 P][P], residual / y
 * [B,Ho,Wo,4 P] bf16, w1n [PN][4 P] + y_next [B,Ho,Wo,PN] optional (PN = 0: none).  Returns 4 where the fused kernel does not
 * apply (shape / size); bit-identical to the layers run one by one through odam_op_conv2d_nhwc_bf16. */
int odam_op_bottleneck_bf16(const void* x, const void* w2, const float* s2, const float* b2, const void* w3, const float* s3,
                            const float* b3, const void* residual, void* y, const void* w1n, const float* s1n, const float* b1n,
                            void* y_next, int B, int H, int W, int P, int stride, int PN, void* stream);
/* fp32 bottleneck tail as one launch (fp32 split mode, odam_op_conv_f32_mode 2): the same operation and layouts in float32 for P = 64
 * (PN = 0 / 64 / 128) and P = 128 (PN = 0); the packed fp32 filters are split into bf16 planes on the host for the call (synchronous).
 * Returns 4 where the fused kernel does not apply (shape, size, configuration).  The 3x3's output is the bits odam_op_conv2d_nhwc
 * returns for it; y and y_next differ from the separate launches only through the summation order of the expand / reduce. */
int odam_op_bottleneck_f32(const float* x, const float* w2, const float* s2, const float* b2, const float* w3, const float* s3,
                           const float* b3, const float* residual, float* y, const float* w1n, const float* s1n, const float* b1n,
                           float* y_next, int B, int H, int W, int P, int stride, int PN, void* stream);
/* Which kernel each contraction ran on (host-side log, no device work, no synchronisation): one token per call of the contraction
 * launcher since the last reset, in launch order, noted where the kernel is chosen.  buf [host][n] receives them '\n'-separated
 * (the newest 4096 if more were noted; as many as fit); returns how many were noted since the reset (-1: n <= 0); reset != 0
 * starts a new log.  buf may be null (count / reset only).  Tokens (a bottleneck launch counts once, whatever number of image
 * groups it runs as):
 *   small tiles   <f32|bf16>.small.<BM>x<BN>.w<waves>[.ut][.x3][.s4]    .ut: LDS-DMA uniform-tap gather (else register-staged),
 *                 .x3: fp32 operands split in registers onto the bf16 instruction (else v_mfma_f32_32x32x2_f32), .s4: four LDS stages
 *   ring kernel   f32.ring.m<2|3|4>.<rows>x<cols>[.pool]   m2 split in registers, m3 pre-split filters 32x32x16, m4 pre-split 16x16x32;
 *                 bf16.ring.<rows>x<cols>[.pool]           .pool: conv1 with the max-pool on its tile
 *   bottleneck    f32.fused.m<3|4>.<l1|chain64|chain128|l2>   l1: 64-channel 3x3 + expand, chain64 / chain128: + the next reduce,
 *                 bf16.fused.p<P>[.chain<PN>]                 l2: 128-channel 3x3 + expand
 *   mxfp8         mx8.<BN>x<BM>.w<waves>                      every MXFP8 convolution (odam_op_conv2d_nhwc_mxfp8, the mxfp8 body)
 * The fp32 tokens, all of them (tests/test_conv_f32_gpu.py covers each):
 *   FP32-TOKENS-BEGIN
 *   f32.small.128x64.w4 f32.small.128x64.w4.ut f32.small.128x64.w4.ut.x3 f32.small.128x64.w8 f32.small.128x64.w8.ut
 *   f32.small.128x64.w8.ut.x3 f32.small.64x64.w4 f32.small.64x64.w4.ut f32.small.64x64.w4.ut.x3 f32.small.64x64.w4.ut.s4
 *   f32.small.64x64.w4.ut.x3.s4 f32.small.128x128.w4 f32.small.128x128.w4.ut f32.small.128x128.w4.ut.x3 f32.small.128x128.w8
 *   f32.small.128x128.w8.ut f32.small.128x128.w8.ut.x3
 *   f32.ring.m2.256x64 f32.ring.m2.256x128 f32.ring.m2.256x256 f32.ring.m3.256x64 f32.ring.m3.256x128 f32.ring.m3.256x256
 *   f32.ring.m4.256x64 f32.ring.m4.256x128 f32.ring.m4.256x256 f32.ring.m4.512x64 f32.ring.m4.512x64.pool
 *   f32.fused.m3.l1 f32.fused.m3.chain64 f32.fused.m3.chain128 f32.fused.m3.l2 f32.fused.m4.l1 f32.fused.m4.chain64
 *   f32.fused.m4.chain128 f32.fused.m4.l2
 *   FP32-TOKENS-END
 * The bf16 tokens, all of them (tests/test_conv_bf16_gpu.py covers each):
 *   BF16-TOKENS-BEGIN
 *   bf16.small.128x64.w4 bf16.small.128x64.w4.ut bf16.small.128x64.w8 bf16.small.128x64.w8.ut bf16.small.64x64.w4
 *   bf16.small.64x64.w4.ut bf16.small.64x64.w4.ut.s4 bf16.small.128x128.w4 bf16.small.128x128.w4.ut bf16.small.128x128.w8
 *   bf16.small.128x128.w8.ut
 *   bf16.ring.256x64 bf16.ring.256x128 bf16.ring.256x256 bf16.ring.512x64 bf16.ring.512x64.pool
 *   bf16.fused.p64 bf16.fused.p64.chain64 bf16.fused.p64.chain128 bf16.fused.p128 bf16.fused.p128.chain128 bf16.fused.p256
 *   BF16-TOKENS-END
 * conv1 on the centred uint8 frame (odam_detr_forward_u8, odam_op_stem_u8; the activations as one bf16 plane, three products per block)
 * reports f32.ring.m5.512x64.pool, or f32.ring.m5.512x64 where the pool runs as its own kernel (tests/test_stem_u8_gpu.py covers both). */
long long odam_op_conv_paths(char* buf, int n, int reset);
/* which layers the bf16-native 256-row schedule of the contraction kernel takes: 0 none, 1 those large enough to fill
 * the device (default), 2 every eligible layer (parity tests on small shapes).  Process-wide; also ODAM_CG_BIG. */
int odam_op_conv_bf16_mode(int mode);
/* how fp32 layers large enough for the 256-row schedule are multiplied: 0 = v_mfma_f32_32x32x2_f32 on 128x128 tiles
 * (the k-ordered fp32 FMA chain), 1 = the same instruction in the ring
 * kernel, 2 (default) = every fp32 operand split exactly into three bf16 values and the six significant cross products taken on
 * v_mfma_f32_32x32x16_bf16 (fp32-class accuracy -- 0.8-1.4e-7 of sum |a b| against float64, the fp32 instruction
 * 1.1-1.9e-7 -- at 2.7x the matrix rate; last bits differ from mode 0).  Process-wide; also ODAM_CG_BIG_F32. */
int odam_op_conv_f32_mode(int mode);
/* diagnostics: launches of conv1 with the max-pool on its tile (odam_config stem.pool) since the library was loaded -- lets a
 * test see that the fused path, not the conv1 + max-pool pair, produced what it compares */
long long odam_op_pooled_stem_launches(void);
/* the stem of odam_detr_forward_u8 alone: rgb [dev][B,h,w,3] uint8 -> resize to H x W -> conv1 (conv1_w [host][64,3,7,7]) -> scale / bias
 * ([dev][64], the folded FrozenBN) -> ReLU -> 3x3 / stride 2 max-pool -> y [dev][B,H2,W2,64] fp32, through the code the forward runs.
 * mean, std: host float[3].  *path (nullable) = 1 where conv1 read the centred bf16 frame, 0 where the normalised fp32 image was built
 * first.  Returns 4 where conv1 would not run as the row convolution at all (cg.f32 = 0, stem.rows = 0, too few rows without cg.pin). */
int odam_op_stem_u8(const unsigned char* rgb, int B, int h, int w, int H, int W, const float* conv1_w, const float* scale,
                    const float* bias, const float* mean, const float* std_dev, float* y, int* path, void* stream);
int odam_op_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo,
                      int B, int H, int Lq, int Lk, void* stream);
/* the same op on bf16 tensors (config 4: nn.MultiheadAttention's scaled-dot-product core, src/models/transformer.py:154-167, on
 * v_mfma_f32_32x32x16_bf16): Q / K / V / O [dev] bf16 with the given row pitches (multiples of 8 / 8 / 8 / 4 elements), head h at columns
 * 32 h .. 32 h + 31; standalone entry for tests and timing -- the detector calls the same launcher */
int odam_op_attention_bf16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                           int B, int H, int Lq, int Lk, void* stream);
int odam_op_add_layernorm(const float* x, const float* r, const float* gamma, const float* beta, float* y, int M,
                          void* stream);
/* Attention as the networks call it, for parity tests.  head_dim 32: dtype 0 fp32 / 1 bf16 (row pitches multiples of 4 / 8
 * elements, ldo of 4), key_mask [dev][B][Lk] nullable (non-zero = padded key), the detector's kernel choice (att.x3 /
 * att.bf16_mfma apply).  head_dim 64: dtype 0 and key_mask null only (the associator's kernel, scale 1/8).  Code 1 for any
 * other head_dim / dtype / mask combination. */
int odam_op_attention_ex(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                         int B, int H, int Lq, int Lk, int head_dim, int dtype, const unsigned char* key_mask, void* stream);
/* residual add + LayerNorm over 256 channels as the forward calls it: x, r (nullable), y, y_pos (nullable) [dev][M][256] of
 * dtype 0 fp32 / 1 bf16, gamma / beta / pos fp32; y = LN(x + r) * gamma + beta, y_pos[row] = y[row] + pos[row % L] */
int odam_op_add_layernorm_ex(const void* x, const void* r, const float* gamma, const float* beta, void* y,
                             const float* pos, int L, void* y_pos, int M, int dtype, void* stream);
/* The detector's attention at any head width it builds: head_dim 32 or 64, dtype 0 fp32 / 1 bf16 (row pitches multiples of 4 /
 * 8 elements, ldo of 4), key_mask [dev][B][Lk] nullable; scale float32(sqrt(1 / head_dim)); the kernel the forward would choose
 * (att.x3 / att.bf16_mfma apply).  Head h at columns h * head_dim ..  At head_dim 32 the same launches as odam_op_attention_ex. */
int odam_op_attention_hd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                         int B, int H, int Lq, int Lk, int head_dim, int dtype, const unsigned char* key_mask, void* stream);
/* odam_op_add_layernorm_ex over C channels, C a multiple of 64 in 128 .. 1024 (C = 256: the same kernel as _ex) */
int odam_op_add_layernorm_c(const void* x, const void* r, const float* gamma, const float* beta, void* y,
                            const float* pos, int L, void* y_pos, int M, int C, int dtype, void* stream);
/* MXFP8 tensors (format above).  n elements, n % 32 == 0: x [dev] fp32 (src_dtype 0) or bf16 (1) -> q [dev][n] + s [dev][n / 32] */
int odam_op_quantize_mxfp8(const void* x, int src_dtype, long long n, void* q, void* s, void* stream);
int odam_op_dequantize_mxfp8(const void* q, const void* s, long long n, float* y, void* stream);
/* MXFP8 convolution (the mxfp8 forward's kernel, one launch): x / xs [dev] MXFP8 NHWC input [B,H,W,Cin] (Cin % 64 == 0),
 * w_packed / ws [dev] MXFP8 filters [Cout][Kpad] (Cout % 32 == 0, Kpad = KH KW Cin, k_order 0 only; dil 1 only), scale / bias fp32
 * nullable, residual [dev] bf16 [M][Cout] nullable; epilogue act(acc * scale + bias + residual) in fp32, then per 32-channel block
 * of a pixel the outputs y / ys MXFP8 (nullable together), y_bf16 (nullable) and y_f32 (nullable: the values before quantization).
 * Notes token mx8.128x128.w4. */
int odam_op_conv2d_nhwc_mxfp8(const void* x, const void* xs, const void* w_packed, const void* ws, const float* scale,
                              const float* bias, const void* residual, void* y, void* ys, void* y_bf16, float* y_f32,
                              int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                              int Kpad, int relu, int k_order, void* stream);
/* ---- the kernels between the contractions, one launch each through the launcher the forward calls (tests/test_detr_elementwise_gpu.py
 * holds each to an exact or float64 reference).  Every entry checks its arguments before any HIP call -- null pointers, dtype 0 (fp32)
 * / 1 (bf16), negative extents and what is noted per entry -- and returns 1 (ODAM_E_INVALID) with its name in odam_last_error(); an
 * extent of 0 is a successful call that launches nothing.  bf16 tensors are raw bfloat16 (the upper 16 bits of the float32), written
 * with round-to-nearest-even. */
/* torchvision's stem pool, nn.MaxPool2d(3, stride 2, padding 1), on NHWC: x [dev][B,H,W,C] -> y [dev][B,Ho,Wo,C], Ho = (H - 1) / 2 + 1,
 * Wo = (W - 1) / 2 + 1, x and y of `dtype`, C % 4 == 0.  A window tap outside the image counts as -inf, so an all-negative window
 * gives its (negative) maximum and -inf inputs pass through; the result is one of the inputs, bit for bit.  NaN inputs are outside the
 * contract: the kernel takes fmaxf, which drops a NaN where torch.nn.functional.max_pool2d propagates it. */
int odam_op_maxpool3x3s2_nhwc_ex(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
/* the same for fp32 tensors (= _ex with dtype 0) */
int odam_op_maxpool3x3s2_nhwc(const float* x, float* y, int B, int H, int W, int C, void* stream);
/* The network input into the stem's layout: in [dev][B,3,H,W] float32 (NCHW) -> pixel-major out of `dtype`, every element of it written.
 *   framed == 0, dtype 0:  out [B][H][W][4] float32        -- channels 0-2 the image, channel 3 = +0.0
 *   framed == 0, dtype 1:  out [B][H][W][8] bf16           -- one 16-byte chunk per pixel: 3 real channels and 5 of +0.0
 *   framed != 0:           out [B][H + 6][W + 8][4] of `dtype` (4 channels in bf16 too) -- the picture at rows 3 .. H + 2, columns
 *                          3 .. W + 2 (pixel (y, x) at [y + 3][x + 3]), channel 3 = +0.0, and every pixel of the frame (3 rows above
 *                          and below, 3 columns left, 5 right) +0.0: what the stem as a 7x1 convolution over 8-pixel rows reads.  The
 *                          frame is written by every call, never left over from the call before.
 * bf16 values are the float32 inputs rounded to nearest even. */
int odam_op_nchw_to_nhwc4(const float* in, void* out, int B, int H, int W, int dtype, int framed, void* stream);
/* in [dev][B,H,W,C] of `dtype` (NHWC, any C >= 0) -> out [dev][B,C,H,W] float32 (NCHW); values unchanged (bf16 widened exactly) */
int odam_op_nhwc_to_nchw(const void* in, float* out, int B, int H, int W, int C, int dtype, void* stream);
/* out[row][c] = x[row][c] + pos[row % L][c] (x null: out[row][c] = pos[row % L][c]) for row < M: x (nullable), out [dev][M][C] of
 * `dtype`, pos [dev][L][C] float32, C % 4 == 0, L > 0.  One float32 addition, then for bf16 one rounding to nearest even.  C == 256 runs
 * the kernel the shipped width uses, any other C the general one. */
int odam_op_add_pos(const void* x, const float* pos, int L, void* out, int M, int C, int dtype, void* stream);
/* in [dev][n] of `dtype` -> out [dev][n] float32, exactly (dtype 0: a copy).  n % 4 == 0, else code 1 and nothing is written. */
int odam_op_to_f32(const void* in, float* out, long long n, int dtype, void* stream);
/* x[i] = 1 / (1 + expf(-x[i])) in place, x [dev][n] float32 (the box head's sigmoid, detr.py:76) */
int odam_op_sigmoid(float* x, int n, void* stream);
/* odam_detr_postprocess without a model handle: n queries (any batch flattened), n_cls1 >= 2 logits per query (the last one "no
 * object"), n_bins >= 1 angle logits; logits [dev][n][n_cls1], boxes [n][4] (cx, cy, w, h in 0 .. 1), angle [n][n_bins], offset [n][2],
 * size [n][3], depth [n], K9 [host] row-major 3x3 intrinsics -> rows [dev][n][16] as odam_detr_postprocess writes them: the score is the
 * largest softmax probability among the first n_cls1 - 1 classes, class and angle bin the FIRST index of the maximum. */
int odam_op_postprocess(const float* logits, const float* boxes, const float* angle, const float* offset, const float* size,
                        const float* depth, int n, int n_cls1, int n_bins, const float* K9, float img_w, float img_h, float* rows,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
