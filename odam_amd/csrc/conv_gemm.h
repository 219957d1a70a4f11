// conv_gemm.h -- implicit-GEMM convolution / linear layer on the CDNA4 matrix cores, fp32 or bf16 operands.
//
//   C[m, n] = epilogue( sum_k A(m, k) * W[n, k] )
//     m = output pixel (b, oy, ox) of an NHWC tensor, n = output channel,
//     k = (ky * KW + kx) * Cin + ci  -- the input is gathered on the fly (no im2col buffer); see k_order.
//   epilogue: * scale[n] + bias[n] (FrozenBatchNorm folded to scale/bias, or a Linear bias),
//             + residual[m, n], ReLU -- all optional.
//
// A Linear layer is the 1x1 case with H = 1, W = M.  One entry therefore serves every
// contraction of the detector: ResNet stem/bottleneck convolutions, input_proj, the attention
// projections, the FFN and the prediction heads (reference: src/models/backbone.py:59-94 via
// torchvision ResNet, src/models/detr.py:45,70,73-78, src/models/transformer.py:132-238) -- and the association network's.
//
// Arguments: cg_args.h.  Which kernel runs a call -- the 128x128 / 128x64 / 64x64 tiles of conv_gemm.hip, the 256-row LDS-DMA ring
// kernel of cg_big.hpp, a bottleneck or the pooled stem on its tile -- is decided by choose() in cg_choice.h, which also declares
// the predicates (fused_second_ok, fused_bf16_ok, pooled_stem_ok) and mode switches (set_big_mode, set_f32_mode, f32_mode).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cg_choice.h"

namespace odam_cg {

// chooses the kernel (cg_choice.h), notes its token and launches it; a refused call returns the choice's code with its text in
// odam_last_error
int launch_conv_gemm(const ConvGemmArgs& a, hipStream_t stream);

// host: exact three-way bf16 split (truncation) of packed fp32 filters w[Cout][Kpad] (Kpad % 16 == 0) into the Wt3 layout
void split3_filters(const float* w, int Cout, int Kpad, unsigned short* out);

// kernel-choice log (include/odam_detr.h odam_op_conv_paths): one token per launch_conv_gemm call, noted there from the choice
// (cg_mx8.hip notes its own).  Host only (a mutex and a bounded ring of PATH_LOG_N tokens); no device work, no synchronisation.
constexpr int PATH_LOG_N = 4096;
void note_path(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// '\n'-joined tokens noted since the last reset (the newest PATH_LOG_N of them) into buf [n]; returns how many were noted
// (more than the buffer shows when the ring wrapped or buf was too short), or -1 for a bad buffer
long long read_paths(char* buf, int n, int reset);

}  // namespace odam_cg
