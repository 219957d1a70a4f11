// cg_launch.h -- entry points of the ring-kernel translation units, called by launch_conv_gemm (conv_gemm.hip) with what choose()
// (cg_choice.h) decided: they read no configuration and note nothing.
#pragma once
#include "conv_gemm.h"

namespace odam_cg {

// plain layers, fp32 operands: mode 2 (split in registers), 3 (pre-split filters, 32x32x16), 4 (pre-split, 16x16x32);
// bn = tile columns 64 / 128 / 256; nth = 512, or 1024 for the sixteen-wave 512 x 64 tiles of mode 4 and of mode 5 (mode 4 on activations
// stored as one bf16 plane, ConvGemmArgs::a_bf16)
int launch_big_f32(int mode, int bn, int nth, const ConvGemmArgs& a, hipStream_t stream);
// plain layers, bf16 operands: bn 64 / 128 / 256, nth 512 or 1024 (bn 64 and 256)
int launch_big_bf16(int bn, int nth, int s1_window, const ConvGemmArgs& a, hipStream_t stream);
// bottleneck on the tile, fp32 split mode (ConvGemmArgs F_* / G_*): mode 3 (32x32x16) or 4 (16x16x32)
int launch_big_fused(int mode, const ConvGemmArgs& a, hipStream_t stream);
// bottleneck on the tile, bf16 (ConvGemmArgs F_Wt / G_Wt)
int launch_fused_bf16(int s1_window, const ConvGemmArgs& a, hipStream_t stream);

}  // namespace odam_cg
