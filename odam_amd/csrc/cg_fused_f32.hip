// cg_fused_f32.hip -- layer1 / layer2 bottlenecks as one launch, fp32 split mode.  See cg_big.hpp, cg_tails_f32.hpp.
#include "cg_big.hpp"

#include <algorithm>

namespace odam_cg {

template <int MODE>
static int launch_big_fused_as(const ConvGemmArgs& a, hipStream_t stream) {
    static const bool attr_ok = [] {
        return hipFuncSetAttribute((const void*)conv_gemm_big_kernel<MODE, 64, 4, 512, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, FUSE_LDS_BYTES) == hipSuccess &&
               hipFuncSetAttribute((const void*)conv_gemm_big_kernel<MODE, 64, 4, 512, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, FUSE_LDS_BYTES) == hipSuccess &&
               hipFuncSetAttribute((const void*)conv_gemm_big_kernel<MODE, 128, 4, 512, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, FUSE_LDS_BYTES) == hipSuccess &&
               hipFuncSetAttribute((const void*)conv_gemm_big_kernel<MODE, 64, 4, 512, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, FUSE_LDS_BYTES) == hipSuccess;
    }();
    if (!attr_ok) return odam_fail(2, "conv_gemm: cannot raise the dynamic LDS limit");
    const int tiles = (a.M + 255) / 256;
    if (a.Cout == 128) hipLaunchKernelGGL((conv_gemm_big_kernel<MODE, 128, 4, 512, 3>), dim3(tiles), dim3(512), FUSE_LDS_BYTES, stream, a);
    else if (a.G_Wt3 && a.G_N == 128) hipLaunchKernelGGL((conv_gemm_big_kernel<MODE, 64, 4, 512, 4>), dim3(tiles), dim3(512), FUSE_LDS_BYTES, stream, a);
    else if (a.G_Wt3) hipLaunchKernelGGL((conv_gemm_big_kernel<MODE, 64, 4, 512, 2>), dim3(tiles), dim3(512), FUSE_LDS_BYTES, stream, a);
    else hipLaunchKernelGGL((conv_gemm_big_kernel<MODE, 64, 4, 512, 1>), dim3(tiles), dim3(512), FUSE_LDS_BYTES, stream, a);
    ODAM_HIP(hipGetLastError());
    return 0;
}
int launch_big_fused(int mode, const ConvGemmArgs& a, hipStream_t stream) {
    // The tails address the residual and the output through buffer descriptors with 31-bit byte offsets from F_res / F_C.  A batch
    // whose output reaches 2 GiB (layer1 from 40 frames of 800 x 1066) runs as one launch per group of whole images, with the
    // pointers offset to the group's first image: a row's products, order and roundings do not depend on the tile it falls in,
    // so the bits are those of one launch -- and the kernel choice stays the same whatever the batch (cg.pin).
    const long img_rows = (long)a.Ho * a.Wo, img_bytes = img_rows * a.F_ldc * 4;
    const int group = (int)std::min<long>(a.B, (0x7fffffffL - 1) / img_bytes);      // fused_second_ok: one image fits
    if (group < 1) return odam_fail(1, "conv_gemm: fused bottleneck: one image's output exceeds 2 GiB");
    const long lda = a.lda > 0 ? a.lda : a.Cin;
    for (int b0 = 0; b0 < a.B; b0 += group) {
        ConvGemmArgs g = a;
        g.B = std::min(group, a.B - b0);
        g.M = (int)(g.B * img_rows);
        g.A = reinterpret_cast<const float*>(a.A) + (size_t)b0 * a.H * a.W * lda;
        if (a.F_res) g.F_res = a.F_res + (size_t)b0 * img_rows * a.F_ldc;
        g.F_C = a.F_C + (size_t)b0 * img_rows * a.F_ldc;
        if (a.G_C) g.G_C = a.G_C + (size_t)b0 * img_rows * a.G_N;
        const int rc = mode == 4 ? launch_big_fused_as<4>(g, stream) : launch_big_fused_as<3>(g, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace odam_cg

#if CG_STAMP
extern "C" int odam_cg_tail_stamps(unsigned long long* out8, int reset) {      // diagnostic builds only (-DCG_STAMP=1)
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(odam_cg::g_tail_stamps), 8 * sizeof(unsigned long long)) != hipSuccess) return 2;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(odam_cg::g_tail_stamps), z, sizeof(z)) != hipSuccess) return 2;
    }
    return 0;
}
#endif
