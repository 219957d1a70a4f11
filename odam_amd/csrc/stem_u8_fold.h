// stem_u8_fold.h -- conv1 on the centred uint8 frame: the input normalisation folded into the filters.  Plain C++ (no HIP): the model
// (detr_weights.hip) and the host test (tests/native/stem_u8_check.cpp) share it.
//
// The resized frame is uint8 by construction, and the reference normalises it as x_k = (u_k / 255 - mean_k) / std_k before conv1.
// With the integer centre c_k = lrint(255 mean_k) the same value is x_k = (u_k - c_k) / (255 std_k) + (c_k / 255 - mean_k) / std_k, so
//   sum_k w_k x_k = sum_k [w_k / (255 std_k)] (u_k - c_k)  +  [sum_k w_k (c_k / 255 - mean_k) / std_k] * 1.
// The producer (detr_kernels.hip preprocess_u8_bf16x4_framed_kernel) writes the pixel as (u_0 - c_0, u_1 - c_1, u_2 - c_2, 1): three
// integers of magnitude <= 255 and an indicator, all exact in one bf16 value.  The zero frame around the image has indicator 0, so a tap
// on it contributes nothing -- its share of the mean term included -- which is the reference's zero padding in normalised space.
// Centring keeps the second bracket small (|c_k / 255 - mean_k| <= 1 / 510): the sum has no cancellation of large terms.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define ODAM_STEM_U8_HD __host__ __device__
#else
#define ODAM_STEM_U8_HD
#endif

namespace odam_dm {

// The framed image [H + 6][W + 8]: pixel (Xp, Yp) of it is pixel (Xp - 3, Yp - 3) of the H x W frame where that exists (3 rows above and
// below, 3 columns left and 5 right are the frame)
ODAM_STEM_U8_HD inline bool stem_u8_inside(int Xp, int Yp, int H, int W, int& X, int& Y) {
    X = Xp - 3; Y = Yp - 3;
    return (unsigned)X < (unsigned)W && (unsigned)Y < (unsigned)H;
}
// an integer of magnitude <= 256 as bf16: the top half of its fp32 form (eight significant bits: exact)
ODAM_STEM_U8_HD inline unsigned stem_u8_bf16(int d) { return __builtin_bit_cast(unsigned, (float)d) >> 16; }
// one pixel inside the image as four bf16 in two words: (u0 - c0, u1 - c1 | u2 - c2, 1); a frame pixel is two zero words
ODAM_STEM_U8_HD inline void stem_u8_pixel(int u0, int u1, int u2, int c0, int c1, int c2, unsigned& w0, unsigned& w1) {
    w0 = stem_u8_bf16(u0 - c0) | (stem_u8_bf16(u1 - c1) << 16);
    w1 = stem_u8_bf16(u2 - c2) | (stem_u8_bf16(1) << 16);
}

// c_k = lrint(255 mean_k) in double (mean taken as the exact value of its fp32 input)
inline void stem_u8_centres(const float mean[3], int centre[3]) {
    for (int k = 0; k < 3; k++) centre[k] = (int)std::lrint(255.0 * (double)mean[k]);
}

// w [Cout][3][7][7] fp32 (PyTorch) -> rows [Cout][224] in the layout of the row-convolution stem, k = ky * 32 + kx * 4 + c, the
// kx = 7 slot zero: computed in double, rounded ONCE to fp32
inline void stem_u8_fold(const float* w, int Cout, const float mean[3], const float stdv[3], float* rows) {
    int c[3];
    stem_u8_centres(mean, c);
    for (int o = 0; o < Cout; o++)
        for (int ky = 0; ky < 7; ky++)
            for (int kx = 0; kx < 8; kx++) {
                float* r = rows + (size_t)o * 224 + ky * 32 + kx * 4;
                r[0] = r[1] = r[2] = r[3] = 0.0f;
                if (kx == 7) continue;
                double ind = 0.0;
                for (int k = 0; k < 3; k++) {
                    const double wk = (double)w[(((size_t)o * 3 + k) * 7 + ky) * 7 + kx];
                    r[k] = (float)(wk / (255.0 * (double)stdv[k]));
                    ind += wk * ((double)c[k] / 255.0 - (double)mean[k]) / (double)stdv[k];
                }
                r[3] = (float)ind;
            }
}

}  // namespace odam_dm
