// view_keys.h -- the 64-bit sort key of a detection row (sq_prepare.hip, track_merge.hip): image << 32 | index, all ones when the
// row's frame id names no image (which frame id names an image is each kernel's own rule).  Sorted ascending, the keys are in
// image order with the lowest index of an image first and the rows without an image at the end.
#pragma once
constexpr unsigned long long VIEW_NONE = ~0ull;

__device__ __forceinline__ unsigned long long view_key(int img, int idx) { return ((unsigned long long)(unsigned)img << 32) | (unsigned)idx; }
__device__ __forceinline__ int view_image(unsigned long long key) { return (int)(key >> 32); }
__device__ __forceinline__ int view_index(unsigned long long key) { return (int)(key & 0xffffffffu); }

// sorted entry j is the first of its image's run: the row that stands for the image
__device__ __forceinline__ bool first_of_image(const unsigned long long* keys, int j) {
    const unsigned long long k = keys[j];
    return k != VIEW_NONE && (j == 0 || view_image(keys[j - 1]) != view_image(k));
}
