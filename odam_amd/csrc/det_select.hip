// det_select.hip -- the step between odam_detr_postprocess and the association, on the device: score threshold, greedy
// nms_3d and the detection rows of run_detector for a whole batch of frames in one launch (include/odam_detr.h:
// odam_detr_select_pack).  Reference: src/models/detr.py:124-125 (keep = score > threshold), :161-205 (nms_3d),
// src/processor.py:269-288 (row layout), :318-319 (30 detections per frame).
//
// The yardstick is the host chain -- odam_detr_select (detr_model.hip), processor.detection_array, parallel.pack_detections --
// and the result equals it bit for bit: the pair tests below are odam_detr_select's, the same fp32 operations in the same
// order (no contraction, IEEE division, std::max / std::min spelled out so that a NaN takes the same way through them).
//
// One workgroup of ONE wavefront per frame, Q <= 256 queries: a lane owns up to four candidates, so the whole pass needs no
// barrier after the set-up and the suppression state is four 64-bit ballots.
//   1. the frame's [Q,16] rows are staged in LDS (row pitch 17: column reads are conflict-free);
//   2. candidates (score > threshold; a NaN is none) are compacted in query order by ballot + prefix count;
//   3. a candidate's rank in the host's order (stable ascending sort, reversed: descending score, equal scores by descending
//      query index) is counted over the candidates -- no sort;
//   4. greedy pass: the first live rank is kept, every lane tests its live candidates against it, the ballots of the hits
//      join the suppression masks.  One iteration per KEPT detection, at most 30 (what process_frame keeps);
//   5. the kept rows are written as [30,15] float32 in the detection_array layout, unused slots -1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/odam_detr.h"
#include "../../include/odam_sq.h"
#include "odam_err.h"

#pragma clang fp contract(off)

namespace {

constexpr int SP_MAX_Q = 256;
constexpr int SP_SLOTS = SP_MAX_Q / 64;      // candidates per lane
constexpr int SP_DETS = 30;                  // parallel.MAX_DETS
constexpr int SP_COLS = 15;                  // parallel.DET_COLS
constexpr int SP_PITCH = 17;                 // LDS row pitch in floats

// std::max / std::min as the host's odam_detr_select calls them
__device__ __forceinline__ float host_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float host_min(float a, float b) { return b < a ? b : a; }

struct Box {      // what a pair test reads of one candidate
    float cls, x0, y0, x1, y1;
    float lo[3], hi[3];
};

__device__ __forceinline__ Box load_box(const float* r) {
    Box c;
    c.cls = r[1];
    c.x0 = r[2]; c.y0 = r[3]; c.x1 = r[4]; c.y1 = r[5];
    for (int k = 0; k < 3; k++) {
        c.lo[k] = (-r[10 + k]) / 2.0f + r[6 + k];
        c.hi[k] = r[10 + k] / 2.0f + r[6 + k];
    }
    return c;
}

// does the kept detection s suppress the later candidate t?  (detr_model.hip, odam_detr_select's inner loop)
__device__ __forceinline__ bool suppresses(const Box& s, const Box& t, int nms_2d) {
    const float dx = host_max(0.0f, host_min(s.hi[0], t.hi[0]) - host_max(s.lo[0], t.lo[0]));
    const float dy = host_max(0.0f, host_min(s.hi[1], t.hi[1]) - host_max(s.lo[1], t.lo[1]));
    const float dz = host_max(0.0f, host_min(s.hi[2], t.hi[2]) - host_max(s.lo[2], t.lo[2]));
    const float inter = dx * dy * dz;
    const float va = (s.hi[0] - s.lo[0]) * (s.hi[1] - s.lo[1]) * (s.hi[2] - s.lo[2]);
    const float vb = (t.hi[0] - t.lo[0]) * (t.hi[1] - t.lo[1]) * (t.hi[2] - t.lo[2]);
    const float iou3 = inter / (va + vb - inter);
    if (t.cls == s.cls && iou3 > 0.25f) return true;
    if (!nms_2d) return false;
    const float ix = host_max(0.0f, host_min(s.x1, t.x1) - host_max(s.x0, t.x0));
    const float iy = host_max(0.0f, host_min(s.y1, t.y1) - host_max(s.y0, t.y0));
    const float ia = ix * iy;
    const float aa = (s.x1 - s.x0) * (s.y1 - s.y0);
    const float ab = (t.x1 - t.x0) * (t.y1 - t.y0);
    return ia / (aa + ab - ia) > 0.5f;
}

__global__ __launch_bounds__(64) void select_pack_kernel(const float* __restrict__ rows16, int Q, float threshold, int nms_2d,
                                                         const float* __restrict__ frame_ids, float seq_w, float seq_h,
                                                         const float* __restrict__ sincos, int n_bins,
                                                         float* __restrict__ det_block, int* __restrict__ det_count,
                                                         int* __restrict__ keep_idx) {
    __shared__ float srow[SP_MAX_Q * SP_PITCH];
    __shared__ float cscore[SP_MAX_Q];      // candidates in query order: score ...
    __shared__ int cquery[SP_MAX_Q];        // ... and query index
    __shared__ int order[SP_MAX_Q];         // query index by rank
    __shared__ int kept[SP_DETS];
    const int b = blockIdx.x, lane = threadIdx.x;

    const float4* src = reinterpret_cast<const float4*>(rows16 + (size_t)b * Q * 16);
    for (int i = lane; i < Q * 4; i += 64) {
        const float4 v = src[i];
        float* d = srow + (i >> 2) * SP_PITCH + (i & 3) * 4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();

    int n = 0;
    for (int q0 = 0; q0 < Q; q0 += 64) {
        const int q = q0 + lane;
        const float sc = q < Q ? srow[q * SP_PITCH] : 0.0f;
        const bool cand = q < Q && sc > threshold;
        const unsigned long long m = __ballot(cand);
        if (cand) {
            const int p = n + __popcll(m & ((1ull << lane) - 1ull));
            cscore[p] = sc;
            cquery[p] = q;
        }
        n += __popcll(m);
    }
    __syncthreads();

    for (int p = lane; p < n; p += 64) {
        const float sc = cscore[p];
        int rank = 0;
        for (int k = 0; k < n; k++) {      // candidates are in query order: a larger index is a larger k
            const float o = cscore[k];
            rank += (o > sc || (o == sc && k > p)) ? 1 : 0;
        }
        order[rank] = cquery[p];
    }
    __syncthreads();

    Box mine[SP_SLOTS];
    unsigned long long dead[SP_SLOTS];      // per rank: kept already, suppressed, or past the last candidate (wave-uniform)
#pragma unroll
    for (int s = 0; s < SP_SLOTS; s++) {
        const int j = s * 64 + lane;
        mine[s] = load_box(srow + (j < n ? order[j] : 0) * SP_PITCH);
        dead[s] = ~__ballot(j < n);
    }

    int n_kept = 0;
    for (int it = 0; it < SP_DETS; it++) {
        int i = -1;      // the first rank that is neither kept nor suppressed
#pragma unroll
        for (int s = SP_SLOTS - 1; s >= 0; s--)
            if (~dead[s]) i = s * 64 + __ffsll((long long)~dead[s]) - 1;
        if (i < 0) break;
        const int qs = order[i];
        if (lane == 0) kept[n_kept] = qs;
        n_kept++;
        const Box top = load_box(srow + qs * SP_PITCH);
#pragma unroll
        for (int s = 0; s < SP_SLOTS; s++) {
            if (s == (i >> 6)) dead[s] |= 1ull << (i & 63);
            const bool live = !((dead[s] >> lane) & 1ull);      // a live rank is behind i: everything before it is kept or suppressed
            dead[s] |= __ballot(live && suppresses(top, mine[s], nms_2d));
        }
    }
    __syncthreads();

    float* out = det_block + (size_t)b * SP_DETS * SP_COLS;
    const float fid = frame_ids[b];
    for (int idx = lane; idx < SP_DETS * SP_COLS; idx += 64) {
        const int k = idx / SP_COLS, c = idx - k * SP_COLS;
        float v = -1.0f;
        if (k < n_kept) {
            const float* r = srow + kept[k] * SP_PITCH;
            if (c == 0) v = fid;
            else if (c == 1) v = truncf(r[1]);                  // .astype(np.int64)
            else if (c == 2 || c == 4) v = r[c] / seq_w;
            else if (c == 3 || c == 5) v = r[c] / seq_h;
            else if (c < 9) v = r[10 + (c - 6)];                // dimensions
            else if (c < 12) v = r[6 + (c - 9)];                // translate
            else if (c < 14) {
                const int bin = (int)r[9];
                v = (bin >= 0 && bin < n_bins) ? sincos[bin * 2 + (c - 12)] : __builtin_nanf("");
            } else v = r[0];
        }
        out[idx] = v;
    }
    if (lane == 0) det_count[b] = n_kept;
    if (keep_idx && lane < SP_DETS) keep_idx[(size_t)b * SP_DETS + lane] = lane < n_kept ? kept[lane] : -1;
}

}  // namespace

extern "C" int odam_detr_select_pack(const float* rows16, int B, int Q, float threshold, int nms_2d, const float* frame_ids,
                                     float seq_w, float seq_h, const float* sincos, int n_bins, float* det_block,
                                     int* det_count, int* keep_idx, void* stream) {
    if (!rows16 || !frame_ids || !sincos || !det_block || !det_count)
        return odam_fail(ODAM_E_INVALID, "odam_detr_select_pack: null pointer");
    if (B < 0 || Q < 0 || n_bins < 1) return odam_fail(ODAM_E_INVALID, "odam_detr_select_pack: bad size");
    if (Q > SP_MAX_Q)
        return odam_fail(ODAM_E_LIMIT, "odam_detr_select_pack: more than 256 queries per frame (one wavefront holds four per lane); "
                                       "use the host path (odam_detr_select)");
    if (reinterpret_cast<uintptr_t>(rows16) & 15)
        return odam_fail(ODAM_E_INVALID, "odam_detr_select_pack: rows16 must be 16-byte aligned");
    if (B == 0) return 0;
    hipLaunchKernelGGL(select_pack_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, rows16, Q, threshold, nms_2d, frame_ids,
                       seq_w, seq_h, sincos, n_bins, det_block, det_count, keep_idx);
    ODAM_HIP(hipGetLastError());
    return 0;
}
