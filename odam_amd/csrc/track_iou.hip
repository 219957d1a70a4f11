// track_iou.hip -- network-free association: the reference's IoU tracker (likojack/ODAM src/scripts/run_tracking.py:106-170
// match_tracks over :37-52 convert_det_to_list, :55-103 init_tracks without its ORB / depth side data, src/utils/box_utils.py:123-144
// iou_2d and :424-447 iou_3d), the frame loop of whole sequences in ONE launch (include/odam_track.h).  Restated in numpy by
// tests/track_iou_ref.py; the kernel equals it bit for bit.
//
// One workgroup of ONE wavefront per sequence; it walks the sequence's frames in order, no host round trip per frame.  Per frame:
//   1. lane d < count forms detection d: clipped pixel box, t_wo in a fixed order, 3D box; all binary64, no contraction;
//   2. a detection's rank in the host order (descending score, equal scores by descending index) is counted over the frame's
//      detections by shuffles, as det_select.hip counts it -- no sort;
//   3. detections are scanned in rank order.  The tracks are spread over the lanes in chunks of 64; a lane computes both IoUs of
//      its track once per (detection, chunk).  The reference's scan over the tracks is sequential and order-dependent, but between
//      two updates its state (max_iou_2d, max_iou_3d) is constant, and the next update is the first track after the cursor whose
//      lane satisfies the condition against that state: ballot, lowest set lane, broadcast its two values, move the cursor, until no
//      lane qualifies; then the next chunk.  Iterations = updates, not tracks;
//   4. nothing of the state is written while a frame is matched (the tracks matched in this frame are flag bits in LDS), so a frame
//      that would take the sequence past max_tracks is abandoned BEFORE any write: the state is as after the frame before it;
//   5. lane d then writes detection d's track -- appended to (running sums, count, last frame, last box) or started -- and re-forms
//      that track's 3D box from the new means.  A track changes at most once per frame and is out of the frame's scans once it
//      has: its box is formed once per change, never per pair.  Distinct detections own distinct tracks: no two lanes write one word.
// The state stays in global memory (L2-resident: 140 bytes per track, structure of arrays, 64 consecutive tracks per load); LDS
// holds the frame's 30 detections and one flag bit per track.  Workgroup barriers order a frame's state writes before the next
// frame's reads (one wavefront: they cost a fence).
#include <hip/hip_runtime.h>

#include "../../include/odam_track.h"
#include "odam_err.h"

#pragma clang fp contract(off)

namespace {

constexpr int TI_DETS = ODAM_TRACK_DETS;
constexpr int TI_COLS = 15;
constexpr int TI_HDR = ODAM_TRACK_HEADER_WORDS;
constexpr int TI_FIELDS = 16;      // doubles per track: sum dims 0-2, sum t_wo 3-5, box lo 6-8, box hi 9-11, last pixel box 12-15

__host__ __device__ inline long long state_bytes(int M) {
    const long long b = (long long)TI_HDR * 4 + (long long)M * (TI_FIELDS * 8 + 12);
    return (b + 15) & ~15ll;
}

struct State {
    int* hdr;
    double* f;      // [TI_FIELDS][M]
    float* cls;
    int* nobs;
    int* last;
};

__device__ __forceinline__ State state_of(char* base, int M) {
    State S;
    S.hdr = reinterpret_cast<int*>(base);
    S.f = reinterpret_cast<double*>(base + TI_HDR * 4);
    S.cls = reinterpret_cast<float*>(base + TI_HDR * 4 + (size_t)M * TI_FIELDS * 8);
    S.nobs = reinterpret_cast<int*>(S.cls + M);
    S.last = S.nobs + M;
    return S;
}

// Python's max(a, b) / min(a, b): the second argument wins only when strictly greater / less; max(0, v)
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_pos(double v) { return v > 0.0 ? v : 0.0; }
__device__ __forceinline__ double np_clip(double x, double hi) {
    const double v = x < 0.0 ? 0.0 : x;
    return v > hi ? hi : v;
}

struct StepArgs {
    const int* seq_off;
    const float* blk;
    const int* cnt;
    const int* fid;
    const double* T;
    double img_w, img_h, thr2, thr_track, thr3;
    char* state;
    long long stride;
    int n_frames, max_gap, M;
    int* out_ids;
    double* out2;
    double* out3;
    int* out_n;
};

__global__ __launch_bounds__(64) void track_iou_kernel(StepArgs A) {
    __shared__ unsigned long long s_used[ODAM_TRACK_MAX_TRACKS / 64];      // bit t: track t took a detection of this frame
    __shared__ double s_det[10][32];                                      // pixel box 0-3, 3D lo 4-6, 3D hi 7-9
    __shared__ float s_cls[32];
    __shared__ int s_order[32];                                           // detection index by rank
    const int s = blockIdx.x, lane = threadIdx.x;
    const int M = A.M;
    const State S = state_of(A.state + (size_t)s * (size_t)A.stride, M);
    int T = S.hdr[0];
    if (S.hdr[2] != M || T < 0 || T > M) {      // not a block odam_track_iou_reset made for this capacity: block-uniform, before any barrier
        if (lane == 0) {
            S.hdr[1] = -2;
            A.out_n[s] = -1;
        }
        return;
    }
    int f0 = A.seq_off[s], f1 = A.seq_off[s + 1];
    f0 = f0 < 0 ? 0 : f0;
    f1 = f1 > A.n_frames ? A.n_frames : f1;
    int overflow = -1;
    for (int f = f0; f < f1; f++) {
        int n = A.cnt[f];
        n = n < 0 ? 0 : (n > TI_DETS ? TI_DETS : n);
        const int fid = A.fid[f];
        // ---- 1. this lane's detection
        double box[4] = {0, 0, 0, 0}, dd[3] = {0, 0, 0}, tw[3] = {0, 0, 0}, dlo[3] = {0, 0, 0}, dhi[3] = {0, 0, 0}, sc = 0.0;
        float cl = 0.0f;
        if (lane < n) {
            const float* r = A.blk + ((size_t)f * TI_DETS + lane) * TI_COLS;
            const double* Tm = A.T + (size_t)f * 16;
            box[0] = np_clip((double)r[2] * A.img_w, A.img_w);
            box[1] = np_clip((double)r[3] * A.img_h, A.img_h);
            box[2] = np_clip((double)r[4] * A.img_w, A.img_w);
            box[3] = np_clip((double)r[5] * A.img_h, A.img_h);
            const double x = (double)r[9], y = (double)r[10], z = (double)r[11];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                dd[k] = (double)r[6 + k];
                tw[k] = ((x * Tm[k * 4 + 0] + y * Tm[k * 4 + 1]) + z * Tm[k * 4 + 2]) + Tm[k * 4 + 3];
                dlo[k] = (-dd[k]) / 2.0 + tw[k];
                dhi[k] = dd[k] / 2.0 + tw[k];
            }
            cl = r[1];
            sc = (double)r[14];
        }
        // ---- 2. rank in the host order: descending score, equal scores by descending index; a NaN is the largest
        int rank = 0;
        for (int k = 0; k < n; k++) {
            const double o = __shfl(sc, k, 64);
            const bool gt = o > sc || (o != o && sc == sc);
            const bool eq = o == sc || (o != o && sc != sc);
            rank += (gt || (eq && k > lane)) ? 1 : 0;
        }
        if (lane < n) {
            s_order[rank] = lane;
#pragma unroll
            for (int k = 0; k < 4; k++) s_det[k][lane] = box[k];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s_det[4 + k][lane] = dlo[k];
                s_det[7 + k][lane] = dhi[k];
            }
            s_cls[lane] = cl;
        }
        for (int w = lane; w * 64 < T; w += 64) s_used[w] = 0ull;
        __syncthreads();
        // ---- 3. the ordered scans
        int my_id = -1;
        double my2 = -1.0, my3 = -1.0;
        for (int r = 0; r < n; r++) {
            const int d = s_order[r];
            double b[10];
#pragma unroll
            for (int k = 0; k < 10; k++) b[k] = s_det[k][d];
            const float dcl = s_cls[d];
            double m2 = -1.0, m3 = -1.0;
            int best = -1;
            for (int c = 0; c * 64 < T; c++) {
                const int t = c * 64 + lane;
                const bool live = t < T && !((s_used[c] >> lane) & 1ull);
                double i2 = 0.0, i3 = 0.0;
                bool recent = false, ceq = false;
                if (t < T) {
                    double a[10];      // the track: last pixel box 0-3, 3D lo 4-6, hi 7-9
#pragma unroll
                    for (int k = 0; k < 4; k++) a[k] = S.f[(size_t)(12 + k) * M + t];
#pragma unroll
                    for (int k = 0; k < 6; k++) a[4 + k] = S.f[(size_t)(6 + k) * M + t];
                    ceq = dcl == S.cls[t];
                    recent = !((long long)fid - (long long)S.last[t] > (long long)A.max_gap);
                    {      // iou_2d(track, detection)
                        const double x_min = py_max(a[0], b[0]), y_min = py_max(a[1], b[1]);
                        const double x_max = py_min(a[2], b[2]), y_max = py_min(a[3], b[3]);
                        const double inter = py_pos(x_max - x_min) * py_pos(y_max - y_min);
                        const double area_a = (a[2] - a[0]) * (a[3] - a[1]), area_b = (b[2] - b[0]) * (b[3] - b[1]);
                        i2 = inter / (area_a + area_b - inter);
                    }
                    {      // iou_3d(detection, track)
                        const double x_min = py_max(b[4], a[4]), y_min = py_max(b[5], a[5]), z_min = py_max(b[6], a[6]);
                        const double x_max = py_min(b[7], a[7]), y_max = py_min(b[8], a[8]), z_max = py_min(b[9], a[9]);
                        const double inter = py_pos(x_max - x_min) * py_pos(y_max - y_min) * py_pos(z_max - z_min);
                        const double vol_a = (b[7] - b[4]) * (b[8] - b[5]) * (b[9] - b[6]);
                        const double vol_b = (a[7] - a[4]) * (a[8] - a[5]) * (a[9] - a[6]);
                        i3 = inter / (vol_a + vol_b - inter);
                    }
                }
                const unsigned long long recent_mask = __ballot(recent);
                int cursor = 0;
                for (;;) {
                    const bool q = live && ceq && lane >= cursor && (recent ? (i2 > m2 && i3 > m3) : (i3 > m3));
                    const unsigned long long hit = __ballot(q);
                    if (!hit) break;
                    const int l = __ffsll((long long)hit) - 1;
                    const double v2 = __shfl(i2, l, 64), v3 = __shfl(i3, l, 64);
                    if ((recent_mask >> l) & 1ull) m2 = v2;
                    m3 = v3;
                    best = c * 64 + l;
                    cursor = l + 1;
                }
            }
            const bool attach = best >= 0 && (m2 > A.thr2 || m3 > A.thr3);
            if (lane == d) {
                my2 = m2;
                my3 = m3;
                if (attach) my_id = best;
            }
            if (attach && lane == 0) s_used[best >> 6] |= 1ull << (best & 63);
            __syncthreads();
        }
        // ---- 4. new tracks, in detection index order; a frame that does not fit is abandoned before any write
        const bool fresh = lane < n && my_id < 0 && !(sc < A.thr_track);
        const unsigned long long fresh_mask = __ballot(fresh);
        const int n_new = __popcll(fresh_mask);
        if (T + n_new > M) {
            overflow = f;
            break;
        }
        if (fresh) my_id = T + __popcll(fresh_mask & ((1ull << lane) - 1ull));
        // ---- 5. the state of the tracks this frame changed (one lane per track), and the frame's 30 output slots
        if (lane < n && my_id >= 0) {
            const int t = my_id;      // < T + n_new <= M
            double sum[6];
            int cntv = 1;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                sum[k] = dd[k];
                sum[3 + k] = tw[k];
            }
            if (!fresh) {
#pragma unroll
                for (int k = 0; k < 6; k++) sum[k] = S.f[(size_t)k * M + t] + sum[k];
                cntv = S.nobs[t] + 1;
            } else {
                S.cls[t] = cl;
            }
            const double nn = (double)cntv;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double md = sum[k] / nn, mt = sum[3 + k] / nn;
                S.f[(size_t)k * M + t] = sum[k];
                S.f[(size_t)(3 + k) * M + t] = sum[3 + k];
                S.f[(size_t)(6 + k) * M + t] = (-md) / 2.0 + mt;
                S.f[(size_t)(9 + k) * M + t] = md / 2.0 + mt;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) S.f[(size_t)(12 + k) * M + t] = box[k];
            S.nobs[t] = cntv;
            S.last[t] = fid;
        }
        T += n_new;
        if (lane < TI_DETS) {
            const size_t o = (size_t)f * TI_DETS + lane;
            A.out_ids[o] = lane < n ? my_id : -1;
            A.out2[o] = lane < n ? my2 : -1.0;
            A.out3[o] = lane < n ? my3 : -1.0;
        }
        __syncthreads();      // this frame's state writes before the next frame's reads
    }
    if (lane == 0) {
        S.hdr[0] = T;
        S.hdr[1] = overflow;
        A.out_n[s] = T;
    }
}

__global__ void track_iou_reset_kernel(char* state, long long stride, int n_seq, int M) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seq) return;
    int* hdr = reinterpret_cast<int*>(state + (size_t)s * (size_t)stride);
    hdr[0] = 0;
    hdr[1] = -1;
    hdr[2] = M;
    for (int k = 3; k < TI_HDR; k++) hdr[k] = 0;
}

}  // namespace

extern "C" long long odam_track_iou_state_bytes(int max_tracks) {
    if (max_tracks < 1 || max_tracks > ODAM_TRACK_MAX_TRACKS) return -1;
    return state_bytes(max_tracks);
}

extern "C" int odam_track_iou_reset(odam_sq_ctx* ctx, void* state, int n_seq, int max_tracks, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_track_iou_reset: null context");
    if (n_seq < 0) return odam_fail(ODAM_E_INVALID, "odam_track_iou_reset: bad size");
    if (max_tracks < 1) return odam_fail(ODAM_E_INVALID, "odam_track_iou_reset: max_tracks < 1");
    if (max_tracks > ODAM_TRACK_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_track_iou_reset: more than 65536 tracks per sequence");
    if (n_seq == 0) return ODAM_OK;
    if (!state) return odam_fail(ODAM_E_INVALID, "odam_track_iou_reset: null pointer");
    hipLaunchKernelGGL(track_iou_reset_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (char*)state,
                       state_bytes(max_tracks), n_seq, max_tracks);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_track_iou_step(odam_sq_ctx* ctx, int n_seq, const int* seq_off, int n_frames, const float* det_block,
                                   const int* det_count, const int* frame_ids, const double* T_wc, double img_w, double img_h,
                                   double match_threshold, double track_threshold, double iou3d_threshold, int max_gap, void* state,
                                   int max_tracks, int* out_ids, double* out_iou2d, double* out_iou3d, int* out_n_tracks, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_track_iou_step: null context");
    if (n_seq < 0 || n_frames < 0) return odam_fail(ODAM_E_INVALID, "odam_track_iou_step: bad size");
    if (max_tracks < 1) return odam_fail(ODAM_E_INVALID, "odam_track_iou_step: max_tracks < 1");
    if (max_tracks > ODAM_TRACK_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_track_iou_step: more than 65536 tracks per sequence");
    if (n_seq == 0) return ODAM_OK;
    if (!seq_off || !state || !out_n_tracks) return odam_fail(ODAM_E_INVALID, "odam_track_iou_step: null pointer");
    if (n_frames > 0 && (!det_block || !det_count || !frame_ids || !T_wc || !out_ids || !out_iou2d || !out_iou3d))
        return odam_fail(ODAM_E_INVALID, "odam_track_iou_step: null pointer");
    StepArgs A{};
    A.seq_off = seq_off; A.blk = det_block; A.cnt = det_count; A.fid = frame_ids; A.T = T_wc; A.img_w = img_w; A.img_h = img_h;
    A.thr2 = match_threshold; A.thr_track = track_threshold; A.thr3 = iou3d_threshold; A.state = (char*)state;
    A.stride = state_bytes(max_tracks); A.n_frames = n_frames; A.max_gap = max_gap; A.M = max_tracks; A.out_ids = out_ids;
    A.out2 = out_iou2d; A.out3 = out_iou3d; A.out_n = out_n_tracks;
    hipLaunchKernelGGL(track_iou_kernel, dim3((unsigned)n_seq), dim3(64), 0, (hipStream_t)stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
