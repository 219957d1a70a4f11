// assoc_samples.hip -- validation samples of the association network, cut from a scene table that lives on the device
// (include/odam_samples.h; likojack/ODAM src/datasets/scan_net_track.py:173-243, 285-341: get_by_sequence without its file reads).
//
// The store is the COMPACTED table: the valid observation rows object after object in frame order ([n_obs, 78] float64, the
// ground-truth id column removed), so the rows a track keeps for a sampled frame -- its last n_times valid rows before that frame --
// are one contiguous block of k x 78 doubles.  The host plans which block belongs to which track slot (odam_amd/assoc_samples.py);
// one launch then serves a whole batch: workgroup i < sum_t builds track slot i, workgroup sum_t + b the detections of sample b.
//
// Track slot: the block is read linearly (consecutive lanes, consecutive doubles), every copied value goes to an LDS tile
// [79][n_times | 1] float at (channel, time) -- consecutive lanes hold consecutive channels, the odd stride spreads them over the 64
// banks --, the camera-frame centre and the azimuth pair are computed by one lane per row, and the tile is written out channel-major
// with the time index fastest: every store instruction covers consecutive addresses, padding (-1) and the four box channels, which are
// the same on every time step, included.  The detection slots take the same route through a [79][31] tile.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../include/odam_samples.h"
#include "odam_err.h"

namespace {

constexpr int COLS = 78, CH = 79, ND = 30, DS = 31;
constexpr int MAX_B = 64, MAX_SLOTS = 1024, MAX_TIMES = 128;
constexpr int NTH = 256, RING = 4;

// the plan of one launch: one pinned slot of a ring, one device mirror (as assoc_batch.hip's Desc)
struct Plan {
    int frame[MAX_B], n_det[MAX_B];
    int det_src[MAX_B * ND];
    int slot_sample[MAX_SLOTS], slot_obj[MAX_SLOTS], slot_row0[MAX_SLOTS], slot_k[MAX_SLOTS];
};

// channel of column c of a 78-column row where the value is a copy; -1: the column feeds a computed channel (box 2-5, centre 9-11,
// azimuth 12)
__device__ __forceinline__ int copy_channel(int c) {
    if (c < 2) return c;
    if (c < 6) return -1;
    if (c < 9) return c;
    if (c < 13) return -1;
    return c + 1;      // score 13 -> 14, shape code 14..77 -> 15..78
}

// channels 9-13 of one row: t_co = ((x c0 + y c1) + z c2) + c3 per camera row, every product and sum rounded to nearest on its own,
// and sin / cos of azimuth - cam_azi, all binary64
__device__ __forceinline__ void pose_channels(const double* __restrict__ r, const double* __restrict__ cam, float* __restrict__ tile, int stride,
                                              int pos) {
    const double x = r[9], y = r[10], z = r[11];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double* c = cam + 4 * i;
        const double v = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, c[0]), __dmul_rn(y, c[1])), __dmul_rn(z, c[2])), c[3]);
        tile[(9 + i) * stride + pos] = (float)v;
    }
    const double rel = __dsub_rn(r[12], cam[12]);
    tile[12 * stride + pos] = (float)sin(rel);
    tile[13 * stride + pos] = (float)cos(rel);
}

__device__ __forceinline__ double clip_box(double x) { return x < -1.0 ? -1.0 : (x > 2.0 ? 2.0 : x); }

__global__ __launch_bounds__(NTH) void samples_cut_kernel(const double* __restrict__ obs, const double* __restrict__ unm,
                                                          const double* __restrict__ proj, const double* __restrict__ cams,
                                                          const Plan* __restrict__ plan, int n_frames, int sum_t, int n_times, double img_w,
                                                          double img_h, float* __restrict__ tracks, float* __restrict__ detections,
                                                          int* __restrict__ status) {
    extern __shared__ float tile[];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < sum_t) {
        // ---- one track slot ----
        const int slot = blockIdx.x;
        const int b = plan->slot_sample[slot], o = plan->slot_obj[slot], k = plan->slot_k[slot];
        const int f = plan->frame[b];
        const int S = n_times | 1;
        const double* blk = obs + (size_t)plan->slot_row0[slot] * COLS;
        const double* cam = cams + (size_t)f * 13;
        const double* pb = proj + ((size_t)o * n_frames + f) * 4;
        for (int i = tid; i < k * COLS; i += NTH) {
            const int r = i / COLS, c = i - r * COLS;
            const int ch = copy_channel(c);
            if (ch >= 0) tile[ch * S + r] = (float)blk[i];
        }
        for (int r = tid; r < k; r += NTH) pose_channels(blk + (size_t)r * COLS, cam, tile, S, r);
        const double p0 = pb[0], p1 = pb[1], p2 = pb[2], p3 = pb[3];
        if (tid == 0 && p0 == -1.0 && p1 == -1.0 && p2 == -1.0 && p3 == -1.0) atomicOr(&status[b], 1);
        const float box[4] = {(float)clip_box(p0 / img_w), (float)clip_box(p1 / img_h), (float)clip_box(p2 / img_w), (float)clip_box(p3 / img_h)};
        __syncthreads();
        float* out = tracks + (size_t)slot * CH * n_times;
        for (int i = tid; i < CH * n_times; i += NTH) {
            const int ch = i / n_times, t = i - ch * n_times;
            float v = -1.0f;
            if (t < k) {
                const float bx = ch == 2 ? box[0] : (ch == 3 ? box[1] : (ch == 4 ? box[2] : box[3]));
                v = (ch >= 2 && ch < 6) ? bx : tile[ch * S + t];
            }
            out[i] = v;
        }
        return;
    }
    // ---- the detections of one sample ----
    const int b = blockIdx.x - sum_t;
    const int n = plan->n_det[b];
    const double* cam = cams + (size_t)plan->frame[b] * 13;
    const int* src = plan->det_src + b * ND;
    for (int i = tid; i < n * COLS; i += NTH) {
        const int j = i / COLS, c = i - j * COLS;
        const int s = src[j];
        const double* r = s >= 0 ? obs + (size_t)s * COLS : unm + (size_t)(-(s + 1)) * COLS;
        const int ch = copy_channel(c);
        if (ch >= 0) tile[ch * DS + j] = (float)r[c];
        else if (c < 6) tile[c * DS + j] = (float)(r[c] / ((c & 1) ? img_h : img_w));      // the row's own box, not clipped (_preprocess)
    }
    if (tid < n) {
        const int s = src[tid];
        pose_channels(s >= 0 ? obs + (size_t)s * COLS : unm + (size_t)(-(s + 1)) * COLS, cam, tile, DS, tid);
    }
    __syncthreads();
    float* out = detections + (size_t)b * CH * ND;
    for (int i = tid; i < CH * ND; i += NTH) {
        const int ch = i / ND, j = i - ch * ND;
        out[i] = j < n ? tile[ch * DS + j] : -1.0f;
    }
}

size_t lds_bytes(int n_times) {
    const size_t a = (size_t)CH * (size_t)(n_times | 1), d = (size_t)CH * DS;
    return sizeof(float) * (a > d ? a : d);
}

}  // namespace

struct odam_samples {
    int n_obj = 0, n_frames = 0;
    long long n_obs = 0, n_unm = 0;
    bool loaded = false;
    double img_w = 0.0, img_h = 0.0;
    long long* h_obs_off = nullptr;      // host copy: the cut checks every slot against its object's block
    double *obs = nullptr, *unm = nullptr, *proj = nullptr, *cam = nullptr;
    Plan* dev = nullptr;
    Plan* pin[RING] = {};
    hipEvent_t ev[RING] = {};
    bool used[RING] = {};
    int slot = 0;
};

extern "C" int odam_samples_create(int n_obj, int n_frames, long long n_obs, long long n_unm, odam_samples** out) {
    if (!out) return odam_fail(1, "odam_samples_create: null pointer");
    if (n_obj < 1 || n_frames < 1 || n_obs < 1 || n_unm < 0)
        return odam_fail(3, "odam_samples_create: n_obj >= 1, n_frames >= 1, n_obs >= 1 and n_unm >= 0");
    if (n_obs > (long long)n_obj * n_frames) return odam_fail(3, "odam_samples_create: more observations than n_obj * n_frames");
    if (n_obs > 0x7fffffffLL || n_unm > 0x7fffffffLL) return odam_fail(3, "odam_samples_create: a row count that does not fit 31 bits");
    odam_samples* s = new odam_samples();
    s->n_obj = n_obj; s->n_frames = n_frames; s->n_obs = n_obs; s->n_unm = n_unm;
    s->h_obs_off = new long long[(size_t)n_obj + 1]();
    *out = s;
    return 0;
}

extern "C" int odam_samples_destroy(odam_samples* s) {
    if (!s) return 0;
    for (double* p : {s->obs, s->unm, s->proj, s->cam}) if (p) (void)hipFree(p);
    if (s->dev) (void)hipFree(s->dev);
    for (int i = 0; i < RING; i++) {
        if (s->pin[i]) (void)hipHostFree(s->pin[i]);
        if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
    }
    delete[] s->h_obs_off;
    delete s;
    return 0;
}

extern "C" int odam_samples_load(odam_samples* s, const double* obs, const long long* obs_off, const double* proj, const double* cam,
                                 const double* unm, const long long* unm_off, double img_w, double img_h, void* stream) {
    if (!s || !obs || !obs_off || !proj || !cam || !unm_off || (!unm && s->n_unm > 0)) return odam_fail(1, "odam_samples_load: null pointer");
    if (!(img_w > 0.0) || !(img_h > 0.0)) return odam_fail(1, "odam_samples_load: the image size must be positive");
    if (obs_off[0] != 0 || unm_off[0] != 0) return odam_fail(1, "odam_samples_load: obs_off and unm_off must start at 0");
    for (int o = 0; o < s->n_obj; o++) {
        if (obs_off[o + 1] < obs_off[o]) return odam_fail(1, "odam_samples_load: obs_off must not decrease");
        if (obs_off[o + 1] - obs_off[o] > s->n_frames) return odam_fail(1, "odam_samples_load: an object with more rows than the scene has frames");
    }
    for (int f = 0; f < s->n_frames; f++)
        if (unm_off[f + 1] < unm_off[f]) return odam_fail(1, "odam_samples_load: unm_off must not decrease");
    if (obs_off[s->n_obj] != s->n_obs || unm_off[s->n_frames] != s->n_unm)
        return odam_fail(1, "odam_samples_load: obs_off / unm_off do not end at the row counts the store was created with");
    // ---- the device is touched from here on ----
    hipStream_t st = (hipStream_t)stream;
    const size_t obs_b = sizeof(double) * (size_t)s->n_obs * COLS, unm_b = sizeof(double) * (size_t)(s->n_unm > 0 ? s->n_unm : 1) * COLS;
    const size_t proj_b = sizeof(double) * (size_t)s->n_obj * s->n_frames * 4, cam_b = sizeof(double) * (size_t)s->n_frames * 13;
    if (!s->obs) {
        ODAM_HIP(hipMalloc((void**)&s->obs, obs_b));
        ODAM_HIP(hipMalloc((void**)&s->unm, unm_b));
        ODAM_HIP(hipMalloc((void**)&s->proj, proj_b));
        ODAM_HIP(hipMalloc((void**)&s->cam, cam_b));
        ODAM_HIP(hipMalloc((void**)&s->dev, sizeof(Plan)));
        for (int i = 0; i < RING; i++) {
            ODAM_HIP(hipHostMalloc((void**)&s->pin[i], sizeof(Plan), hipHostMallocDefault));
            ODAM_HIP(hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming));
        }
    }
    s->loaded = false;
    ODAM_HIP(hipMemcpyAsync(s->obs, obs, obs_b, hipMemcpyHostToDevice, st));
    if (s->n_unm > 0) ODAM_HIP(hipMemcpyAsync(s->unm, unm, sizeof(double) * (size_t)s->n_unm * COLS, hipMemcpyHostToDevice, st));
    ODAM_HIP(hipMemcpyAsync(s->proj, proj, proj_b, hipMemcpyHostToDevice, st));
    ODAM_HIP(hipMemcpyAsync(s->cam, cam, cam_b, hipMemcpyHostToDevice, st));
    ODAM_HIP(hipStreamSynchronize(st));      // the host arrays are the caller's again
    std::memcpy(s->h_obs_off, obs_off, sizeof(long long) * ((size_t)s->n_obj + 1));
    s->img_w = img_w; s->img_h = img_h;
    s->loaded = true;
    return 0;
}

extern "C" int odam_samples_cut(odam_samples* s, int B, const int* frames, const int* n_det, const int* det_src, int sum_t,
                                const int* slot_sample, const int* slot_obj, const int* slot_row0, const int* slot_k, int n_times,
                                float* tracks, float* detections, int* status, void* stream) {
    char msg[200];
    if (!s || !frames || !n_det || !det_src || !slot_sample || !slot_obj || !slot_row0 || !slot_k || !tracks || !detections || !status)
        return odam_fail(1, "odam_samples_cut: null pointer");
    if (B < 1 || B > MAX_B) return odam_fail(3, "odam_samples_cut: 1 <= B <= 64");
    if (sum_t < 1 || sum_t > MAX_SLOTS) return odam_fail(3, "odam_samples_cut: 1 <= sum_t <= 1024");
    if (n_times < 1 || n_times > MAX_TIMES) return odam_fail(3, "odam_samples_cut: 1 <= n_times <= 128");
    for (int b = 0; b < B; b++) {
        if (n_det[b] < 1 || n_det[b] > ND) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: sample %d has n_det = %d (1 <= n_det <= 30 after the cap)", b, n_det[b]);
            return odam_fail(3, msg);
        }
    }
    for (int i = 0; i < sum_t; i++) {
        if (slot_k[i] < 1 || slot_k[i] > n_times) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: slot %d keeps %d rows (1 <= k <= n_times = %d)", i, slot_k[i], n_times);
            return odam_fail(3, msg);
        }
    }
    for (int b = 0; b < B; b++) {
        if (frames[b] < 0 || frames[b] >= s->n_frames) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: sample %d names frame %d, the scene has %d", b, frames[b], s->n_frames);
            return odam_fail(1, msg);
        }
        for (int j = 0; j < n_det[b]; j++) {
            const long long r = det_src[b * ND + j];
            if (r >= 0 ? r >= s->n_obs : -(r + 1) >= s->n_unm) {
                std::snprintf(msg, sizeof(msg), "odam_samples_cut: detection %d of sample %d has source %lld, outside the store", j, b, r);
                return odam_fail(1, msg);
            }
        }
    }
    for (int i = 0; i < sum_t; i++) {
        if (slot_sample[i] < 0 || slot_sample[i] >= B || (i && slot_sample[i] < slot_sample[i - 1])) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: slot %d names sample %d (0 .. B - 1, not decreasing)", i, slot_sample[i]);
            return odam_fail(1, msg);
        }
        const int o = slot_obj[i];
        if (o < 0 || o >= s->n_obj) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: slot %d names object %d, the scene has %d", i, o, s->n_obj);
            return odam_fail(1, msg);
        }
        if (slot_row0[i] < 0 || (long long)slot_row0[i] + slot_k[i] > s->n_obs) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: slot %d reads rows %d .. %d, outside the store's %lld", i, slot_row0[i],
                          slot_row0[i] + slot_k[i], s->n_obs);
            return odam_fail(1, msg);
        }
        if (!s->loaded) continue;      // (no offsets to check against yet: refused below)
        if (slot_row0[i] < s->h_obs_off[o] || (long long)slot_row0[i] + slot_k[i] > s->h_obs_off[o + 1]) {
            std::snprintf(msg, sizeof(msg), "odam_samples_cut: slot %d reads rows %d .. %d, outside the block of object %d", i, slot_row0[i],
                          slot_row0[i] + slot_k[i], o);
            return odam_fail(1, msg);
        }
    }
    if (!s->loaded) return odam_fail(1, "odam_samples_cut: call odam_samples_load first");
    // ---- the device is touched from here on ----
    hipStream_t st = (hipStream_t)stream;
    const int slot = s->slot;
    s->slot = (slot + 1) % RING;
    if (s->used[slot]) ODAM_HIP(hipEventSynchronize(s->ev[slot]));      // waits only if the stream is RING calls behind
    Plan* p = s->pin[slot];
    std::memcpy(p->frame, frames, sizeof(int) * B);
    std::memcpy(p->n_det, n_det, sizeof(int) * B);
    std::memcpy(p->det_src, det_src, sizeof(int) * (size_t)B * ND);
    std::memcpy(p->slot_sample, slot_sample, sizeof(int) * sum_t);
    std::memcpy(p->slot_obj, slot_obj, sizeof(int) * sum_t);
    std::memcpy(p->slot_row0, slot_row0, sizeof(int) * sum_t);
    std::memcpy(p->slot_k, slot_k, sizeof(int) * sum_t);
    ODAM_HIP(hipMemcpyAsync(s->dev, p, sizeof(Plan), hipMemcpyHostToDevice, st));
    ODAM_HIP(hipEventRecord(s->ev[slot], st));
    s->used[slot] = true;
    ODAM_HIP(hipMemsetAsync(status, 0, sizeof(int) * B, st));
    hipLaunchKernelGGL(samples_cut_kernel, dim3(sum_t + B), dim3(NTH), lds_bytes(n_times), st, s->obs, s->unm, s->proj, s->cam, s->dev,
                       s->n_frames, sum_t, n_times, s->img_w, s->img_h, tracks, detections, status);
    ODAM_HIP(hipGetLastError());
    return 0;
}
