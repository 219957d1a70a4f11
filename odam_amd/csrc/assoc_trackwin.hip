// assoc_trackwin.hip -- device-resident track windows (likojack/ODAM OdamProcess._preprocess_tracks, src/processor.py:133-170).
//
// Every frame the reference rebuilds, on the host, the associator's track input [T, 79, 100]: the last 100 observations of every
// live track moved into the CURRENT camera frame (centre through inv(T_wc), azimuth relative to the camera's, the box replaced
// by the projected extent of the fitted surface).  At 40 tracks that is a 1.3 MB tensor built in numpy and uploaded per frame.
// Here the observations stay on the device in the WORLD frame (append-only ring per track: 14 float64 per observation), and one
// launch builds the tensor from them: the same float64 arithmetic per value, rounded to float32 once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/odam_assoc.h"
#include "../../include/odam_sq.h"
#include "odam_err.h"

struct odam_trackwin {
    int max_tracks = 0, window = 0;
    double* rows = nullptr;     // [max_tracks][window][14]: frame id, class, bbox px x4, dims x3, t_wo x3, az_wo, score
    int* count = nullptr;       // [max_tracks] observations appended so far
    double* stage = nullptr;    // pinned [8][32][14 + 1]: rows + track id of one append
    double* h_load = nullptr;   // pinned [max_tracks][window][14]: what odam_trackwin_load's kernel reads (mapped host memory; allocated once -- the
    int* h_load_meta = nullptr; // load path has no allocation, no hipFree (it waits for every stream of the device) and no copy command)
    unsigned slot = 0;
    hipEvent_t copied[8] = {};  // recorded behind the upload from pinned slot i: the host rewrites a slot only after its copy has run
    bool copied_armed[8] = {};
    // host side of OdamProcess._prepare_tracks (src/processor.py:172-180): what the surface of a track is evaluated from -- the
    // means of all its observations' centre, azimuth and dimensions -- kept as running sums, extended by every append
    struct Sums { long n = 0; double st[3] = {0, 0, 0}, sd[3] = {0, 0, 0}; std::vector<double> az; };
    std::vector<Sums> sums;
    bool sums_ok = true;        // false once an append skipped ids or a load came without the full columns
    float* h_params = nullptr;  // pinned [8][max_tracks][9]
    double* d_proj = nullptr;   // [max_tracks][4]
    hipEvent_t params_copied[8] = {};
    bool params_armed[8] = {};
    unsigned params_slot = 0;
};

namespace {
constexpr int TW_COLS = 14;
__global__ void trackwin_append_kernel(const double* __restrict__ st, int n, double* __restrict__ rows, int* __restrict__ count, int window) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int tid_ = (int)st[i * (TW_COLS + 1) + TW_COLS];
    const int c = count[tid_];      // one block per observation; observations of one append go to different tracks
    if (threadIdx.x < TW_COLS) rows[((size_t)tid_ * window + (c % window)) * TW_COLS + threadIdx.x] = st[i * (TW_COLS + 1) + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) count[tid_] = c + 1;
}

// track t: its last k = min(c, window) observations to the ring positions an append sequence of c rows would have left them in
__global__ __launch_bounds__(128) void trackwin_load_kernel(const double* __restrict__ src, const int* __restrict__ meta, int T,
                                                            double* __restrict__ rows, int* __restrict__ count, int window) {
    const int t = blockIdx.x, l = threadIdx.x;
    const int first = meta[t], c = meta[T + t], k = c < window ? c : window;
    if (l < k) {
        const double* r = src + (size_t)(first + l) * TW_COLS;
        double* o = rows + ((size_t)t * window + ((c - k + l) % window)) * TW_COLS;
#pragma unroll
        for (int j = 0; j < TW_COLS; j++) o[j] = r[j];
    }
    if (l == 0) count[t] = c;
}

// out [T][79][window] float32; cam: T_cw rows 0..2 (12), cam_azi, img_w, img_h
struct Cam15 { double v[15]; };      // travels in the kernel arguments
__global__ __launch_bounds__(128) void trackwin_build_kernel(const double* __restrict__ rows, const int* __restrict__ count, int window,
                                                             const double* __restrict__ proj_px, const Cam15 camv,
                                                             float* __restrict__ out) {
    const double* cam = camv.v;
    const int t = blockIdx.x, l = threadIdx.x;
    if (l >= window) return;
    const int c = count[t], k = c < window ? c : window;
    float* o = out + (size_t)t * 79 * window + l;
    if (l >= k) {
#pragma unroll 1
        for (int ch = 0; ch < 79; ch++) o[(size_t)ch * window] = -1.0f;
        return;
    }
    const double* r = rows + ((size_t)t * window + ((c - k + l) % window)) * TW_COLS;
    const double iw = cam[13], ih = cam[14];
    auto clip = [](double x) { return x < -1.0 ? -1.0 : (x > 2.0 ? 2.0 : x); };
    double v[15];
    v[0] = r[0]; v[1] = r[1];
    v[2] = clip(proj_px[t * 4 + 0] / iw); v[3] = clip(proj_px[t * 4 + 1] / ih);
    v[4] = clip(proj_px[t * 4 + 2] / iw); v[5] = clip(proj_px[t * 4 + 3] / ih);
    v[6] = r[6]; v[7] = r[7]; v[8] = r[8];
    const double x = r[9], y = r[10], z = r[11];
    v[9] = x * cam[0] + y * cam[1] + z * cam[2] + cam[3];
    v[10] = x * cam[4] + y * cam[5] + z * cam[6] + cam[7];
    v[11] = x * cam[8] + y * cam[9] + z * cam[10] + cam[11];
    const double rel = r[12] - cam[12];
    v[12] = sin(rel); v[13] = cos(rel);
    v[14] = r[13];
#pragma unroll
    for (int ch = 0; ch < 15; ch++) o[(size_t)ch * window] = (float)v[ch];
#pragma unroll 1
    for (int ch = 15; ch < 79; ch++) o[(size_t)ch * window] = -1.0f;
}
}  // namespace

extern "C" int odam_trackwin_create(int max_tracks, int window, odam_trackwin** out) {
    if (!out || max_tracks < 1 || max_tracks > 4096 || window < 1 || window > 128) return odam_fail(1, "odam_trackwin_create: bad argument");
    odam_trackwin* w = new odam_trackwin();
    w->max_tracks = max_tracks; w->window = window;
    if (hipMalloc((void**)&w->rows, sizeof(double) * (size_t)max_tracks * window * TW_COLS) != hipSuccess ||
        hipMalloc((void**)&w->count, sizeof(int) * (size_t)max_tracks) != hipSuccess ||
        hipHostMalloc((void**)&w->h_load, sizeof(double) * (size_t)max_tracks * window * TW_COLS, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&w->h_load_meta, sizeof(int) * 2 * (size_t)max_tracks, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&w->stage, sizeof(double) * 8 * 32 * (TW_COLS + 1), hipHostMallocDefault) != hipSuccess) {
        (void)odam_trackwin_destroy(w);      // frees what was allocated (null pointers and events are skipped)
        return odam_fail(2, "odam_trackwin_create: allocation failed");
    }
    // counts start at zero, and are zero when this call returns: through a private non-blocking stream -- hipMemset would be
    // ordered on the NULL stream, may still be pending when it returns and then land behind a load / append the caller issues on
    // a stream of its own (it did: the counts of a freshly loaded store went back to zero -- GPU test
    // test_stores_created_while_the_default_stream_is_busy); waiting for the NULL stream instead would wait for whatever another
    // thread has queued there
    {
        hipStream_t init = nullptr;
        const bool ok = hipStreamCreateWithFlags(&init, hipStreamNonBlocking) == hipSuccess &&
                        hipMemsetAsync(w->count, 0, sizeof(int) * (size_t)max_tracks, init) == hipSuccess &&
                        hipStreamSynchronize(init) == hipSuccess;
        if (init) (void)hipStreamDestroy(init);
        if (!ok) {
            (void)odam_trackwin_destroy(w);
            return odam_fail(2, "odam_trackwin_create: initialisation failed");
        }
    }
    for (int i = 0; i < 8; i++)
        if (hipEventCreateWithFlags(&w->copied[i], hipEventDisableTiming) != hipSuccess) {
            w->copied[i] = nullptr;
            (void)odam_trackwin_destroy(w);
            return odam_fail(2, "odam_trackwin_create: event creation failed");
        }
    *out = w;
    return 0;
}

extern "C" int odam_trackwin_destroy(odam_trackwin* w) {
    if (!w) return 0;
    for (int i = 0; i < 8; i++) {
        if (w->params_armed[i]) (void)hipEventSynchronize(w->params_copied[i]);
        if (w->params_copied[i]) (void)hipEventDestroy(w->params_copied[i]);
        if (w->copied_armed[i]) (void)hipEventSynchronize(w->copied[i]);      // no upload may still be reading the pinned ring
        if (w->copied[i]) (void)hipEventDestroy(w->copied[i]);
    }
    if (w->h_params) (void)hipHostFree(w->h_params);
    if (w->d_proj) (void)hipFree(w->d_proj);
    (void)hipFree(w->rows); (void)hipFree(w->count); (void)hipHostFree(w->h_load); (void)hipHostFree(w->h_load_meta); (void)hipHostFree(w->stage);
    delete w;
    return 0;
}

extern "C" int odam_trackwin_reset(odam_trackwin* w, void* stream) {
    if (!w) return odam_fail(1, "odam_trackwin_reset: null handle");
    ODAM_HIP(hipMemsetAsync(w->count, 0, sizeof(int) * (size_t)w->max_tracks, (hipStream_t)stream));
    w->sums.clear(); w->sums_ok = true;
    return 0;
}

extern "C" int odam_trackwin_append(odam_trackwin* w, int n, const int* track_ids, const double* rows14, void* stream) {
    if (!w || n < 0 || n > 32 || (n && (!track_ids || !rows14))) return odam_fail(1, "odam_trackwin_append: bad argument (at most 32 observations per call)");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n; i++)
        if (track_ids[i] < 0 || track_ids[i] >= w->max_tracks) return odam_fail(3, "odam_trackwin_append: track id outside the handle's capacity");
    // the kernel takes one block per observation and reads the track's count once: two rows of one track in one call would land in the same ring slot
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++)
            if (track_ids[i] == track_ids[j]) return odam_fail(1, "odam_trackwin_append: a track is named twice in one call (one observation per track and call)");
    // The ring slot may be rewritten only once the kernel that read it eight appends ago has run -- appends can queue behind long
    // kernels on the stream (a detector forward, a rebuild).
    const int si = (int)(w->slot++ & 7);
    if (w->copied_armed[si]) ODAM_HIP(hipEventSynchronize(w->copied[si]));
    double* slot = w->stage + (size_t)si * 32 * (TW_COLS + 1);
    for (int i = 0; i < n; i++) {
        for (int c = 0; c < TW_COLS; c++) slot[i * (TW_COLS + 1) + c] = rows14[i * TW_COLS + c];
        slot[i * (TW_COLS + 1) + TW_COLS] = (double)track_ids[i];
    }
    // the kernel reads the pinned slot itself (mapped host memory; <= 3.8 KB): no copy command in the frame's chain.  The slot is the
    // host's again once that kernel has run -- the event behind it is what the next use of the slot waits for.
    hipLaunchKernelGGL(trackwin_append_kernel, dim3(n), dim3(64), 0, st, slot, n, w->rows, w->count, w->window);
    ODAM_HIP(hipGetLastError());
    ODAM_HIP(hipEventRecord(w->copied[si], st));
    w->copied_armed[si] = true;
    for (int i = 0; i < n; i++) {
        const size_t t = (size_t)track_ids[i];
        if (t > w->sums.size()) w->sums_ok = false;        // a gap in the ids: no sums for the skipped tracks
        if (t >= w->sums.size()) w->sums.resize(t + 1);
        odam_trackwin::Sums& q = w->sums[t];
        const double* r = rows14 + (size_t)i * TW_COLS;
        q.n++;
        for (int c = 0; c < 3; c++) { q.sd[c] += r[6 + c]; q.st[c] += r[9 + c]; }      // row after row: numpy's axis-0 reduce of an [n, 3] block
        q.az.push_back(r[12]);
    }
    return 0;
}

// Bulk (re)build of the mirror: track t gets the last min(lengths[t], window) of its observations -- rows14 holds exactly those,
// track after track -- and the count lengths[t].  One upload and one launch; synchronises the stream (a rebuild is rare: first
// use, or the host edited its track list).
extern "C" int odam_trackwin_load(odam_trackwin* w, int T, const int* lengths, const double* rows14, void* stream) {
    if (!w || T < 0 || T > w->max_tracks || (T && (!lengths || !rows14))) return odam_fail(1, "odam_trackwin_load: bad argument");
    hipStream_t st = (hipStream_t)stream;
    ODAM_HIP(hipMemsetAsync(w->count, 0, sizeof(int) * (size_t)w->max_tracks, st));
    w->sums.clear(); w->sums_ok = T == 0;
    if (T == 0) return 0;
    std::vector<int> meta(2 * (size_t)T);      // [t] = first row of track t in rows14, [T + t] = its length
    long total = 0;
    for (int t = 0; t < T; t++) {
        if (lengths[t] < 0) return odam_fail(1, "odam_trackwin_load: negative track length");
        meta[t] = (int)total; meta[T + t] = lengths[t];
        total += lengths[t] < w->window ? lengths[t] : w->window;
    }
    // The kernel reads the handle's pinned staging itself (mapped host memory, sized for max_tracks full windows at creation): no
    // allocation here, no hipFree (it waits for every stream of the device -- for a detector running beside this caller) and no
    // copy command (free: every load ends with a stream synchronisation, so the staging is the caller's again when this returns).
    int rc = 0;
    std::memcpy(w->h_load, rows14, sizeof(double) * (size_t)total * TW_COLS);
    std::memcpy(w->h_load_meta, meta.data(), sizeof(int) * 2 * (size_t)T);
    {
        hipLaunchKernelGGL(trackwin_load_kernel, dim3(T), dim3(128), 0, st, w->h_load, w->h_load_meta, T, w->rows, w->count, w->window);
        if (hipGetLastError() != hipSuccess) rc = odam_fail(2, "odam_trackwin_load: launch failed");
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = odam_fail(2, "odam_trackwin_load: stream synchronisation failed");
    return rc;
}

// np.add.reduce of a 1-D float64 array (numpy/core/src/umath/loops_utils.h.src, pairwise sum, started from the identity):
// fewer than 8 values one after the other; up to 128 in eight interleaved partial sums combined as a tree, the tail after; longer
// arrays halved (the first half a multiple of 8) -- tests/test_assoc_gpu.py checks it against numpy bit for bit
static double np_pairwise(const double* a, size_t n) {
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; i++) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; j++) r[j] = a[j];
        size_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise(a, n2) + np_pairwise(a + n2, n - n2);
}

// the sums of a host track list in one go (after odam_trackwin_load): cols7 [host][sum_t lengths[t]][7] = columns 6..12 (dims x3,
// t_wo x3, az_wo) of EVERY observation of track 0, then of track 1, ...
extern "C" int odam_trackwin_load_sums(odam_trackwin* w, int T, const int* lengths, const double* cols7) {
    if (!w || T < 0 || T > w->max_tracks || (T && (!lengths || !cols7))) return odam_fail(1, "odam_trackwin_load_sums: bad argument");
    w->sums.assign((size_t)T, odam_trackwin::Sums());
    const double* r = cols7;
    for (int t = 0; t < T; t++) {
        odam_trackwin::Sums& q = w->sums[t];
        if (lengths[t] < 1) return odam_fail(1, "odam_trackwin_load_sums: a track without observations");
        q.n = lengths[t];
        q.az.resize((size_t)lengths[t]);
        for (int i = 0; i < lengths[t]; i++, r += 7) {
            for (int c = 0; c < 3; c++) { q.sd[c] += r[c]; q.st[c] += r[3 + c]; }
            q.az[i] = r[6];
        }
    }
    w->sums_ok = true;
    return 0;
}

// parameter rows the surfaces of the tracks are evaluated from, as sq.init_params / _prepare_tracks build them (processor.py:172-180):
// mean centre, mean azimuth, sqrt(max(mean dims, 0.05) / 2), shape exponents -0;  out [host][T][9] float32
extern "C" int odam_trackwin_params(odam_trackwin* w, int T, float* out) {
    if (!w || T < 0 || (T && !out)) return odam_fail(1, "odam_trackwin_params: bad argument");
    if (!w->sums_ok || (size_t)T != w->sums.size()) return odam_fail(4, "odam_trackwin_params: the running sums do not cover these tracks (load them: odam_trackwin_load_sums)");
    for (int t = 0; t < T; t++) {
        const odam_trackwin::Sums& q = w->sums[t];
        const double n = (double)q.n;
        float* o = out + (size_t)t * 9;
        for (int c = 0; c < 3; c++) o[c] = (float)(q.st[c] / n);
        o[3] = (float)((0.0 + np_pairwise(q.az.data(), q.az.size())) / n);
        for (int c = 0; c < 3; c++) {
            const double d = q.sd[c] / n;
            o[4 + c] = (float)std::sqrt((d > 0.05 ? d : 0.05) / 2);       // np.maximum(., 0.05); NaN stays NaN in numpy -- not reachable, dims come from a sigmoid
        }
        o[7] = o[8] = -0.0f;
    }
    return 0;
}

// One call for OdamProcess._prepare_tracks: parameter rows (above) -> upload -> odam_sq_project_extents on `sq` -> the window tensor
// out [dev][T][79][window] for the camera T_cw12_K9 = rows 0..2 of inv(T_wc) (12) + K (9), azimuth cam_azi, image size.  Stream-ordered.
extern "C" int odam_trackwin_build_tracks(odam_trackwin* w, struct odam_sq_ctx* sq, int T, const double* T_cw12_K9, double cam_azi,
                                          double img_w, double img_h, float* out, void* stream) {
    if (!w || !sq || T < 0 || T > w->max_tracks || (T && (!T_cw12_K9 || !out))) return odam_fail(1, "odam_trackwin_build_tracks: bad argument");
    if (T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (!w->h_params) {
        if (hipHostMalloc((void**)&w->h_params, sizeof(float) * 8 * (size_t)w->max_tracks * 9, hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void**)&w->d_proj, sizeof(double) * (size_t)w->max_tracks * 4) != hipSuccess) {
            if (w->h_params) { (void)hipHostFree(w->h_params); w->h_params = nullptr; }
            return odam_fail(2, "odam_trackwin_build_tracks: allocation failed");
        }
        for (int i = 0; i < 8; i++) ODAM_HIP(hipEventCreateWithFlags(&w->params_copied[i], hipEventDisableTiming));
    }
    const int si = (int)(w->params_slot++ & 7);
    if (w->params_armed[si]) ODAM_HIP(hipEventSynchronize(w->params_copied[si]));
    float* hp = w->h_params + (size_t)si * w->max_tracks * 9;
    if (int rc = odam_trackwin_params(w, T, hp)) return rc;
    // the surface kernel reads the pinned rows itself (mapped host memory, 36 bytes per track): no copy command; the slot is free
    // again when the launches that read it have run
    if (int rc = odam_sq_project_extents(sq, T, hp, T_cw12_K9, w->d_proj, stream)) return rc;
    ODAM_HIP(hipEventRecord(w->params_copied[si], st));
    w->params_armed[si] = true;
    double cam15[15];
    for (int i = 0; i < 12; i++) cam15[i] = T_cw12_K9[i];
    cam15[12] = cam_azi; cam15[13] = img_w; cam15[14] = img_h;
    return odam_trackwin_build(w, T, w->d_proj, cam15, out, stream);
}

extern "C" int odam_trackwin_build(odam_trackwin* w, int T, const double* proj_px, const double* cam15, float* out, void* stream) {
    if (!w || T < 0 || T > w->max_tracks || (T && (!proj_px || !cam15 || !out))) return odam_fail(1, "odam_trackwin_build: bad argument");
    if (T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    Cam15 cam;
    for (int i = 0; i < 15; i++) cam.v[i] = cam15[i];
    hipLaunchKernelGGL(trackwin_build_kernel, dim3(T), dim3(128), 0, st, w->rows, w->count, w->window, proj_px, cam, out);
    ODAM_HIP(hipGetLastError());
    return 0;
}
