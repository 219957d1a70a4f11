// track_emit.hip -- the IoU tracker's detections written to the resident row store as track rows (include/odam_rows.h:
// odam_rows_emit_tracked, odam_rows_marks).  DESIGN.md section 6t.
//
// A slot is one of the 30 detection places of a frame: slot i = 30 k + d.  It is EMITTED iff d < min(max(det_count[k], 0), 30) and
// 0 <= ids[k][d] < n_tracks, and its row goes to log position base + (number of emitted slots in front of it): the (k, d)
// lexicographic order, which is the arrival order OdamProcess._track_frames_iou builds on the host.  Chunks of ODAM_ROWS_CHUNK = 4096
// slots, three plain launches:
//   emit_count_kernel    one workgroup per chunk: the chunk's emitted slots and whether it saw an id >= n_tracks -> work; the
//                        per-track outputs of the call start here (count 0, positions -1), grid-strided
//   emit_scan_kernel     ONE workgroup: exclusive scan of the chunk counts in place (at most 4096 chunks), n_emitted, and the status
//                        word -- whether base + n_emitted fits in cap is decided HERE, before any row is stored
//   emit_scatter_kernel  one workgroup per chunk: flags again (the same function), the four waves own consecutive quarters of the
//                        chunk and walk them 64 slots at a time in order, the rank of a slot in its step is a ballot's popcount
//                        below the lane; the lane of an emitted slot forms the 14 doubles and stores them, 16 bytes at a time
// Every position is a sum of integer counts, so the log has the same bits on every run.  Integer atomics touch the per-track row
// counts and the smallest / largest position of a track only, all of them order-independent.  Binary64 without contraction.
//
// Bounds: a frame's count is clamped before it is compared; an id is compared with [0, n_tracks) before it indexes anything; a
// position is compared with [base, cap) before the store (the scan's check makes that true of every one of them; the comparison
// stays).  odam_rows_marks compares a position with [0, n_log) before it reads the row.
#include <hip/hip_runtime.h>

#include "../../include/odam_rows.h"
#include "odam_err.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = ODAM_ROWS_CHUNK;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int STEPS = CHUNK / THREADS;      // 64-slot steps of one wave
constexpr int DETS = ODAM_ROWS_EMIT_DETS, DET_COLS = 15;
constexpr int MAX_SLOTS = ODAM_ROWS_MAX_ROWS;
static_assert(CHUNK == WAVES * STEPS * 64, "a chunk is four waves' quarters");
static_assert(MAX_SLOTS / CHUNK <= 4096, "the scan's one workgroup walks at most 4096 chunk counts");

struct EmitArgs {
    const float* blk;
    const int* cnt;
    const int* ids;
    const double* T;
    const double* azi;
    double* rows;
    int* tid;
    int* n_emitted;
    int* counts;
    int* first_pos;
    int* last_pos;
    int* status;
    int* chunk_off;      // [n_chunks]: the chunk's count, after the scan the emitted slots in front of the chunk
    int* chunk_bad;      // [n_chunks]
    double img_w, img_h;
    int n_slots, n_tracks, n_chunks, base, cap;
};

// the id of slot i where the slot is emitted, -1 otherwise; bad: a live slot whose id is beyond the track list
__device__ __forceinline__ int slot_id(const EmitArgs& A, int i, bool& bad) {
    bad = false;
    if (i >= A.n_slots) return -1;
    const int k = i / DETS, d = i - k * DETS;
    const int c = A.cnt[k];
    const int n = c < 0 ? 0 : c > DETS ? DETS : c;
    if (d >= n) return -1;
    const int t = A.ids[i];
    if (t < 0) return -1;
    bad = t >= A.n_tracks;
    return bad ? -1 : t;
}

__global__ __launch_bounds__(THREADS) void emit_count_kernel(EmitArgs A) {
    __shared__ int s_w[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x;
    for (int t = chunk * THREADS + tid; t < A.n_tracks; t += gridDim.x * THREADS) {
        A.counts[t] = 0;
        A.first_pos[t] = -1;
        A.last_pos[t] = -1;
    }
    int n = 0;
    bool bad = false;
#pragma unroll
    for (int it = 0; it < STEPS; it++) {
        bool b;
        n += slot_id(A, chunk * CHUNK + it * THREADS + tid, b) >= 0;
        bad |= b;
    }
    int total;
    wg_exclusive_scan(n, total, s_w, lane, wave, WAVES);
    const bool any_bad = __syncthreads_or(bad);
    if (tid == 0) {
        A.chunk_off[chunk] = total;
        A.chunk_bad[chunk] = any_bad;
    }
}

__global__ __launch_bounds__(THREADS) void emit_scan_kernel(EmitArgs A) {
    __shared__ int s_w[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    bool bad = false;
    for (int c0 = 0; c0 < A.n_chunks; c0 += THREADS) {
        const int c = c0 + tid;
        const int v = c < A.n_chunks ? A.chunk_off[c] : 0;
        bad |= c < A.n_chunks && A.chunk_bad[c] != 0;
        int total;
        const int excl = wg_exclusive_scan(v, total, s_w, lane, wave, WAVES);
        if (c < A.n_chunks) A.chunk_off[c] = carry + excl;
        carry += total;
        __syncthreads();
    }
    const bool any_bad = __syncthreads_or(bad);
    if (tid == 0) {
        *A.n_emitted = carry;
        *A.status = (any_bad ? ODAM_ROWS_EMIT_BAD_ID : 0) | (carry > A.cap - A.base ? ODAM_ROWS_EMIT_OVERFLOW : 0);
    }
}

// the 14 doubles of slot i of frame k, detection row r (15 float32), as seven 16-byte words at log position pos
__device__ __forceinline__ void store_row(const EmitArgs& A, int k, const float* r, long long pos) {
    const double* T = A.T + 16ll * k;
    const double x = (double)r[9], y = (double)r[10], z = (double)r[11];
    double v[14];
    v[0] = (double)r[0];
    v[1] = (double)r[1];
    v[2] = (double)r[2] * A.img_w;
    v[3] = (double)r[3] * A.img_h;
    v[4] = (double)r[4] * A.img_w;
    v[5] = (double)r[5] * A.img_h;
    v[6] = (double)r[6];
    v[7] = (double)r[7];
    v[8] = (double)r[8];
#pragma unroll
    for (int q = 0; q < 3; q++) v[9 + q] = ((x * T[4 * q] + y * T[4 * q + 1]) + z * T[4 * q + 2]) + T[4 * q + 3];
    v[12] = atan2((double)r[12], (double)r[13]) + A.azi[k];
    v[13] = (double)r[14];
    double2* out = (double2*)(A.rows + 14ll * pos);
#pragma unroll
    for (int q = 0; q < 7; q++) out[q] = make_double2(v[2 * q], v[2 * q + 1]);
}

__global__ __launch_bounds__(THREADS) void emit_scatter_kernel(EmitArgs A) {
    __shared__ int s_w[WAVES];
    if (*A.status & ODAM_ROWS_EMIT_OVERFLOW) return;      // (the scan's word: the same for every workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x;
    int id[STEPS];
    int mine = 0;      // emitted slots of this wave's quarter (the same in every lane)
#pragma unroll
    for (int it = 0; it < STEPS; it++) {
        bool b;
        id[it] = slot_id(A, chunk * CHUNK + (wave * STEPS + it) * 64 + lane, b);
        mine += __popcll(__ballot(id[it] >= 0));
    }
    if (lane == 0) s_w[wave] = mine;
    __syncthreads();
    int run = A.base + A.chunk_off[chunk];
    for (int w = 0; w < wave; w++) run += s_w[w];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int it = 0; it < STEPS; it++) {
        const bool on = id[it] >= 0;
        const unsigned long long m = __ballot(on);
        const int pos = run + __popcll(m & below);
        run += __popcll(m);
        if (on && pos >= A.base && pos < A.cap) {
            const int i = chunk * CHUNK + (wave * STEPS + it) * 64 + lane;
            store_row(A, i / DETS, A.blk + (long long)DET_COLS * i, pos);
            A.tid[pos] = id[it];
            atomicAdd(&A.counts[id[it]], 1);
            atomicMin((unsigned*)&A.first_pos[id[it]], (unsigned)pos);      // -1 is the largest unsigned
            atomicMax(&A.last_pos[id[it]], pos);
        }
    }
}

// thread t < n_tracks: the track's row of the block; thread n_tracks: the call's own row
__global__ __launch_bounds__(THREADS) void rows_marks_kernel(const double* rows, int n_log, const int* counts, const int* first_pos,
                                                             const int* last_pos, const int* n_emitted, const int* status, int n_tracks,
                                                             double* out) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t > n_tracks) return;
    double* o = out + 4ll * t;
    if (t == n_tracks) {
        o[0] = (double)*n_emitted;
        o[1] = (double)*status;
        o[2] = 0.0;
        o[3] = 0.0;
        return;
    }
    const int f = first_pos[t], l = last_pos[t];
    const bool has_f = (unsigned)f < (unsigned)n_log, has_l = (unsigned)l < (unsigned)n_log;
    o[0] = (double)counts[t];
    o[1] = has_f ? rows[14ll * f] : -1.0;
    o[2] = has_l ? rows[14ll * l] : -1.0;
    o[3] = has_l ? rows[14ll * l + 9] : -1.0;
}

inline int n_chunks_of(long long slots) { return (int)((slots + CHUNK - 1) / CHUNK); }

inline size_t emit_work_bytes(int N) { return N == 0 ? 0 : (sizeof(int) * 2 * (size_t)n_chunks_of((long long)N * DETS) + 15) / 16 * 16; }

}  // namespace

extern "C" int odam_rows_emit_workspace(int N, size_t* bytes) {
    if (!bytes) return odam_fail(ODAM_E_INVALID, "odam_rows_emit_workspace: null pointer");
    if (N < 0) return odam_fail(ODAM_E_INVALID, "odam_rows_emit_workspace: bad size");
    if ((long long)N * DETS > MAX_SLOTS) return odam_fail(ODAM_E_LIMIT, "odam_rows_emit_workspace: more than 2^24 detection slots");
    *bytes = emit_work_bytes(N);
    return ODAM_OK;
}

extern "C" int odam_rows_emit_tracked(const float* det_block, const int* det_count, const int* ids, const double* T_wc,
                                      const double* cam_azi, int N, double img_w, double img_h, int n_tracks, double* rows, int* tid,
                                      int base, int cap, int* n_emitted, int* counts, int* first_pos, int* last_pos, int* status,
                                      void* work, size_t work_bytes, void* stream) {
    if (N < 0 || n_tracks < 0) return odam_fail(ODAM_E_INVALID, "odam_rows_emit_tracked: bad size");
    if ((long long)N * DETS > MAX_SLOTS) return odam_fail(ODAM_E_LIMIT, "odam_rows_emit_tracked: more than 2^24 detection slots");
    if (n_tracks > ODAM_ROWS_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_rows_emit_tracked: more than 65536 tracks");
    if (N == 0) return ODAM_OK;
    if (!det_block || !det_count || !ids || !T_wc || !cam_azi || !rows || !tid || !n_emitted || !counts || !first_pos || !last_pos ||
        !status || !work)
        return odam_fail(ODAM_E_INVALID, "odam_rows_emit_tracked: null pointer");
    if (base < 0 || cap < base) return odam_fail(ODAM_E_INVALID, "odam_rows_emit_tracked: base outside 0 .. cap");
    if (work_bytes < emit_work_bytes(N) || ((size_t)work & 15))
        return odam_fail(ODAM_E_INVALID, "odam_rows_emit_tracked: the workspace is smaller than odam_rows_emit_workspace says, or not 16-byte aligned");
    if ((size_t)rows & 15) return odam_fail(ODAM_E_INVALID, "odam_rows_emit_tracked: the log must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    EmitArgs A{};
    A.blk = det_block; A.cnt = det_count; A.ids = ids; A.T = T_wc; A.azi = cam_azi; A.rows = rows; A.tid = tid;
    A.n_emitted = n_emitted; A.counts = counts; A.first_pos = first_pos; A.last_pos = last_pos; A.status = status;
    A.img_w = img_w; A.img_h = img_h; A.n_slots = N * DETS; A.n_tracks = n_tracks; A.base = base; A.cap = cap;
    A.n_chunks = n_chunks_of(A.n_slots);
    A.chunk_off = (int*)work; A.chunk_bad = A.chunk_off + A.n_chunks;
    hipLaunchKernelGGL(emit_count_kernel, dim3((unsigned)A.n_chunks), dim3(THREADS), 0, st, A);
    ODAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(emit_scan_kernel, dim3(1), dim3(THREADS), 0, st, A);
    ODAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(emit_scatter_kernel, dim3((unsigned)A.n_chunks), dim3(THREADS), 0, st, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_rows_marks(const double* rows, int n_log, const int* counts, const int* first_pos, const int* last_pos,
                               const int* n_emitted, const int* status, int n_tracks, double* out, void* stream) {
    if (n_log < 0 || n_tracks < 0) return odam_fail(ODAM_E_INVALID, "odam_rows_marks: bad size");
    if (n_tracks > ODAM_ROWS_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_rows_marks: more than 65536 tracks");
    if (!n_emitted || !status || !out || (n_tracks > 0 && (!rows || !counts || !first_pos || !last_pos)))
        return odam_fail(ODAM_E_INVALID, "odam_rows_marks: null pointer");
    hipLaunchKernelGGL(rows_marks_kernel, dim3((unsigned)(n_tracks / THREADS + 1)), dim3(THREADS), 0, (hipStream_t)stream, rows, n_log,
                       counts, first_pos, last_pos, n_emitted, status, n_tracks, out);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
