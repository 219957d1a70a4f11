// track_rows.hip -- the device-resident track-row store's two kernels (include/odam_rows.h): the stable order of a row log by track
// (odam_rows_group) and the gather of whole 112-byte rows (odam_rows_gather14).  DESIGN.md section 6p.
//
// odam_rows_group is an LSD radix sort of the log indices on the track id, 8-bit digits: one pass for n_tracks <= 256, two beyond.
// A pass is a stable counting sort over chunks of ODAM_ROWS_CHUNK = 4096 rows, three plain launches:
//   rows_hist_kernel     one workgroup per chunk: the chunk's digit histogram (integer LDS atomics) -> hist[digit][chunk]
//   rows_scan_kernel     one workgroup per digit: exclusive scan of hist[digit][.] over the chunks in place, the digit's total
//   rows_scatter_kernel  one workgroup per chunk: start of every digit (scan of the 256 totals) + the chunk's offset, then the four
//                        waves own consecutive quarters of the chunk and walk them 64 rows at a time IN ORDER: the rank of a row among
//                        the rows of its digit in the step comes from a ballot match over the 8 digit bits, the running count of the
//                        digit lives in the wave's own LDS row -- no atomic touches a position, so the order is the log's
// A log of one chunk (N <= 4096) needs neither histogram nor scan: rows_scatter_kernel counts for itself, ONE launch per pass.
// The counts are sums of integers: the permutation is the same on every run, whatever order the workgroups finish in.  Nothing waits
// on another workgroup inside a launch.
//
// Bounds: an id is compared with [0, n_tracks) before it is a key (a bad one sorts as track 0 and sets status 1); an index read from
// the first pass's output is compared with [0, N) before it is used; a position is compared with [0, N) before the store.  row_off
// is read at a checked id only, and only to be compared: the last pass asks of every row whether its place lies inside its track's
// range, and of every track whether the range is well-formed -- with all ids good that is the statement "every track has
// row_off[t+1] - row_off[t] rows and row_off[0] = 0" (the ranges then tile [0, N), and N rows in N places fill every one of them).
#include <hip/hip_runtime.h>

#include "../../include/odam_rows.h"
#include "odam_err.h"
#include "wave_ops.h"

namespace {

constexpr int CHUNK = ODAM_ROWS_CHUNK;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int STEPS = CHUNK / THREADS;      // 64-row steps of one wave, rows of one thread
static_assert(CHUNK == WAVES * STEPS * 64, "a chunk is four waves' quarters");

struct GroupArgs {
    const int* tid;
    const int* row_off;
    const int* src_in;      // indices in the order of the pass before; null in the first pass: the log's own order
    int* dst;
    int* hist;              // [256][n_chunks]
    int* tot;               // [256]
    int* status;
    int N, n_tracks, n_chunks, shift, first, last;
    int solo;               // the log is ONE chunk: the scatter kernel counts for itself, no histogram and no scan launch
};

// the log index at place i of this pass's input and its key: the id where it is one, track 0 otherwise
__device__ __forceinline__ void key_at(const GroupArgs& A, int i, int& src, int& key, bool& good) {
    src = A.src_in ? A.src_in[i] : i;
    if ((unsigned)src >= (unsigned)A.N) src = 0;
    const int t = A.tid[src];
    good = (unsigned)t < (unsigned)A.n_tracks;
    key = good ? t : 0;
}

__global__ __launch_bounds__(THREADS) void rows_hist_kernel(GroupArgs A) {
    __shared__ int s_hist[256];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int it = 0; it < STEPS; it++) {
        const int i = chunk * CHUNK + it * THREADS + tid;
        if (i < A.N) {
            int src, key;
            bool good;
            key_at(A, i, src, key, good);
            bad |= !good;
            atomicAdd(&s_hist[(key >> A.shift) & 255], 1);
        }
    }
    __syncthreads();
    A.hist[(size_t)tid * A.n_chunks + chunk] = s_hist[tid];
    if (A.first && bad) *A.status = ODAM_ROWS_BAD_ID;      // (every writer stores the same word)
}

__global__ __launch_bounds__(THREADS) void rows_scan_kernel(int* hist, int* tot, int n_chunks) {
    __shared__ int s_w[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* h = hist + (size_t)blockIdx.x * n_chunks;
    int carry = 0;
    for (int base = 0; base < n_chunks; base += THREADS) {
        const int c = base + tid;
        const int v = c < n_chunks ? h[c] : 0;
        int total;
        const int excl = wg_exclusive_scan(v, total, s_w, lane, wave, WAVES);
        if (c < n_chunks) h[c] = carry + excl;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) tot[blockIdx.x] = carry;
}

__global__ __launch_bounds__(THREADS) void rows_scatter_kernel(GroupArgs A) {
    __shared__ int s_cnt[WAVES][256];
    __shared__ int s_w[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x;
#pragma unroll
    for (int w = 0; w < WAVES; w++) s_cnt[w][tid] = 0;
    __syncthreads();
    int key[STEPS], src[STEPS];      // key -1: no row (past the end of the log)
    bool bad = false;
#pragma unroll
    for (int it = 0; it < STEPS; it++) {
        const int i = chunk * CHUNK + (wave * STEPS + it) * 64 + lane;
        key[it] = -1;
        src[it] = 0;
        if (i < A.N) {
            bool good;
            key_at(A, i, src[it], key[it], good);
            bad |= !good;
            atomicAdd(&s_cnt[wave][(key[it] >> A.shift) & 255], 1);
        }
    }
    // (a log of several chunks learnt of a bad id in rows_hist_kernel, a launch of its own)
    const bool any_bad = A.solo && A.first && __syncthreads_or(bad);
    if (any_bad && tid == 0) *A.status = ODAM_ROWS_BAD_ID;
    __syncthreads();
    // thread d: where digit d starts in the output, where this chunk's share of it starts, and from there the four waves' shares
    int total;
    const int of_digit = A.solo ? s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid] : A.tot[tid];
    const int start = wg_exclusive_scan(of_digit, total, s_w, lane, wave, WAVES);
    int run = start + (A.solo ? 0 : A.hist[(size_t)tid * A.n_chunks + chunk]);
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const int c = s_cnt[w][tid];
        s_cnt[w][tid] = run;
        run += c;
    }
    __syncthreads();
    int* mine = s_cnt[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
    bool off_ok = true;
#pragma unroll
    for (int it = 0; it < STEPS; it++) {
        const bool active = key[it] >= 0;
        const int d = active ? (key[it] >> A.shift) & 255 : 0;
        unsigned long long same = __ballot(active);      // the lanes of this step that hold a row of the same digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1;
            const unsigned long long has = __ballot(active && bit);
            same &= bit ? has : ~has;
        }
        const int rank = __popcll(same & below);
        const int at = active ? mine[d] : 0;
        wave_lds_sync();
        if (active && rank == 0) mine[d] = at + __popcll(same);
        wave_lds_sync();
        const int pos = at + rank;
        if (active && (unsigned)pos < (unsigned)A.N) {
            A.dst[pos] = src[it];
            if (A.last) off_ok &= A.row_off[key[it]] <= pos && pos < A.row_off[key[it] + 1];
        }
    }
    if (A.last) {
        // the ranges themselves: ascending from 0 to N
        for (int t = chunk * THREADS + tid; t < A.n_tracks; t += gridDim.x * THREADS) {
            const int lo = A.row_off[t], hi = A.row_off[t + 1];
            off_ok &= lo <= hi && (t > 0 || lo == 0) && (t < A.n_tracks - 1 || hi == A.N);
        }
        // a bad id stays: it was written a launch ago at the latest, or by this workgroup (any_bad)
        if (!off_ok && !any_bad) atomicCAS(A.status, ODAM_ROWS_OK, ODAM_ROWS_BAD_COUNT);
    }
}

// seven 16-byte words per row, one per thread
__global__ __launch_bounds__(THREADS) void rows_gather14_kernel(const uint4* log, const int* src, int N, uint4* out) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= 7ll * N) return;
    const int i = (int)(g / 7);
    const int p = (int)(g - 7ll * i);
    const int s = src[i];
    if ((unsigned)s >= (unsigned)N) return;
    out[g] = log[7ll * s + p];
}

inline int n_chunks_of(int N) { return (N + CHUNK - 1) / CHUNK; }

inline size_t work_ints(int N, int n_tracks) {
    if (N == 0 || n_tracks == 0) return 0;
    return (size_t)256 * n_chunks_of(N) + 256 + (n_tracks > 256 ? (size_t)N : 0);
}

}  // namespace

extern "C" int odam_rows_group_workspace(int N, int n_tracks, size_t* bytes) {
    if (!bytes) return odam_fail(ODAM_E_INVALID, "odam_rows_group_workspace: null pointer");
    if (N < 0 || n_tracks < 0) return odam_fail(ODAM_E_INVALID, "odam_rows_group_workspace: bad size");
    if (N > ODAM_ROWS_MAX_ROWS) return odam_fail(ODAM_E_LIMIT, "odam_rows_group_workspace: more than 2^24 rows");
    if (n_tracks > ODAM_ROWS_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_rows_group_workspace: more than 65536 tracks");
    *bytes = (sizeof(int) * work_ints(N, n_tracks) + 15) / 16 * 16;
    return ODAM_OK;
}

extern "C" int odam_rows_group(const int* tid, int N, int n_tracks, const int* row_off, int* src_out, int* status, void* work,
                               size_t work_bytes, void* stream) {
    if (N < 0 || n_tracks < 0) return odam_fail(ODAM_E_INVALID, "odam_rows_group: bad size");
    if (N > ODAM_ROWS_MAX_ROWS) return odam_fail(ODAM_E_LIMIT, "odam_rows_group: more than 2^24 rows");
    if (n_tracks > ODAM_ROWS_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_rows_group: more than 65536 tracks");
    if (N == 0 || n_tracks == 0) return ODAM_OK;
    if (!tid || !row_off || !src_out || !status || !work) return odam_fail(ODAM_E_INVALID, "odam_rows_group: null pointer");
    if (work_bytes < sizeof(int) * work_ints(N, n_tracks) || ((size_t)work & 15))
        return odam_fail(ODAM_E_INVALID, "odam_rows_group: the workspace is smaller than odam_rows_group_workspace says, or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int n_chunks = n_chunks_of(N);
    const int passes = n_tracks > 256 ? 2 : 1;
    GroupArgs A{};
    A.tid = tid; A.row_off = row_off; A.status = status; A.N = N; A.n_tracks = n_tracks; A.n_chunks = n_chunks;
    A.hist = (int*)work; A.tot = A.hist + (size_t)256 * n_chunks; A.solo = n_chunks == 1;
    int* mid = A.tot + 256;      // the order after the first of two passes
    ODAM_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    for (int p = 0; p < passes; p++) {
        A.shift = 8 * p; A.first = p == 0; A.last = p == passes - 1;
        A.src_in = p == 0 ? nullptr : mid;
        A.dst = A.last ? src_out : mid;
        if (!A.solo) {
            hipLaunchKernelGGL(rows_hist_kernel, dim3((unsigned)n_chunks), dim3(THREADS), 0, st, A);
            ODAM_HIP(hipGetLastError());
            hipLaunchKernelGGL(rows_scan_kernel, dim3(256), dim3(THREADS), 0, st, A.hist, A.tot, n_chunks);
            ODAM_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(rows_scatter_kernel, dim3((unsigned)n_chunks), dim3(THREADS), 0, st, A);
        ODAM_HIP(hipGetLastError());
    }
    return ODAM_OK;
}

extern "C" int odam_rows_gather14(const double* log, const int* src, int N, double* out, void* stream) {
    if (N < 0) return odam_fail(ODAM_E_INVALID, "odam_rows_gather14: bad size");
    if (N > ODAM_ROWS_MAX_ROWS) return odam_fail(ODAM_E_LIMIT, "odam_rows_gather14: more than 2^24 rows");
    if (N == 0) return ODAM_OK;
    if (!log || !src || !out) return odam_fail(ODAM_E_INVALID, "odam_rows_gather14: null pointer");
    if (((size_t)log & 15) || ((size_t)out & 15)) return odam_fail(ODAM_E_INVALID, "odam_rows_gather14: rows must be 16-byte aligned");
    const long long words = 7ll * N;
    hipLaunchKernelGGL(rows_gather14_kernel, dim3((unsigned)((words + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       (const uint4*)log, src, N, (uint4*)out);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
