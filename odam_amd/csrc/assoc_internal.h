// assoc_internal.h -- what crosses the association's translation units (assoc.hip, assoc_sinkhorn.hip, assoc_batch.hip); not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "odam_err.h"

namespace odam_assoc_internal {

// Barrier words of the persistent matching kernels (assoc.hip), zero before every launch: generation + error flag line, PG_GROUPS group
// counters and PG_GROUPS per-XCD counters (each on its own 128-byte line), one line of PG_GROUPS placement words (gnn_rowpart_kernel:
// XCC id + 1 of each group).  The one-wavefront Sinkhorn kernel behind a persistent launch reads the flag and zeroes them all again.
constexpr int PG_GROUPS = 8, PG_BAR_WORDS = 32 * (2 + 2 * PG_GROUPS);

// log_optimal_transport on the device: the one-wavefront kernel where it applies, the 31-column kernel, the general one otherwise.
// n_dev (device, may be null): the column count of THIS launch, n_cap its bound.  err (may be null): the persistent kernel's flag word
// (bar + 1) -- when set, Z_out becomes NaN and *lost_count moves; *cleans_bar: this launch leaves the barrier words at zero.
__attribute__((visibility("hidden"))) int launch_sinkhorn(const float* scores, int lds_, int m_, int n_, int n_cap, float alpha, int iters,
                                                          float* Z_out, const int* n_dev, hipStream_t st, const unsigned* err = nullptr,
                                                          unsigned* lost_count = nullptr, bool* cleans_bar = nullptr);

struct Lin { float* w = nullptr; float* b = nullptr; int K = 0, N = 0; };
struct Prop { Lin qkv, merge, m0, m2; };   // AttentionalPropagation (associator.py:85-97); q, k, v stacked

struct HostT { std::vector<long long> shape; std::vector<float> data; };

// The batched forward (assoc_batch.hip) takes at most this many samples: the encoder's workspaces (feat, h256, catT) hold the 30 detection
// rows of every sample behind the tracks' rows.
constexpr int MAX_BATCH = 64;

// One pinned slot + device mirror of the per-sample descriptors of a batched forward (assoc_batch.hip)
struct BatchState;

// y[M, L.N] = act(x[M, L.K] L.w^T + L.b (+ res)) on the tiles of conv_gemm.hip (assoc.hip)
__attribute__((visibility("hidden"))) int assoc_lin(const Lin& L, const float* x, int lda, int M, const float* res, bool relu, float* y, int ldc,
                                                    const float* scale, hipStream_t st);

}  // namespace odam_assoc_internal

struct odam_assoc {
    using Lin = odam_assoc_internal::Lin;
    using Prop = odam_assoc_internal::Prop;
    using HostT = odam_assoc_internal::HostT;
    int max_tracks = 0, n_self = 0, n_gnn = 0, iters = 100;
    std::vector<int> gnn_cross;          // per GNN layer: 1 = cross
    std::map<std::string, HostT> host;
    bool finalized = false;
    std::vector<void*> allocs;
    Lin enc0, enc2, final_proj;
    std::vector<Prop> fuser, gnn;
    float bin_score = 1.0f;
    float *div_term = nullptr, *sc16 = nullptr;
    // workspace
    float *feat = nullptr, *h256 = nullptr, *catT = nullptr, *kv = nullptr, *att = nullptr, *h512 = nullptr;
    float *kvX = nullptr, *kvX2 = nullptr, *attX = nullptr, *hX = nullptr;
    float *catTr = nullptr, *mT = nullptr, *scores = nullptr;
    // persistent matching kernel: barrier counters (+ error flag), zeroed on the stream before every launch
    unsigned* bar = nullptr;
    bool persist = true;
    int resident_capacity = 0;               // workgroups of the persistent kernel the device can hold at once (with the guide's margin)
    unsigned long long timeout_ticks = 2000000ull;   // 20 ms per barrier wait (100 MHz ticks); a healthy wait is ~2 us, ~1 ms under a saturated device
    unsigned* lost_count = nullptr;          // pinned host word: launches abandoned at a barrier so far (the Sinkhorn kernel bumps it)
    unsigned long long* stamps = nullptr;    // device, 128 entries; written only while want_stamps
    bool want_stamps = false;
    bool fake_misplaced = false;             // tests: odam_assoc_debug_misplace
    bool bar_clean = false;                  // the counters are zero: the one-wavefront Sinkhorn kernel zeroes them behind the launch that used them
    bool merged = false;                     // odam_config assoc.merge as read by odam_assoc_finalize: every Prop's m0 holds the merge projection too
    odam_assoc_internal::BatchState* batch = nullptr;      // the batched forward's workspaces (odam_assoc_reserve_batch), or null

    // Zeroing goes through a private non-blocking stream that finalize waits for: hipMemset would be ordered on the NULL stream -- it
    // may still be pending when it returns (and then land behind the first results of a caller that works on a stream of its own),
    // and waiting for the NULL stream instead would wait for whatever another thread has queued there (a detector's chunk copies).
    hipStream_t init_stream = nullptr;
    int alloc(float** p, size_t n) {
        ODAM_HIP(hipMalloc((void**)p, n * sizeof(float)));
        if (!init_stream) ODAM_HIP(hipStreamCreateWithFlags(&init_stream, hipStreamNonBlocking));
        ODAM_HIP(hipMemsetAsync(*p, 0, n * sizeof(float), init_stream));
        allocs.push_back(*p);
        return 0;
    }
    int init_done() {
        if (init_stream) { ODAM_HIP(hipStreamSynchronize(init_stream)); ODAM_HIP(hipStreamDestroy(init_stream)); init_stream = nullptr; }
        return 0;
    }
    int upload(float** p, const std::vector<float>& v) {
        if (int rc = alloc(p, v.size())) return rc;
        ODAM_HIP(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, init_stream));   // behind the memset of the same buffer
        ODAM_HIP(hipStreamSynchronize(init_stream));        // v may be a temporary
        return 0;
    }
};

namespace odam_assoc_internal {

// encoder + frame-index encoding + the fuser layers over n_seq tracks [n_seq, 79, 100] and n_det_rows detection slots (30 per sample,
// channel-first [.., 79, 30]): m->catT rows 0 .. 100 n_seq - 1 hold the fuser's output, rows 100 n_seq .. the encoded detections (assoc.hip)
__attribute__((visibility("hidden"))) int encode_and_fuse(odam_assoc* m, const float* tracks, int n_seq, const float* detections, int n_det_rows,
                                                          hipStream_t st);
// frees what odam_assoc_reserve_batch made (assoc_batch.hip); called by odam_assoc_destroy
__attribute__((visibility("hidden"))) void batch_release(odam_assoc* m);
// odam_assoc_debug_read's which = 3 (the padded row block as assembled), 4 (its descriptors), both [(B Tmax + 30 B), 256], and 5 (the
// score blocks [sum T, 32]) (assoc_batch.hip)
__attribute__((visibility("hidden"))) int batch_debug_read(odam_assoc* m, int which, float* out, long long n);

}  // namespace odam_assoc_internal
