// assoc_internal.h -- what crosses the association's translation units (assoc.hip, assoc_sinkhorn.hip); not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace odam_assoc_internal
