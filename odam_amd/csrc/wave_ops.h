// wave_ops.h -- the cross-lane and cross-wave pieces of the scene-side kernels: reductions over a 64-lane wavefront, the workgroup
// scan, the bitonic sort of LDS keys and the two searches over an offsets table.  Device-only, header-only, every function inlined.
//
// THE reduction tree.  wave_sum and wave_reduce merge the 64 lanes through a butterfly of six rounds, partner = lane XOR 32, 16, 8,
// 4, 2, 1 in this order, each round x <- x (+) partner's x, the lane's own value on the left; for a commutative (+) every lane ends
// with the same bits.  The order is part of the contract of the kernels whose sums are checked bit for bit: tests/dq_ref.wave_sums
// (reproject_ref.wave_sums, quadric_svd_ref) restates it.  sk_wave.h (and wave_sum_f64, wave_or of det_loss.hip) is the OTHER tree:
// lane bit 0 first and bit 5 last on DPP / v_permlane*_swap, a different order of additions and different bits
// (tests/criterion_ref.py restates that one).  The two are not interchangeable.
#pragma once
#include <hip/hip_runtime.h>

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
    return x;
}

// the same exchange with the caller's combiner: x <- op(x, partner's x)
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T x, Op op) {
    for (int off = 32; off >= 1; off >>= 1) x = op(x, __shfl_xor(x, off, 64));
    return x;
}

// ... and for a (value, index) pair: the partner's pair replaces the lane's own when better(partner's v, i, own v, i)
template <typename V, typename Better>
__device__ __forceinline__ void wave_reduce_pair(V& v, int& i, Better better) {
    for (int off = 32; off >= 1; off >>= 1) {
        const V ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// LDS traffic between the lanes of ONE wavefront: the wave runs in lockstep and its LDS operations complete in order; this keeps
// the compiler from moving an access across the point
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum of x over the lanes 0 .. lane of the wavefront
__device__ __forceinline__ int wave_inclusive_scan(int x, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(x, off, 64);
        if (lane >= off) x += up;
    }
    return x;
}

// Workgroup scan of N values per thread at once, in thread order: x[k] becomes the sum of x[k] over the threads in front, total[k]
// the sum over the whole workgroup.  s_w: N * n_waves words of LDS from the caller.  ONE __syncthreads, so every thread of the
// workgroup has to come here; the caller puts a barrier of its own before s_w is written again.
template <int N>
__device__ __forceinline__ void wg_exclusive_scan(int (&x)[N], int (&total)[N], int* s_w, int lane, int wave, int n_waves) {
    for (int k = 0; k < N; k++) {
        const int incl = wave_inclusive_scan(x[k], lane);
        if (lane == 63) s_w[k * n_waves + wave] = incl;
        x[k] = incl - x[k];
        total[k] = 0;
    }
    __syncthreads();
    for (int w = 0; w < n_waves; w++)
        for (int k = 0; k < N; k++) {
            const int t = s_w[k * n_waves + w];
            if (w < wave) x[k] += t;
            total[k] += t;
        }
}

// one value: returns the exclusive prefix
__device__ __forceinline__ int wg_exclusive_scan(int x, int& total, int* s_w, int lane, int wave, int n_waves) {
    int xs[1] = {x}, ts[1];
    wg_exclusive_scan<1>(xs, ts, s_w, lane, wave, n_waves);
    total = ts[0];
    return xs[0];
}

// bitonic sort of the n2 keys in LDS, ascending; n2 a power of two, thread tid of T.  Barriers: the caller's before, its own at the end.
__device__ __forceinline__ void lds_bitonic_sort(unsigned long long* keys, int n2, int tid, int T) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < (n2 >> 1); idx += T) {
                const int a = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
                const int b = a | j;
                const unsigned long long ka = keys[a], kb = keys[b];
                const bool up = (a & k) == 0;
                if ((ka > kb) == up) { keys[a] = kb; keys[b] = ka; }
            }
            __syncthreads();
        }
}

// The owner of a slot in a table of ascending offsets, as two bare searches; whether the answer can be trusted is the caller's check.
// the last q in [0, n) with off[q] <= j; 0 when there is none
__device__ __forceinline__ int last_le(const int* off, int n, int j) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// the first s in [0, n) with off[s + 1] > g; n when there is none
__device__ __forceinline__ int first_owner(const int* off, int n, int g) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= g) lo = mid + 1; else hi = mid;
    }
    return lo;
}
