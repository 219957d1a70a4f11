// track_merge.hip -- the track merge between the two fit passes on the device (include/odam_merge.h): average-linkage clustering of
// every scene's tracks on the IoU block odam_box3d_iou_batch left, and the assembly of the merged tracks.  Restates (likojack/ODAM)
//   src/scripts/run_merge.py:119-124   sklearn's AgglomerativeClustering on the precomputed cost -> scipy linkage(method="average")
//                                      (nearest-neighbour chain), its union-find relabelling, sklearn's _hc_cut with CPython's heapq
//   src/scripts/run_merge.py:24-58     merge_tracks
// The decisions that have to equal the libraries' are functions of track_merge_core.h; tests/merge_ref.py restates both kernels.
//
// Clustering: one workgroup per scene.  The n x n costs live in the caller's scratch (binary64, symmetric, both halves kept up to date so
// that the neighbour search reads one contiguous row); sizes, the chain and the merges live in LDS.  A chain step is a workgroup-wide
// argmin that carries the index (the lowest index wins among equal values), decided by lane 0; a merge is one pass over the live
// clusters.  Sorting the n - 1 merges is a rank by counting; the union-find relabelling and the heap of _hc_cut are sequential by
// definition and run on one lane (O(n log n) LDS operations at n <= 1024).
//
// Assembly: one workgroup per (scene, label).  The members are ranked by (rows descending, track ascending); their rows, enumerated in
// that order, become the keys (image << 32 | candidate, view_keys.h) of the rows whose frame id names an image; after the LDS sort the
// first key of every image run is the row the host path would keep.  A scan over all clusters gives the dense offsets, a gather
// writes the rows.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/odam_merge.h"
#include "odam_err.h"
#include "track_merge_core.h"
#include "view_keys.h"
#include "wave_ops.h"

namespace {

constexpr int MAXN = ODAM_MERGE_MAX_TRACKS;
constexpr int MAX_WAVES = 16;
constexpr int N_CLASS = 64;

// the scene that owns track (or cluster slot) g, or -1 when the offsets do not say so consistently
__device__ inline int scene_of(const int* a_off, int n_scene, int n_tracks, int g) {
    const int lo = first_owner(a_off, n_scene, g);
    if (lo >= n_scene) return -1;
    const int t0 = a_off[lo], t1 = a_off[lo + 1];
    if (t0 < 0 || t1 > n_tracks || g < t0 || g >= t1 || t1 - t0 > MAXN) return -1;
    return lo;
}

// ------------------------------------------------------------------------------------------------------------------ clustering

struct ClusterArgs {
    const int* a_off;
    const long long* pair_off;
    int n_scene, n_tracks, max_tracks;
    long long n_pairs;
    const double* iou;
    double thr;
    double* D;
    double* link;
    int *labels, *n_cluster, *status;
};

enum { C_LEN = 0, C_LOW, C_MERGE, C_X, C_Y, C_NX, C_NY, C_ERR, C_WORDS };

__global__ __launch_bounds__(512) void merge_cluster_kernel(ClusterArgs A) {
    __shared__ int s_pool[2 * MAXN];      // sizes and the chain; then the union-find's sizes; then the heap
    __shared__ int s_mx[MAXN], s_my[MAXN], s_mc[MAXN], s_ord[MAXN], s_ca[MAXN], s_cb[MAXN];
    __shared__ int s_par[2 * MAXN];       // the union-find's parents; then the label of every node
    __shared__ double s_md[MAXN];
    __shared__ double s_wv[MAX_WAVES];
    __shared__ int s_wi[MAX_WAVES];
    __shared__ int s_ctl[C_WORDS];
    int* s_size = s_pool;
    int* s_chain = s_pool + MAXN;

    const int s = blockIdx.x;
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = T >> 6;
    const int t0 = A.a_off[s];
    const int n = A.a_off[s + 1] - t0;
    const long long p0 = A.pair_off[s];
    const long long np = A.pair_off[s + 1] - p0;
    // workgroup-uniform refusals, before any word of the scene is touched
    if (n < 0 || n > A.max_tracks || n > MAXN || t0 < 0 || (long long)t0 + n > A.n_tracks || p0 < 0 || np != (long long)n * n ||
        p0 + np > A.n_pairs) {
        if (tid == 0) { A.n_cluster[s] = 0; A.status[s] = ODAM_MERGE_BAD_OFFSETS; }
        return;
    }
    if (n <= 1) {
        if (tid == 0) {
            if (n == 1) A.labels[t0] = 0;
            A.n_cluster[s] = n;
            A.status[s] = 0;
        }
        return;
    }
    const double* iou = A.iou + p0;
    double* D = A.D + p0;

    // cost = 1 - iou of the upper triangle, mirrored; zero diagonal
    int bad = 0;
    for (int idx = tid; idx < n * n; idx += T) {
        const int i = idx / n, j = idx - i * n;
        double c = 0.0;
        if (i != j) c = 1.0 - (i < j ? iou[(size_t)i * n + j] : iou[(size_t)j * n + i]);
        if (!(fabs(c) <= 1.7976931348623157e308)) bad = 1;
        D[idx] = c;
    }
    for (int i = tid; i < n; i += T) s_size[i] = 1;
    if (tid == 0) {
        s_chain[0] = 0;
        s_ctl[C_LEN] = 1; s_ctl[C_LOW] = 0; s_ctl[C_MERGE] = 0; s_ctl[C_ERR] = 0;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) { A.n_cluster[s] = 0; A.status[s] = ODAM_MERGE_BAD_COST; }
        return;
    }

    // nearest-neighbour chain
    int k = 0;
    while (k < n - 1) {
        __syncthreads();      // the chain, the sizes and the costs of the step before
        const int len = s_ctl[C_LEN];
        const int x = s_chain[len - 1];
        const double* row = D + (size_t)x * n;
        double bv = INFINITY;
        int bi = INT_MAX;
        for (int i = tid; i < n; i += T) {
            if (s_size[i] == 0 || i == x) continue;
            const double v = row[i];
            if (tm_better(v, i, bv, bi)) { bv = v; bi = i; }
        }
        wave_reduce_pair(bv, bi, [](double ov, int oi, double v, int i) { return tm_better(ov, oi, v, i); });
        if (lane == 0) { s_wv[wave] = bv; s_wi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < n_waves; w++)
                if (tm_better(s_wv[w], s_wi[w], bv, bi)) { bv = s_wv[w]; bi = s_wi[w]; }
            if (bi == INT_MAX) {
                s_ctl[C_ERR] = 1;
            } else {
                int y = bi;
                bool merge = false;
                if (len > 1) {
                    const int prev = s_chain[len - 2];
                    if (!(bv < row[prev])) y = prev;      // the previous element wins an exact tie
                    merge = y == prev;
                }
                if (merge) {
                    const int xx = x < y ? x : y, yy = x < y ? y : x;
                    const int nx = s_size[xx], ny = s_size[yy];
                    s_mx[k] = xx; s_my[k] = yy; s_md[k] = bv; s_mc[k] = nx + ny;
                    s_size[xx] = 0; s_size[yy] = nx + ny;
                    s_ctl[C_X] = xx; s_ctl[C_Y] = yy; s_ctl[C_NX] = nx; s_ctl[C_NY] = ny;
                    int nl = len - 2;
                    if (nl == 0 && k + 1 < n - 1) {      // the chain restarts at the lowest live index
                        int low = s_ctl[C_LOW];
                        while (low < n - 1 && s_size[low] == 0) low++;
                        s_ctl[C_LOW] = low;
                        s_chain[0] = low;
                        nl = 1;
                    }
                    s_ctl[C_LEN] = nl;
                } else if (len >= n) {      // the chain holds live clusters, each once: it cannot grow past n
                    s_ctl[C_ERR] = 1;
                } else {
                    s_chain[len] = y;
                    s_ctl[C_LEN] = len + 1;
                }
                s_ctl[C_MERGE] = merge ? 1 : 0;
            }
        }
        __syncthreads();
        if (s_ctl[C_ERR]) break;
        if (s_ctl[C_MERGE]) {
            const int xx = s_ctl[C_X], yy = s_ctl[C_Y], nx = s_ctl[C_NX], ny = s_ctl[C_NY];
            const double* rx = D + (size_t)xx * n;
            double* ry = D + (size_t)yy * n;
            for (int i = tid; i < n; i += T) {
                if (s_size[i] == 0 || i == yy) continue;
                const double v = tm_average(nx, rx[i], ny, ry[i]);
                ry[i] = v;
                D[(size_t)i * n + yy] = v;
            }
            k++;
        }
    }
    __syncthreads();
    if (s_ctl[C_ERR]) {      // no finite neighbour: cannot happen with finite costs
        if (tid == 0) { A.n_cluster[s] = 0; A.status[s] = ODAM_MERGE_BAD_COST; }
        return;
    }

    // stable sort of the merges by distance: rank by counting
    const int m = n - 1;
    for (int a = tid; a < m; a += T) {
        const double d = s_md[a];
        int r = 0;
        for (int b = 0; b < m; b++) {
            const double e = s_md[b];
            r += (e < d || (e == d && b < a)) ? 1 : 0;
        }
        s_ord[r] = a;
    }
    int* s_usize = s_pool;
    for (int v = tid; v < 2 * n - 1; v += T) { s_par[v] = v; s_usize[v] = 1; }
    __syncthreads();

    if (tid == 0) {
        // scipy's label(): children become the roots of the union-find, the smaller first
        double* link = A.link + (size_t)t0 * 4;
        int n_cl = 1;
        for (int r = 0; r < m; r++) {
            const int a = s_ord[r];
            const int ra = tm_uf_find(s_par, s_mx[a]), rb = tm_uf_find(s_par, s_my[a]);
            const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
            const int sz = s_usize[ra] + s_usize[rb];
            s_par[ra] = n + r; s_par[rb] = n + r;
            s_usize[n + r] = sz;
            s_ca[r] = lo; s_cb[r] = hi;
            const double d = s_md[a];
            link[(size_t)r * 4 + 0] = (double)lo; link[(size_t)r * 4 + 1] = (double)hi;
            link[(size_t)r * 4 + 2] = d; link[(size_t)r * 4 + 3] = (double)sz;
            n_cl += d >= A.thr ? 1 : 0;
        }
        // sklearn's _hc_cut: a heap of negated node ids; the label of a cluster is its position in the heap array
        int* heap = s_pool;
        int hl = 1, err = 0;
        heap[0] = -((s_ca[m - 1] > s_cb[m - 1] ? s_ca[m - 1] : s_cb[m - 1]) + 1);
        for (int c = 0; c + 1 < n_cl; c++) {
            const int r = -heap[0] - n;
            if (r < 0 || r >= m) { err = 1; break; }
            const int a = s_ca[r], b = s_cb[r];
            tm_heappush(heap, &hl, -a);
            tm_heappushpop(heap, hl, -b);
        }
        int* s_nl = s_par;
        for (int v = 0; v < 2 * n - 1; v++) s_nl[v] = -1;
        for (int i = 0; i < hl; i++) {
            const int v = -heap[i];
            if (v < 0 || v >= 2 * n - 1) { err = 1; continue; }
            s_nl[v] = i;
        }
        for (int v = 2 * n - 2; v >= n; v--) {      // a child's id is below its parent's
            const int l = s_nl[v];
            if (l >= 0) { s_nl[s_ca[v - n]] = l; s_nl[s_cb[v - n]] = l; }
        }
        A.n_cluster[s] = err ? 0 : n_cl;
        A.status[s] = err ? ODAM_MERGE_BAD_COST : 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) A.labels[t0 + i] = s_par[i];
}

// -------------------------------------------------------------------------------------------------------------------- assembly

struct AsmArgs {
    const int* a_off;
    int n_scene, n_tracks, n_rows, n_imgs, cap;
    const int *labels, *n_cluster, *cluster_status, *row_off;
    const double* rows;
    const int* img_off;
    const long long* img_ids;
    const int* img_order;
    int *sel_rank, *slot_cnt, *slot_cls, *slot_base, *dense_excl;
    int *out_off, *out_src, *out_cls;
    double* out_rows14;
    int *out_n_out, *out_status, *out_total;
};

__global__ __launch_bounds__(1024) void merge_select_kernel(AsmArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    __shared__ int s_mem[MAXN], s_len[MAXN], s_ord[MAXN], s_r0[MAXN], s_base[MAXN + 1];
    __shared__ int s_hist[N_CLASS];
    __shared__ int s_wcnt[MAX_WAVES];
    __shared__ int s_bad, s_total;

    const int g = blockIdx.x;
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = T >> 6;
    const int s = scene_of(A.a_off, A.n_scene, A.n_tracks, g);
    if (s < 0) {
        if (tid == 0) A.slot_cnt[g] = 0;
        return;
    }
    const int t0 = A.a_off[s], n = A.a_off[s + 1] - t0;
    const int c = g - t0;
    const int n_cl = A.n_cluster[s];
    if (A.cluster_status[s] != 0 || n_cl > n || c >= n_cl) {      // uniform: not a cluster
        if (tid == 0) A.slot_cnt[g] = 0;
        return;
    }
    const int i0 = A.img_off[s], n_img = A.img_off[s + 1] - i0;
    if (tid < N_CLASS) s_hist[tid] = 0;
    if (tid == 0) s_bad = (i0 < 0 || n_img < 0 || (long long)i0 + n_img > A.n_imgs) ? ODAM_MERGE_BAD_OFFSETS : 0;
    __syncthreads();

    // the members, in track order
    int M = 0;
    for (int base = 0; base < n; base += T) {
        const int t = base + tid;
        const bool in = t < n && A.labels[t0 + t] == c;
        int tot;
        const int before = wg_exclusive_scan(in ? 1 : 0, tot, s_wcnt, lane, wave, n_waves);
        if (in) s_mem[M + before] = t;
        M += tot;
        __syncthreads();
    }
    for (int q = tid; q < M; q += T) {
        const int trk = t0 + s_mem[q];
        const int r0 = A.row_off[trk], len = A.row_off[trk + 1] - r0;
        if (r0 < 0 || len < 0 || (long long)r0 + len > A.n_rows) { atomicMax(&s_bad, ODAM_MERGE_BAD_OFFSETS); s_len[q] = 0; s_r0[q] = 0; }
        else { s_len[q] = len; s_r0[q] = r0; }
    }
    __syncthreads();
    // rank by (rows descending, track ascending): the candidate of the longest member comes first, the first such member on a tie
    for (int q = tid; q < M; q += T) {
        const int len = s_len[q];
        int r = 0;
        for (int p = 0; p < M; p++) {
            const int lp = s_len[p];
            r += (lp > len || (lp == len && p < q)) ? 1 : 0;
        }
        s_ord[r] = q;
    }
    __syncthreads();
    if (tid == 0) {
        long long acc = 0;
        s_base[0] = 0;
        for (int q = 0; q < M; q++) {
            acc += s_len[s_ord[q]];
            if (acc > A.cap) { acc = (long long)A.cap + 1; s_base[q + 1] = A.cap + 1; continue; }
            s_base[q + 1] = (int)acc;
        }
        s_total = (int)acc;
    }
    __syncthreads();
    const int C = s_total, bad0 = s_bad;
    __syncthreads();      // every thread has read s_bad before the key loop may raise it
    if (bad0 != 0 || C > A.cap || C == 0 || M == 0) {      // uniform
        if (tid == 0) {
            A.slot_cnt[g] = 0;
            const int code = bad0 != 0 ? bad0 : (C > A.cap ? ODAM_MERGE_TOO_MANY_ROWS : 0);
            if (code) atomicMax(&A.out_status[s], code);
        }
        return;
    }
    int n2 = 1;
    while (n2 < C) n2 <<= 1;      // <= cap: cap is a power of two

    const long long* ids = A.img_ids + i0;
    const int* order = A.img_order + i0;
    for (int j = tid; j < n2; j += T) {
        unsigned long long key = VIEW_NONE;
        if (j < C) {
            const int q = last_le(s_base, M, j);      // the ranked member that owns candidate j
            const int mq = s_ord[q];
            const double* row = A.rows + ((size_t)s_r0[mq] + (size_t)(j - s_base[q])) * 14;
            const double f = row[0];
            int lo = 0, hi = n_img;      // first id >= f; a NaN ends anywhere and equals nothing
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((double)ids[mid] < f) lo = mid + 1; else hi = mid;
            }
            if (lo < n_img && (double)ids[lo] == f) {
                const int img = order[lo];
                if (img >= 0 && img < n_img) key = view_key(img, j);
            }
            const double cl = row[1];
            if (cl >= 0.0 && cl <= (double)(N_CLASS - 1) && cl == floor(cl)) atomicAdd(&s_hist[(int)cl], 1);
            else atomicMax(&s_bad, ODAM_MERGE_BAD_CLASS);
        }
        keys[j] = key;
    }
    __syncthreads();

    lds_bitonic_sort(keys, n2, tid, T);

    // every thread owns a run of L sorted entries; winners in front of it = where its own winners go
    const int L = n2 > T ? n2 / T : 1;
    const int j0 = tid * L;
    const int j1 = j0 < C ? (j0 + L < C ? j0 + L : C) : j0;
    int cnt = 0;
    for (int j = j0; j < j1; j++) {
        if (first_of_image(keys, j)) { cnt++; continue; }
        const unsigned long long key = keys[j];
        if (key == VIEW_NONE) continue;
        // same image as its left neighbour: two members saw the image, or one member holds the frame id twice
        const int qa = last_le(s_base, M, view_index(keys[j - 1])), qb = last_le(s_base, M, view_index(key));
        if (qa == qb) atomicMax(&s_bad, ODAM_MERGE_REPEATED_FRAME);
    }
    int total;
    int p = wg_exclusive_scan(cnt, total, s_wcnt, lane, wave, n_waves);
    for (int j = j0; j < j1; j++) {
        if (!first_of_image(keys, j)) continue;
        const int cand = view_index(keys[j]);
        const int q = last_le(s_base, M, cand);
        A.sel_rank[s_r0[s_ord[q]] + (cand - s_base[q])] = p;
        p++;
    }
    if (tid == 0) {
        const int code = s_bad;
        int best = 0, cls = 0;
        for (int b = 0; b < N_CLASS; b++)
            if (s_hist[b] > best) { best = s_hist[b]; cls = b; }      // the smallest of the most frequent
        A.slot_cls[g] = cls;
        A.slot_cnt[g] = code ? 0 : total;
        if (code) atomicMax(&A.out_status[s], code);
    }
}

// dense offsets over all cluster slots: ONE workgroup
__global__ __launch_bounds__(1024) void merge_scan_kernel(AsmArgs A) {
    __shared__ int s_w[2 * MAX_WAVES];      // kept clusters, rows
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = T >> 6;
    const int G = A.n_tracks;
    int carry_k = 0, carry_r = 0;
    for (int base = 0; base < G; base += T) {
        const int g = base + tid;
        int cnt = 0;
        if (g < G) {
            const int s = scene_of(A.a_off, A.n_scene, A.n_tracks, g);
            if (s >= 0 && A.cluster_status[s] == 0 && A.out_status[s] == 0) cnt = A.slot_cnt[g];
            if (cnt < 0 || cnt > A.n_rows) cnt = 0;
        }
        const int keep = cnt > 0 ? 1 : 0;
        int excl[2] = {keep, cnt}, tot[2];
        wg_exclusive_scan(excl, tot, s_w, lane, wave, n_waves);
        const int ek = carry_k + excl[0], er = carry_r + excl[1];
        if (g < G) {
            A.dense_excl[g] = ek;
            A.slot_base[g] = er <= A.n_rows - cnt ? er : -1;      // (rows are chosen once each: the sum cannot pass n_rows)
            if (keep) { A.out_off[ek] = er; A.out_cls[ek] = A.slot_cls[g]; }
        }
        carry_k += tot[0]; carry_r += tot[1];
        __syncthreads();
    }
    if (tid == 0) {
        A.dense_excl[G] = carry_k;
        A.out_off[carry_k] = carry_r;
        A.out_total[0] = carry_k; A.out_total[1] = carry_r;
    }
    __syncthreads();
    for (int s = tid; s < A.n_scene; s += T) {
        const int t0 = A.a_off[s], t1 = A.a_off[s + 1];
        if (t0 < 0 || t1 < t0 || t1 > G || t1 - t0 > MAXN) {
            A.out_n_out[s] = 0;
            A.out_status[s] = ODAM_MERGE_BAD_OFFSETS;
            continue;
        }
        A.out_n_out[s] = A.dense_excl[t1] - A.dense_excl[t0];
        if (A.cluster_status[s] != 0 && A.out_status[s] == 0) A.out_status[s] = ODAM_MERGE_NOT_CLUSTERED;
    }
}

__global__ __launch_bounds__(256) void merge_gather_kernel(AsmArgs A) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n_rows) return;
    const int p = A.sel_rank[r];
    if (p < 0) return;
    const int lo = first_owner(A.row_off, A.n_tracks, r);      // the track that owns row r
    if (lo >= A.n_tracks || A.row_off[lo] > r) return;
    const int s = scene_of(A.a_off, A.n_scene, A.n_tracks, lo);
    if (s < 0 || A.cluster_status[s] != 0 || A.out_status[s] != 0) return;
    const int label = A.labels[lo];
    const int t0 = A.a_off[s];
    if (label < 0 || label >= A.a_off[s + 1] - t0) return;
    const int g = t0 + label;
    const int base = A.slot_base[g];
    if (base < 0 || p >= A.slot_cnt[g]) return;
    const int pos = base + p;      // < n_rows: slot_base + slot_cnt <= n_rows
    A.out_src[pos] = r;
    if (A.out_rows14) {
        const double* src = A.rows + (size_t)r * 14;
        double* dst = A.out_rows14 + (size_t)pos * 14;
#pragma unroll
        for (int k = 0; k < 14; k++) dst[k] = k == 1 ? (double)A.slot_cls[g] : src[k];
    }
}

}  // namespace

extern "C" int odam_merge_cluster(odam_sq_ctx* ctx, int n_scene, const int* a_off, const long long* pair_off, int n_tracks,
                                  long long n_pairs, int max_tracks, const double* iou3d, double threshold, double* scratch,
                                  double* out_linkage, int* out_labels, int* out_n_cluster, int* out_status, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_merge_cluster: null context");
    if (n_scene < 0 || n_tracks < 0 || n_pairs < 0 || max_tracks < 0) return odam_fail(ODAM_E_INVALID, "odam_merge_cluster: bad size");
    if (max_tracks > ODAM_MERGE_MAX_TRACKS) return odam_fail(ODAM_E_LIMIT, "odam_merge_cluster: more than 1024 tracks in a scene");
    if (threshold != threshold) return odam_fail(ODAM_E_INVALID, "odam_merge_cluster: the threshold is not a number");
    if (n_scene == 0) return ODAM_OK;
    if (!a_off || !pair_off || !iou3d || !scratch || !out_linkage || !out_labels || !out_n_cluster || !out_status)
        return odam_fail(ODAM_E_INVALID, "odam_merge_cluster: null pointer");
    int threads = (max_tracks + 63) / 64 * 64;
    threads = threads < 64 ? 64 : (threads > 512 ? 512 : threads);
    ClusterArgs A{};
    A.a_off = a_off; A.pair_off = pair_off; A.n_scene = n_scene; A.n_tracks = n_tracks; A.max_tracks = max_tracks; A.n_pairs = n_pairs;
    A.iou = iou3d; A.thr = threshold; A.D = scratch; A.link = out_linkage; A.labels = out_labels; A.n_cluster = out_n_cluster;
    A.status = out_status;
    hipLaunchKernelGGL(merge_cluster_kernel, dim3((unsigned)n_scene), dim3((unsigned)threads), 0, (hipStream_t)stream, A);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_merge_assemble(odam_sq_ctx* ctx, int n_scene, const int* a_off, int n_tracks, const int* labels, const int* n_cluster,
                                   const int* cluster_status, const int* row_off, const double* rows, int n_rows, int max_cand,
                                   const int* img_off, const long long* img_ids, const int* img_order, int n_imgs, int* scratch,
                                   int* out_off, int* out_src, int* out_cls, double* out_rows14, int* out_n_out, int* out_status,
                                   int* out_total, void* stream) {
    if (!ctx) return odam_fail(ODAM_E_INVALID, "odam_merge_assemble: null context");
    if (n_scene < 0 || n_tracks < 0 || n_rows < 0 || n_imgs < 0 || max_cand < 0) return odam_fail(ODAM_E_INVALID, "odam_merge_assemble: bad size");
    if (n_scene == 0) return ODAM_OK;
    if (!a_off || !labels || !n_cluster || !cluster_status || !row_off || !rows || !img_off || !img_ids || !img_order || !scratch ||
        !out_off || !out_src || !out_cls || !out_n_out || !out_status || !out_total)
        return odam_fail(ODAM_E_INVALID, "odam_merge_assemble: null pointer");
    int cap = 1;
    while (cap < max_cand && cap < ODAM_SQ_PREPARE_MAX_ROWS) cap <<= 1;
    int threads = cap / 2;
    threads = threads < 64 ? 64 : (threads > 1024 ? 1024 : threads);
    const size_t lds = sizeof(unsigned long long) * (size_t)cap;
    if (lds > 32 * 1024)
        ODAM_HIP(hipFuncSetAttribute((const void*)merge_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipStream_t st = (hipStream_t)stream;
    AsmArgs A{};
    A.a_off = a_off; A.n_scene = n_scene; A.n_tracks = n_tracks; A.n_rows = n_rows; A.n_imgs = n_imgs; A.cap = cap;
    A.labels = labels; A.n_cluster = n_cluster; A.cluster_status = cluster_status; A.row_off = row_off; A.rows = rows;
    A.img_off = img_off; A.img_ids = img_ids; A.img_order = img_order;
    A.sel_rank = scratch; A.slot_cnt = scratch + n_rows; A.slot_cls = A.slot_cnt + n_tracks; A.slot_base = A.slot_cls + n_tracks;
    A.dense_excl = A.slot_base + n_tracks;
    A.out_off = out_off; A.out_src = out_src; A.out_cls = out_cls; A.out_rows14 = out_rows14; A.out_n_out = out_n_out;
    A.out_status = out_status; A.out_total = out_total;
    if (n_rows > 0) ODAM_HIP(hipMemsetAsync(A.sel_rank, 0xff, sizeof(int) * (size_t)n_rows, st));      // -1: no row is chosen
    ODAM_HIP(hipMemsetAsync(out_status, 0, sizeof(int) * (size_t)n_scene, st));
    if (n_tracks > 0) {
        hipLaunchKernelGGL(merge_select_kernel, dim3((unsigned)n_tracks), dim3((unsigned)threads), lds, st, A);
        ODAM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(merge_scan_kernel, dim3(1), dim3(1024), 0, st, A);
    ODAM_HIP(hipGetLastError());
    if (n_rows > 0) {
        hipLaunchKernelGGL(merge_gather_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, A);
        ODAM_HIP(hipGetLastError());
    }
    return ODAM_OK;
}
