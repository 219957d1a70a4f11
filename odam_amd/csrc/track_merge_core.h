// track_merge_core.h -- the decisions of the track merge (include/odam_merge.h) that have to equal scipy's, sklearn's and CPython's,
// as plain functions of host and device: the kernels of track_merge.hip call them, a host program can too.
//   scipy/cluster/_hierarchy.pyx            nn_chain (the average update, the neighbour search), label / LinkageUnionFind
//   sklearn/cluster/_agglomerative.py       _hc_cut
//   CPython Lib/heapq.py                    heappush, heappushpop, _siftdown, _siftup
// Compiled with -ffp-contract=off: every product and sum is rounded on its own.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define TM_HD __host__ __device__ inline
#else
#define TM_HD inline
#endif

// a candidate (v, i) replaces the best (bv, bi) of a neighbour search: strictly smaller, or equal with the lower index.  Applied in
// any order over a set of candidates this leaves the lowest index among the strictly smallest values.
TM_HD bool tm_better(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

// Lance-Williams for average linkage, in scipy's operation order
TM_HD double tm_average(int nx, double d_ix, int ny, double d_iy) {
    return ((double)nx * d_ix + (double)ny * d_iy) / (double)(nx + ny);
}

// LinkageUnionFind.find with its path compression
TM_HD int tm_uf_find(int* parent, int x) {
    int p = x;
    while (parent[x] != x) x = parent[x];
    while (parent[p] != x) {
        const int q = parent[p];
        parent[p] = x;
        p = q;
    }
    return x;
}

// heapq._siftdown
TM_HD void tm_siftdown(int* heap, int startpos, int pos) {
    const int newitem = heap[pos];
    while (pos > startpos) {
        const int parentpos = (pos - 1) >> 1;
        const int parent = heap[parentpos];
        if (newitem < parent) {
            heap[pos] = parent;
            pos = parentpos;
            continue;
        }
        break;
    }
    heap[pos] = newitem;
}

// heapq._siftup: the smaller child bubbles up until a leaf is reached, then the item sifts down into place
TM_HD void tm_siftup(int* heap, int len, int pos) {
    const int startpos = pos;
    const int newitem = heap[pos];
    int childpos = 2 * pos + 1;
    while (childpos < len) {
        const int rightpos = childpos + 1;
        if (rightpos < len && !(heap[childpos] < heap[rightpos])) childpos = rightpos;
        heap[pos] = heap[childpos];
        pos = childpos;
        childpos = 2 * pos + 1;
    }
    heap[pos] = newitem;
    tm_siftdown(heap, startpos, pos);
}

TM_HD void tm_heappush(int* heap, int* len, int item) {
    heap[*len] = item;
    *len += 1;
    tm_siftdown(heap, 0, *len - 1);
}

// heapq.heappushpop (the popped item is not needed)
TM_HD void tm_heappushpop(int* heap, int len, int item) {
    if (len > 0 && heap[0] < item) {
        heap[0] = item;
        tm_siftup(heap, len, 0);
    }
}
