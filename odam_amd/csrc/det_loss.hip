// det_loss.hip -- the detector's validation loss on the device (include/odam_loss.h): the matcher's cost matrix, the assignment
// of every frame and the losses under it -- the reference's HungarianMatcher (likojack/ODAM src/models/matcher.py:11-82) and
// SetCriterion (src/models/detr.py:258-481; one decoder layer per call, or all of them through the *_layers entries, whose
// kernels are the <true> instantiations of the same templates with the layer in one more grid dimension).  Arithmetic in
// det_loss_core.h; restated in numpy by tests/criterion_ref.py.
//
// Four small kernels, each running to completion on its own:
//   match_cost_kernel       one workgroup per frame, lanes over queries.  A lane keeps its query's box, its corners and the maximum
//                           and sum of its softmax; the frame's target rows pass through LDS 32 at a time (once, when there are
//                           no more than 32).  Every (query, target) cost is one plain store.
//   lsap_wave_kernel        one wavefront per problem: scipy's rectangular shortest-augmenting-path solver as hungarian_wave_kernel
//                           (assoc_match.hip) restates it -- lanes own columns, the scan over the remaining columns is one
//                           lexicographic reduction, wave-level fences and no workgroup barrier -- on raw float32 costs widened to
//                           binary64, with scipy's refusal of NaN / -inf entries and one store per row at the end.
//   criterion_frame_kernel  one wavefront per frame: a lane walks its queries in ascending order and adds every term to its own
//                           binary64 accumulators; the 64 lanes are then added by a fixed exchange tree (a + b is computed on both
//                           sides of every exchange, so all lanes hold the same bits).  Lane 0 stores the frame's 11 partial sums.
//   criterion_table_kernel  one wavefront: lane e adds entry e over the frames in index order; lane 0 forms the table.
// No floating-point atomics, no counters between workgroups: the same inputs give the same bits on every dispatch.
#include <hip/hip_runtime.h>

#include "../../include/odam_loss.h"
#include "det_loss_core.h"
#include "odam_err.h"
#include "sk_wave.h"

namespace {

using namespace odam_loss;

constexpr int STAGE = ODAM_LOSS_STAGE;
constexpr int COST_BLOCK = 128;
constexpr int LS_MAXR = ODAM_LSAP_MAX_SMALL, LS_MAXC = ODAM_LSAP_MAX_LARGE;
constexpr int N_PART = ODAM_LOSS_N_PARTIAL, N_ENT = ODAM_LOSS_N_ENTRIES, N_W = ODAM_LOSS_N_WEIGHTS;
static_assert(LS_MAXC == 128 && LS_MAXR == 32, "the key of the column scan packs a column into 7 bits and a row into 5");

// what lane (l ^ (1 << BIT)) holds, on DPP / v_permlane*_swap (sk_wave.h): bit moves, any payload
template <int BIT> __device__ __forceinline__ unsigned ls_xor(unsigned v) { return __builtin_bit_cast(unsigned, sk_xor<BIT>(__builtin_bit_cast(float, v))); }
template <int BIT> __device__ __forceinline__ double ls_xor_f64(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = ls_xor<BIT>((unsigned)b), hi = ls_xor<BIT>((unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// the sum over the 64 lanes by a fixed tree; every lane ends with the same bits (both sides of an exchange add the same two numbers)
__device__ __forceinline__ double wave_sum_f64(double v) {
    v = v + ls_xor_f64<0>(v); v = v + ls_xor_f64<1>(v); v = v + ls_xor_f64<2>(v);
    v = v + ls_xor_f64<3>(v); v = v + ls_xor_f64<4>(v); return v + ls_xor_f64<5>(v);
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
    v |= ls_xor<0>(v); v |= ls_xor<1>(v); v |= ls_xor<2>(v); v |= ls_xor<3>(v); v |= ls_xor<4>(v); return v | ls_xor<5>(v);
}

// ---- the cost matrix (matcher.py:49-73) ------------------------------------------------------------------------------------------
struct CostArgs {
    const float* logits; const float* boxes; const float* objects; const int* obj_off;
    int B, Q, n_logit, n_obj, W;
    float cost_class, cost_bbox, cost_giou;
    float* out; int* status;
};

// LAYERS: [L][B][Q][.] predictions, grid (B, L) -- workgroup (b, l) is frame b of the single-layer call on layer l's tensors, cost
// blocks and status words.  The <false> instantiation is the kernel as it was
template <bool LAYERS> __global__ __launch_bounds__(COST_BLOCK) void match_cost_kernel(CostArgs K) {
    if constexpr (LAYERS) {
        const size_t l = blockIdx.y, rows = l * (size_t)K.B * K.Q;
        K.logits += rows * K.n_logit; K.boxes += rows * 4;
        K.out += l * (size_t)K.Q * K.n_obj; K.status += l * (size_t)K.B;
    }
    __shared__ float s_box[STAGE][4], s_xy[STAGE][4];
    __shared__ int s_lab[STAGE];
    __shared__ int s_flag;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = K.obj_off[b], g1 = K.obj_off[b + 1];
    if (g0 < 0 || g1 < g0 || g1 > K.n_obj) {      // (the same for every lane)
        if (tid == 0) K.status[b] = ODAM_LOSS_ST_OFFSETS;
        return;
    }
    const int G = g1 - g0;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    int flag = 0;
    float* out = K.out + (size_t)K.Q * g0;
    for (int qb = 0; qb < K.Q; qb += COST_BLOCK) {
        const int q = qb + tid;
        const bool live = q < K.Q;
        float box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, xy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, m = 0.0f, s = 1.0f;
        const float* row = K.logits;
        if (live) {
            const size_t bq = (size_t)b * K.Q + q;
#pragma unroll
            for (int k = 0; k < 4; k++) box[k] = K.boxes[bq * 4 + k];
            xyxy_of(box, xy);
            if (!xyxy_ok(xy)) flag |= ODAM_LOSS_ST_DEGENERATE;
            row = K.logits + bq * K.n_logit;
            int am;
            m = row_max(row, K.n_logit, &am);      // the softmax of the row: its maximum and its sum, once
            s = row_sumexp(row, K.n_logit, m);
        }
        for (int t0 = 0; t0 < G; t0 += STAGE) {
            const int cnt = min(STAGE, G - t0);
            if (qb == 0 || G > STAGE) {      // no more than 32 targets: staged once for all queries
                __syncthreads();
                if (tid < cnt) {
                    const float* obj = K.objects + (size_t)(g0 + t0 + tid) * K.W;
                    float tb[4], txy[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) tb[k] = obj[1 + k];
                    xyxy_of(tb, txy);
                    if (!xyxy_ok(txy)) flag |= ODAM_LOSS_ST_DEGENERATE;
                    const int lab = class_of(obj[0], K.n_logit);
                    if (lab < 0) flag |= ODAM_LOSS_ST_CLASS;
                    s_lab[tid] = lab;
#pragma unroll
                    for (int k = 0; k < 4; k++) { s_box[tid][k] = tb[k]; s_xy[tid][k] = txy[k]; }
                }
                __syncthreads();
            }
            if (live) {
                for (int j = 0; j < cnt; j++) {
                    const int lab = s_lab[j];
                    const float p = lab >= 0 ? softmax_at(row[lab], m, s) : 0.0f;
                    const float l1 = l1_f32(box, s_box[j], 4);
                    const float gi = giou_xyxy(xy, s_xy[j]);
                    out[(size_t)q * G + t0 + j] = (K.cost_bbox * l1 + K.cost_class * (-p)) + K.cost_giou * (-gi);
                }
            }
        }
    }
    if (flag) atomicOr(&s_flag, flag);      // (an integer OR in LDS: order-free)
    __syncthreads();
    if (tid == 0) K.status[b] = s_flag;
}

// ---- linear_sum_assignment, one wavefront per problem (matcher.py:76) -------------------------------------------------------------
struct LsapArgs {
    const float* cost; const long long* cost_off; const int* rows; const int* cols; const long long* match_off;
    long long n_cost, n_match;
    int* col_of_row; int* n_pairs; int* status;
};
struct LsKey { double c; unsigned t; };      // reduced cost; tail = not-free << 19 | tie key << 12 | column << 5 | row of the column (if assigned)
template <int BIT> __device__ __forceinline__ void ls_step(LsKey& b) {
    const double oc = ls_xor_f64<BIT>(b.c);
    const unsigned ot = ls_xor<BIT>(b.t);
    if (oc < b.c || (oc == b.c && ot < b.t)) { b.c = oc; b.t = ot; }
}

__global__ __launch_bounds__(64) void lsap_wave_kernel(LsapArgs K) {
    __shared__ double cost[LS_MAXR * LS_MAXC];
    __shared__ double u[LS_MAXR], spc_l[LS_MAXC];
    __shared__ int col4row[LS_MAXR], row4col[LS_MAXC], path_l[LS_MAXC], remaining[LS_MAXC];
    __shared__ unsigned char SR[LS_MAXR];
    const int lane = threadIdx.x, p = blockIdx.x;
    // ONE wavefront: its LDS operations execute in program order, so a wave-level fence (no s_barrier) orders a lane's write before the others' reads
    auto sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    const int R = K.rows[p], C = K.cols[p];
    const long long coff = K.cost_off[p], moff = K.match_off[p];
    const bool tr = C < R;                       // scipy transposes a tall matrix
    const int nr = tr ? C : R, nc = tr ? R : C;
    if (R < 0 || C < 0 || nr > LS_MAXR || nc > LS_MAXC || coff < 0 || moff < 0 || (long long)R * C > K.n_cost - coff || R > K.n_match - moff) {
        if (lane == 0) K.status[p] = 3;
        return;
    }
    int* out = K.col_of_row + moff;
    // the end of every path: one store per row of the problem
    auto finish = [&](int st) {
        sync();
        for (int r = lane; r < R; r += 64) out[r] = st ? -1 : (tr ? row4col[r] : col4row[r]);
        if (lane == 0) { K.status[p] = st; K.n_pairs[p] = st ? 0 : nr; }
    };
    const float* src = K.cost + coff;
    const int total = R * C;
    bool bad = false;
    for (int idx = lane; idx < total; idx += 64) {
        const float x = src[idx];
        const int r = idx / C, c = idx - r * C;
        cost[(tr ? c : r) * LS_MAXC + (tr ? r : c)] = (double)x;      // widened by the solver, as scipy widens a float32 matrix
        bad |= (x != x) || x == -__builtin_huge_valf();
    }
    for (int j = lane; j < nc; j += 64) row4col[j] = -1;
    if (lane < nr) { u[lane] = 0.0; col4row[lane] = -1; }
    if (__ballot(bad) != 0ull) { finish(1); return; }      // "matrix contains invalid numeric entries"
    // a lane keeps the state of its two columns (lane, lane + 64) in registers; rows, the scan list and what lane 0's augmentation walks are in LDS
    const int jc[2] = {lane, lane + 64};
    const bool has[2] = {jc[0] < nc, jc[1] < nc};
    double vv[2] = {0.0, 0.0}, spc[2];
    int r4c[2] = {-1, -1}, pth[2] = {-1, -1}, pos[2];
    bool SC[2];
    sync();
    const double INF = __builtin_huge_val();
    for (int cur = 0; cur < nr; cur++) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (has[q]) { remaining[nc - 1 - jc[q]] = jc[q]; r4c[q] = row4col[jc[q]]; }      // list position it holds column nc - it - 1
            pos[q] = nc - 1 - jc[q]; spc[q] = INF; SC[q] = !has[q];
        }
        if (lane < nr) SR[lane] = 0;
        sync();
        double minVal = 0.0;
        int i = cur, num_remaining = nc, sink = -1;
        while (sink == -1) {
            if (lane == 0) SR[i] = 1;
            const double ui = u[i];
            LsKey best{INF, 0xffffffffu};
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (SC[q]) continue;
                const double r = minVal + cost[i * LS_MAXC + jc[q]] - ui - vv[q];
                if (r < spc[q]) { pth[q] = i; spc[q] = r; }
                const bool free_ = r4c[q] == -1;
                // among equal reduced costs: the LAST free column of the scan (largest list position), else the first assigned one
                const unsigned t = (free_ ? 0u : 1u << 19) | (unsigned)(free_ ? 127 - pos[q] : pos[q]) << 12 | (unsigned)jc[q] << 5 | (unsigned)(free_ ? 0 : r4c[q]);
                if (spc[q] < best.c || (spc[q] == best.c && t < best.t)) { best.c = spc[q]; best.t = t; }
            }
            ls_step<0>(best); ls_step<1>(best); ls_step<2>(best); ls_step<3>(best); ls_step<4>(best); ls_step<5>(best);
            minVal = best.c;
            if (!(minVal < INF)) { finish(1); return; }      // "cost matrix is infeasible" (the same for every lane)
            const int j = (best.t >> 5) & 127, kk = (best.t >> 12) & 127;
            const bool jfree = !(best.t >> 19);
            const int idx = jfree ? 127 - kk : kk;                             // the winner's position in the list
            if (jfree) sink = j; else i = best.t & 31;
            const int last = remaining[num_remaining - 1];
            sync();
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (jc[q] == j) { SC[q] = true; remaining[idx] = last; }
                if (jc[q] == last) pos[q] = idx;
            }
            num_remaining--;
            sync();
        }
        // what the dual update of the rows and lane 0's augmentation read by column index
#pragma unroll
        for (int q = 0; q < 2; q++)
            if (has[q]) { spc_l[jc[q]] = spc[q]; path_l[jc[q]] = pth[q]; if (SC[q]) vv[q] -= minVal - spc[q]; }
        sync();
        if (lane < nr && SR[lane] && lane != cur) u[lane] += minVal - spc_l[col4row[lane]];
        if (lane == 0) u[cur] += minVal;
        sync();
        if (lane == 0) {
            int j = sink;
            while (true) {
                const int ii = path_l[j];
                row4col[j] = ii;
                const int t = col4row[ii]; col4row[ii] = j; j = t;
                if (ii == cur) break;
            }
        }
        sync();
    }
    finish(0);
}

// ---- the losses under an assignment (detr.py:286-384) ------------------------------------------------------------------------------
struct CritArgs {
    const float* logits; const float* boxes; const float* angle; const float* offset; const float* size; const float* depth;
    const float* objects; const int* obj_off; const int* match;
    int B, Q, n_logit, n_angle, n_obj, W;
    float eos;
    double num_boxes;
    double w[N_W];
    double* partial; double* table; int* status;
};

// layer l of [L][B][Q][.] predictions, match [L][B][Q], partial [L][B][11], table [L][10], status [L][B]: the single-layer call on
// that layer's words
__device__ __forceinline__ void crit_layer(CritArgs& K, const size_t l) {
    const size_t frames = l * (size_t)K.B, rows = frames * K.Q;
    K.logits += rows * K.n_logit; K.boxes += rows * 4; K.angle += rows * K.n_angle; K.offset += rows * 2; K.size += rows * 3;
    K.depth += rows; K.match += rows;
    K.partial += frames * N_PART; K.table += l * N_ENT; K.status += frames;
}

// LAYERS: grid (B, L), one wavefront per (frame, layer).  The <false> instantiation is the kernel as it was
template <bool LAYERS> __global__ __launch_bounds__(64) void criterion_frame_kernel(CritArgs K) {
    if constexpr (LAYERS) crit_layer(K, blockIdx.y);
    const int b = blockIdx.x, lane = threadIdx.x;
    double* part = K.partial + (size_t)b * N_PART;
    const int g0 = K.obj_off[b], g1 = K.obj_off[b + 1];
    if (g0 < 0 || g1 < g0 || g1 > K.n_obj) {      // (the same for every lane)
        if (lane < N_PART) part[lane] = 0.0;
        if (lane == 0) K.status[b] = ODAM_LOSS_ST_OFFSETS;
        return;
    }
    const int G = g1 - g0, none = K.n_logit - 1;
    double a_wnll = 0.0, a_w = 0.0, a_hit = 0.0, a_n = 0.0, a_card = 0.0, a_box = 0.0, a_giou = 0.0, a_size = 0.0, a_off = 0.0,
           a_dep = 0.0, a_ang = 0.0;
    unsigned flag = 0;
    for (int q = lane; q < K.Q; q += 64) {      // a lane's queries in ascending order
        const size_t bq = (size_t)b * K.Q + q;
        const float* row = K.logits + bq * K.n_logit;
        int am, ao;
        const float m = row_max(row, K.n_logit, &am);
        const float s = row_sumexp(row, K.n_logit, m);
        // loss_cardinality: the largest softmax over the object classes is the softmax of their largest logit
        const float mo = row_max(row, none, &ao);
        if (softmax_at(mo, m, s) > 0.7f) a_card = a_card + 1.0;
        int t = K.match[bq];
        if (t < -1 || t >= G) { flag |= ODAM_LOSS_ST_OFFSETS; t = -1; }
        const float* obj = K.objects + (size_t)(g0 + (t < 0 ? 0 : t)) * K.W;      // (read only when t >= 0)
        int cls = none;
        if (t >= 0) {
            cls = class_of(obj[0], K.n_logit);
            if (cls < 0) { flag |= ODAM_LOSS_ST_CLASS; cls = none; }
        }
        // loss_labels: cross entropy weighted by the target's class
        const float w = cls == none ? K.eos : 1.0f;
        a_wnll = a_wnll + (double)(w * nll_at(row[cls], m, s));
        a_w = a_w + (double)w;
        if (t < 0) continue;
        a_n = a_n + 1.0;
        if (am == cls) a_hit = a_hit + 1.0;
        // loss_boxes
        float pb[4], tb[4], pxy[4], txy[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { pb[k] = K.boxes[bq * 4 + k]; tb[k] = obj[1 + k]; }
        a_box = a_box + l1_f64(pb, tb, 4);
        xyxy_of(pb, pxy); xyxy_of(tb, txy);
        if (xyxy_ok(pxy) && xyxy_ok(txy)) a_giou = a_giou + (double)(1.0f - giou_xyxy(pxy, txy));
        else flag |= ODAM_LOSS_ST_DEGENERATE;
        // loss_size, loss_offset, loss_depth
        a_size = a_size + l1_f64(K.size + bq * 3, obj + 5, 3);
        a_off = a_off + l1_f64(K.offset + bq * 2, obj + 8, 2);
        a_dep = a_dep + l1_f64(K.depth + bq, obj + K.W - 2, 1);
        // loss_angle
        const int ka = class_of(obj[K.W - 1], K.n_angle);
        if (ka < 0) { flag |= ODAM_LOSS_ST_CLASS; continue; }
        const float* arow = K.angle + bq * K.n_angle;
        int aa;
        const float ma = row_max(arow, K.n_angle, &aa);
        a_ang = a_ang + (double)nll_at(arow[ka], ma, row_sumexp(arow, K.n_angle, ma));
    }
    a_wnll = wave_sum_f64(a_wnll); a_w = wave_sum_f64(a_w); a_hit = wave_sum_f64(a_hit); a_n = wave_sum_f64(a_n);
    a_card = wave_sum_f64(a_card); a_box = wave_sum_f64(a_box); a_giou = wave_sum_f64(a_giou); a_size = wave_sum_f64(a_size);
    a_off = wave_sum_f64(a_off); a_dep = wave_sum_f64(a_dep); a_ang = wave_sum_f64(a_ang);
    flag = wave_or(flag);
    if (lane == 0) {
        const double d = a_card - (double)G;
        part[0] = a_wnll; part[1] = a_w; part[2] = a_hit; part[3] = a_n; part[4] = d < 0.0 ? -d : d; part[5] = a_box;
        part[6] = a_giou; part[7] = a_size; part[8] = a_off; part[9] = a_dep; part[10] = a_ang;
        K.status[b] = (int)flag;
    }
}

// LAYERS: grid (L), one wavefront per layer.  The <false> instantiation is the kernel as it was
template <bool LAYERS> __global__ __launch_bounds__(64) void criterion_table_kernel(CritArgs K) {
    if constexpr (LAYERS) crit_layer(K, blockIdx.x);
    __shared__ double S[N_PART];
    const int lane = threadIdx.x;
    if (lane < N_PART) {
        double s = 0.0;
        for (int b = 0; b < K.B; b++) s = s + K.partial[(size_t)b * N_PART + lane];      // frames in index order
        S[lane] = s;
    }
    __syncthreads();
    if (lane != 0) return;
    double T[N_ENT];
    T[0] = S[0] / S[1];
    T[1] = S[3] > 0.0 ? 100.0 - 100.0 * S[2] / S[3] : 100.0;
    T[2] = S[4] / (double)K.B;
    for (int k = 0; k < 6; k++) T[3 + k] = S[5 + k] / K.num_boxes;
    const int entry_of_weight[N_W] = {0, 3, 4, 5, 6, 7, 8};
    double tot = 0.0;
    for (int k = 0; k < N_W; k++)
        if (K.w[k] != 0.0) tot = tot + K.w[k] * T[entry_of_weight[k]];
    T[9] = tot;
    for (int k = 0; k < N_ENT; k++) K.table[k] = T[k];
}

}  // namespace

extern "C" int odam_detr_match_cost_layers(const float* logits, const float* boxes, int L, int B, int Q, int n_logit,
                                           const float* objects, const int* obj_off, int n_obj, int W, float cost_class,
                                           float cost_bbox, float cost_giou, float* cost_out, int* out_status, void* stream) {
    if (L < 1) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost_layers: at least one layer");
    if (L > 65535) return odam_fail(ODAM_E_LIMIT, "odam_detr_match_cost_layers: more than 65535 layers");
    if (B < 0 || Q < 0 || n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost_layers: bad size");
    if (n_logit < 2) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost_layers: n_logit below 2 (classes and the no-object column)");
    if (W < 12) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost_layers: target rows need W >= 12");
    if (!logits || !boxes || !objects || !obj_off || !cost_out || !out_status)
        return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost_layers: null pointer");
    if (B == 0) return ODAM_OK;
    CostArgs K{logits, boxes, objects, obj_off, B, Q, n_logit, n_obj, W, cost_class, cost_bbox, cost_giou, cost_out, out_status};
    hipLaunchKernelGGL(match_cost_kernel<true>, dim3((unsigned)B, (unsigned)L), dim3(COST_BLOCK), 0, (hipStream_t)stream, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_detr_match_cost(const float* logits, const float* boxes, int B, int Q, int n_logit, const float* objects,
                                    const int* obj_off, int n_obj, int W, float cost_class, float cost_bbox, float cost_giou,
                                    float* cost_out, int* out_status, void* stream) {
    if (B < 0 || Q < 0 || n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost: bad size");
    if (n_logit < 2) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost: n_logit below 2 (classes and the no-object column)");
    if (W < 12) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost: target rows need W >= 12");
    if (!logits || !boxes || !objects || !obj_off || !cost_out || !out_status) return odam_fail(ODAM_E_INVALID, "odam_detr_match_cost: null pointer");
    if (B == 0) return ODAM_OK;
    CostArgs K{logits, boxes, objects, obj_off, B, Q, n_logit, n_obj, W, cost_class, cost_bbox, cost_giou, cost_out, out_status};
    hipLaunchKernelGGL(match_cost_kernel<false>, dim3((unsigned)B), dim3(COST_BLOCK), 0, (hipStream_t)stream, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_lsap_batch(const float* cost, long long n_cost, const long long* cost_off, const int* rows, const int* cols,
                               int n_prob, int max_small, int max_large, const long long* match_off, long long n_match,
                               int* col_of_row, int* n_pairs, int* status, void* stream) {
    if (n_prob < 0 || max_small < 0 || max_large < max_small || n_cost < 0 || n_match < 0) return odam_fail(ODAM_E_INVALID, "odam_lsap_batch: bad size");
    if (!cost || !cost_off || !rows || !cols || !match_off || !col_of_row || !n_pairs || !status)
        return odam_fail(ODAM_E_INVALID, "odam_lsap_batch: null pointer");
    if (max_small > LS_MAXR || max_large > LS_MAXC) return odam_fail(ODAM_E_LIMIT, "odam_lsap_batch: more than 32 x 128 (the caller solves it on the host)");
    if (n_prob == 0) return ODAM_OK;
    LsapArgs K{cost, cost_off, rows, cols, match_off, n_cost, n_match, col_of_row, n_pairs, status};
    hipLaunchKernelGGL(lsap_wave_kernel, dim3((unsigned)n_prob), dim3(64), 0, (hipStream_t)stream, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_detr_criterion(const float* logits, const float* boxes, const float* angle, const float* offset,
                                   const float* size, const float* depth, int B, int Q, int n_logit, int n_angle,
                                   const float* objects, const int* obj_off, int n_obj, int W, const int* match, double num_boxes,
                                   float eos_coef, const double* weights, double* out_partial, double* out_table, int* out_status,
                                   void* stream) {
    if (B < 1 || Q < 0 || n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion: bad size (at least one frame)");
    if (n_logit < 2 || n_angle < 1) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion: n_logit below 2 or n_angle below 1");
    if (W < 12) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion: target rows need W >= 12");
    if (!(num_boxes > 0.0)) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion: num_boxes must be positive");
    if (!logits || !boxes || !angle || !offset || !size || !depth || !objects || !obj_off || !match || !weights || !out_partial ||
        !out_table || !out_status)
        return odam_fail(ODAM_E_INVALID, "odam_detr_criterion: null pointer");
    CritArgs K{};
    K.logits = logits; K.boxes = boxes; K.angle = angle; K.offset = offset; K.size = size; K.depth = depth; K.objects = objects;
    K.obj_off = obj_off; K.match = match; K.B = B; K.Q = Q; K.n_logit = n_logit; K.n_angle = n_angle; K.n_obj = n_obj; K.W = W;
    K.eos = eos_coef; K.num_boxes = num_boxes;
    for (int k = 0; k < N_W; k++) K.w[k] = weights[k];
    K.partial = out_partial; K.table = out_table; K.status = out_status;
    hipLaunchKernelGGL(criterion_frame_kernel<false>, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, K);
    hipLaunchKernelGGL(criterion_table_kernel<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}

extern "C" int odam_detr_criterion_layers(const float* logits, const float* boxes, const float* angle, const float* offset,
                                          const float* size, const float* depth, int L, int B, int Q, int n_logit, int n_angle,
                                          const float* objects, const int* obj_off, int n_obj, int W, const int* match,
                                          double num_boxes, float eos_coef, const double* weights, double* out_partial,
                                          double* out_table, int* out_status, void* stream) {
    if (L < 1) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion_layers: at least one layer");
    if (L > 65535) return odam_fail(ODAM_E_LIMIT, "odam_detr_criterion_layers: more than 65535 layers");
    if (B < 1 || Q < 0 || n_obj < 0) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion_layers: bad size (at least one frame)");
    if (n_logit < 2 || n_angle < 1) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion_layers: n_logit below 2 or n_angle below 1");
    if (W < 12) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion_layers: target rows need W >= 12");
    if (!(num_boxes > 0.0)) return odam_fail(ODAM_E_INVALID, "odam_detr_criterion_layers: num_boxes must be positive");
    if (!logits || !boxes || !angle || !offset || !size || !depth || !objects || !obj_off || !match || !weights || !out_partial ||
        !out_table || !out_status)
        return odam_fail(ODAM_E_INVALID, "odam_detr_criterion_layers: null pointer");
    CritArgs K{};
    K.logits = logits; K.boxes = boxes; K.angle = angle; K.offset = offset; K.size = size; K.depth = depth; K.objects = objects;
    K.obj_off = obj_off; K.match = match; K.B = B; K.Q = Q; K.n_logit = n_logit; K.n_angle = n_angle; K.n_obj = n_obj; K.W = W;
    K.eos = eos_coef; K.num_boxes = num_boxes;
    for (int k = 0; k < N_W; k++) K.w[k] = weights[k];
    K.partial = out_partial; K.table = out_table; K.status = out_status;
    hipLaunchKernelGGL(criterion_frame_kernel<true>, dim3((unsigned)B, (unsigned)L), dim3(64), 0, (hipStream_t)stream, K);
    hipLaunchKernelGGL(criterion_table_kernel<true>, dim3((unsigned)L), dim3(64), 0, (hipStream_t)stream, K);
    ODAM_HIP(hipGetLastError());
    return ODAM_OK;
}
