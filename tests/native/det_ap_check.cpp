// Host build of odam_amd/csrc/det_ap_core.h as a stand-alone program (test infrastructure): reads cases that the numpy restatement
// tests/det_ap_ref.py wrote with its own answers, computes them with the header and compares bit for bit (NaN for NaN).
//   g++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] tests/native/det_ap_check.cpp -o det_ap_check
//   det_ap_check cases.txt        exit status 0 when every case agrees; prints the count and the first disagreements
// One case per line, every float as the hex of its bits:
//   C <48 binary64: 8 corners of A, 8 of B> <iou>       kind 0: aabb_of_corners + iou_3d
//   R <30 binary32: two detection rows> <iou3d> <iou2d> kinds 2, 3: aabb_of_row + iou_3d, iou_2d_rows
//   K <score e> <e> <score d> <d> <0 | 1>               ranks_before
//   V <tp> <fp> <npos> <rec> <prec>                     curve_rec, curve_prec
//   T <i> <threshold>                                   ap11_threshold
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../odam_amd/csrc/det_ap_core.h"

using namespace odam_ap;

static bool same(double a, double b) {
    uint64_t x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x == y || (a != a && b != b);
}

static bool read_d(FILE* f, double* v) {
    uint64_t u;
    if (fscanf(f, "%" SCNx64, &u) != 1) return false;
    memcpy(v, &u, 8);
    return true;
}

static bool read_f(FILE* f, float* v) {
    uint32_t u;
    if (fscanf(f, "%" SCNx32, &u) != 1) return false;
    memcpy(v, &u, 4);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    long n_case = 0, n_bad = 0;
    char tag[4];
    while (fscanf(f, "%3s", tag) == 1) {
        bool ok = true, parsed = true;
        if (tag[0] == 'C') {
            double a[24], b[24], want;
            for (int k = 0; k < 24; k++) parsed = parsed && read_d(f, &a[k]);
            for (int k = 0; k < 24; k++) parsed = parsed && read_d(f, &b[k]);
            parsed = parsed && read_d(f, &want);
            if (parsed) {
                double alo[3], ahi[3], blo[3], bhi[3];
                aabb_of_corners(a, alo, ahi);
                aabb_of_corners(b, blo, bhi);
                ok = same(iou_3d(alo, ahi, blo, bhi), want);
            }
        } else if (tag[0] == 'R') {
            float ra[ROW_WORDS], rb[ROW_WORDS];
            double want3, want2;
            for (int k = 0; k < ROW_WORDS; k++) parsed = parsed && read_f(f, &ra[k]);
            for (int k = 0; k < ROW_WORDS; k++) parsed = parsed && read_f(f, &rb[k]);
            parsed = parsed && read_d(f, &want3) && read_d(f, &want2);
            if (parsed) {
                double alo[3], ahi[3], blo[3], bhi[3];
                aabb_of_row(ra, alo, ahi);
                aabb_of_row(rb, blo, bhi);
                ok = same(iou_3d(alo, ahi, blo, bhi), want3) && same(iou_2d_rows(ra, rb), want2);
            }
        } else if (tag[0] == 'K') {
            double se, sd;
            int e, d, want;
            parsed = read_d(f, &se) && fscanf(f, "%d", &e) == 1 && read_d(f, &sd) && fscanf(f, "%d %d", &d, &want) == 2;
            if (parsed) ok = (ranks_before(se, e, sd, d) ? 1 : 0) == want;
        } else if (tag[0] == 'V') {
            int tp, fp, npos;
            double rec, prec;
            parsed = fscanf(f, "%d %d %d", &tp, &fp, &npos) == 3 && read_d(f, &rec) && read_d(f, &prec);
            if (parsed) ok = same(curve_rec(tp, npos), rec) && same(curve_prec(tp, fp), prec);
        } else if (tag[0] == 'T') {
            int i;
            double want;
            parsed = fscanf(f, "%d", &i) == 1 && read_d(f, &want);
            if (parsed) ok = same(ap11_threshold(i), want);
        } else {
            parsed = false;
        }
        if (!parsed) {
            fprintf(stderr, "case %ld: cannot parse a '%s' line\n", n_case, tag);
            fclose(f);
            return 2;
        }
        if (!ok && n_bad++ < 10) fprintf(stderr, "case %ld (%s) differs from the restatement\n", n_case, tag);
        n_case++;
    }
    fclose(f);
    printf("det_ap_check: %ld cases, %ld differ\n", n_case, n_bad);
    return (n_bad == 0 && n_case > 0) ? 0 : 1;
}
