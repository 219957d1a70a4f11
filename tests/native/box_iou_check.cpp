// box_iou_check.cpp -- the leaf arithmetic of the IoU kernel (odam_amd/csrc/box_iou_core.h) compiled for the host, as a stand-alone
// program: reads n pairs of boxes, writes their 3D and bird's-eye IoU.  tests/test_evaluate_host.py holds the output bit for bit
// against tests/box_iou_ref.py; built with -fsanitize=address,undefined it is the sanitizer pass of that header.
//   g++ -O2 -std=c++17 -ffp-contract=off -o box_iou_check tests/native/box_iou_check.cpp
//   box_iou_check in.bin out.bin      in: int64 n, n x [8][3] float64 (box 1), n x [8][3] float64 (box 2);  out: n x 2 float64
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../odam_amd/csrc/box_iou_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t n = 0;
    if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > (1 << 24)) return 4;
    std::vector<double> a((size_t)n * 24), b((size_t)n * 24), out((size_t)n * 2);
    if (std::fread(a.data(), sizeof(double), a.size(), f) != a.size() || std::fread(b.data(), sizeof(double), b.size(), f) != b.size()) return 5;
    std::fclose(f);
    for (int64_t i = 0; i < n; i++) {
        double bev = 0.0;
        out[2 * i] = odam_biou::box3d_iou(&a[24 * i], &b[24 * i], bev);
        out[2 * i + 1] = bev;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 6;
    if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 7;
    std::fclose(f);
    return 0;
}
