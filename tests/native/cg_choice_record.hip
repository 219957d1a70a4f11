// What a built checkout of this project chooses for a table of contraction calls: calls ITS launch_conv_gemm with placeholder
// operands and reads the token back (read_paths).  Meant for a machine without a GPU: the token is noted before the launch fails,
// a refusal returns before any HIP call.  Used by tests/golden/make_golden_cg_choice.py, which compiles it against the checkout's
// headers and library.
//   cg_choice_record ROWS SETTINGS   (text files: one row of 41 integers per line in the order of tests/cg_choice_rows.py FIELDS;
//                                     one setting of 13 integers per line in the order of SWITCHES)
//   prints one line per (row, setting), rows outermost:  T <token>  |  R <code> <error text>  |  N
#include <cstdio>
#include <cstring>
#include <vector>

#include "conv_gemm.h"

extern "C" int odam_config_set(const char* key, int value);
extern "C" const char* odam_last_error(void);

static std::vector<std::vector<long>> read_table(const char* path, size_t width) {
    std::vector<std::vector<long>> t;
    FILE* f = fopen(path, "r");
    if (!f) return t;
    std::vector<long> row(width);
    for (;;) {
        size_t i = 0;
        for (; i < width; i++)
            if (fscanf(f, "%ld", &row[i]) != 1) break;
        if (i < width) break;
        t.push_back(row);
    }
    fclose(f);
    return t;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    static const char* KEYS[13] = {"cg.ring", "cg.f32", "cg.fuse", "cg.fuse_bf16", "cg.s1", "cg.ut", "cg.tiles", "cg.force", "cg.presplit",
                                   "cg.mfma16", "cg.pin", "cg.small_x3", "stem.pool"};
    const auto rows = read_table(argv[1], 41), settings = read_table(argv[2], 13);
    if (rows.empty() || settings.empty()) return 2;
    static float placeholder[4];
    void* const P = placeholder;
    char buf[256];
    for (const auto& r : rows) {
        odam_cg::ConvGemmArgs a{};
        size_t i = 0;
        auto I = [&] { return (int)r[i++]; };
        auto ptr = [&] { return r[i++] ? P : nullptr; };
        a.A = P; a.Wt = P; a.C = P;
        a.B = I(); a.H = I(); a.W = I(); a.Cin = I(); a.log2Cin = I(); a.Ho = I(); a.Wo = I(); a.Cout = I(); a.KH = I(); a.KW = I();
        a.stride = I(); a.pad = I(); a.Kpad = I(); a.relu = I(); a.M = I(); a.ldc = I(); a.dtype = I(); a.out_f32 = I(); a.lda = I();
        a.k_order = I(); a.F_ldc = I(); a.F_relu = I(); a.G_N = I(); a.dil = I(); a.pool = I(); a.pool_ph = I(); a.pool_pw = I();
        a.Hp = I(); a.Wp = I(); a.no_pin = I();
        a.Wt3 = ptr(); a.scale = (const float*)ptr(); a.bias = (const float*)ptr(); a.res = ptr(); a.F_Wt3 = ptr();
        a.F_res = (const float*)ptr(); a.F_C = (float*)ptr(); a.G_Wt3 = ptr(); a.G_C = (float*)ptr(); a.F_Wt = ptr(); a.G_Wt = ptr();
        for (const auto& s : settings) {
            for (int k = 0; k < 13; k++)
                if (odam_config_set(KEYS[k], (int)s[k]) != 0) { fprintf(stderr, "%s\n", odam_last_error()); return 3; }
            odam_cg::read_paths(nullptr, 0, 1);
            const int rc = odam_cg::launch_conv_gemm(a, nullptr);
            const long long noted = odam_cg::read_paths(buf, sizeof(buf), 1);
            if (noted > 1 || strchr(buf, '\n')) { fprintf(stderr, "more than one token\n"); return 3; }
            if (noted == 1) printf("T %s\n", buf);
            else if (rc != 0) printf("R %d %s\n", rc, odam_last_error());
            else printf("N\n");
        }
    }
    return 0;
}
