// The host side of the uint8 stem as a host program: no HIP, no library.  tests/test_stem_u8_host.py builds it with g++.
//   stem_u8_check choose ROWS SETTINGS   text: 42 integers per row (tests/cg_choice_rows.py FIELDS, then ConvGemmArgs::a_bf16), 13 per
//                                        setting (SWITCHES); row i under setting i.  One line per call:
//                                          <family> <code> <mode> <bm> <bn> <waves> <pool> <bf16_plane_ok> | <token, or the refusal's message>
//   stem_u8_check fold FILE              binary: float mean[3], std[3], w[64][3][7][7].  Prints the three centres, then the 64 x 224 folded
//                                        filters (odam_amd/csrc/stem_u8_fold.h) as hexadecimal floats
//   stem_u8_check frame H W c0 c1 c2 FILE   binary: uint8 [H][W][3].  Prints the framed image [H + 6][W + 8] as two hexadecimal words per
//                                        pixel, built from the functions the producer kernel is built from
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../odam_amd/csrc/cg_choice.hip"
#include "../../odam_amd/csrc/stem_u8_fold.h"

namespace odam_cfg {
static int g_table[N_KEYS];
int get(Key k) { return g_table[k]; }
void set(Key k, int v) { g_table[k] = v; }
}  // namespace odam_cfg

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

static odam_cg::ConvGemmArgs args_of(const std::vector<long>& r) {      // (the field order of tests/native/cg_choice_check.cpp, then a_bf16)
    static float placeholder[4];
    void* const P = placeholder;
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
    a.a_bf16 = I();
    return a;
}

static int choose_mode(const char* rows_path, const char* settings_path) {
    using namespace odam_cfg;
    static const Key KEYS[13] = {CG_RING, CG_F32, CG_FUSE, CG_FUSE_BF16, CG_S1, CG_UT, CG_TILES, CG_FORCE, CG_PRESPLIT, CG_MFMA16, CG_PIN,
                                 CG_SMALL_X3, STEM_POOL};
    static const char* FAMILY[] = {"Refused", "Nothing", "Small", "RingF32", "RingBF16", "FusedF32", "FusedBF16"};
    const auto rows = read_table(rows_path, 42), settings = read_table(settings_path, 13);
    if (rows.empty() || rows.size() != settings.size()) return 2;
    for (size_t r = 0; r < rows.size(); r++) {
        const odam_cg::ConvGemmArgs a = args_of(rows[r]);
        for (int k = 0; k < 13; k++) set(KEYS[k], (int)settings[r][k]);
        const odam_cg::Choice c = odam_cg::choose(a, odam_cg::current_switches());
        char tok[odam_cg::PATH_TOKEN_LEN];
        odam_cg::choice_token(c, tok);
        printf("%s %d %d %d %d %d %d %d | %s\n", FAMILY[(int)c.family], c.code, c.mode, c.bm, c.bn, c.waves, (int)c.pool,
               (int)odam_cg::bf16_plane_ok(a), c.family == odam_cg::Family::Refused ? c.message : tok);
    }
    return 0;
}

static std::vector<unsigned char> read_file(const char* path) {
    std::vector<unsigned char> b;
    FILE* f = fopen(path, "rb");
    if (!f) return b;
    unsigned char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

static int fold_mode(const char* path) {
    const std::vector<unsigned char> b = read_file(path);
    const size_t nw = (size_t)64 * 147;
    if (b.size() != (6 + nw) * 4) return 2;
    std::vector<float> v(6 + nw);
    memcpy(v.data(), b.data(), b.size());
    int c[3];
    odam_dm::stem_u8_centres(v.data(), c);
    printf("%d %d %d\n", c[0], c[1], c[2]);
    std::vector<float> rows((size_t)64 * 224, -1.0f);
    odam_dm::stem_u8_fold(v.data() + 6, 64, v.data(), v.data() + 3, rows.data());
    for (float x : rows) printf("%a\n", (double)x);
    return 0;
}

static int frame_mode(int H, int W, int c0, int c1, int c2, const char* path) {
    const std::vector<unsigned char> img = read_file(path);
    if (img.size() != (size_t)H * W * 3) return 2;
    for (int Yp = 0; Yp < H + 6; Yp++)
        for (int Xp = 0; Xp < W + 8; Xp++) {
            int X, Y;
            unsigned w0 = 0, w1 = 0;
            if (odam_dm::stem_u8_inside(Xp, Yp, H, W, X, Y)) {
                const unsigned char* p = img.data() + ((size_t)Y * W + X) * 3;
                odam_dm::stem_u8_pixel(p[0], p[1], p[2], c0, c1, c2, w0, w1);
            }
            printf("%x %x\n", w0, w1);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "choose")) return choose_mode(argv[2], argv[3]);
    if (argc == 3 && !strcmp(argv[1], "fold")) return fold_mode(argv[2]);
    if (argc == 8 && !strcmp(argv[1], "frame")) return frame_mode(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), argv[7]);
    return 2;
}
