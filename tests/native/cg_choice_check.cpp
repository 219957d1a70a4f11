// odam_cg::choose (odam_amd/csrc/cg_choice.h) as a host program: no HIP, no library.  tests/test_cg_choice_host.py builds it with g++
// and compares what it prints with tests/golden/cg_choice.npz and with the tokens the GPU tests assert.
//   cg_choice_check cross|zip ROWS SETTINGS   (text: 41 integers per row in the order of tests/cg_choice_rows.py FIELDS, 13 per setting
//                                              in the order of SWITCHES; cross = every row under every setting, rows outermost;
//                                              zip = row i under setting i)
//   one line per call:
//     <family> <code> <bm> <bn> <waves> <stages> <ut> <x3> <mode> <pool> <chain> <s1_window> <fused_second_ok> <fused_bf16_ok>
//     <pooled_stem_ok> | <token, or the message of a refusal>
//   The switches reach choose() through current_switches() and the table below, so the snapshot is under test as well.
#include <cstdio>
#include <vector>

#include "../../odam_amd/csrc/cg_choice.hip"

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

static odam_cg::ConvGemmArgs args_of(const std::vector<long>& r) {
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
    return a;
}

static void one(const odam_cg::ConvGemmArgs& a, const std::vector<long>& s) {
    using namespace odam_cfg;
    static const Key KEYS[13] = {CG_RING, CG_F32, CG_FUSE, CG_FUSE_BF16, CG_S1, CG_UT, CG_TILES, CG_FORCE, CG_PRESPLIT, CG_MFMA16, CG_PIN,
                                 CG_SMALL_X3, STEM_POOL};
    for (int k = 0; k < 13; k++) set(KEYS[k], (int)s[k]);
    const odam_cg::Choice c = odam_cg::choose(a, odam_cg::current_switches());
    char tok[odam_cg::PATH_TOKEN_LEN];
    odam_cg::choice_token(c, tok);
    static const char* FAMILY[] = {"Refused", "Nothing", "Small", "RingF32", "RingBF16", "FusedF32", "FusedBF16"};
    printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d | %s\n", FAMILY[(int)c.family], c.code, c.bm, c.bn, c.waves, c.stages, (int)c.ut,
           (int)c.x3, c.mode, (int)c.pool, c.chain, c.s1_window, (int)odam_cg::fused_second_ok(a), (int)odam_cg::fused_bf16_ok(a),
           (int)odam_cg::pooled_stem_ok(a), c.family == odam_cg::Family::Refused ? c.message : tok);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const bool zip = argv[1][0] == 'z';
    const auto rows = read_table(argv[2], 41), settings = read_table(argv[3], 13);
    if (rows.empty() || settings.empty() || (zip && rows.size() != settings.size())) return 2;
    for (size_t r = 0; r < rows.size(); r++) {
        const odam_cg::ConvGemmArgs a = args_of(rows[r]);
        if (zip) one(a, settings[r]);
        else
            for (const auto& s : settings) one(a, s);
    }
    return 0;
}
