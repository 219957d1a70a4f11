// cg_choice.hip -- see cg_choice.h.  Host code only, and plain C++ (no HIP header): tests/native/cg_choice_check.cpp compiles this
// file with the host compiler.
#include "cg_choice.h"

#include <cstdio>

#include "odam_config.h"

namespace odam_cg {

Switches current_switches() {
    using namespace odam_cfg;
    return {get(CG_RING), get(CG_F32),      get(CG_FUSE),   get(CG_FUSE_BF16), get(CG_S1),       get(CG_UT),    get(CG_TILES),
            get(CG_FORCE), get(CG_PRESPLIT), get(CG_MFMA16), get(CG_PIN),       get(CG_SMALL_X3), get(STEM_POOL)};
}

void set_big_mode(int mode) { odam_cfg::set(odam_cfg::CG_RING, mode); }
// (1, the fp32 instruction inside the ring schedule, was measured slower than the 128x128 tiles and is gone)
void set_f32_mode(int mode) { odam_cfg::set(odam_cfg::CG_F32, mode == 1 ? 0 : mode); }
int f32_mode() {
    const Switches sw = current_switches();
    return sw.ring ? sw.f32 : 0;
}

namespace {

inline bool is_bf16(const ConvGemmArgs& a) { return a.dtype == ODAM_CG_BF16; }

// the kernels address through buffer descriptors and 32-bit gather offsets: a byte offset has 31 bits
inline bool fits31(long bytes) { return bytes < 0x7fffffffL; }

// elements between the first image a tile of bm rows touches and the last element it can read (a tile spans at most
// bm / (Ho * Wo) + 2 images)
inline long tile_span(const ConvGemmArgs& a, int bm) {
    const long lda = a.lda > 0 ? a.lda : a.Cin;
    return ((long)bm / ((long)a.Ho * a.Wo) + 2) * a.H * a.W * lda + (long)(a.pad * a.W + a.pad) * lda + a.Cin;
}
// ... and with it the input offsets of a tile and the filter offsets in bytes
inline bool offsets_fit(const ConvGemmArgs& a, int bm) {
    const long esz = is_bf16(a) ? 2 : 4;
    return fits31(tile_span(a, bm) * esz) && fits31((long)a.Cout * a.Kpad * esz);
}
// pre-split filters (three bf16 planes per weight, 16-k groups) exist for the layer and can be addressed
inline bool split_planes_fit(int Cout, int Kpad) { return Kpad % 16 == 0 && fits31((long)Cout * Kpad * 6); }

// cg.pin: the choice a device-filling problem gets, whatever M is -- for callers whose row count depends on how a scene is sharded
// (the detector); a caller whose rows are the same on every rank (the replicated association network) opts out with no_pin
inline bool pinned(const ConvGemmArgs& a, const Switches& sw) { return sw.pin != 0 && !a.no_pin; }
// at least as many 512-row tiles as CUs (fewer: the 256-row ones)
inline bool fills_512_row_tiles(const ConvGemmArgs& a, const Switches& sw) { return (a.M + 511) / 512 >= 256 || pinned(a, sw); }
inline bool is_3x3_stride1(const ConvGemmArgs& a) { return a.KH * a.KW == 9 && a.stride == 1; }

// the ring kernel (256-row tiles, bn columns) takes a layer when its gather is uniform-tap at the ring's k-tile (16 fp32 / 32 bf16)
// and the problem is large enough to give every CU a 256-row tile with a K loop worth pipelining
bool ring_eligible(const ConvGemmArgs& a, const Switches& sw, int bn) {
    const bool bf = is_bf16(a);
    if (!bf && !sw.f32) return false;
    const int bke = bf ? 32 : 16;
    if (a.Cin % bke != 0 || a.KH * a.KW > 32 || a.Kpad % bke != 0) return false;
    if (a.k_order && a.Cin % (2 * bke) != 0) return false;
    if (!offsets_fit(a, 256)) return false;
    if (sw.ring >= 2) return true;
    if (pinned(a, sw)) return a.Cout >= bn;
    const long tiles = (long)((a.M + 255) / 256) * ((a.Cout + bn - 1) / bn);
    return tiles >= 192 && a.Cout >= bn;     // short-K expand layers too: with 16-byte stores its one block per CU streams faster than two 128x128 blocks
}

// fp32 layers on the ring kernel: 2 = both operands split in registers; with pre-split filters (Wt3; cg.presplit) 3 = the 32x32x16
// schedule, 4 = the 16x16x32 one (cg.mfma16)
int ring_mode_f32(const ConvGemmArgs& a, const Switches& sw) {
    const bool pre = sw.f32 == 2 && a.Wt3 != nullptr && sw.presplit != 0 && split_planes_fit(a.Cout, a.Kpad);
    if (!pre) return 2;
    const bool x16 = sw.mfma16 != 0 && (a.Cout & 3) == 0 && (a.ldc & 3) == 0 && a.Kpad % 32 == 0;
    return x16 ? 4 : 3;
}

Choice refuse(const char* message) {
    Choice c;
    c.family = Family::Refused; c.code = 1; c.message = message;
    return c;
}

// a plain layer on the ring kernel: waves = 8 (256-row tiles) or 16 (256 x 256 tiles of four waves per SIMD; 512 x 64 tiles)
Choice ring(const ConvGemmArgs& a, const Switches& sw, int mode, int bn, int waves) {
    Choice c;
    c.family = is_bf16(a) ? Family::RingBF16 : Family::RingF32;
    c.bf16 = is_bf16(a);
    c.mode = mode; c.bn = bn; c.waves = waves; c.bm = (waves == 16 && bn == 64) ? 512 : 256;
    c.pool = a.pool != 0;
    c.s1_window = (is_bf16(a) && waves == 8) ? sw.s1 : 0;      // bf16 3x3 stride 1: window main loop (0: the generic tap gather)
    return c;
}

// the 128x128 / 128x64 / 64x64 tiles.  deep: four LDS stages where the gather is LDS-DMA
Choice small_tiles(const ConvGemmArgs& a, const Switches& sw, int bm, int bn, int waves, bool deep = false) {
    Choice c;
    c.family = Family::Small;
    c.bf16 = is_bf16(a);
    c.bm = bm; c.bn = bn; c.waves = waves;
    // uniform-tap gather: whole k-tiles inside one tap, a 32-bit tap mask, and 31-bit byte offsets from the first image a tile touches
    c.ut = sw.ut != 0 && a.Cin % (c.bf16 ? 64 : 32) == 0 && a.KH * a.KW <= 32 && offsets_fit(a, bm);
    // fp32 split mode reaches the layers too small for the ring kernel as well (cg.small_x3): the same six exact products on
    // v_mfma_f32_32x32x16_bf16, both operands split in registers.  Forward of 2 / 8 / 16 frames 4.89 -> 4.59 / 10.24 -> 9.66 /
    // 17.36 -> 16.84 ms (same box, A/B by config); a batch of 32 has few such layers left (30.45 -> 30.32)
    c.x3 = !c.bf16 && c.ut && sw.f32 == 2 && sw.small_x3 != 0;
    c.stages = (c.ut && deep) ? 4 : 2;
    return c;
}

}  // namespace

// the fused kernel applies: fp32 split mode with pre-split filters on both layers, 64 -> 256 or 128 -> 512 channels, a full device
bool fused_second_ok(const ConvGemmArgs& a, const Switches& sw) {
    if (!sw.fuse || !sw.ring || sw.f32 != 2 || a.dtype != ODAM_CG_F32) return false;
    if (!a.F_Wt3 || !a.F_C || !a.Wt3) return false;
    const bool l1 = a.Cout == 64 && a.F_ldc == 256, l2 = a.Cout == 128 && a.F_ldc == 512 && !a.G_Wt3;     // the two shapes built
    if ((!l1 && !l2) || a.dil != 1) return false;
    // buffer descriptors over the output / residual: 31-bit byte offsets within ONE image (launch_big_fused runs a larger batch as
    // groups of whole images, so that the choice does not depend on the batch)
    if (!split_planes_fit(a.Cout, a.Kpad) || !fits31((long)a.Ho * a.Wo * a.F_ldc * 4)) return false;
    if (a.G_Wt3 && (sw.fuse < 2 || !a.G_C || (a.G_N != 64 && a.G_N != 128))) return false;      // fuse 1: second layer only
    return ring_eligible(a, sw, a.Cout);
}

// bf16: the 3x3 + expand (+ next reduce) kernel applies -- ring kernel eligible for the 3x3, the channel combination built,
// residual / output tensors inside 31-bit byte offsets.  cg.fuse_bf16: 0 off, 1 expand only, 2 with the chained reduce
bool fused_bf16_ok(const ConvGemmArgs& a, const Switches& sw) {
    if (!sw.fuse_bf16 || !sw.ring || a.dtype != ODAM_CG_BF16 || !a.F_Wt || !a.F_C) return false;
    if (a.Cout != 64 && a.Cout != 128 && a.Cout != 256) return false;
    if (a.F_ldc != 4 * a.Cout || a.KH * a.KW != 9 || a.Cin != a.Cout || !a.k_order || a.dil != 1) return false;
    if (!fits31((long)a.M * a.F_ldc * 2)) return false;
    if (a.G_Wt) {
        if (sw.fuse_bf16 < 2 || !a.G_C) return false;
        const bool built = (a.Cout == 64 && (a.G_N == 64 || a.G_N == 128)) || (a.Cout == 128 && a.G_N == 128);
        if (!built) return false;
    }
    return ring_eligible(a, sw, a.Cout);
}

// the stem with the max-pool on the tile: what it takes to run `a` (pool fields set) on the sixteen-wave 512 x 64 tiles -- the
// 16x16x32 split loop or the bf16 one -- the kernels that have the pooling epilogue
bool pooled_stem_ok(const ConvGemmArgs& a, const Switches& sw) {
    if (!sw.ring || !(sw.tiles & 8) || sw.stem_pool == 0) return false;
    if (is_bf16(a)) {       // the sixteen-wave bf16 tiles take conv1 as a row convolution (pixel stride < row length), not a 3x3 stride 1
        if (!(a.lda > 0 && a.lda < a.Cin) && sw.ring < 2) return false;
        if (is_3x3_stride1(a) || a.out_f32) return false;
    } else if (ring_mode_f32(a, sw) != 4) {
        return false;
    }
    if (a.Cout != 64 || a.ldc != 64 || a.res || !a.relu) return false;
    if (a.pool_ph != POOL_PH || a.pool_pw != POOL_PW) return false;
    if (a.Hp != (a.Ho + 2 - 3) / 2 + 1 || a.Wp != (a.Wo + 2 - 3) / 2 + 1) return false;
    return ring_eligible(a, sw, 64) && fills_512_row_tiles(a, sw);
}

// activations as one bf16 plane (a_bf16): the sixteen-wave 512 x 64 tile of the 16x16x32 split loop, nothing else -- pre-split filters, 32 k
// (one 64-byte row) inside one tap, every row's first pixel on a 16-byte boundary (pixel pitch x stride, row pitch and image size in
// bytes), a device-filling problem; with `pool` set, whatever the pooled stem asks as well
bool bf16_plane_ok(const ConvGemmArgs& a, const Switches& sw) {
    if (is_bf16(a) || !sw.ring || !(sw.tiles & 8) || ring_mode_f32(a, sw) != 4) return false;
    if (a.Cout <= 32 || a.Cout > 64 || a.Cin % 32 != 0 || a.res) return false;
    const long lda = a.lda > 0 ? a.lda : a.Cin;
    if ((lda * a.stride * 2) % 16 != 0 || (lda * a.W * 2) % 16 != 0 || (lda * a.pad * 2) % 16 != 0) return false;
    if (a.pool && !pooled_stem_ok(a, sw)) return false;
    return ring_eligible(a, sw, 64) && fills_512_row_tiles(a, sw);
}

bool fused_second_ok(const ConvGemmArgs& a) { return fused_second_ok(a, current_switches()); }
bool bf16_plane_ok(const ConvGemmArgs& a) { return bf16_plane_ok(a, current_switches()); }
bool fused_bf16_ok(const ConvGemmArgs& a) { return fused_bf16_ok(a, current_switches()); }
bool pooled_stem_ok(const ConvGemmArgs& a) { return pooled_stem_ok(a, current_switches()); }
bool presplit_applies(int Cout, int Kpad) { return f32_mode() == 2 && split_planes_fit(Cout, Kpad); }

Choice choose(const ConvGemmArgs& a, const Switches& sw) {
    const bool bf = is_bf16(a);
    const int epc = bf ? 8 : 4, taps = a.KH * a.KW;      // elements per 16-byte chunk; the small tiles' k-tile is eight chunks
    if (a.Kpad % (8 * epc) != 0 || a.Cin < epc || (a.Cin & (a.Cin - 1)) != 0 || a.KW > 7 || taps > 64)
        return refuse("conv_gemm: unsupported shape (Kpad % k-tile, Cin a power of two >= one 16-byte chunk, KW <= 7)");
    if (a.k_order && (a.Cin % (8 * epc) != 0 || taps > 32 || a.Kpad / (8 * epc) >= 2048))
        return refuse("conv_gemm: k_order 1 needs Cin % k-tile == 0, at most 32 taps, fewer than 2048 k-tiles");
    if (a.M <= 0 || a.Cout <= 0) return Choice{};

    // ---- what the caller asked for by name: it runs so, or the call is refused -----------------------------------------------
    if (a.a_bf16) {
        if (!bf16_plane_ok(a, sw)) return refuse("conv_gemm: bf16-plane activations asked for where they do not apply (check bf16_plane_ok)");
        return ring(a, sw, 5, 64, 16);
    }
    if (a.pool) {
        if (!pooled_stem_ok(a, sw)) return refuse("conv_gemm: pooled stem asked for where it does not apply (check pooled_stem_ok)");
        return ring(a, sw, bf ? 0 : 4, 64, 16);
    }
    if (a.F_Wt3) {
        if (!fused_second_ok(a, sw)) return refuse("conv_gemm: fused second layer asked for where it does not apply (check fused_second_ok)");
        Choice c;
        c.family = Family::FusedF32;
        c.bm = 256; c.bn = a.Cout; c.waves = 8; c.chain = a.G_Wt3 ? a.G_N : 0;
        // cg.mfma16 2: the 16x16x32 schedule in the 128-column bottleneck launches too, 3: in the 64-column ones as well
        c.mode = (a.Kpad % 32 == 0 && (sw.mfma16 >= 3 || (sw.mfma16 == 2 && a.Cout == 128))) ? 4 : 3;
        return c;
    }
    if (a.F_Wt) {
        if (!fused_bf16_ok(a, sw)) return refuse("conv_gemm: fused bf16 bottleneck asked for where it does not apply (check fused_bf16_ok)");
        Choice c;
        c.family = Family::FusedBF16;
        c.bf16 = true;
        c.bm = 256; c.bn = a.Cout; c.waves = 8; c.chain = a.G_Wt ? a.G_N : 0;
        c.s1_window = sw.s1;
        return c;
    }

    // ---- plain layers: the ring kernel where the layer fills the device with its tiles (cg.ring 2: wherever it is eligible) ----
    if (sw.ring) {
        const bool x3 = !bf && sw.f32 == 2;
        const int mode = bf ? 0 : ring_mode_f32(a, sw);
        if (a.Cout % 256 == 0 || a.Cout >= 384) {
            if (ring_eligible(a, sw, 256))
                // bf16 plain layers (no window loop): sixteen waves of 64 x 64 (four per SIMD; 128 registers, the epilogue spills):
                // R101 forward 17.19 -> 16.95 ms per 32 frames, the reduce layers of layer3 90 -> 87 us (same box, cg.tiles 15 vs 31)
                return ring(a, sw, mode, 256, (bf && (sw.tiles & 16) && !is_3x3_stride1(a)) ? 16 : 8);
            // too few 256-wide tiles to fill the device (the encoder's N = 256 layers at M = 27,200: 107) but enough 128-wide
            // ones: the ring kernel on 256 x 128 tiles instead of the 128 x 128 tiles of the fp32 matrix instruction
            if (mode >= 3 && ring_eligible(a, sw, 128)) return ring(a, sw, mode, 128, 8);
        } else if (a.Cout > 64 && (sw.ring >= 2 || x3) && ring_eligible(a, sw, 128)) {   // bf16 / fp32: measured slower than the 128x128 tiles (tests only)
            return ring(a, sw, mode, 128, 8);
        } else if (x3 && a.Cout > 32 && a.Cout <= 64 && ring_eligible(a, sw, 64)) {
            // Sixteen waves on 512 x 64 tiles (cg.tiles bit 3): the 64-column loop uses ~105 registers, so FOUR waves fit a SIMD, and a
            // wave of this loop spends more time issuing (5 DMAs of ~150 cycles, two 44-instruction splits, 28 LDS reads per 768
            // cycles of matrix work) than the pipe needs -- with four per SIMD the pipe finds a ready wave more often, and the
            // filter tile is fetched once per 512 rows.  conv1: 1.44 -> 1.15 ms per 32 frames (same box, A/B by config).
            // (128-row tiles with two 4-wave workgroups per CU = the same two waves per SIMD: measured no change, not kept.)
            return ring(a, sw, mode, 64, (mode == 4 && (sw.tiles & 8) && fills_512_row_tiles(a, sw)) ? 16 : 8);
        } else if (bf && (sw.ring >= 2 || (a.lda > 0 && a.lda < a.Cin)) && a.Cout > 32 && a.Cout <= 64 && ring_eligible(a, sw, 64)) {
            // conv1 as a row convolution (pixel stride < row length); tests: layer1's 3x3 alone
            return ring(a, sw, mode, 64, ((sw.tiles & 8) && !is_3x3_stride1(a) && fills_512_row_tiles(a, sw)) ? 16 : 8);
        }
    }

    // ---- everything else: the small tiles (cg.tiles: the 8-wave forms, +2-3 %; cg.force, tests: pin one tile shape) ----------
    if (sw.force == 1) return small_tiles(a, sw, 128, 64, 8);
    if (sw.force == 2) return small_tiles(a, sw, 64, 64, 4, true);
    if (sw.force == 3) return small_tiles(a, sw, 128, 128, 4);
    if (a.Cout <= 64) return small_tiles(a, sw, 128, 64, (sw.tiles & 2) ? 8 : 4);
    const long tiles128 = (long)((a.M + 127) / 128) * ((a.Cout + 127) / 128);
    if (tiles128 < 128) return small_tiles(a, sw, 64, 64, 4, (sw.tiles & 4) != 0);
    return small_tiles(a, sw, 128, 128, (sw.tiles & 1) ? 8 : 4);
}

void choice_token(const Choice& c, char* tok) {
    const int n = PATH_TOKEN_LEN;
    tok[0] = 0;
    switch (c.family) {
    case Family::Small:
        std::snprintf(tok, n, "%s.small.%dx%d.w%d%s%s%s", c.bf16 ? "bf16" : "f32", c.bm, c.bn, c.waves, c.ut ? ".ut" : "", c.x3 ? ".x3" : "",
                      c.stages == 4 ? ".s4" : "");
        break;
    case Family::RingF32: std::snprintf(tok, n, "f32.ring.m%d.%dx%d%s", c.mode, c.bm, c.bn, c.pool ? ".pool" : ""); break;
    case Family::RingBF16: std::snprintf(tok, n, "bf16.ring.%dx%d%s", c.bm, c.bn, c.pool ? ".pool" : ""); break;
    case Family::FusedF32:
        std::snprintf(tok, n, "f32.fused.m%d.%s", c.mode, c.bn == 128 ? "l2" : !c.chain ? "l1" : c.chain == 128 ? "chain128" : "chain64");
        break;
    case Family::FusedBF16:
        if (c.chain) std::snprintf(tok, n, "bf16.fused.p%d.chain%d", c.bn, c.chain);
        else std::snprintf(tok, n, "bf16.fused.p%d", c.bn);
        break;
    case Family::Refused:
    case Family::Nothing: break;
    }
}

}  // namespace odam_cg
