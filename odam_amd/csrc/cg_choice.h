// cg_choice.h -- which kernel a contraction runs on: the policy of launch_conv_gemm (conv_gemm.h), stated once as a pure function of
// the call's integers and a snapshot of the switches.  Plain C++17 without HIP: tests/test_cg_choice_host.py runs choose() on the host
// over a table of shapes and switch settings (tests/golden/cg_choice.npz).  launch_conv_gemm asks choose() and launches what it
// names; the predicates a caller consults before it builds a fused or pooled call are built from the same pieces (cg_choice.hip).
#pragma once
#include "cg_args.h"

namespace odam_cg {

// the cg.* and stem.pool switches (odam_config.h) a choice depends on, read once per call by current_switches()
struct Switches {
    int ring, f32, fuse, fuse_bf16, s1, ut, tiles, force, presplit, mfma16, pin, small_x3, stem_pool;
};
Switches current_switches();

enum class Family { Refused, Nothing, Small, RingF32, RingBF16, FusedF32, FusedBF16 };

struct Choice {
    Family family = Family::Nothing;      // Nothing: an empty problem, no launch and no token
    bool bf16 = false;                    // operand type of the kernel (ConvGemmArgs::dtype)
    int bm = 0, bn = 0, waves = 0;        // tile rows x columns and wavefronts per workgroup (fused: bn = the 3x3's channels, 256 rows, 8 waves)
    int stages = 2;                       // Small: LDS stages (4 = the deep LDS-DMA pipeline)
    bool ut = false, x3 = false;          // Small: uniform-tap LDS-DMA gather; fp32 products through the exact bf16 split
    int mode = 0;                         // RingF32 / FusedF32: 2 split in registers, 3 pre-split filters on 32x32x16, 4 pre-split on 16x16x32,
                                          // 5 = 4 with the activations as one bf16 plane in memory (ConvGemmArgs::a_bf16)
    bool pool = false;                    // ring kernels: the stem's max-pool on the tile
    int chain = 0;                        // fused: output channels of the next block's reduce riding along (0: none)
    int s1_window = 0;                    // ConvGemmArgs::s1_window of the launch
    int code = 0;                         // Refused: what launch_conv_gemm returns, and its error text
    const char* message = nullptr;
};

Choice choose(const ConvGemmArgs& a, const Switches& sw);

// the token of a choice (include/odam_detr.h odam_op_conv_paths) into tok[PATH_TOKEN_LEN]; "" for Refused / Nothing
constexpr int PATH_TOKEN_LEN = 40;
void choice_token(const Choice& c, char* tok);

// what a caller asks before it sets the F_* / G_* or pool fields: whether launch_conv_gemm would run `a` so -- exactly the test
// choose() makes before it refuses.  The one-argument forms answer for the switches in force right now.
bool fused_second_ok(const ConvGemmArgs& a, const Switches& sw);      // fp32 split mode: 3x3 + expand (+ next reduce) as one launch (cg.fuse)
bool fused_bf16_ok(const ConvGemmArgs& a, const Switches& sw);        // bf16: the same with F_Wt [+ G_Wt] (cg.fuse_bf16)
bool pooled_stem_ok(const ConvGemmArgs& a, const Switches& sw);       // the stem with the max-pool on the tile (stem.pool)
bool bf16_plane_ok(const ConvGemmArgs& a, const Switches& sw);        // fp32 layer on activations stored as one bf16 plane (a_bf16; with pool: and pooled)
bool bf16_plane_ok(const ConvGemmArgs& a);
bool fused_second_ok(const ConvGemmArgs& a);
bool fused_bf16_ok(const ConvGemmArgs& a);
bool pooled_stem_ok(const ConvGemmArgs& a);
// whether fp32 layers of Cout x Kpad filters take them pre-split right now (ConvGemmArgs::Wt3, split3_filters)
bool presplit_applies(int Cout, int Kpad);

// experiments / tests: 0 = never use the 256-row ring kernel, 1 = when the problem is large enough (default), 2 = whenever the
// layer is eligible (any size).  = odam_config.h cg.ring.
void set_big_mode(int mode);
// fp32 layers: 0 = v_mfma_f32_32x32x2_f32 on 128x128 tiles, 2 (default) = products on the bf16 matrix instruction through an exact
// three-way bf16 split of both operands (six MFMAs per 16 k; fp32-class accuracy, different last bits).  = odam_config.h cg.f32.
void set_f32_mode(int mode);
// the mode fp32 layers run in right now (0 when the ring kernel is switched off altogether)
int f32_mode();

}  // namespace odam_cg
