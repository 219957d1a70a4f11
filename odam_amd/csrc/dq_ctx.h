// dq_ctx.h -- what the dual-quadric fit (dq_fit.hip) keeps in an odam_sq_ctx (defined in sq_fit.hip, which frees it).
#pragma once

struct odam_sq_ctx;

struct odam_dq_state {
    float* d_adam = nullptr;   // [iters][2]: -(lr / bias_correction1), sqrt(bias_correction2) per step; grow-only
    int adam_iters = 0;
    int group_waves = 4;       // objects (wavefronts) per workgroup: a scheduling choice, no result depends on it
};

odam_dq_state* odam_sq_ctx_dq(odam_sq_ctx* ctx);
