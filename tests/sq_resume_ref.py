"""The super-quadric fit restated as an explicit step loop, so that a fit can stop, hand its state over, change its views and go on.

One step = the CPU oracle's loss and gradient (oracle/sq_oracle.c: oracle_sq_loss_grad, through conftest.Oracle.loss_grad) + float32
Adam with the bias-correction table odam_sq_create uploads (row t - 1 for the t-th step of the fit: -lr / bc1 for the seven pose /
scale parameters, -lr / bc1 for the two shape logits, sqrt(bc2); float64 scalars rounded once).  The moments, the scales the prior is
measured from and the step count are plain variables of a `Fit`.

tests/test_sq_resume_host.py holds this loop to oracle_sq_fit bit for bit on uninterrupted fits before anything is compared with it;
after that it is the reference of tests/test_sq_resume_gpu.py for what no uninterrupted fit can say: a fit whose view set grows between
launches, and the role of the carried scales_init.  It is not a copy of the kernel: nothing here knows about workgroups, view splits
or launch shapes.
"""
import math

import numpy as np

from dq_ref import fma32

f32 = np.float32
REP = {"super_quadric": 0, "cube": 1, "quadric": 2}
STATE_FLOATS = 32


def adam_table(max_iters):
    """[max_iters, 3] float32: the rows of odam_sq_create (torch/optim/adam.py _single_tensor_adam: float64 scalars)"""
    tab = np.zeros((max_iters, 3), np.float32)
    for t in range(1, max_iters + 1):
        bc1 = 1.0 - math.pow(0.9, float(t))
        bc2 = 1.0 - math.pow(0.999, float(t))
        tab[t - 1] = (f32(-(0.01 / bc1)), f32(-(0.1 / bc1)), f32(math.pow(bc2, 0.5)))
    return tab


class Fit:
    """state of one object's fit"""

    def __init__(self, p0, representation="super_quadric"):
        self.rep = representation
        self.p = np.array(p0, np.float32).reshape(9).copy()
        self.m = np.zeros(9, np.float32)
        self.v = np.zeros(9, np.float32)
        self.s0 = self.p[4:7].copy()        # scales_init (sq_libs.py:454,465): fixed at the first step of the fit, whatever follows
        self.t = 0                          # steps taken

    def copy(self):
        c = Fit(self.p, self.rep)
        c.m, c.v, c.s0, c.t = self.m.copy(), self.v.copy(), self.s0.copy(), self.t
        return c

    def row(self):
        """the state row of include/odam_sq.h"""
        r = np.zeros(STATE_FLOATS, np.float32)
        r[0:9], r[9:18], r[18:27], r[27:30], r[30], r[31] = self.p, self.m, self.v, self.s0, self.t, REP[self.rep]
        return r

    @staticmethod
    def from_row(r):
        r = np.asarray(r, np.float32)
        c = Fit(r[0:9], {v: k for k, v in REP.items()}[int(r[31])])
        c.m, c.v, c.s0, c.t = r[9:18].copy(), r[18:27].copy(), r[27:30].copy(), int(r[30])
        return c


def adam_step(fit, g, tab_row, n_opt):
    """torch.optim.Adam's single-tensor step in float32 on the first n_opt parameters (lerp_ and addcmul_ fused, as the torch CPU kernels)"""
    w1, w2, b2 = f32(1.0 - 0.9), f32(1.0 - 0.999), f32(0.999)
    k = slice(0, n_opt)
    gk = np.asarray(g, np.float32)[k]
    fit.m[k] = fma32(w1, gk - fit.m[k], fit.m[k])
    fit.v[k] = fma32(w2 * gk, gk, fit.v[k] * b2)
    denom = np.sqrt(fit.v[k]) / tab_row[2] + f32(1e-8)
    neg_step = np.where(np.arange(n_opt) < 7, tab_row[0], tab_row[1]).astype(np.float32)
    fit.p[k] = fit.p[k] + (neg_step * fit.m[k]) / denom


def run(oracle, fit, P, tgt, mask, cls, n_iters, table):
    """n_iters more steps of `fit` (in place) on the given views; cls < 0 / None: no prior.  -> (traj [n_iters, 9], loss_2d [n_iters])"""
    n_opt = 9 if fit.rep == "super_quadric" else 7
    traj = np.zeros((n_iters, 9), np.float32)
    loss = np.zeros(n_iters, np.float32)
    if fit.t + n_iters > len(table):
        raise ValueError(f"{fit.t} + {n_iters} steps > {len(table)} rows of the table")
    with np.errstate(all="ignore"):
        for i in range(n_iters):
            l2d, _, g, _, _ = oracle.loss_grad(fit.p, P, tgt, mask, cls if cls is not None else -1, fit.s0, optimise_shapes=int(n_opt == 9))
            adam_step(fit, g, table[fit.t], n_opt)
            fit.t += 1
            traj[i] = fit.p
            loss[i] = l2d
    return traj, loss
