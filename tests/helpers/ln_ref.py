"""The float64 LayerNorm reference and its bounds, shared by tests/test_norm_glue.py (gcl_layernorm_fwd / _bwd) and
tests/test_region_glue_kernels.py (gcl_cross_update_fwd, the same normalisation)."""
import torch.nn.functional as Fn

from layouts import U, within

EPS = 1e-5


class LNRef:
    """float64 LayerNorm of fp32 inputs (autograd for the backward) and the bounds the kernels are held to."""

    def __init__(self, x, gm, bt, dy):
        F = x.shape[1]
        x64 = x.double().requires_grad_()
        g64, b64 = gm.double().requires_grad_(), bt.double().requires_grad_()
        self.y = Fn.layer_norm(x64, (F,), g64, b64, EPS)
        self.dy = dy.double()
        self.y.backward(self.dy)
        self.y = self.y.detach()
        self.dx, self.dg, self.db = x64.grad, g64.grad, b64.grad
        xd = x.double()
        self.mean = xd.mean(1)
        self.rstd = (xd.var(1, unbiased=False) + EPS).rsqrt()
        self.xhat = (xd - self.mean[:, None]) * self.rstd[:, None]
        self.mabs = xd.abs().mean(1)
        kappa = self.mean.abs() * self.rstd  # condition of the row: rounding of the mean, relative to the std
        # the variance sees the mean's rounding (U |mean|) once per deviation: the compiler may fuse the mean's multiply
        # into some of the subtractions x - mean and not into others, which centres them differently
        self.tol_rstd = self.rstd * (64 * U + 2 * U * kappa + (16 * U * (kappa + 1)) ** 2)
        hmax = self.xhat.abs().amax(1)
        q = (self.dy * gm.double()).abs().amax(1)
        self.tol_y = (32 * U * (kappa + 1 + hmax) * gm.abs().max() + 2 * U * bt.abs().max())[:, None]
        self.tol_dx = (32 * U * (kappa + 4) * (1 + hmax) * self.rstd * q)[:, None]
        ady = self.dy.abs()
        self.tol_dg = 1e-5 * (ady * self.xhat.abs()).sum(0) + 32 * U * (ady * (kappa + 1)[:, None]).sum(0)
        self.tol_db = 1e-5 * ady.sum(0)
        self.tol_cs = 1e-5 * self.dx.abs().sum(0) + self.tol_dx.sum()

    def check_fwd(self, y, stats, what):
        within(y, self.y, self.tol_y, f"{what}: y")
        within(stats[:, 0], self.mean, 32 * U * self.mabs, f"{what}: mean")
        within(stats[:, 1], self.rstd, self.tol_rstd, f"{what}: rstd")

    def check_bwd(self, dx, dg, db, cs, what):
        within(dx, self.dx, self.tol_dx, f"{what}: dx")
        within(dg, self.dg, self.tol_dg, f"{what}: dgamma")
        within(db, self.db, self.tol_db, f"{what}: dbeta")
        if cs is not None:
            within(cs, self.dx.sum(0), self.tol_cs, f"{what}: colsum(dx) vs float64")
            dxk = dx.double()
            within(cs, dxk.sum(0), 1e-5 * dxk.abs().sum(0), f"{what}: colsum(dx) vs the kernel's own dx")
