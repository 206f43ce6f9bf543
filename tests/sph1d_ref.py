"""Test-only numpy restatement of the 1-D SPH step that dmcf_sph1d_rollout implements (include/dmcf_hip.h; the reference's
SPH1D.step, datasets/column_gen.py:159-186), with the precision the reference's numpy gives each operation: float32 state,
distances and spline values; float64 products with masses / densities / pressures and float64 sums over j; updates rounded to
float32 once.  Written from the formulas, one [n, n] pair matrix per pass; the product never imports this."""
import numpy as np

F32 = np.float32


def spline(q, c43):
    """W(q), q = |x_i - x_j| >= 0 (the raw distance), float32 in and out."""
    inner = F32(6) * (q ** 3 - q * q) + F32(1)
    outer = F32(2) * (F32(1) - q) ** 3
    return c43 * np.where(q <= 1, np.where(q <= F32(0.5), inner, outer), F32(0))


def spline_grad(d, c43):
    """W'(d), d = x_i - x_j signed, float32 in and out (two branches)."""
    a, sg = np.abs(d), np.sign(d)
    inner = F32(18) * sg * (d * d) - F32(12) * d
    t = F32(1) - a
    outer = F32(-6) * sg * (t * t)
    return c43 * np.where(a <= 1, np.where(a <= F32(0.5), inner, outer), F32(0))


class Solver:
    def __init__(self, h, rest_dens, stiffness, visc, gravity, dt, eps=0.01, max_iter=10000, bcnt=2):
        self.rest, self.stiffness, self.visc, self.gravity = float(rest_dens), float(stiffness), float(visc), float(gravity)
        self.dt, self.eps, self.max_iter, self.bcnt = float(dt), float(eps), int(max_iter), int(bcnt)
        self.c43, self.soft = F32(4 / (3 * h)), F32(0.01 * h ** 2)

    def density(self, x, m):
        q = np.abs(x[:, None] - x[None, :])
        return (m.astype(np.float64)[None, :] * spline(q, self.c43).astype(np.float64)).sum(axis=1)

    def step(self, p):
        """One step on ``p`` [n, 3] float32 = (x, v, m), boundary first, in place -> the number of pressure iterations."""
        b, dt = self.bcnt, self.dt
        x, v, m = p[:, 0], p[:, 1], p[:, 2]
        m64 = m.astype(np.float64)
        # viscosity, then the advance
        dens = self.density(x, m)
        d = x[:, None] - x[None, :]
        dv = v[:, None] - v[None, :]
        w = (m64 / dens)[None, :] * dv.astype(np.float64) * d.astype(np.float64) * spline_grad(d, self.c43).astype(np.float64)
        w /= (d * d + self.soft).astype(np.float64)
        f_visc = self.visc * (2.0 * w.sum(axis=1))
        v[b:] = (v[b:].astype(np.float64) + dt * (self.gravity + f_visc[b:])).astype(F32)
        x[b:] = x[b:] + F32(dt) * v[b:]
        for it in range(1, self.max_iter + 1):
            dens = self.density(x, m)
            pres = np.maximum(self.stiffness * ((dens / self.rest) ** 7 - 1.0), 0.0)
            pres[:b] = pres[b]
            err = np.maximum(dens - self.rest, 0.0)[b:].max()
            a = pres / (dens * dens)
            g = spline_grad(x[:, None] - x[None, :], self.c43).astype(np.float64)
            s = (m64[None, :] * (a[:, None] + a[None, :]) * g).sum(axis=1)
            f = (-(m64 / dens) * (dens * s))[b:]
            v[b:] = (v[b:].astype(np.float64) + dt * f / m64[b:]).astype(F32)
            x[b:] = (x[b:].astype(np.float64) + dt * dt * f / m64[b:]).astype(F32)
            if err < self.eps:
                break
        return it


def rollout(state, frames, **constants):
    """-> (sequence [frames, n, 2] float32 recorded before each step, final state [n, 3], iterations [frames] int32)."""
    s = Solver(**constants)
    p = np.array(state, dtype=F32)
    seq = np.empty((frames, len(p), 2), F32)
    iters = np.empty(frames, np.int32)
    for t in range(frames):
        seq[t] = p[:, :2]
        iters[t] = s.step(p)
    return seq, p, iters
