"""NumPy restatement of primal-dual total variation (include/pdeip.h, csrc/pdeip_tvpd.hip): the recurrence of the header in float32,
operation for operation, so that the device result equals it bit for bit.  Two statements: whole-array (`step`) and a per-pixel loop
(`step_loops`), held equal by tests/test_tvpd_ref.py.  Planes are [rows, cols(, frames)]; i runs down a column."""
import numpy as np

import edt_ref

F32 = np.float32
L1, L2 = 0, 1
MODELS = {"l1": L1, "l2": L2}
TAU, SIGMA = 0.25, 0.5


class Consts:
    """The call's constants, each formed once in float32 as the host does."""

    def __init__(self, model, lam, huber=0.0, tau=None, sigma=None):
        self.model = MODELS.get(model, model)
        assert self.model in (L1, L2)
        self.tau = F32(TAU if tau is None else tau)
        self.sigma = F32(SIGMA if sigma is None else sigma)
        self.tl = F32(self.tau * F32(lam))
        self.onep_tl = F32(F32(1.0) + self.tl)
        self.huber = bool(F32(huber) > 0)
        self.hub_den = F32(F32(1.0) + F32(self.sigma * F32(huber)))


def start(f, u0=None):
    """The start: u0, or f with its NaNs replaced by the nearest known pixel of the frame (all-NaN frames stay NaN)."""
    if u0 is not None:
        return np.array(u0, dtype=F32, order="F")
    return np.array(edt_ref.nearest_fill(np.asarray(f, F32), 0)[0], dtype=F32, order="F")


def step(u, up, px, py, f, c):
    """One iteration on a plane [rows, cols], whole-array.  -> u', u_prev', px', py'."""
    with np.errstate(all="ignore"):
        ub = (u + u) - up
        gx, gy = np.zeros_like(u), np.zeros_like(u)
        gx[:-1, :] = ub[1:, :] - ub[:-1, :]
        gy[:, :-1] = ub[:, 1:] - ub[:, :-1]
        qx, qy = px + c.sigma * gx, py + c.sigma * gy
        if c.huber:
            qx, qy = qx / c.hub_den, qy / c.hub_den
        s = np.sqrt(qx * qx + qy * qy)
        n = np.where(s > 1, s, F32(1.0))
        pxn, pyn = qx / n, qy / n
        dx, dy = pxn.copy(), pyn.copy()
        dx[1:, :] = pxn[1:, :] - pxn[:-1, :]
        dy[:, 1:] = pyn[:, 1:] - pyn[:, :-1]
        v = u + c.tau * (dx + dy)
        if c.model == L2:
            un = (v + c.tl * f) / c.onep_tl
        else:
            r = v - f
            un = np.where(r > c.tl, v - c.tl, np.where(r < -c.tl, v + c.tl, f))
        un = np.where(np.isnan(f), v, un)
    for a in (un, pxn, pyn):
        assert a.dtype == F32
    return un, u, pxn, pyn


def _dual_pixel(ub, px, py, i, j, c):
    rows, cols = ub.shape
    gx = ub[i + 1, j] - ub[i, j] if i + 1 < rows else F32(0.0)
    gy = ub[i, j + 1] - ub[i, j] if j + 1 < cols else F32(0.0)
    qx, qy = px[i, j] + c.sigma * gx, py[i, j] + c.sigma * gy
    if c.huber:
        qx, qy = qx / c.hub_den, qy / c.hub_den
    s = np.sqrt(qx * qx + qy * qy)
    n = s if s > 1 else F32(1.0)
    return qx / n, qy / n


def step_loops(u, up, px, py, f, c):
    """The same iteration, one pixel at a time, every neighbour's p' recomputed as k_tvpd_step does."""
    rows, cols = u.shape
    un, pxn, pyn = (np.zeros_like(u) for _ in range(3))
    with np.errstate(all="ignore"):
        ub = (u + u) - up
        for j in range(cols):
            for i in range(rows):
                qx, qy = _dual_pixel(ub, px, py, i, j, c)
                dx = qx - _dual_pixel(ub, px, py, i - 1, j, c)[0] if i > 0 else qx
                dy = qy - _dual_pixel(ub, px, py, i, j - 1, c)[1] if j > 0 else qy
                v = u[i, j] + c.tau * (dx + dy)
                fv = f[i, j]
                if np.isnan(fv):
                    w = v
                elif c.model == L2:
                    w = (v + c.tl * fv) / c.onep_tl
                else:
                    r = v - fv
                    w = v - c.tl if r > c.tl else (v + c.tl if r < -c.tl else fv)
                un[i, j], pxn[i, j], pyn[i, j] = w, qx, qy
    return un, u, pxn, pyn


def iterate(f, u0, c, iters, stepper=step):
    """The state (u, u_prev, px, py) of one plane after `iters` iterations from the start u0."""
    f = np.asarray(f, F32)
    u = np.array(u0, dtype=F32)
    state = (u, u.copy(), np.zeros_like(u), np.zeros_like(u))
    for _ in range(int(iters)):
        state = stepper(*state, f, c)
    return state


def tv_pd(f, model, lam, iter, huber=0.0, u0=None, tau=None, sigma=None):
    """pdeip_tv_pd: -> u [rows, cols(, frames)] float32, column-major."""
    f = np.asarray(f, F32)
    c = Consts(model, lam, huber, tau, sigma)
    s = start(f, u0)
    if f.ndim == 2:
        return np.asfortranarray(iterate(f, s, c, iter)[0])
    return np.asfortranarray(np.stack([iterate(f[:, :, k], s[:, :, k], c, iter)[0] for k in range(f.shape[2])], axis=2))
