"""Reference pieces for the far-field tests: a numpy restatement of the characteristic far-field condition (in
fp64) and FarCase, the oracle-composed reference of test_gpu_open_boundaries.OpenCase with far-field faces."""
import numpy as np

from test_gpu_open_boundaries import OpenCase

GAMMA = 1.4
BRANCHES = ("supersonic inflow", "supersonic outflow", "subsonic, inside reference", "subsonic, far-field reference")


def prim(s):
    s = np.asarray(s, np.float64)
    rho = s[:, 0]
    v = s[:, 1:4] / rho[:, None]
    p = (GAMMA - 1) * (s[:, 4] - 0.5 * rho * (v * v).sum(1))
    return rho, v, p


def farfield_outside(sL, n3, far):
    """outside conservative states (fp64) of far-field faces with inside states sL[m, 5], outward unit normals n3[m, 3] and
    far-field states far[m, 5]; and the branch of every face (index into BRANCHES)"""
    sL, n3, far = (np.asarray(a, np.float64) for a in (sL, n3, far))
    ri, vi, pi = prim(sL)
    rf, vf, pf = prim(far)
    ci, cf = np.sqrt(GAMMA * pi / ri), np.sqrt(GAMMA * pf / rf)
    qi, qf = (vi * n3).sum(1), (vf * n3).sum(1)
    rp, rm = qi + 5 * ci, qf - 5 * cf
    qb, cb = 0.5 * (rp + rm), (rp - rm) / 10
    inside_ref = qb > 0
    rr, cr, qr = np.where(inside_ref, ri, rf), np.where(inside_ref, ci, cf), np.where(inside_ref, qi, qf)
    vr = np.where(inside_ref[:, None], vi, vf)
    rb = rr * (cb / cr) ** 5
    pb = rb * cb * cb / GAMMA
    vb = vr + (qb - qr)[:, None] * n3
    built = np.concatenate([rb[:, None], rb[:, None] * vb, (pb / (GAMMA - 1) + 0.5 * rb * (vb * vb).sum(1))[:, None]], 1)
    sup_in, sup_out = qi <= -ci, qi >= ci
    guard = ~sup_in & ~sup_out & ~(cb > 0)
    out = np.where(sup_in[:, None], far, np.where((sup_out | guard)[:, None], sL, built))
    branch = np.where(sup_in, 0, np.where(sup_out | guard, 1, np.where(inside_ref, 2, 3)))
    return out, branch


class FarCase(OpenCase):
    """OpenCase whose open faces may be far-field faces (kinds 10 + k): their outside state from farfield_outside in fp64,
    cast to the dtype. `branches` counts the faces of every branch over all stages run."""

    def __init__(self, part, dtype, state, inflow):
        super().__init__(part, dtype, state, inflow)
        self.branches = np.zeros(4, np.int64)

    def _outside(self, sL):
        sR = sL.copy()
        k = self.open_kind
        inf = (k >= 2) & (k < 10)
        if inf.any():
            sR[inf] = self.inflow[k[inf] - 2]
        far = k >= 10
        if far.any():
            out, br = farfield_outside(sL[far], self.open_n3[far], self.inflow[k[far] - 10])
            sR[far] = out.astype(sL.dtype)
            self.branches += np.bincount(br, minlength=4)
        return sR
