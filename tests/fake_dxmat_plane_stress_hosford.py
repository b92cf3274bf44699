"""``tests/fake_dxmat_plane_stress.py`` for plane-stress Hosford plasticity (DXM_LAW_PS_HOSFORD = 33): the same hidden ``PlasticStrain``
state field 0, 9-wide tangent and Newton controls, what ``build_ps_hosford`` refuses, the arithmetic done by
``plane_stress_hosford_ref``.  TEST INFRASTRUCTURE ONLY: it lets the Python layer above the C ABI run without a GPU."""
import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import _Handle
from fake_dxmat_plane_stress import FakeDxmatPlaneStress
import fake_dxmat_plane_stress as base
import plane_stress_hosford_ref as psh

LAW = _lib.LAW_PS_HOSFORD


def refusal(p):
    """the sentence of ``build_ps_hosford`` (its distinguishing part); None: accepted"""
    names = ("E", "nu", "sig0", "a", "tangent")
    for k, v in enumerate(p):
        if not np.isfinite(v):
            return f"{names[k]} must be finite"
    if not p[0] > 0:
        return "E must be > 0"
    if not -1 < p[1] < 1:
        return "nu must lie in (-1, 1)"
    if not p[2] > 0:
        return "sig0 must be > 0"
    if not p[3] >= psh.A_MIN:
        return "the exponent a must be >= 2"
    if not p[3] <= psh.A_MAX:
        return "the exponent a must be <= 100"
    if p[4] not in (0.0, 1.0):
        return "tangent must be 0"
    return None


class FakeDxmatPlaneStressHosford(FakeDxmatPlaneStress):
    def dxm_create(self, law, params, nparams, npoints, device):
        if law != LAW:
            return super().dxm_create(law, params, nparams, npoints, device)
        if nparams != 5:
            self._fail(-1, f"law {law} expects 5 parameters, got {nparams}")
            return None
        p = [params[i] for i in range(nparams)]
        why = refusal(p)
        if why:
            self._fail(-1, f"plane-stress Hosford plasticity: {why}")
            return None
        self._next += 8
        h = _Handle(law, p, int(npoints))
        h.state = [{"epsp": np.zeros((int(npoints), 3))} for _ in range(2)]
        h.newton = (25, 1e-14)
        self._handles[self._next] = h
        return self._next

    def dxm_set_params(self, h, params, nparams):
        m = self._h(h)
        if m.law == LAW:
            why = refusal([params[i] for i in range(nparams)])
            if why:
                return self._fail(-1, f"plane-stress Hosford plasticity: {why}")
        return super().dxm_set_params(h, params, nparams)

    def dxm_kernel_name(self, h):
        return b"plane_stress_hosford_kernel<0" if self._h(h).law == LAW else super().dxm_kernel_name(h)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        old = base.LAWS
        base.LAWS = old + (LAW,)    # the parent's hot call serves the laws of this tuple through _step
        try:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        finally:
            base.LAWS = old

    def _step(self, m, grad):
        if m.law != LAW:
            return super()._step(m, grad)
        m.io_valid[1] = 0
        r = psh.update(grad, m.state[0]["epsp"], np.array(m.params), *m.newton)
        m.state[1] = {"epsp": r["state"].copy()}
        m.s1_alias, m.launched = False, True
        m.stats = dict(n_points=m.n, **psh.stats(r, m.params[4] != 0))
        return dict(sig=r["stress"], Ct=r["tangent"], n_plastic=m.stats["n_plastic"], n_not_converged=m.stats["n_not_converged"])
