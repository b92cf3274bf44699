"""``tests/fake_dxmat_ogden.py`` for plane-strain Ogden hyperelasticity (DXM_LAW_OGDEN_PE): widths 5 / 25 / 4, one state field
``PK2Stress`` that every update writes and none reads, the parameter validation of law 7 and the refusals of ``csrc/dxmat.hip`` with
this law's sentences, the arithmetic done by ``ogden_plane_ref.restricted_closed_form`` (the definition of the law).  TEST
INFRASTRUCTURE ONLY, like the class it wraps."""
import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import _addr, _rows
from fake_dxmat_ogden import FakeDxmatOgden
from ogden_plane_ref import restricted_closed_form

SET_REFUSAL = ("the plane-strain Ogden tangent dP/dF is a 5x5 block of 25 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is available, "
               "no packed record (sym / coef / pack4) exists for this law")
NO_DISPLACEMENT = ("plane-strain Ogden hyperelasticity takes the 5-wide deformation gradient [F00, F11, F22, F01, F10]: the mesh gradient "
                   "kernels produce the 9-wide F, so the displacement forms (dxm_integrate_displacement*) and the fused displacement "
                   "gradient are not served; pass the 5-wide F [1 + H00, 1 + H11, 1, H01, H10] of the displacement gradient H as an array")


class FakeDxmatOgdenPlane(FakeDxmatOgden):
    """Law 7 of the parent class with the widths (NG, NCT, NS) and the arithmetic swapped for law 38's."""
    FIELDS = (("PK2Stress", 4),)
    LAW, NG, NCT, NS = _lib.LAW_OGDEN_PE, 5, 25, 4

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != self.LAW:
            return super().dxm_create(law, params, nparams, npoints, device)
        h = super().dxm_create(_lib.LAW_OGDEN, params, nparams, npoints, device)   # law 7's parameter checks
        if h is None:
            return None
        m = self._handles[h]
        m.law = law
        n = int(npoints)
        m.state = [dict(PK2Stress=np.zeros((n, self.NS))), dict(PK2Stress=np.zeros((n, self.NS)))]
        return h

    def _plane(self, h):
        return self._h(h).law == self.LAW

    def dxm_set_tangent_layout(self, h, layout):
        if self._plane(h) and layout != 0:
            return self._fail(-1, SET_REFUSAL)
        return super().dxm_set_tangent_layout(h, layout)

    def dxm_tangent_size(self, h):
        return self.NCT if self._plane(h) else super().dxm_tangent_size(h)

    def dxm_integrate_displacement(self, h, mesh, u, dt, flux, isv, ct, stats):
        if self._plane(h):
            return self._fail(-1, NO_DISPLACEMENT)
        return super().dxm_integrate_displacement(h, mesh, u, dt, flux, isv, ct, stats)

    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if m.law != self.LAW:
            return super().dxm_set_state(h, which, field, host)
        if field != 0:
            return self._fail(-1, "state field out of range")
        m.materialize_s1()
        m.state_of(which)["PK2Stress"][...] = _rows(host, m.n, self.NS)
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if m.law != self.LAW:
            return super().dxm_get_state(h, which, field, host)
        if field != 0:
            return self._fail(-1, "state field out of range")
        if m.n:
            _rows(host, m.n, self.NS)[...] = m.state_of(which)["PK2Stress"]
        return 0

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.law != self.LAW:
            return super().dxm_isv_host(h, which, host)
        if m.n:
            _rows(host, m.n, self.NS)[...] = m.state_of(which)["PK2Stress"]
        return 0

    def dxm_get_io(self, h, which, kind, host):
        m = self._h(h)
        if m.law != self.LAW:
            return super().dxm_get_io(h, which, kind, host)
        if not m.io_mask(which) & (1 << kind):
            return self._fail(-1, f"the {'flux' if kind else 'gradient'} of that state is not held on the device")
        first = which == _lib.S0 or m.s1_alias
        self.downloads.append((which, kind))
        if m.n:
            _rows(host, m.n, self.NG)[...] = m.io[0 if first else 1]["flux" if kind else "grad"]
        return 0

    def _update(self, m, grad):
        if m.law != self.LAW:
            return super()._update(m, grad)
        m.io_valid[1] = 0
        P, A, isv = restricted_closed_form(grad, *m.params)
        m.state[1] = dict(PK2Stress=isv.copy())
        m.s1_alias = False
        m.launched = True
        nan = int(np.isnan(P).any(axis=1).sum())
        m.stats = dict(n_points=m.n, n_plastic=0, n_not_converged=0, n_nan=nan, max_local_iters=0)
        return dict(sig=P, Ct=A, n_plastic=0, n_not_converged=0)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.law != self.LAW:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, self.NG)
        r = self._update(m, g)
        if _addr(flux):
            _rows(flux, m.n, self.NG)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, self.NCT)[...] = r["Ct"].reshape(m.n, self.NCT)
        if _addr(isv):
            _rows(isv, m.n, self.NS)[...] = m.state[1]["PK2Stress"]
        return self._finish(m, g, r, stats)
