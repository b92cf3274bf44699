"""``tests/fake_dxmat.py`` for the Ogden hyperelastic law (DXM_LAW_OGDEN): widths 9 / 81 / 6, one state field ``PK2Stress`` that
every update writes and none reads, the parameter validation and the two refusals of ``csrc/dxmat.hip`` (packed tangent layouts,
fused displacement gradient), the arithmetic done by ``ogden_ref.closed_form``.  TEST INFRASTRUCTURE ONLY, like the class it wraps."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
from ogden_ref import closed_form


class FakeDxmatOgden(FakeDxmat):
    FIELDS = (("PK2Stress", 6),)

    def __init__(self, real):
        super().__init__(real)
        self.last_params = None

    def _check(self, prm):
        alpha, mu, K = prm
        if not (alpha != 0.0 and np.isfinite(alpha)):
            return self._fail(-1, f"Ogden: alpha must be finite and non-zero, got {alpha:g}")
        if not (mu > 0.0 and np.isfinite(mu)):
            return self._fail(-1, f"Ogden: mu must be finite and > 0, got {mu:g}")
        if not (K > 0.0 and np.isfinite(K)):
            return self._fail(-1, f"Ogden: K must be finite and > 0, got {K:g}")
        return 0

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != _lib.LAW_OGDEN:
            return super().dxm_create(law, params, nparams, npoints, device)
        prm = [params[i] for i in range(nparams)]
        if nparams != 3:
            self._fail(-1, f"law {law} expects 3 parameters, got {nparams}")
            return None
        if self._check(prm):
            return None
        self._next += 8
        h = _Handle(law, prm, int(npoints))
        n = int(npoints)
        h.state = [dict(PK2Stress=np.zeros((n, 6))), dict(PK2Stress=np.zeros((n, 6)))]
        self._handles[self._next] = h
        self.last_params = prm
        return self._next

    def dxm_set_params(self, h, params, nparams):
        prm = [params[i] for i in range(nparams)]
        if self._check(prm):
            return -1
        self.last_params = prm
        return super().dxm_set_params(h, params, nparams)

    def dxm_set_tangent_layout(self, h, layout):
        if layout != 0:
            return self._fail(-1, "the Ogden kernel writes the full 81-entry dP/dF only: no packed tangent record (sym / coef / pack4) exists for this law")
        return super().dxm_set_tangent_layout(h, layout)

    def dxm_tangent_size(self, h):
        return 81

    def dxm_integrate_displacement(self, h, mesh, u, dt, flux, isv, ct, stats):
        return self._fail(-1, "the Ogden kernel has no fused displacement-gradient form: set option fused_gradient to 0 (F is then evaluated "
                              "by the gradient kernel) or pass F as an array")

    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if field != 0:
            return self._fail(-1, "state field out of range")
        m.materialize_s1()
        m.state_of(which)["PK2Stress"][...] = _rows(host, m.n, 6)
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if field != 0:
            return self._fail(-1, "state field out of range")
        if m.n:
            _rows(host, m.n, 6)[...] = m.state_of(which)["PK2Stress"]
        return 0

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.n:
            _rows(host, m.n, 6)[...] = m.state_of(which)["PK2Stress"]
        return 0

    def dxm_get_io(self, h, which, kind, host):
        m = self._h(h)
        if not m.io_mask(which) & (1 << kind):
            return self._fail(-1, f"the {'flux' if kind else 'gradient'} of that state is not held on the device")
        first = which == _lib.S0 or m.s1_alias
        self.downloads.append((which, kind))
        if m.n:
            _rows(host, m.n, 9)[...] = m.io[0 if first else 1]["flux" if kind else "grad"]
        return 0

    def dxm_bind_isv_output(self, h, field, host):
        if field != 0:
            return self._fail(-1, "state field out of range")
        self._h(h).isv_out[field] = _addr(host) or None
        return 0

    def _update(self, m, grad):
        m.io_valid[1] = 0
        P, A, isv = closed_form(grad, *m.params)
        m.state[1] = dict(PK2Stress=isv.copy())
        m.s1_alias = False
        m.launched = True
        nan = int(np.isnan(P).any(axis=1).sum())
        m.stats = dict(n_points=m.n, n_plastic=0, n_not_converged=0, n_nan=nan, max_local_iters=0)
        return dict(sig=P, Ct=A, n_plastic=0, n_not_converged=0)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, 9)
        r = self._update(m, g)
        if _addr(flux):
            _rows(flux, m.n, 9)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 81)[...] = r["Ct"].reshape(m.n, 81)
        if _addr(isv):
            _rows(isv, m.n, 6)[...] = m.state[1]["PK2Stress"]
        return self._finish(m, g, r, stats)

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        g = _rows(grad, m.n, 9)
        r = self._update(m, g)
        top = int(idx.max()) + 1
        _rows(flux_base, top, 9)[idx] = r["sig"]
        _rows(ct_base, top, 81)[idx] = r["Ct"].reshape(m.n, 81)
        return self._finish(m, g, r, stats, idx)
