"""``tests/fake_dxmat.py`` for logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_J2): widths 9 / 81 / 7, the state fields
``ElasticStrain`` (written by every update, never read), ``EquivalentPlasticStrain`` and the hidden ``PlasticStrain`` the update is
driven by, the parameter validation and the refusals of ``csrc/dxmat.hip`` (packed tangent layouts, fused displacement gradient),
the arithmetic done by ``log_strain_ref.update``.  TEST INFRASTRUCTURE ONLY, like the class it wraps."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
from log_strain_ref import update


class FakeDxmatLogStrain(FakeDxmat):
    FIELDS = (("ElasticStrain", 6), ("EquivalentPlasticStrain", 1), ("PlasticStrain", 6))

    def __init__(self, real):
        super().__init__(real)
        self.last_params = None
        self.state_sets = []         # (which, field) of every dxm_set_state: what a test looks at

    def _check(self, prm):
        E, nu, s0, H0 = prm
        for name, v in zip(("E", "nu", "s0", "H0"), prm):
            if not np.isfinite(v):
                return self._fail(-1, f"logarithmic-strain plasticity: {name} must be finite, got {v:g}")
        if not (E > 0.0 and -1.0 < nu < 0.5):
            return self._fail(-1, f"invalid elastic constants E={E:g} nu={nu:g}")
        if not s0 > 0.0:
            return self._fail(-1, f"logarithmic-strain plasticity: s0 must be > 0, got {s0:g}")
        if not H0 >= 0.0:
            return self._fail(-1, f"logarithmic-strain plasticity: the hardening slope H0 must be >= 0, got {H0:g}")
        return 0

    @staticmethod
    def _zeros(n):
        return dict(ElasticStrain=np.zeros((n, 6)), EquivalentPlasticStrain=np.zeros((n, 1)), PlasticStrain=np.zeros((n, 6)))

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != _lib.LAW_LOG_STRAIN_J2:
            return super().dxm_create(law, params, nparams, npoints, device)
        prm = [params[i] for i in range(nparams)]
        if nparams != 4:
            self._fail(-1, f"law {law} expects 4 parameters, got {nparams}")
            return None
        if self._check(prm):
            return None
        self._next += 8
        h = _Handle(law, prm, int(npoints))
        h.state = [self._zeros(int(npoints)), self._zeros(int(npoints))]
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
            return self._fail(-1, "the logarithmic-strain plasticity kernel writes the full 81-entry dP/dF only: no packed tangent record "
                                  "(sym / coef / pack4) exists for this law")
        return super().dxm_set_tangent_layout(h, layout)

    def dxm_tangent_size(self, h):
        return 81

    def dxm_integrate_displacement(self, h, mesh, u, dt, flux, isv, ct, stats):
        return self._fail(-1, "the logarithmic-strain plasticity kernel has no fused displacement-gradient form: set option fused_gradient "
                              "to 0 (F is then evaluated by the gradient kernel) or pass F as an array")

    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if not 0 <= field < 3:
            return self._fail(-1, f"law {m.law} has no state field {field}")
        m.materialize_s1()
        name, dim = self.FIELDS[field]
        m.state_of(which)[name][...] = _rows(host, m.n, dim)
        self.state_sets.append((which, field))
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if not 0 <= field < 3:
            return self._fail(-1, f"law {m.law} has no state field {field}")
        name, dim = self.FIELDS[field]
        if m.n:
            _rows(host, m.n, dim)[...] = m.state_of(which)[name]
        return 0

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.n:
            out = _rows(host, m.n, 7)
            st = m.state_of(which)
            out[:, :6], out[:, 6:] = st["ElasticStrain"], st["EquivalentPlasticStrain"]
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
        if not 0 <= field < 2:
            return self._fail(-1, "state field out of range")
        self._h(h).isv_out[field] = _addr(host) or None
        return 0

    def _update(self, m, grad):
        m.io_valid[1] = 0
        s0 = m.state[0]
        r = update(grad, s0["PlasticStrain"], s0["EquivalentPlasticStrain"][:, 0], *m.params)
        m.state[1] = dict(ElasticStrain=r["eel"].copy(), EquivalentPlasticStrain=r["p"].reshape(-1, 1).copy(), PlasticStrain=r["Ep"].copy())
        m.s1_alias = False
        m.launched = True
        nan = int(np.isnan(r["P"]).any(axis=1).sum())
        m.stats = dict(n_points=m.n, n_plastic=int(r["plastic"].sum()), n_not_converged=0, n_nan=nan, max_local_iters=0)
        return dict(sig=r["P"], Ct=r["A"], n_plastic=m.stats["n_plastic"], n_not_converged=0)

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
            out = _rows(isv, m.n, 7)
            out[:, :6], out[:, 6:] = m.state[1]["ElasticStrain"], m.state[1]["EquivalentPlasticStrain"]
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
