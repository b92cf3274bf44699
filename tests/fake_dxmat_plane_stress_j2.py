"""``tests/fake_dxmat.py`` for plane-stress J2 plasticity with hardening (DXM_LAW_PS_J2_LINEAR = 30, DXM_LAW_PS_J2_VOCE = 31): 3-wide
gradient and flux, the 9-wide tangent, the state fields ``p`` (1) and ``epsp`` (3), the Newton controls, the arithmetic done by
``plane_stress_j2_ref`` (the restatement of the kernel).  TEST INFRASTRUCTURE ONLY, like the class it wraps: it lets the Python layer
above the C ABI run without a GPU."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
import plane_stress_j2_ref as pj

LAWS = (_lib.LAW_PS_J2_LINEAR, _lib.LAW_PS_J2_VOCE)
NPARAMS = {LAWS[0]: 4, LAWS[1]: 5}
REFUSAL = ("the plane-stress tangent is a 3x3 block of 9 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is available, no packed "
           "record (sym / coef / pack4) exists for this law")


class FakeDxmatPlaneStressJ2(FakeDxmat):
    PE_FIELDS = (("p", 1), ("epsp", 3))

    def _mine(self, h):
        return self._h(h).law in LAWS

    def dxm_create(self, law, params, nparams, npoints, device):
        if law not in LAWS:
            return super().dxm_create(law, params, nparams, npoints, device)
        if nparams != NPARAMS[law]:
            self._fail(-1, f"law {law} expects {NPARAMS[law]} parameters, got {nparams}")
            return None
        p = [params[i] for i in range(nparams)]
        if not (p[0] > 0.0 and -1.0 < p[1] < 0.5):
            self._fail(-1, f"invalid elastic constants E={p[0]:g} nu={p[1]:g}")
            return None
        self._next += 8
        n = int(npoints)
        h = _Handle(law, p, n)
        h.state = [dict(p=np.zeros(n), epsp=np.zeros((n, 3))) for _ in range(2)]
        h.newton = (pj.MAXIT, pj.RTOL)
        self._handles[self._next] = h
        return self._next

    def dxm_set_newton(self, h, maxit, rtol):
        if maxit < 1 or not rtol > 0:
            return self._fail(-1, f"invalid Newton controls maxit={maxit} rtol={rtol:g}")
        self._h(h).newton = (int(maxit), float(rtol))
        return super().dxm_set_newton(h, maxit, rtol)

    def dxm_set_tangent_layout(self, h, layout):
        if not self._mine(h):
            return super().dxm_set_tangent_layout(h, layout)
        if layout != 0:
            return self._fail(-1, REFUSAL)
        self._h(h).epoch += 1
        return 0

    def dxm_tangent_size(self, h):
        return 9 if self._mine(h) else super().dxm_tangent_size(h)

    def dxm_kernel_name(self, h):
        return f"plane_stress_j2_kernel<{1 + LAWS.index(self._h(h).law)}".encode() if self._mine(h) else super().dxm_kernel_name(h)

    def dxm_algorithmic_bytes(self, h):
        return 184

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def _field(self, m, field):
        if not 0 <= field < 2:
            self._fail(-1, f"law {m.law} has no state field {field}")
            return None
        return self.PE_FIELDS[field]

    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_set_state(h, which, field, host)
        f = self._field(m, field)
        if f is None:
            return -1
        m.materialize_s1()
        if m.n:
            m.state_of(which)[f[0]][...] = _rows(host, m.n, f[1]).reshape(m.state_of(which)[f[0]].shape)
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_get_state(h, which, field, host)
        f = self._field(m, field)
        if f is None:
            return -1
        if m.n:
            _rows(host, m.n, f[1])[...] = m.state_of(which)[f[0]].reshape(m.n, f[1])
        return 0

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_isv_host(h, which, host)
        if m.n == 0:
            return 0
        out, st = _rows(host, m.n, 4), m.state_of(which)
        out[:, 0], out[:, 1:] = st["p"], st["epsp"]
        return 0

    def dxm_bind_isv_output(self, h, field, host):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_bind_isv_output(h, field, host)
        if self._field(m, field) is None:
            return -1
        m.isv_out[field] = _addr(host) or None
        return 0

    def dxm_get_io(self, h, which, kind, host):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_get_io(h, which, kind, host)
        if not m.io_mask(which) & (1 << kind):
            return self._fail(-1, f"the {'flux' if kind else 'gradient'} of that state is not held on the device")
        first = which == _lib.S0 or m.s1_alias
        self.downloads.append((which, kind))
        if m.n:
            _rows(host, m.n, 3)[...] = m.io[0 if first else 1]["flux" if kind else "grad"]
        return 0

    # ---- the hot call -------------------------------------------------------------------------------------------------------------
    def _step(self, m, grad):
        m.io_valid[1] = 0
        s0 = m.state[0]
        r = pj.update(m.law, grad, s0["epsp"], s0["p"], m.params, *m.newton)
        m.state[1] = dict(p=r["p"].copy(), epsp=r["epsp"].copy())
        m.s1_alias, m.launched = False, True
        m.stats = dict(n_points=m.n, **pj.stats(r))
        return dict(sig=r["stress"], Ct=r["tangent"])

    def _finish(self, m, grad, r, stats, idx=None):
        if m.law not in LAWS:
            return super()._finish(m, grad, r, stats, idx)
        for field, addr in m.isv_out.items():
            if addr:
                name, dim = self.PE_FIELDS[field]
                rows = _rows(addr, m.n if idx is None else int(idx.max()) + 1, dim)
                rows[slice(None) if idx is None else idx] = m.state[1][name].reshape(m.n, dim)
        m.io[1] = dict(grad=np.array(grad), flux=r["sig"].copy())
        m.io_valid[1] = 3
        self._fill_stats(m, stats)
        return min(m.stats["n_not_converged"], 0x7FFFFFFF)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, 3)
        r = self._step(m, g)
        if _addr(flux):
            _rows(flux, m.n, 3)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 9)[...] = r["Ct"]
        if _addr(isv):
            out = _rows(isv, m.n, 4)
            out[:, 0], out[:, 1:] = m.state[1]["p"], m.state[1]["epsp"]
        return self._finish(m, g, r, stats)

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_integrate_rows(h, grad, dt, flux_base, ct_base, rows, stats)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        g = _rows(grad, m.n, 3)
        r = self._step(m, g)
        top = int(idx.max()) + 1
        _rows(flux_base, top, 3)[idx] = r["sig"]
        _rows(ct_base, top, 9)[idx] = r["Ct"]
        return self._finish(m, g, r, stats, idx)
