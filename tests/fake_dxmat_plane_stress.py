"""``tests/fake_dxmat.py`` for the two plane-stress return mappings (DXM_LAW_PS_QUADRATIC = 23, DXM_LAW_PS_POLYGON = 24): the hidden
``PlasticStrain`` state field 0 of a handle, the 9-wide tangent, the Newton controls, what ``dxm_create`` refuses, the arithmetic done
by ``plane_stress_ref``.  TEST INFRASTRUCTURE ONLY, like the class it wraps: it lets the Python layer above the C ABI run without a GPU."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
import plane_stress_ref as ps

LAWS = (_lib.LAW_PS_QUADRATIC, _lib.LAW_PS_POLYGON)
S1 = _lib.S1


def refusal(law, p):
    """the sentence of ``build_ps_quadratic`` / ``build_ps_polygon`` (its distinguishing part); None: accepted"""
    if law == _lib.LAW_PS_POLYGON:
        return ps.check_polygon(p)
    names = ("E", "nu", "sig0", "q", "tangent")
    for k, v in enumerate(p):
        if not np.isfinite(v):
            return f"{names[k]} must be finite"
    if not p[0] > 0:
        return "E must be > 0"
    if not -1 < p[1] < 1:
        return "nu must lie in (-1, 1)"
    if not p[2] > 0:
        return "sig0 must be > 0"
    if not p[3] > 0:
        return "the shear weight q must be > 0"
    if p[4] not in (0.0, 1.0):
        return "tangent must be 0"
    return None


class FakeDxmatPlaneStress(FakeDxmat):
    FIELDS = (("epsp", 3),)

    def dxm_create(self, law, params, nparams, npoints, device):
        if law not in LAWS:
            return super().dxm_create(law, params, nparams, npoints, device)
        want = 5 if law == _lib.LAW_PS_QUADRATIC else 15
        if nparams != want:
            self._fail(-1, f"law {law} expects {want} parameters, got {nparams}")
            return None
        p = [params[i] for i in range(nparams)]
        why = refusal(law, p)
        if why:
            self._fail(-1, f"plane-stress yield set: {why}")
            return None
        self._next += 8
        h = _Handle(law, p, int(npoints))
        n = int(npoints)
        h.state = [{"epsp": np.zeros((n, 3))} for _ in range(2)]
        h.newton = (25, 1e-14)
        self._handles[self._next] = h
        return self._next

    def dxm_set_params(self, h, params, nparams):
        m = self._h(h)
        if m.law in LAWS:
            p = [params[i] for i in range(nparams)]
            why = refusal(m.law, p)
            if why:
                return self._fail(-1, f"plane-stress yield set: {why}")
        return super().dxm_set_params(h, params, nparams)

    def dxm_set_newton(self, h, maxit, rtol):
        if maxit < 1 or not rtol > 0:
            return self._fail(-1, f"invalid Newton controls maxit={maxit} rtol={rtol:g}")
        self._h(h).newton = (int(maxit), float(rtol))
        return super().dxm_set_newton(h, maxit, rtol)

    def dxm_set_tangent_layout(self, h, layout):
        if layout != 0:
            return self._fail(-1, "the plane-stress tangent is a 3x3 block of 9 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is available")
        self._h(h).epoch += 1
        return 0

    def dxm_tangent_size(self, h):
        return 9

    def dxm_kernel_name(self, h):
        return f"plane_stress_kernel<{LAWS.index(self._h(h).law)}".encode()

    def dxm_algorithmic_bytes(self, h):
        return 168

    # ---- state: the hidden plastic strain -----------------------------------------------------------------------------------------
    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if field != 0:
            return self._fail(-1, f"law {m.law} has no state field {field}")
        m.materialize_s1()
        if m.n:
            m.state_of(which)["epsp"][...] = _rows(host, m.n, 3)
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if field != 0:
            return self._fail(-1, f"law {m.law} has no state field {field}")
        if m.n:
            _rows(host, m.n, 3)[...] = m.state_of(which)["epsp"]
        return 0

    def dxm_isv_host(self, h, which, host):
        return 0    # no user-visible state

    def dxm_bind_isv_output(self, h, field, host):
        return self._fail(-1, f"state field {field} out of range")

    def dxm_get_io(self, h, which, kind, host):
        m = self._h(h)
        if not m.io_mask(which) & (1 << kind):
            return self._fail(-1, f"the {'flux' if kind else 'gradient'} of that state is not held on the device")
        first = which == _lib.S0 or m.s1_alias
        self.downloads.append((which, kind))
        if m.n:
            _rows(host, m.n, 3)[...] = m.io[0 if first else 1]["flux" if kind else "grad"]
        return 0

    # ---- the hot call -----------------------------------------------------------------------------------------------------------
    def _step(self, m, grad):
        m.io_valid[1] = 0
        r = ps.update(m.law, grad, m.state[0]["epsp"], np.array(m.params), *m.newton)
        m.state[1] = {"epsp": r["state"].copy()}
        m.s1_alias, m.launched = False, True
        tangent = m.law == _lib.LAW_PS_QUADRATIC and m.params[4] != 0
        m.stats = dict(n_points=m.n, **ps.stats(r, tangent))
        return dict(sig=r["stress"], Ct=r["tangent"], n_plastic=m.stats["n_plastic"], n_not_converged=m.stats["n_not_converged"])

    def _finish(self, m, grad, r, stats, idx=None):
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
        return self._finish(m, g, r, stats)

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
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
