"""``tests/fake_dxmat.py`` for the two heat-transfer laws (DXM_LAW_HEAT_STATIONARY, DXM_LAW_HEAT_PHASE_CHANGE): the external state
variable of a handle (uniform after ``dxm_create`` at 293.15, a field kept by the handle, the launch generation that moves with the
kind and the uniform value but not with a field rewritten in place), the 12 / 13-wide tangent, the ``Enthalpy`` state field, the
arithmetic done by ``heat_transfer_ref``.  TEST INFRASTRUCTURE ONLY, like the class it wraps: it lets the Python layer above the C
ABI run without a GPU."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
import heat_transfer_ref as ht

LAWS = (_lib.LAW_HEAT_STATIONARY, _lib.LAW_HEAT_PHASE_CHANGE)
S1 = _lib.S1


class FakeDxmatHeat(FakeDxmat):
    FIELDS = (("h", 1),)

    def __init__(self, real):
        super().__init__(real)
        self.ext_calls = []          # ("uniform", value) / ("field", size) of every accepted setter

    def dxm_create(self, law, params, nparams, npoints, device):
        if law not in LAWS:
            return super().dxm_create(law, params, nparams, npoints, device)
        want = 2 if law == _lib.LAW_HEAT_STATIONARY else 7
        if nparams != want:
            self._fail(-1, f"law {law} expects {want} parameters, got {nparams}")
            return None
        self._next += 8
        h = _Handle(law, [params[i] for i in range(nparams)], int(npoints))
        n = int(npoints)
        h.state = [{"h": np.zeros((n, 1))} for _ in range(2)]
        h.ext_kind, h.ext_uniform, h.ext_field = 0, ht.T_DEFAULT, None
        self._handles[self._next] = h
        return self._next

    def dxm_set_tangent_layout(self, h, layout):
        if layout != 0:
            return self._fail(-1, "only DXM_TANGENT_FULL is available")
        self._h(h).epoch += 1
        return 0

    def dxm_tangent_size(self, h):
        return ht.WIDTH[self._h(h).law]

    def dxm_kernel_name(self, h):
        m = self._h(h)
        return f"heat_transfer_kernel<{LAWS.index(m.law)}, {m.ext_kind}".encode()

    def dxm_algorithmic_bytes(self, h):
        m = self._h(h)
        return (120 if m.law == _lib.LAW_HEAT_STATIONARY else 136) + 8 * m.ext_kind

    # ---- the external state variable ----------------------------------------------------------------------------------------
    def dxm_set_external_state(self, h, index, host):
        m = self._h(h)
        if index != 0:
            return self._fail(-1, f"law {m.law} has no external state variable {index}")
        if not _addr(host):
            if m.ext_kind:
                m.ext_kind, m.epoch = 0, m.epoch + 1
            return 0
        v = np.array(_rows(host, m.n, 1)).reshape(-1) if m.n else np.zeros(0)
        bad = np.flatnonzero(~np.isfinite(v))
        if len(bad):
            return self._fail(-1, f"Temperature is not finite at point {bad[0]} ({v[bad[0]]:g})")
        m.ext_field = v
        if not m.ext_kind:
            m.ext_kind, m.epoch = 1, m.epoch + 1
        self.ext_calls.append(("field", len(v)))
        return 0

    def dxm_set_external_state_uniform(self, h, index, value):
        m = self._h(h)
        if index != 0:
            return self._fail(-1, f"law {m.law} has no external state variable {index}")
        if not np.isfinite(value):
            return self._fail(-1, f"Temperature must be finite, got {value:g}")
        if m.ext_kind == 0 and m.ext_uniform == value:
            return 0
        m.ext_uniform, m.ext_kind, m.epoch = float(value), 0, m.epoch + 1
        self.ext_calls.append(("uniform", float(value)))
        return 0

    def dxm_external_state_kind(self, h, index):
        return self._h(h).ext_kind if index == 0 else -1

    # ---- state: Enthalpy ------------------------------------------------------------------------------------------------------
    def _has_state(self, m, field):
        return m.law == _lib.LAW_HEAT_PHASE_CHANGE and field == 0

    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if not self._has_state(m, field):
            return self._fail(-1, f"law {m.law} has no state field {field}")
        m.materialize_s1()
        if m.n:
            m.state_of(which)["h"][...] = _rows(host, m.n, 1)
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if not self._has_state(m, field):
            return self._fail(-1, f"law {m.law} has no state field {field}")
        if m.n:
            _rows(host, m.n, 1)[...] = m.state_of(which)["h"]
        return 0

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.law == _lib.LAW_HEAT_PHASE_CHANGE and m.n:
            _rows(host, m.n, 1)[...] = m.state_of(which)["h"]
        return 0

    def dxm_bind_isv_output(self, h, field, host):
        m = self._h(h)
        if not self._has_state(m, field):
            return self._fail(-1, f"state field {field} out of range")
        m.isv_out[field] = _addr(host) or None
        return 0

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
        T = m.ext_field if m.ext_kind else m.ext_uniform     # point i reads entry i of the handle's field
        r = ht.update(m.law, grad, T, np.array(m.params))
        if m.law == _lib.LAW_HEAT_PHASE_CHANGE:
            m.state[1] = {"h": r["enthalpy"].reshape(m.n, 1).copy()}
        m.s1_alias, m.launched = False, True
        m.stats = dict(n_points=m.n, n_plastic=0, n_not_converged=0, n_nan=ht.n_nan(r), max_local_iters=0)
        return dict(sig=r["flux"], Ct=r["tangent"], n_plastic=0, n_not_converged=0)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, 3)
        r = self._step(m, g)
        w = ht.WIDTH[m.law]
        if _addr(flux):
            _rows(flux, m.n, 3)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, w)[...] = r["Ct"]
        if _addr(isv):
            self.dxm_isv_host(h, S1, isv)
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
        _rows(ct_base, top, ht.WIDTH[m.law])[idx] = r["Ct"]
        return self._finish(m, g, r, stats, idx)
