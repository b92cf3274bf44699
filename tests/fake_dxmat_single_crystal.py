"""``tests/fake_dxmat.py`` for FCC single-crystal viscoplasticity (DXM_LAW_SINGLE_CRYSTAL_FCC): the four state fields, the three frame
states of a handle with the library's frame check, the full tangent layout only, the ``dt`` of every call (recorded in ``dt_calls``
and validated as the library does), the arithmetic done by ``single_crystal_ref.update``.  TEST INFRASTRUCTURE ONLY, like the class
it wraps: it lets the Python layer above the C ABI run without a GPU."""
import ctypes as C
import math

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
import single_crystal_ref as sc

LAW = _lib.LAW_SINGLE_CRYSTAL_FCC
S1 = _lib.S1


class FakeDxmatSingleCrystal(FakeDxmat):
    FIELDS = (("eel", 6), ("g", 12), ("p", 12), ("a", 12))

    def __init__(self, real):
        super().__init__(real)
        self.frame_calls = []        # ("uniform" | "field" | "none", handle) of every accepted setter
        self.dt_calls = []           # the dt of every integrate call, as the library received it

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != LAW:
            return super().dxm_create(law, params, nparams, npoints, device)
        if nparams != 22:
            self._fail(-1, f"law {law} expects 22 parameters, got {nparams}")
            return None
        self._next += 8
        h = _Handle(law, [params[i] for i in range(nparams)], int(npoints))
        n = int(npoints)
        h.state = [{k: np.zeros((n, d)) for k, d in self.FIELDS} for _ in range(2)]
        h.frame = None
        h.maxit, h.rtol = 25, 1e-14
        self._handles[self._next] = h
        return self._next

    def dxm_set_tangent_layout(self, h, layout):
        if layout != 0:
            return self._fail(-1, "the single-crystal tangent is not symmetric (interaction hardening): only DXM_TANGENT_FULL is available")
        self._h(h).epoch += 1
        return 0

    def dxm_set_newton(self, h, maxit, rtol):
        if maxit < 1 or not rtol > 0.0:
            return self._fail(-1, f"invalid Newton controls maxit={maxit} rtol={rtol:g}")
        m = self._h(h)
        m.maxit, m.rtol = int(maxit), float(rtol)
        m.epoch += 1
        return 0

    def dxm_kernel_name(self, h):
        return f"single_crystal_kernel<{self.dxm_frame_kind(h)}".encode()

    def dxm_algorithmic_bytes(self, h):
        return 1080 if self.dxm_frame_kind(h) == 2 else 1008

    # ---- frames: the library's check ------------------------------------------------------------------------------------
    def _frames(self, p, count):
        R = np.array(_rows(p, count, 9)).reshape(count, 3, 3)
        for i, r in enumerate(R):
            if not np.isfinite(r).all():
                return self._fail(-1, f"the frame of point {i} is not finite"), None
            if np.abs(r @ r.T - np.eye(3)).max() > 1e-8:
                return self._fail(-1, f"the frame of point {i} is not orthonormal"), None
        return 0, R

    def dxm_set_frame(self, h, r9):
        m = self._h(h)
        if not _addr(r9):
            m.frame = None
            self.frame_calls.append(("none", _addr(h)))
        else:
            rc, R = self._frames(r9, 1)
            if rc:
                return rc
            m.frame = R[0]
            self.frame_calls.append(("uniform", _addr(h)))
        m.epoch += 1
        return 0

    def dxm_set_frame_field(self, h, host):
        m = self._h(h)
        if not _addr(host):
            return self.dxm_set_frame(h, None)
        rc, R = self._frames(host, m.n)
        if rc:
            return rc
        m.frame = R
        m.epoch += 1
        self.frame_calls.append(("field", _addr(h)))
        return 0

    def dxm_frame_kind(self, h):
        f = getattr(self._h(h), "frame", None)
        return 0 if f is None else (1 if f.shape == (3, 3) else 2)

    # ---- state: four fields -----------------------------------------------------------------------------------------------
    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if not 0 <= field < 4:
            return self._fail(-1, f"law {m.law} has no state field {field}")
        m.materialize_s1()
        name, dim = self.FIELDS[field]
        if m.n:
            m.state_of(which)[name][...] = _rows(host, m.n, dim)
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if not 0 <= field < 4:
            return self._fail(-1, f"law {m.law} has no state field {field}")
        name, dim = self.FIELDS[field]
        if m.n:
            _rows(host, m.n, dim)[...] = m.state_of(which)[name]
        return 0

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.n:
            _rows(host, m.n, 42)[...] = np.concatenate([m.state_of(which)[k] for k, _ in self.FIELDS], axis=1)
        return 0

    def dxm_bind_isv_output(self, h, field, host):
        if not 0 <= field < 4:
            return self._fail(-1, f"state field {field} out of range")
        self._h(h).isv_out[field] = _addr(host) or None
        return 0

    # ---- the hot call -----------------------------------------------------------------------------------------------------
    def _take_dt(self, dt):
        if not math.isfinite(dt) or dt < 0.0:
            return self._fail(-1, f"law {LAW} is rate-dependent: dt must be finite and >= 0, got {dt:g}")
        self.dt_calls.append(float(dt))
        return 0

    def _step(self, m, grad, dt):
        m.io_valid[1] = 0
        r = sc.update(grad, m.state[0], np.array(m.params), dt, R=m.frame, rtol=getattr(m, "rtol", 1e-14), maxit=getattr(m, "maxit", 25))
        m.state[1] = sc.next_state(r)
        m.s1_alias, m.launched = False, True
        bad = int((r["status"] != 0).sum())
        m.stats = dict(n_points=m.n, n_plastic=int(r["plastic"].sum()), n_not_converged=bad, n_nan=int(np.isnan(r["stress"]).any(axis=1).sum()),
                       max_local_iters=int(r["iters"].max(initial=0)))
        return dict(sig=r["stress"], Ct=r["tangent"].reshape(m.n, 36), n_plastic=m.stats["n_plastic"], n_not_converged=bad)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if rc := self._take_dt(dt):
            return rc
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, 6)
        r = self._step(m, g, dt)
        if _addr(flux):
            _rows(flux, m.n, 6)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 36)[...] = r["Ct"]
        if _addr(isv):
            self.dxm_isv_host(h, S1, isv)
        return self._finish(m, g, r, stats)

    def dxm_integrate_device(self, h, grad, dt, flux, ct, stream):
        """the device-pointer form, with ordinary memory standing for the device's: no transfer, no state download"""
        m = self._h(h)
        if rc := self._take_dt(dt):
            return rc
        if m.n == 0:
            return 0
        r = self._step(m, _rows(grad, m.n, 6), dt)
        if _addr(flux):
            _rows(flux, m.n, 6)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 36)[...] = r["Ct"]
        return 0

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
        if rc := self._take_dt(dt):
            return rc
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        g = _rows(grad, m.n, 6)
        r = self._step(m, g, dt)              # frame and state of point i are the handle's own row i, not row rows[i]
        top = int(idx.max()) + 1
        _rows(flux_base, top, 6)[idx] = r["sig"]
        _rows(ct_base, top, 36)[idx] = r["Ct"]
        return self._finish(m, g, r, stats, idx)
