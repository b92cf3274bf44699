"""``tests/fake_dxmat.py`` for finite-strain FCC single-crystal viscoplasticity (DXM_LAW_FS_SINGLE_CRYSTAL_FCC): the four state
fields (the plastic part of F starts as the identity), the frame states and the ``dt`` handling of the small-strain double it
extends, the full tangent layout only, the arithmetic done by ``fs_single_crystal_ref.update``.  TEST INFRASTRUCTURE ONLY, like the
classes it wraps: it lets the Python layer above the C ABI run without a GPU."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import _addr, _Handle, _rows
from fake_dxmat_single_crystal import FakeDxmatSingleCrystal
import fs_single_crystal_ref as fx

LAW = _lib.LAW_FS_SINGLE_CRYSTAL_FCC
S1 = _lib.S1


class FakeDxmatFsSingleCrystal(FakeDxmatSingleCrystal):
    FIELDS = (("g", 12), ("p", 12), ("a", 12), ("Fp", 9))

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != LAW:
            return super().dxm_create(law, params, nparams, npoints, device)
        if nparams != 16:
            self._fail(-1, f"law {law} expects 16 parameters, got {nparams}")
            return None
        self._next += 8
        h = _Handle(law, [params[i] for i in range(nparams)], int(npoints))
        h.state = [fx.zero_state(int(npoints)) for _ in range(2)]
        h.frame = None
        h.maxit, h.rtol = 25, 1e-14
        self._handles[self._next] = h
        return self._next

    def dxm_set_tangent_layout(self, h, layout):
        if layout != 0:
            return self._fail(-1, "the finite-strain single-crystal tangent dP/dF is 81 independent numbers: only DXM_TANGENT_FULL is available")
        self._h(h).epoch += 1
        return 0

    def dxm_kernel_name(self, h):
        return f"fs_single_crystal_kernel<{self.dxm_frame_kind(h)}".encode()

    def dxm_algorithmic_bytes(self, h):
        return 1584 if self.dxm_frame_kind(h) == 2 else 1512

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.n:
            _rows(host, m.n, 45)[...] = np.concatenate([m.state_of(which)[k] for k, _ in self.FIELDS], axis=1)
        return 0

    def _step(self, m, grad, dt):
        m.io_valid[1] = 0
        r = fx.update(grad, m.state[0], np.array(m.params), dt, R=m.frame, rtol=getattr(m, "rtol", 1e-14), maxit=getattr(m, "maxit", 25))
        m.state[1] = fx.next_state(r)
        m.s1_alias, m.launched = False, True
        bad = int((r["status"] != 0).sum())
        m.stats = dict(n_points=m.n, n_plastic=int(r["plastic"].sum()), n_not_converged=bad, n_nan=int(np.isnan(r["stress"]).any(axis=1).sum()),
                       max_local_iters=int(r["iters"].max(initial=0)))
        return dict(sig=r["stress"], Ct=r["tangent"].reshape(m.n, 81), n_plastic=m.stats["n_plastic"], n_not_converged=bad)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if rc := self._take_dt(dt):
            return rc
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, 9)
        r = self._step(m, g, dt)
        if _addr(flux):
            _rows(flux, m.n, 9)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 81)[...] = r["Ct"]
        if _addr(isv):
            self.dxm_isv_host(h, S1, isv)
        return self._finish(m, g, r, stats)

    def dxm_integrate_device(self, h, grad, dt, flux, ct, stream):
        m = self._h(h)
        if rc := self._take_dt(dt):
            return rc
        if m.n == 0:
            return 0
        r = self._step(m, _rows(grad, m.n, 9), dt)
        if _addr(flux):
            _rows(flux, m.n, 9)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 81)[...] = r["Ct"]
        return 0

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
        if rc := self._take_dt(dt):
            return rc
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        g = _rows(grad, m.n, 9)
        r = self._step(m, g, dt)              # frame and state of point i are the handle's own row i, not row rows[i]
        top = int(idx.max()) + 1
        _rows(flux_base, top, 9)[idx] = r["sig"]
        _rows(ct_base, top, 81)[idx] = r["Ct"]
        return self._finish(m, g, r, stats, idx)
