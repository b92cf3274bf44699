"""``tests/fake_dxmat.py`` for orthotropic elasticity (DXM_LAW_ORTHOTROPIC_ELASTIC): no state, the three frame states of a handle
(``dxm_set_frame`` / ``dxm_set_frame_field`` / ``dxm_frame_kind`` with the library's frame check), tangent layouts full and sym, the
arithmetic done by ``orthotropic_ref.update``.  TEST INFRASTRUCTURE ONLY, like the class it wraps: it lets the Python layer above
the C ABI -- ``HIPMaterial.rotation_matrix`` / ``set_frame`` / the rotate hooks, ``AcceleratedUpdate`` with a ``frame_fused``
material -- run without a GPU."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
from orthotropic_ref import update

LAW = _lib.LAW_ORTHOTROPIC_ELASTIC
IU = np.triu_indices(6)


class FakeDxmatOrthotropic(FakeDxmat):
    FIELDS = ()

    def __init__(self, real):
        super().__init__(real)
        self.frame_calls = []        # ("uniform" | "field" | "none", handle) of every accepted setter: what a test counts

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != LAW:
            return super().dxm_create(law, params, nparams, npoints, device)
        if nparams != 9:
            self._fail(-1, f"law {law} expects 9 parameters, got {nparams}")
            return None
        self._next += 8
        h = _Handle(law, [params[i] for i in range(nparams)], int(npoints))
        h.state = [{}, {}]
        h.frame, h.layout = None, 0
        self._handles[self._next] = h
        return self._next

    def dxm_set_tangent_layout(self, h, layout):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_set_tangent_layout(h, layout)
        if layout not in (0, 1):
            return self._fail(-1, "the orthotropic tangent Q^T C Q is a general symmetric 6x6: no coefficients (coef / pack4)")
        m.layout = layout
        m.epoch += 1
        return 0

    def dxm_tangent_size(self, h):
        m = self._h(h)
        return (21 if m.layout else 36) if m.law == LAW else super().dxm_tangent_size(h)

    def dxm_kernel_name(self, h):
        m = self._h(h)
        return f"orthotropic_kernel<{self.dxm_frame_kind(h)}".encode() if m.law == LAW else super().dxm_kernel_name(h)

    def dxm_algorithmic_bytes(self, h):
        return 456 if self.dxm_frame_kind(h) == 2 else 384

    # ---- frames ---------------------------------------------------------------------------------------------------------
    def _frames(self, h, p, count):
        m = self._h(h)
        if m.law != LAW:
            return self._fail(-1, f"law {m.law} takes no material frame: this law is isotropic"), None
        R = np.array(_rows(p, count, 9)).reshape(count, 3, 3)
        for i, r in enumerate(R):
            if not np.isfinite(r).all():
                return self._fail(-1, f"the frame of point {i} is not finite"), None
            if np.abs(r @ r.T - np.eye(3)).max() > 1e-8:
                return self._fail(-1, f"the frame of point {i} is not orthonormal"), None
        return 0, R

    def dxm_set_frame(self, h, r9):
        m = self._h(h)
        if m.law != LAW:
            return self._fail(-1, f"law {m.law} takes no material frame: this law is isotropic")
        if not _addr(r9):
            m.frame = None
            self.frame_calls.append(("none", _addr(h)))
        else:
            rc, R = self._frames(h, r9, 1)
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
        rc, R = self._frames(h, host, m.n)
        if rc:
            return rc
        m.frame = R
        m.epoch += 1
        self.frame_calls.append(("field", _addr(h)))
        return 0

    def dxm_frame_kind(self, h):
        f = getattr(self._h(h), "frame", None)
        return 0 if f is None else (1 if f.shape == (3, 3) else 2)

    # ---- state: none ------------------------------------------------------------------------------------------------------
    def dxm_set_state(self, h, which, field, host):
        return super().dxm_set_state(h, which, field, host) if self._h(h).law != LAW else self._fail(-1, "state field out of range")

    def dxm_get_state(self, h, which, field, host):
        return super().dxm_get_state(h, which, field, host) if self._h(h).law != LAW else self._fail(-1, "state field out of range")

    def dxm_isv_host(self, h, which, host):
        return super().dxm_isv_host(h, which, host) if self._h(h).law != LAW else 0

    def dxm_bind_isv_output(self, h, field, host):
        return super().dxm_bind_isv_output(h, field, host) if self._h(h).law != LAW else self._fail(-1, "state field out of range")

    # ---- the hot call -----------------------------------------------------------------------------------------------------
    def _update(self, m, grad):
        if m.law != LAW:
            return super()._update(m, grad)
        m.io_valid[1] = 0
        sig, ct = update(grad, m.params, m.frame)
        m.s1_alias, m.launched = False, True
        m.stats = dict(n_points=m.n, n_plastic=0, n_not_converged=0, n_nan=int(np.isnan(sig).any(axis=1).sum()), max_local_iters=0)
        return dict(sig=sig, Ct=ct, n_plastic=0, n_not_converged=0)

    def _tangent(self, m, r):
        ct = r["Ct"].reshape(m.n, 6, 6)
        return ct[:, IU[0], IU[1]] if m.layout else ct.reshape(m.n, 36)

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.law != LAW or m.n == 0:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        g = _rows(grad, m.n, 6)
        r = self._update(m, g)
        if _addr(flux):
            _rows(flux, m.n, 6)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 21 if m.layout else 36)[...] = self._tangent(m, r)
        return self._finish(m, g, r, stats)

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
        if m.law != LAW or m.n == 0:
            return super().dxm_integrate_rows(h, grad, dt, flux_base, ct_base, rows, stats)
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        g = _rows(grad, m.n, 6)
        r = self._update(m, g)                        # the frame of point i is the handle's own row i, not row rows[i]
        top = int(idx.max()) + 1
        _rows(flux_base, top, 6)[idx] = r["sig"]
        _rows(ct_base, top, 21 if m.layout else 36)[idx] = self._tangent(m, r)
        return self._finish(m, g, r, stats, idx)
