"""``tests/fake_dxmat.py`` for plane-strain logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_PE = 42): the 5-wide gradient and flux
``[00, 11, 22, 01, 10]``, the 25-wide tangent, the state fields ``ElasticStrain`` (4), ``EquivalentPlasticStrain`` (1) and the hidden
``PlasticStrain`` (4, field 2) that drives the update, the parameter validation of ``csrc/dxmat.hip::build_log_strain`` and the refusals
of the law's row with its own sentences; the arithmetic is done by ``log_strain_plane_ref.restricted`` (the definition of the law: law
19's restatement on the embedded F, restricted).  The double has no meshes: the displacement forms answer with the law's sentence.
TEST INFRASTRUCTURE ONLY, like the class it wraps."""
import ctypes as C
import math

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import FakeDxmat, _addr, _Handle, _rows
import log_strain_plane_ref as lp

LAW = _lib.LAW_LOG_STRAIN_PE
SET_REFUSAL = ("the plane-strain logarithmic-strain plasticity tangent dP/dF is a 5x5 block of 25 entries, not a symmetric 6x6: only "
               "DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for this law")
NO_DISPLACEMENT = ("plane-strain logarithmic-strain plasticity takes the 5-wide deformation gradient [F00, F11, F22, F01, F10]: the mesh "
                   "gradient kernels produce the 9-wide F, so the displacement forms (dxm_integrate_displacement*) and the fused "
                   "displacement gradient are not served; pass the 5-wide F [1 + H00, 1 + H11, 1, H01, H10] of the displacement gradient "
                   "H as an array")
NO_FIELDS = ("per-point parameter fields are not served for plane-strain logarithmic-strain plasticity: the kernel takes its constants per "
             "handle")
NO_FRAME = "plane-strain logarithmic-strain plasticity is isotropic (Hooke, Mises): a material frame changes nothing in its update"
STOCK_ONLY = ("plane-strain logarithmic-strain plasticity takes linear hardening only: it is served by the stock libdxmat, not by a "
              "custom-hardening build")


def _check(p):
    """The sentences of build_log_strain (and of the elastic constants inside it), or None."""
    names = ("E", "nu", "s0", "H0")
    for name, v in zip(names, p):
        if not math.isfinite(v):
            return f"logarithmic-strain plasticity: {name} must be finite, got {v:g}"
    E, nu, s0, H0 = p
    if not (E > 0.0 and -1.0 < nu < 0.5):
        return f"invalid elastic constants E={E:g} nu={nu:g}"
    if not s0 > 0.0:
        return f"logarithmic-strain plasticity: s0 must be > 0, got {s0:g}"
    if not H0 >= 0.0:
        return f"logarithmic-strain plasticity: the hardening slope H0 must be >= 0, got {H0:g}"
    return None


class FakeDxmatLogStrainPlane(FakeDxmat):
    LSP_FIELDS = (("ElasticStrain", 4), ("EquivalentPlasticStrain", 1), ("PlasticStrain", 4))

    def __init__(self, real):
        super().__init__(real)
        self.last_params = None

    def _mine(self, h):
        return self._h(h).law == LAW

    def dxm_create(self, law, params, nparams, npoints, device):
        if law != LAW:
            return super().dxm_create(law, params, nparams, npoints, device)
        if nparams != 4:
            self._fail(-1, f"law {law} expects 4 parameters, got {nparams}")
            return None
        p = [params[i] for i in range(nparams)]
        msg = _check(p)
        if msg:
            self._fail(-1, msg)
            return None
        self._next += 8
        n = int(npoints)
        h = _Handle(law, p, n)
        h.state = [{name: np.zeros((n, dim)) for name, dim in self.LSP_FIELDS} for _ in range(2)]
        self._handles[self._next] = h
        self.last_params = p
        return self._next

    def dxm_set_params(self, h, params, nparams):
        if not self._mine(h):
            return super().dxm_set_params(h, params, nparams)
        p = [params[i] for i in range(nparams)]
        msg = f"law {LAW} expects 4 parameters, got {nparams}" if nparams != 4 else _check(p)
        if msg:
            return self._fail(-1, msg)
        self.last_params = p
        return super().dxm_set_params(h, params, nparams)

    def dxm_set_tangent_layout(self, h, layout):
        if not self._mine(h):
            return super().dxm_set_tangent_layout(h, layout)
        if layout != 0:
            return self._fail(-1, SET_REFUSAL)
        self._h(h).epoch += 1
        return 0

    def dxm_tangent_size(self, h):
        return 25 if self._mine(h) else super().dxm_tangent_size(h)

    def dxm_kernel_name(self, h):
        return b"log_strain_plane_kernel" if self._mine(h) else super().dxm_kernel_name(h)

    def dxm_algorithmic_bytes(self, h):
        return 392 if self._mine(h) else self._real.dxm_algorithmic_bytes(h)

    def dxm_set_param_field(self, h, index, host):
        if self._mine(h):
            return self._fail(-1, NO_FIELDS)
        return self._fail(-1, "fake library: no parameter fields")

    def dxm_set_frame(self, h, host):
        if self._mine(h):
            return self._fail(-1, NO_FRAME)
        return self._fail(-1, "fake library: no material frames")

    def dxm_integrate_displacement(self, h, mesh, u, dt, flux, isv, ct, stats):
        if self._mine(h):
            return self._fail(-1, NO_DISPLACEMENT)
        return self._fail(-1, "fake library: no meshes")

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def _field(self, field):
        if not 0 <= field < 3:
            self._fail(-1, f"law {LAW} has no state field {field}")
            return None
        return self.LSP_FIELDS[field]

    def dxm_set_state(self, h, which, field, host):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_set_state(h, which, field, host)
        f = self._field(field)
        if f is None:
            return -1
        m.materialize_s1()
        if m.n:
            m.state_of(which)[f[0]][...] = _rows(host, m.n, f[1])
        return 0

    def dxm_get_state(self, h, which, field, host):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_get_state(h, which, field, host)
        f = self._field(field)
        if f is None:
            return -1
        if m.n:
            _rows(host, m.n, f[1])[...] = m.state_of(which)[f[0]]
        return 0

    @staticmethod
    def _isv(st):
        return np.concatenate([st["ElasticStrain"], st["EquivalentPlasticStrain"]], axis=1)

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_isv_host(h, which, host)
        if m.n:
            _rows(host, m.n, 5)[...] = self._isv(m.state_of(which))
        return 0

    def dxm_bind_isv_output(self, h, field, host):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_bind_isv_output(h, field, host)
        if not 0 <= field < 2:
            return self._fail(-1, f"law {LAW} has no internal state variable field {field}")
        m.isv_out[field] = _addr(host) or None
        return 0

    def dxm_get_io(self, h, which, kind, host):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_get_io(h, which, kind, host)
        if not m.io_mask(which) & (1 << kind):
            return self._fail(-1, f"the {'flux' if kind else 'gradient'} of that state is not held on the device")
        first = which == _lib.S0 or m.s1_alias
        self.downloads.append((which, kind))
        if m.n:
            _rows(host, m.n, 5)[...] = m.io[0 if first else 1]["flux" if kind else "grad"]
        return 0

    # ---- the hot call -------------------------------------------------------------------------------------------------------------
    def _step(self, m, grad):
        m.io_valid[1] = 0
        s0 = m.state[0]
        E, nu, s0_, H0 = m.params
        r = lp.restricted(grad, s0["PlasticStrain"], s0["EquivalentPlasticStrain"][:, 0], E=E, nu=nu, s0=s0_, H0=H0)
        m.state[1] = {"ElasticStrain": r["eel"].copy(), "EquivalentPlasticStrain": r["p"][:, None].copy(), "PlasticStrain": r["Ep"].copy()}
        m.s1_alias, m.launched = False, True
        nan = int((~np.isfinite(r["P"])).any(axis=1).sum())
        m.stats = dict(n_points=m.n, n_plastic=int(r["plastic"].sum()), n_not_converged=0, n_nan=nan, max_local_iters=0)
        return dict(sig=r["P"], Ct=r["A"].reshape(m.n, 25))

    def _finish(self, m, grad, r, stats, idx=None):
        if m.law != LAW:
            return super()._finish(m, grad, r, stats, idx)
        for field, addr in m.isv_out.items():
            if addr:
                name, dim = self.LSP_FIELDS[field]
                rows = _rows(addr, m.n if idx is None else int(idx.max()) + 1, dim)
                rows[slice(None) if idx is None else idx] = m.state[1][name]
        m.io[1] = dict(grad=np.array(grad), flux=r["sig"].copy())
        m.io_valid[1] = 3
        self._fill_stats(m, stats)
        return 0

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        g = _rows(grad, m.n, 5)
        r = self._step(m, g)
        if _addr(flux):
            _rows(flux, m.n, 5)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, 25)[...] = r["Ct"]
        if _addr(isv):
            _rows(isv, m.n, 5)[...] = self._isv(m.state[1])
        return self._finish(m, g, r, stats)

    def dxm_integrate_rows(self, h, grad, dt, flux_base, ct_base, rows, stats):
        m = self._h(h)
        if m.law != LAW:
            return super().dxm_integrate_rows(h, grad, dt, flux_base, ct_base, rows, stats)
        if m.n == 0:
            self._fill_stats(m, stats)
            return 0
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        g = _rows(grad, m.n, 5)
        r = self._step(m, g)
        top = int(idx.max()) + 1
        _rows(flux_base, top, 5)[idx] = r["sig"]
        _rows(ct_base, top, 25)[idx] = r["Ct"]
        return self._finish(m, g, r, stats, idx)
