"""``tests/fake_dxmat_heat.py`` for the two-dimensional heat-transfer laws (ids 35, 36) and the scalar mesh: the 6 / 7-wide tangent, the
``Enthalpy`` state field, ``dxm_mesh_create_plane_scalar`` and the nodal forms ``dxm_integrate_displacement`` / ``_rows``, which
interpolate the temperature themselves and neither read nor change the handle's own external state.  The arithmetic is done by
``heat_plane_ref``.  TEST INFRASTRUCTURE ONLY: it lets the Python layer above the C ABI run without a GPU."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from fake_dxmat import _addr, _Handle, _rows
from fake_dxmat_heat import FakeDxmatHeat
import heat_plane_ref as hp
import heat_transfer_ref as ht

LAWS = hp.LAWS_2D
S1 = _lib.S1


def _ints(p, n, dim):
    return np.ctypeslib.as_array((C.c_int32 * (n * dim)).from_address(_addr(p))).reshape(n, dim).copy()


class FakeDxmatHeatPlane(FakeDxmatHeat):
    def __init__(self, real):
        super().__init__(real)
        self._meshes = {}
        self.nodal_calls = []        # ("host" | "rows", n_dofs) of every nodal call

    def dxm_create(self, law, params, nparams, npoints, device):
        if law not in LAWS:
            return super().dxm_create(law, params, nparams, npoints, device)
        want = 2 if law == hp.STATIONARY_2D else 7
        if nparams != want:
            self._fail(-1, f"law {law} expects {want} parameters, got {nparams}")
            return None
        self._next += 8
        n = int(npoints)
        h = _Handle(law, [params[i] for i in range(nparams)], n)
        h.state = [{"h": np.zeros((n, 1))} for _ in range(2)]
        h.ext_kind, h.ext_uniform, h.ext_field = 0, ht.T_DEFAULT, None
        self._handles[self._next] = h
        return self._next

    def dxm_tangent_size(self, h):
        m = self._h(h)
        return hp.WIDTH[m.law] if m.law in LAWS else super().dxm_tangent_size(h)

    def dxm_kernel_name(self, h):
        m = self._h(h)
        return f"heat_plane_kernel<{LAWS.index(m.law)}, 0".encode() if m.law in LAWS else super().dxm_kernel_name(h)

    def dxm_algorithmic_bytes(self, h):
        m = self._h(h)
        return hp.BYTES[m.law] + 8 * m.ext_kind if m.law in LAWS else super().dxm_algorithmic_bytes(h)

    def _has_state(self, m, field):
        return (m.law == hp.PHASE_CHANGE_2D and field == 0) or super()._has_state(m, field)

    def dxm_isv_host(self, h, which, host):
        m = self._h(h)
        if m.law == hp.PHASE_CHANGE_2D and m.n:
            _rows(host, m.n, 1)[...] = m.state_of(which)["h"]
            return 0
        return super().dxm_isv_host(h, which, host)

    # ---- the scalar mesh ----------------------------------------------------------------------------------------------------------
    def dxm_mesh_create_plane_scalar(self, coords, n_vertices, conn, nv, n_cells, dofmap, nd, n_dofs, gd, phi, dphi, nqp, device):
        self._next += 8
        self._meshes[self._next] = dict(coords=_rows(coords, n_vertices, 3).copy(), cells=_ints(conn, n_cells, nv), dofmap=_ints(dofmap, n_cells, nd),
                                        n_dofs=int(n_dofs), geom_dphi=_rows(gd, nqp * nv, 2).reshape(nqp, nv, 2).copy(),
                                        phi=_rows(phi, nqp, nd).copy(), dphi=_rows(dphi, nqp * nd, 2).reshape(nqp, nd, 2).copy(),
                                        npoints=int(n_cells) * int(nqp))
        return self._next

    def dxm_mesh_destroy(self, mesh):
        self._meshes.pop(_addr(mesh), None)
        return 0

    def dxm_mesh_npoints(self, mesh):
        return self._meshes[_addr(mesh)]["npoints"]

    def dxm_mesh_displacement_size(self, mesh):
        return self._meshes[_addr(mesh)]["n_dofs"]

    # ---- the hot calls ------------------------------------------------------------------------------------------------------------
    def _step2(self, m, g2, T):
        m.io_valid[1] = 0
        r = hp.update(m.law, g2, T, np.array(m.params))
        if m.law == hp.PHASE_CHANGE_2D:
            m.state[1] = {"h": r["enthalpy"].reshape(m.n, 1).copy()}
        m.s1_alias, m.launched = False, True
        m.stats = dict(n_points=m.n, n_plastic=0, n_not_converged=0, n_nan=r["n_nan"], max_local_iters=0)
        return dict(sig=r["flux"], Ct=r["tangent"], n_plastic=0, n_not_converged=0)

    def _nodal(self, h, mesh, t):
        m, case = self._h(h), self._meshes[_addr(mesh)]
        if m.law not in LAWS:
            self._fail(-1, "a scalar mesh (dxm_mesh_create_plane_scalar) carries a temperature, not a displacement")
            return m, None, None
        if case["npoints"] != m.n:
            self._fail(-1, f"mesh has {case['npoints']} Gauss points, material {m.n}")
            return m, None, None
        tn = _rows(t, case["n_dofs"], 1).reshape(-1)
        T, g2, _ = hp.reference(case, tn)
        return m, g2, self._step2(m, g2, T)      # the handle's own external state is not read

    def dxm_integrate(self, h, grad, dt, flux, isv, ct, stats):
        m = self._h(h)
        if m.law not in LAWS:
            return super().dxm_integrate(h, grad, dt, flux, isv, ct, stats)
        g = _rows(grad, m.n, 2)
        r = self._step2(m, g, m.ext_field if m.ext_kind else m.ext_uniform)
        return self._deliver(h, m, g, r, flux, isv, ct, stats)

    def _deliver(self, h, m, g, r, flux, isv, ct, stats):
        if _addr(flux):
            _rows(flux, m.n, 2)[...] = r["sig"]
        if _addr(ct):
            _rows(ct, m.n, hp.WIDTH[m.law])[...] = r["Ct"]
        if _addr(isv):
            self.dxm_isv_host(h, S1, isv)
        return self._finish(m, g, r, stats)

    def dxm_integrate_displacement(self, h, mesh, t, dt, flux, isv, ct, stats):
        m, g, r = self._nodal(h, mesh, t)
        if r is None:
            return -1
        self.nodal_calls.append(("host", self._meshes[_addr(mesh)]["n_dofs"]))
        return self._deliver(h, m, g, r, flux, isv, ct, stats)

    def dxm_integrate_displacement_rows(self, h, mesh, t, dt, flux_base, ct_base, rows, stats):
        m, g, r = self._nodal(h, mesh, t)
        if r is None:
            return -1
        self.nodal_calls.append(("rows", self._meshes[_addr(mesh)]["n_dofs"]))
        idx = np.ctypeslib.as_array((C.c_int64 * m.n).from_address(_addr(rows)))
        top = int(idx.max()) + 1
        _rows(flux_base, top, 2)[idx] = r["sig"]
        _rows(ct_base, top, hp.WIDTH[m.law])[idx] = r["Ct"]
        return self._finish(m, g, r, stats, idx)
