"""GPU: the axisymmetric gradient kernels (``csrc/axisym_gradient.hip``) against ``axisym_gradient_ref`` (a numpy restatement, held to
its own longdouble evaluation within 1e-14 by ``test_axisym_gradient_ref_cpu.py``), the refusals of the three gradient entry points,
and the displacement forms on an ``AxisymmetricMesh`` (laws 26, 27, 28, 40: kind 0; law 1: kind 2; law 7: kind 3) against "gradient
kernel, then array form" bit for bit.

Stand-alone kernels: bound 1e-13 absolute under ``|H| < 0.15`` and ``|u_r / r| < 0.15`` at ``r >= 1`` (the bound and condition of
``test_gpu_plane_gradient.py``; ``test_axisym_gradient_ref_cpu.py`` asserts the condition on every input used here), the four kinds
with and without the radius array, a random field and the affine patch field, outputs with 8 rows more than the mesh has points and
filled with NaN beforehand.  Each test prints its largest error.

Observed on an MI355X: kernels within 4.4e-16 of the restatement on every mesh (bound 1e-13), the radius within 4.4e-16 relative (bound
1e-14); displacement forms bit for bit in every case; laws 26-28 against the numpy restatement on the reference strain within
6.9e-15 of the field scale (bound 1e-12)."""
import ctypes as C

import numpy as np
import pytest

import axisym_gradient_ref as ag
import gradient_ref as gr
import plane_gradient_ref as pg
import test_gpu_plane_gradient as pgt
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.gradient import AxisymmetricMesh, PlaneMesh, PlaneScalarMesh
from helpers import to_device, to_host
from plane_laws_2d import LAWS, increments, parity_bounds, reference_update

pytestmark = pytest.mark.gpu
BOUND = 1e-13      # absolute, |H| < 0.15 and |u_r / r| < 0.15: the bound of test_gpu_plane_gradient.py
RADIUS_BOUND = 1e-14   # relative
EXTRA = 8          # rows past the mesh's last point: they keep their NaN
bits, same, err = pgt.bits, pgt.same, pgt.err


def _mesh(case, cells=None):
    sel = slice(None) if cells is None else cells
    return AxisymmetricMesh(case["coords"], case["cells"][sel], case["dofmap"][sel], case["n_dofs"], case["geom_phi"], case["geom_dphi"],
                            case["phi"], case["dphi"])


def _against_reference(tag, case):
    """the four kinds, with and without the radius array, for the random and the patch field; returns the largest error"""
    import torch

    mesh = _mesh(case)
    assert mesh.tdim == 2 and mesh.axisymmetric and mesh.displacement_size == case["xd"].size
    st = torch.cuda.current_stream().cuda_stream
    n = mesh.npoints
    rad_ref = ag.radius(case)
    assert n == case["npoints"] == len(rad_ref) and np.array_equal(mesh.radii(), rad_ref)
    worst, worst_rad = 0.0, 0.0
    for name in ("random", "patch"):
        u = case["u_" + name]
        H, hoop, _ = ag.reference(case, u)
        assert np.abs(H).max() < 0.15 and np.abs(hoop).max() < 0.15 and rad_ref.min() >= 1.0
        ud = to_device(np.array(u))
        for kind in range(4):
            ref = ag.rows(H, hoop, kind)
            assert ref.shape == (n, ag.WIDTH[kind])
            for with_radius in (False, True):
                out = torch.full((n + EXTRA, ref.shape[1]), float("nan"), dtype=torch.float64, device="cuda:0")
                rad = torch.full((n + EXTRA,), float("nan"), dtype=torch.float64, device="cuda:0")
                mesh.axisymmetric_gradient_device(ud.data_ptr(), kind, out.data_ptr(), rad.data_ptr() if with_radius else 0, st)
                torch.cuda.synchronize()
                got, got_rad = to_host(out), to_host(rad)
                assert np.isfinite(got[:n]).all(), f"{tag} {name} kind {kind}: rows left unwritten"
                assert np.isnan(got[n:]).all(), f"{tag} {name} kind {kind}: rows past the last point written"
                e = float(np.abs(got[:n] - ref).max())
                worst = max(worst, e)
                assert e < BOUND, (tag, name, kind, with_radius, e)
                if kind == 2:
                    assert np.all(got[:n, 4:] == 0.0)
                elif kind == 3:
                    assert np.all(got[:n, 5:] == 0.0)
                if with_radius:
                    assert np.isfinite(got_rad[:n]).all() and np.isnan(got_rad[n:]).all()
                    er = float(np.abs(got_rad[:n] / rad_ref - 1).max())
                    worst_rad = max(worst_rad, er)
                    assert er < RADIUS_BOUND, (tag, name, kind, er)
                else:
                    assert np.isnan(got_rad).all()          # no radius asked for: none written
    print(f"axisymmetric gradient kernels {tag}: {n} points, error {worst:.3e} (bound {BOUND:.0e}), radius {worst_rad:.3e} (bound {RADIUS_BOUND:.0e})")
    mesh.close()
    return worst


@pytest.mark.parametrize("tag", list(pg.QUAD_CASES))
def test_quadrilaterals(tag):
    """Q1 at 1 point per cell (81 points: one ragged block) and at 4 (324: a block boundary inside a cell run), Q2 at 5 arbitrary
    interior points (405) and at 9 Gauss points (729), on the distorted 9 x 9 grid at r = x + 1"""
    case = ag.quad_case(tag)
    assert case["npoints"] == {"q1-x1": 81, "q1-x4": 324, "q2-x5": 405, "q2-x9": 729}[tag] and case["npoints"] % 256 != 0
    _against_reference(f"quad {tag}", case)


@pytest.mark.parametrize("rule", gr.SIMPLEX_RULES)
@pytest.mark.parametrize("element", ag.TRI_ELEMENTS)
def test_triangles(element, rule):
    _against_reference(f"tri {element}-{rule}", ag.tri_case(element, rule))


def test_refusals_write_nothing():
    """the wrong mesh for either displacement-gradient entry point and for the scalar one, kinds 4 and -1, a misaligned output"""
    import torch

    lib = _lib.load()
    case = ag.quad_case("q1-x1")
    axi = _mesh(case)
    plane_case = pg.quad_case("q1-x1")
    plane = PlaneMesh(plane_case["coords"], plane_case["cells"], plane_case["dofmap"], plane_case["n_dofs"], plane_case["geom_dphi"], plane_case["dphi"])
    scalar = PlaneScalarMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"], case["phi"], case["dphi"])
    u = to_device(np.zeros(case["xd"].size))
    out = torch.full((axi.npoints + EXTRA, 9), float("nan"), dtype=torch.float64, device="cuda:0")
    for kind in range(4):
        for other in (plane, scalar):
            assert lib.dxm_mesh_axisymmetric_gradient_device(other._handle, u.data_ptr(), kind, out.data_ptr(), None, None) < 0
            assert "needs an axisymmetric mesh (dxm_mesh_create_axisymmetric)" in err(lib) and "dxm_mesh_gradient_device" in err(lib), err(lib)
    for kind in (0, 1, 2, 3, 4, -1):
        assert lib.dxm_mesh_gradient_device(axi._handle, u.data_ptr(), kind, out.data_ptr(), None) < 0
        assert "an axisymmetric mesh (dxm_mesh_create_axisymmetric)" in err(lib) and "dxm_mesh_axisymmetric_gradient_device" in err(lib), err(lib)
    with pytest.raises(_lib.DxmError, match="dxm_mesh_axisymmetric_gradient_device"):
        axi.gradient_device(u.data_ptr(), 2, out.data_ptr())
    assert lib.dxm_mesh_scalar_gradient_device(axi._handle, u.data_ptr(), out.data_ptr(), None, None) < 0
    assert "needs a scalar mesh (dxm_mesh_create_plane_scalar)" in err(lib), err(lib)
    for kind in (4, -1):
        assert lib.dxm_mesh_axisymmetric_gradient_device(axi._handle, u.data_ptr(), kind, out.data_ptr(), None, None) < 0
        assert "axisymmetric gradient kind must be 0" in err(lib), err(lib)
        assert lib.dxm_mesh_gradient_device(plane._handle, u.data_ptr(), kind, out.data_ptr(), None) < 0
        assert "gradient kind must be 0 (strain), 1 (F), 2 (plane-strain 4-vector) or 3 (in-plane 3-vector)" in err(lib), err(lib)
    for kind in (0, 2):
        assert out.data_ptr() % 16 == 0
        assert lib.dxm_mesh_axisymmetric_gradient_device(axi._handle, u.data_ptr(), kind, out.data_ptr() + 8, None, None) < 0
        assert "16-byte aligned for axisymmetric gradient kinds 0 and 2" in err(lib), err(lib)
        with pytest.raises(_lib.DxmError, match="16-byte aligned"):
            axi.axisymmetric_gradient_device(u.data_ptr(), kind, out.data_ptr() + 8)
    for args in ((None, u.data_ptr(), 0, out.data_ptr()), (axi._handle, None, 0, out.data_ptr()), (axi._handle, u.data_ptr(), 0, None)):
        assert lib.dxm_mesh_axisymmetric_gradient_device(*args, None, None) < 0 and "null argument" in err(lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                       # a refused call wrote nothing
    for m in (axi, plane, scalar):
        m.close()


# ---- the displacement forms -------------------------------------------------------------------------------------------------------------
OGDEN = [28.8, 27778.0, 69444444.0]                      # alpha, mu, K of the .mfront file (ogden_ref.DEFAULTS)
#: law id -> (parameters, the kind an axisymmetric mesh evaluates for it, the law whose load steps drive it, does it yield)
FORMS = {
    26: (LAWS[26]["prm"], 0, 26, False),
    27: (LAWS[27]["prm"], 0, 27, True),
    28: (LAWS[28]["prm"], 0, 28, True),
    40: ([70e3, 0.3, 250.0, 5e3, 10.0], 0, 27, True),   # plane-strain Hosford: E, nu, R0, H, a
    1: (LAWS[27]["prm"], 2, 27, True),                  # the 6-wide J2 law with linear hardening
    7: (OGDEN, 3, 26, False),                           # the 9-wide Ogden law
}


class Handle(pgt.Handle):
    """``test_gpu_plane_gradient.Handle`` with the visible state fields of every law (``dxm_law_info_get``), and the rows forms"""

    def __init__(self, law, n, prm):
        super().__init__(law, n, prm)
        info = _lib.law_info(law)
        self.fields = tuple(int(info.isv_dim[f]) for f in range(info.n_isv_fields))

    def displacement_rows(self, mesh, u, rows, n_all):
        f, c, st = np.full((n_all, self.w), -7.25), np.full((n_all, self.nt), -7.25), _lib.Stats()
        rc = self.lib.dxm_integrate_displacement_rows(self.h, mesh._handle, u.ctypes.data, 0.0, f.ctypes.data, c.ctypes.data, rows.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()

    def rows(self, eps, rows, n_all):
        f, c, st = np.full((n_all, self.w), -7.25), np.full((n_all, self.nt), -7.25), _lib.Stats()
        rc = self.lib.dxm_integrate_rows(self.h, eps.ctypes.data, 0.0, f.ctypes.data, c.ctypes.data, rows.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()


def _gradient(mesh, ud, kind):
    import torch

    grad = torch.full((mesh.npoints, ag.WIDTH[kind]), float("nan"), dtype=torch.float64, device="cuda:0")
    mesh.axisymmetric_gradient_device(ud.data_ptr(), kind, grad.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return grad


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("mesh_name", pg.LAW_MESHES)
@pytest.mark.parametrize("law", sorted(FORMS))
def test_displacement_forms_equal_gradient_then_update_bit_for_bit(law, mesh_name, fused):
    """``dxm_integrate_displacement_device`` against ``dxm_mesh_axisymmetric_gradient_device(kind)`` -> ``dxm_integrate_device``,
    ``dxm_integrate_displacement`` against ``dxm_integrate`` on the downloaded gradient, and ``dxm_integrate_displacement_rows`` on a
    mesh of every second cell against ``dxm_integrate_rows`` on that mesh's downloaded gradient: the same kernels, arrays and grids,
    so stress, tangent and state agree bit for bit, over two increments with an advance between, at both settings of
    ``fused_gradient`` (no fused form exists).  Laws 26-28 also against the numpy restatement on the reference strain."""
    prm, kind, drive, yields = FORMS[law]
    case = ag.law_mesh(mesh_name)
    mesh = _mesh(case)
    n, nqp = mesh.npoints, case["dphi"].shape[0]
    every_second = np.arange(0, len(case["cells"]), 2)
    sub = _mesh(case, every_second)
    rows = np.ascontiguousarray((every_second[:, None] * nqp + np.arange(nqp)).ravel(), dtype=np.int64)
    others = np.setdiff1d(np.arange(n), rows)
    hs = [Handle(law, n, prm) for _ in range(4)] + [Handle(law, sub.npoints, prm) for _ in range(2)]
    for h in hs:
        h.option("fused_gradient", fused)
    a, b, c, d, e, f = hs
    assert a.w == ag.WIDTH[kind]
    carry = None
    for k, u in enumerate(increments(drive, mesh_name)):
        u = np.array(u)
        ud = to_device(u)
        grad = _gradient(mesh, ud, kind)
        got_a, got_b = a.displacement_device(mesh, ud), b.device(grad)
        eps = to_host(grad)
        got_c, got_d = c.displacement_host(mesh, u), d.host(eps)
        assert same(got_a, got_b), f"law {law} {mesh_name} increment {k + 1}: device form"
        assert same(got_c, got_d), f"law {law} {mesh_name} increment {k + 1}: host form"
        assert same(got_a, got_c)                                   # and the two forms with each other: the same launches
        eps_sub = to_host(_gradient(sub, ud, kind))
        assert np.array_equal(bits(eps_sub), bits(eps[rows]))       # the restricted mesh evaluates the same rows
        got_e, got_f = e.displacement_rows(sub, u, rows, n), f.rows(eps_sub, rows, n)
        assert same(got_e, got_f), f"law {law} {mesh_name} increment {k + 1}: rows form"
        assert np.array_equal(bits(got_e[0][rows]), bits(got_a[0][rows])) and np.array_equal(bits(got_e[1][rows]), bits(got_a[1][rows]))
        assert np.all(got_e[0][others] == -7.25) and np.all(got_e[1][others] == -7.25)      # the rows of the other cells keep what they held
        for got in (got_a, got_c):
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and got[3]["n_nan"] == 0 and got[3]["n_points"] == n
        share = got_a[3]["n_plastic"] / n
        print(f"axisymmetric displacement forms law {law} {mesh_name} fused_gradient {fused} increment {k + 1}: n_plastic {got_a[3]['n_plastic']} of {n}")
        assert (0.1 <= share <= 0.9) if yields else share == 0.0
        err_eps = float(np.abs(eps - ag.strain(case, u, kind)).max())
        assert err_eps < BOUND, err_eps
        if law in (26, 27, 28):
            want = reference_update(law, ag.strain(case, u, 0), carry)
            carry = want["carry"]
            s0, Em = LAWS[law]["sig0"], prm[0]
            dev = (np.abs(got_a[0] - want["stress"]).max() / s0, np.abs(got_a[1] - want["tangent"]).max() / Em,
                   (np.abs(got_a[2] - want["state"]).max() / (s0 / Em)) if want["state"].size else 0.0)
            bound = parity_bounds(law)
            print(f"axisymmetric displacement forms law {law} {mesh_name} increment {k + 1} against the numpy restatement on the reference strain: "
                  f"stress {dev[0]:.3e} ({bound[0]:.2e})  tangent {dev[1]:.3e} ({bound[1]:.2e})  state {dev[2]:.3e} ({bound[2]:.2e})")
            assert got_a[3]["n_plastic"] == int(want["plastic"].sum())
            assert all(x <= y for x, y in zip(dev, bound)), (law, mesh_name, k, dev, bound)
        for h in hs:
            h.advance()
    for h in hs:
        h.close()
    mesh.close()
    sub.close()


def test_chunked_host_form_whose_second_chunk_starts_inside_a_cell():
    """tri6 with 3 Gauss points on ``triangle_grid(210)`` at r = x + 1: 264 600 points, which a handle of the full tangent layout cuts
    into two chunks, the second at 132 352 = 1 mod 3, inside a cell.  The gradient kernel fills the whole scratch array first; every
    chunk's update kernel reads its part of it.  Law 27 through ``dxm_integrate_displacement`` equals the strain-array form bit for bit."""
    import tile_loop_cases as tc
    from helpers import triangle_grid

    xv, cells = triangle_grid(210, seed=3)
    mesh, xd = AxisymmetricMesh.lagrange(xv + np.array([ag.SHIFT, 0.0]), cells, degree=2)
    n, nqp = mesh.npoints, 3
    nchunks, csize = tc.plan_chunks(n, False, False, 64)
    assert n == 264600 and (nchunks, csize) == (2, 132352) and csize % nqp == 1
    u = np.ascontiguousarray(((xd - np.array([ag.SHIFT, 0.0])) * pg.STRETCH + 2.5e-3 / 210 * np.random.default_rng(5).standard_normal(xd.shape)).ravel())
    a, b = Handle(27, n, LAWS[27]["prm"]), Handle(27, n, LAWS[27]["prm"])
    got_a = a.displacement_host(mesh, u)
    eps = to_host(_gradient(mesh, to_device(u), 0))
    got_b = b.host(eps)
    print(f"chunked host form law 27 on an axisymmetric mesh: {n} points, {nchunks} chunks of {csize}, n_plastic {got_a[3]['n_plastic']}")
    assert same(got_a, got_b) and 0 < got_a[3]["n_plastic"] < n and got_a[3]["n_nan"] == 0
    for off in range(0, n, csize):          # per chunk as well
        sl = slice(off, min(off + csize, n))
        assert np.array_equal(bits(got_a[0][sl]), bits(got_b[0][sl])) and np.array_equal(bits(got_a[1][sl]), bits(got_b[1][sl]))
    from dolfinx_materials_amd import gradient as gm

    pts = gm.simplex_quadrature(2, 2)
    coords = np.pad(xv, ((0, 0), (0, 1)))
    coords[:, 0] += ag.SHIFT
    case = dict(coords=coords, cells=cells, dofmap=gm.p2_dofmap(cells)[0], geom_phi=gm.lagrange_simplex_values(2, 1, pts),
                geom_dphi=gm.lagrange_simplex_table(2, 1, pts), phi=gm.lagrange_simplex_values(2, 2, pts), dphi=gm.lagrange_simplex_table(2, 2, pts))
    assert np.array_equal(mesh.radii(), ag.radius(case)) and np.abs(eps - ag.strain(case, u, 0)).max() < BOUND
    a.close()
    b.close()
    mesh.close()


def test_laws_an_axisymmetric_mesh_does_not_serve_are_refused_and_the_handle_stays_usable():
    """a plane-stress law (30), the 5-wide Ogden law (38) and a heat-transfer law (35), each with its sentence, through the device and
    the host form; afterwards the handle integrates an array"""
    import heat_plane_ref as hp
    import torch

    lib = _lib.load()
    case = ag.law_mesh("quad4x4")
    mesh = _mesh(case)
    n = mesh.npoints
    u = np.zeros(case["xd"].size)
    ud = to_device(u)
    natural = {30: [0.0, 0.0, 0.0], 38: [1.0, 1.0, 1.0, 0.0, 0.0], 35: [0.0, 0.0]}
    for law, prm, words in ((30, LAWS[30]["prm"], ("plane stress and axisymmetry exclude each other",)),
                            (38, OGDEN, ("takes the 5-wide deformation gradient", "as an array")),
                            (35, list(hp.PARAMS[hp.STATIONARY_2D]), ("carries a displacement (u_r, u_z)", "dxm_mesh_create_plane_scalar"))):
        h = Handle(law, n, prm)
        f, c = h._device_outputs()
        assert lib.dxm_integrate_displacement_device(h.h, mesh._handle, ud.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) < 0
        assert all(w in err(lib) for w in words), (law, err(lib))
        fh, ch = np.full((n, h.w), np.nan), np.full((n, h.nt), np.nan)
        assert lib.dxm_integrate_displacement(h.h, mesh._handle, u.ctypes.data, 0.0, fh.ctypes.data, None, ch.ctypes.data, None) < 0
        assert all(w in err(lib) for w in words), (law, err(lib))
        torch.cuda.synchronize()
        assert bool(torch.isnan(f).all()) and bool(torch.isnan(c).all()) and np.isnan(fh).all() and np.isnan(ch).all()
        grad = to_device(np.ascontiguousarray(np.tile(np.array(natural[law]), (n, 1))))
        got = h.device(grad)                                   # the handle is as it was: the natural state gives no flux
        assert np.abs(got[0]).max() <= 1e-6 and np.isfinite(got[1]).all() and got[3]["n_nan"] == 0 and got[3]["n_points"] == n, law
        h.close()
    # a point-count mismatch, with its sentence
    h = Handle(27, n + 1, LAWS[27]["prm"])
    f, c = h._device_outputs()
    assert lib.dxm_integrate_displacement_device(h.h, mesh._handle, ud.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) < 0
    assert f"mesh has {n} Gauss points, material {n + 1}" in err(lib), err(lib)
    h.close()
    mesh.close()
