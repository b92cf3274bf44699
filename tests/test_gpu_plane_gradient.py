"""GPU: the plane gradient kernels (``csrc/plane_gradient.hip``) against ``plane_gradient_ref`` (an independent numpy restatement,
held to its own longdouble evaluation within 1e-14 by ``test_plane_gradient_ref_cpu.py``), and the displacement forms of the eight
two-dimensional laws (23, 24, 26, 27, 28, 30, 31, 33) against "gradient kernel, then update kernel" bit for bit.

Stand-alone kernels: bound 1e-13 absolute with ``|H| < 0.15`` (the bound and condition of ``test_gpu_gradient_kernels.py``), the four
kinds, a random field and the affine patch field, outputs with 8 rows more than the mesh has points and filled with NaN beforehand.

Observed on an MI355X (largest error per kernel and kind over every mesh and field below; each test prints its own):

==========================================  =========  =========  =========  =========  =========
``plane_gradient_kernel`` on                kind 0     kind 1     kind 2     kind 3     bound
==========================================  =========  =========  =========  =========  =========
quadrilaterals (``PlaneMesh``)              4.3e-16    4.4e-16    4.3e-16    4.3e-16    1e-13
triangles (``PlaneMesh``)                   3.6e-16    4.4e-16    3.6e-16    3.6e-16    1e-13
triangles (``SimplexMesh``)                 (``simplex_gradient_kernel``)  3.6e-16    3.6e-16    1e-13
==========================================  =========  =========  =========  =========  =========

Displacement forms: bit for bit in every case; against the numpy restatements on the reference gradient the largest deviation is
6.4e-15 of the field scale (law 27, stress), each family within the bound of its own GPU test file.  Law 1 on quadrilaterals: 0.0
(bit for bit) where the bound is 1e-13.  Rows form: 9.1e-16 of the field where the bound is 1e-11."""
import ctypes as C

import numpy as np
import pytest

import gradient_ref as gr
import plane_gradient_ref as pg
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd.gradient import PlaneMesh, SimplexMesh, Tet4Mesh
from helpers import to_device, to_host
from plane_laws_2d import LAWS, PARITY_LAWS, increments, parity_bounds, reference_update

pytestmark = pytest.mark.gpu
BOUND = 1e-13      # absolute, |H| < 0.15: the bound of test_gpu_gradient_kernels.py
EXTRA = 8          # rows past the mesh's last point: they keep their NaN


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def _plane_mesh(case):
    return PlaneMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"], case["dphi"])


def _simplex_mesh(case):
    return SimplexMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["dphi"])


def _against_reference(tag, mesh, case, kinds=(0, 1, 2, 3)):
    """the kinds of the mesh's gradient kernel for the random and the patch field; returns {kind: largest error}"""
    import torch

    assert mesh.tdim == 2 and mesh.displacement_size == case["xd"].size
    st = torch.cuda.current_stream().cuda_stream
    worst = {}
    for name in ("random", "patch"):
        u = case["u_" + name]
        H = pg.reference(case, u)
        n = mesh.npoints
        assert n == len(H) and np.abs(H).max() < 0.15
        ud = to_device(np.array(u))
        for kind in kinds:
            ref = pg.rows(H, kind)
            out = torch.full((n + EXTRA, ref.shape[1]), float("nan"), dtype=torch.float64, device="cuda:0")
            mesh.gradient_device(ud.data_ptr(), kind, out.data_ptr(), st)
            torch.cuda.synchronize()
            got = to_host(out)
            assert np.isfinite(got[:n]).all(), f"{tag} {name} kind {kind}: rows left unwritten"
            assert np.isnan(got[n:]).all(), f"{tag} {name} kind {kind}: rows past the last point written"
            e = float(np.abs(got[:n] - ref).max())
            worst[kind] = max(worst.get(kind, 0.0), e)
            print(f"plane gradient kernels {tag} {name} kind {kind}: {n} points, error {e:.3e} (bound {BOUND:.0e})")
            assert e < BOUND
            if kind == 0:
                assert np.all(got[:n, [2, 4, 5]] == 0.0)
            elif kind == 1:
                assert np.all(got[:n, 2] == 1.0) and np.all(got[:n, 5:] == 0.0)
            elif kind == 2:
                assert np.all(got[:n, 2] == 0.0) and not np.signbit(got[:n, 2]).any()      # eps_zz is exactly 0.0
    return worst


@pytest.mark.parametrize("tag", list(pg.QUAD_CASES))
def test_quadrilaterals(tag):
    """Q1 at 1 point per cell (81 points: one ragged block) and at 4 (324: a block boundary inside a cell run), Q2 at 5 arbitrary
    interior points (405) and at 9 Gauss points (729), on the distorted 9 x 9 grid: J differs from point to point."""
    case = pg.quad_case(tag)
    mesh = _plane_mesh(case)
    assert mesh.npoints == {"q1-x1": 81, "q1-x4": 324, "q2-x5": 405, "q2-x9": 729}[tag] and mesh.npoints % 256 != 0
    _against_reference(f"quad {tag}", mesh, case)
    mesh.close()


@pytest.mark.parametrize("rule", gr.SIMPLEX_RULES)
@pytest.mark.parametrize("element", ["p1tri", "p2tri"])
@pytest.mark.parametrize("via", ["simplex", "plane"])
def test_triangles(via, element, rule):
    """``gr.simplex_case`` on ``triangle_grid(7)``: kinds 2 and 3 of an existing ``SimplexMesh`` (its constant geometry table is built
    at creation), and the four kinds of a ``PlaneMesh`` handed the same tables."""
    case = pg.tri_case(element, rule)
    mesh = _simplex_mesh(case) if via == "simplex" else _plane_mesh(case)
    _against_reference(f"tri {via} {element}-{rule}", mesh, case, kinds=(2, 3) if via == "simplex" else (0, 1, 2, 3))
    mesh.close()


def test_kinds_two_and_three_need_a_two_dimensional_mesh_and_kind_four_is_none():
    import torch

    lib = _lib.load()
    coords, conn = gr.tet_mesh()
    tet = Tet4Mesh(coords, conn, nqp=1)
    u = to_device(np.zeros(coords.size))
    out = torch.full((tet.npoints + EXTRA, 9), float("nan"), dtype=torch.float64, device="cuda:0")
    for kind in (2, 3):
        assert lib.dxm_mesh_gradient_device(tet._handle, u.data_ptr(), kind, out.data_ptr(), None) < 0
        assert "two-dimensional meshes only" in err(lib) and "three-dimensional" in err(lib), err(lib)
    case = pg.quad_case("q1-x1")
    quad = _plane_mesh(case)
    u2 = to_device(np.zeros(case["xd"].size))
    for mesh, ud in ((tet, u), (quad, u2)):
        for kind in (4, -1):
            assert lib.dxm_mesh_gradient_device(mesh._handle, ud.data_ptr(), kind, out.data_ptr(), None) < 0
            assert "gradient kind must be 0 (strain), 1 (F), 2 (plane-strain 4-vector) or 3 (in-plane 3-vector)" in err(lib), err(lib)
        with pytest.raises(_lib.DxmError):
            mesh.gradient_device(ud.data_ptr(), 4, out.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                       # a refused call wrote nothing
    tet.close()
    quad.close()


# ---- the displacement forms of the two-dimensional laws ---------------------------------------------------------------------------------
class Handle:
    """one dxm_material of a two-dimensional law, driven through ctypes alone"""

    def __init__(self, law, n, prm=None):
        p = [float(v) for v in (LAWS[law]["prm"] if prm is None else prm)]
        self.lib, self.n, self.law = _lib.load(), n, law
        self.h = self.lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        info = _lib.law_info(law)
        self.w, self.nt = info.n_grad, self.lib.dxm_tangent_size(self.h)
        self.fields = LAWS[law]["fields"] if law in LAWS else ()

    def state(self, which=_lib.S1):
        out = []
        for f, dim in enumerate(self.fields):
            a = np.full((self.n, dim), np.nan)
            assert self.lib.dxm_get_state(self.h, which, f, a.ctypes.data) == 0, err(self.lib)
            out.append(a)
        return np.concatenate(out, axis=1) if out else np.zeros((self.n, 0))

    def stats(self):
        st = _lib.Stats()
        assert self.lib.dxm_get_stats(self.h, C.byref(st)) >= 0, err(self.lib)
        return st.as_dict()

    def _device_outputs(self):
        import torch

        new = lambda cols: torch.full((self.n, cols), float("nan"), dtype=torch.float64, device="cuda:0")   # noqa: E731
        return new(self.w), new(self.nt)

    def displacement_device(self, mesh, ud):
        import torch

        f, c = self._device_outputs()
        assert self.lib.dxm_integrate_displacement_device(self.h, mesh._handle, ud.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.state(), self.stats()

    def device(self, grad):
        import torch

        f, c = self._device_outputs()
        assert self.lib.dxm_integrate_device(self.h, grad.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.state(), self.stats()

    def displacement_host(self, mesh, u):
        f, c, st = np.full((self.n, self.w), np.nan), np.full((self.n, self.nt), np.nan), _lib.Stats()
        rc = self.lib.dxm_integrate_displacement(self.h, mesh._handle, u.ctypes.data, 0.0, f.ctypes.data, None, c.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()

    def host(self, eps):
        f, c, st = np.full((self.n, self.w), np.nan), np.full((self.n, self.nt), np.nan), _lib.Stats()
        rc = self.lib.dxm_integrate(self.h, eps.ctypes.data, 0.0, f.ctypes.data, None, c.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def advance(self):
        assert self.lib.dxm_advance(self.h) == 0, err(self.lib)

    def close(self):
        self.lib.dxm_destroy(self.h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[:3], b[:3])) and a[3]["n_plastic"] == b[3]["n_plastic"] and a[3]["n_nan"] == b[3]["n_nan"]


def _law_mesh(name):
    case = pg.law_mesh(name)
    return (_simplex_mesh(case) if name == "tri6x3" else _plane_mesh(case)), case


def _gradient(mesh, ud, kind):
    import torch

    grad = torch.full((mesh.npoints, pg.WIDTH[kind]), float("nan"), dtype=torch.float64, device="cuda:0")
    mesh.gradient_device(ud.data_ptr(), kind, grad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return grad


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("mesh_name", pg.LAW_MESHES)
@pytest.mark.parametrize("law", sorted(LAWS))
def test_displacement_forms_equal_gradient_then_update_bit_for_bit(law, mesh_name, fused):
    """``dxm_integrate_displacement_device`` against ``dxm_mesh_gradient_device(kind)`` -> ``dxm_integrate_device``, and
    ``dxm_integrate_displacement`` against ``dxm_integrate`` on the downloaded gradient: the same kernels, arrays and grids, so stress,
    tangent and state agree bit for bit, over two increments with an advance between, at both settings of ``fused_gradient`` (which
    makes no difference: these laws have no fused form).  tri6 x 3 through ``SimplexMesh``, quad4 x 4 through ``PlaneMesh``."""
    spec = LAWS[law]
    mesh, case = _law_mesh(mesh_name)
    n = mesh.npoints
    hs = [Handle(law, n) for _ in range(4)]
    for h in hs:
        h.option("fused_gradient", fused)
    a, b, c, d = hs
    carry = None
    for k, u in enumerate(increments(law, mesh_name)):
        ud = to_device(np.array(u))
        grad = _gradient(mesh, ud, spec["kind"])
        got_a, got_b = a.displacement_device(mesh, ud), b.device(grad)
        eps = to_host(grad)
        got_c, got_d = c.displacement_host(mesh, np.array(u)), d.host(eps)
        assert same(got_a, got_b), f"law {law} {mesh_name} increment {k + 1}: device form"
        assert same(got_c, got_d), f"law {law} {mesh_name} increment {k + 1}: host form"
        assert same(got_a, got_c)                                   # and the two forms with each other: the same launches
        for got in (got_a, got_c):
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and got[3]["n_nan"] == 0 and got[3]["n_points"] == n
        share = got_a[3]["n_plastic"] / n
        print(f"displacement forms law {law} {mesh_name} fused_gradient {fused} increment {k + 1}: n_plastic {got_a[3]['n_plastic']} of {n}")
        assert (0.1 <= share <= 0.9) if spec["yields"] else share == 0.0
        if law in PARITY_LAWS:
            want = reference_update(law, pg.rows(pg.reference(case, u), spec["kind"]), carry)
            carry = want["carry"]
            s0, Em = spec["sig0"], spec["prm"][0]
            dev = (np.abs(got_a[0] - want["stress"]).max() / s0, np.abs(got_a[1] - want["tangent"]).max() / Em,
                   np.abs(got_a[2] - want["state"]).max() / (s0 / Em))
            bound = parity_bounds(law)
            print(f"displacement forms law {law} {mesh_name} increment {k + 1} against the numpy restatement on the reference gradient: "
                  f"stress {dev[0]:.3e} ({bound[0]:.2e})  tangent {dev[1]:.3e} ({bound[1]:.2e})  state {dev[2]:.3e} ({bound[2]:.2e})")
            assert got_a[3]["n_plastic"] == int(want["plastic"].sum())
            assert all(x <= y for x, y in zip(dev, bound)), (law, mesh_name, k, dev, bound)
        for h in hs:
            h.advance()
    for h in hs:
        h.close()
    mesh.close()


def _chunk_mesh(size):
    """``gradient_ref.chunk_case("tri6x3")`` (66 150 points), or the same construction on ``triangle_grid(210)`` (264 600 points)"""
    if size == "66150":
        return gr.chunk_case("tri6x3")
    from dolfinx_materials_amd.gradient import lagrange_simplex_table, p2_dofmap, simplex_quadrature
    from helpers import triangle_grid

    xv, cells = triangle_grid(210, seed=3)
    dofmap, n_dofs, edges = p2_dofmap(cells)
    xd = np.concatenate([xv, 0.5 * (xv[edges[:, 0]] + xv[edges[:, 1]])], axis=0)
    u = xd * pg.STRETCH + 2.5e-3 / 210 * np.random.default_rng(5).standard_normal(xd.shape)
    return dict(coords=np.ascontiguousarray(np.pad(xv, ((0, 0), (0, 1)))), cells=cells, dofmap=np.ascontiguousarray(dofmap, dtype=np.int32),
                n_dofs=n_dofs, dphi=lagrange_simplex_table(2, 2, simplex_quadrature(2, 2)), nqp=3, npoints=3 * len(cells), u=u.ravel())


@pytest.mark.parametrize("size", ["66150", "264600"])
@pytest.mark.parametrize("law", [27, 30])
def test_chunked_host_form_whose_second_chunk_starts_inside_a_cell(law, size):
    """``gradient_ref.chunk_case("tri6x3")``, 66 150 points: where the fused 6-wide laws are cut into chunks from 65 536 points on, a
    handle of the full tangent layout -- the only one these laws have -- is cut from 262 144 on (``plan_chunks``: 131 072 points per
    chunk), so that mesh runs as ONE chunk here.  The same construction on ``triangle_grid(210)`` has 264 600 points: two chunks, the
    second at 132 352 = 1 mod 3, inside a cell.  The gradient kernel fills the whole scratch array first; every chunk's update
    kernel reads its part of it.  Law 27 and law 30 through ``dxm_integrate_displacement`` equal the strain-array form bit for bit."""
    import tile_loop_cases as tc

    case = _chunk_mesh(size)
    n, nqp = case["npoints"], case["nqp"]
    nchunks, csize = tc.plan_chunks(n, False, False, 64)
    assert n == int(size) and (nchunks, csize) == {"66150": (1, 66304), "264600": (2, 132352)}[size] and (nchunks == 1 or csize % nqp == 1)
    mesh = _simplex_mesh(case)
    a, b = Handle(law, n), Handle(law, n)
    u = np.array(case["u"])
    got_a = a.displacement_host(mesh, u)
    eps = to_host(_gradient(mesh, to_device(u), LAWS[law]["kind"]))
    got_b = b.host(eps)
    print(f"chunked host form law {law}: {n} points, {nchunks} chunk(s) of {csize}, n_plastic {got_a[3]['n_plastic']}")
    assert same(got_a, got_b) and 0 < got_a[3]["n_plastic"] < n and got_a[3]["n_nan"] == 0
    for off in range(0, n, csize):          # per chunk as well
        sl = slice(off, min(off + csize, n))
        assert np.array_equal(bits(got_a[0][sl]), bits(got_b[0][sl])) and np.array_equal(bits(got_a[1][sl]), bits(got_b[1][sl]))
    ref = pg.rows(pg.plane_gradient(case["coords"], case["cells"], case["dofmap"], u, gr.p1_table(2, nqp), case["dphi"]), LAWS[law]["kind"])
    assert np.abs(eps - ref).max() < BOUND
    a.close()
    b.close()
    mesh.close()


def test_rows_form_through_a_map_over_every_second_cell():
    """A ``QuadratureFieldMap`` over every second cell of the quadrilateral grid with ``register_device_gradient`` and a ``PlaneMesh``
    restricted to those cells: law 27 over three load steps against the same map fed with host-evaluated strains, within the bound of
    the rows path in ``tests/test_gpu_quadrature_map.py`` (1e-11 of the field); the rows of the other cells keep what they held."""
    import dolfinx_materials_amd.materials as jm
    from dolfinx_materials_amd.field_map import QuadratureFieldMap
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    case = pg.law_mesh("quad4x4")
    ncell, nqp = len(case["cells"]), case["dphi"].shape[0]
    cells = np.arange(0, ncell, 2, dtype=np.int32)
    others = np.setdiff1d(np.arange(ncell), cells)
    prm = LAWS[27]["prm"]
    behaviour = lambda: jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=prm[0], nu=prm[1]), jm.LinearHardening(prm[2], prm[3]),   # noqa: E731
                                                      hypothesis="plane_strain")
    now = {}

    def strain(c):
        H = pg.plane_gradient(case["coords"], case["cells"][c], case["dofmap"][c], now["u"], case["geom_dphi"], case["dphi"])
        return pg.rows(H, 2)

    SENTINEL = -7.25
    fields = {}
    for route in ("host", "device"):
        mat = JAXMaterial(behaviour())
        assert mat.gradients == {next(iter(mat.gradients)): 4}
        q = QuadratureFieldMap(ncell, nqp, mat, cells=cells)
        q.register_gradient(next(iter(mat.gradients)), strain)
        if route == "device":
            sub = PlaneMesh(case["coords"], case["cells"][cells], case["dofmap"][cells], case["n_dofs"], case["geom_dphi"], case["dphi"])
            q.register_device_gradient(sub, lambda: now["u"])
            assert q._accel_plan().row_outputs
        arrays = {**{k: f.x.array for k, f in q.fluxes.items()}, "jacobian": q.jacobian_flatten.x.array}
        for a in arrays.values():
            a.reshape(ncell, -1)[others] = SENTINEL
        for t in (0.42, 0.56, 0.7):
            now["u"] = pg.stretch_field("quad4x4", t=t)
            q.update()
            q.advance()
        arrays.update({k: f.x.array for k, f in q.internal_state_variables.items()})
        fields[route] = {k: np.array(v) for k, v in arrays.items()}
        for k in ("jacobian", *q.fluxes):
            assert np.all(fields[route][k].reshape(ncell, -1)[others] == SENTINEL), (route, k)       # untouched rows stay untouched
        assert mat.last_stats["n_plastic"] > 0
        q.close()
        mat.close()
        if route == "device":
            sub.close()
    for name, host in fields["host"].items():
        e = float(np.abs(fields["device"][name] - host).max() / max(np.abs(host).max(), 1e-300))
        print(f"rows form law 27 {name}: {e:.3e} (bound 1e-11)")
        assert e <= 1e-11, name
    assert np.abs(fields["host"]["p"]).max() > 0


@pytest.mark.parametrize("fused", [1, 0])
def test_a_six_wide_law_on_quadrilaterals(fused):
    """Law 1 (6-wide J2, linear hardening) on the quad4 x 4 mesh through ``dxm_integrate_displacement`` (kind 0 of the plane kernel,
    then the update kernel: a plane mesh has no fused form) against ``dxm_integrate`` on ``conventions.embed_plane_strain`` of the
    kind-2 gradient, within 1e-13 relative: the same arithmetic up to contraction of the gradient kernel."""
    mesh, case = _law_mesh("quad4x4")
    n = mesh.npoints
    prm = LAWS[27]["prm"]
    a, b = Handle(_lib.LAW_J2_LINEAR, n, prm), Handle(_lib.LAW_J2_LINEAR, n, prm)
    a.option("fused_gradient", fused)
    for k, u in enumerate(increments(27, "quad4x4")):
        got = a.displacement_host(mesh, np.array(u))
        eps6 = np.ascontiguousarray(conventions.embed_plane_strain(to_host(_gradient(mesh, to_device(np.array(u)), 2))))
        want = b.host(eps6)
        ef = float(np.abs(got[0] - want[0]).max() / np.abs(want[0]).max())
        ec = float(np.abs(got[1] - want[1]).max() / np.abs(want[1]).max())
        print(f"6-wide law on quadrilaterals fused_gradient {fused} increment {k + 1}: n_plastic {got[3]['n_plastic']} of {n}, flux {ef:.3e} tangent {ec:.3e} (bound 1e-13)")
        assert ef <= 1e-13 and ec <= 1e-13 and got[3]["n_plastic"] == want[3]["n_plastic"] and 0 < got[3]["n_plastic"] < n
        a.advance()
        b.advance()
    a.close()
    b.close()
    mesh.close()
