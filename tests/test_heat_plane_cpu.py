"""CPU: the two-dimensional heat-transfer laws (DXM_LAW_HEAT_STATIONARY_2D = 35, DXM_LAW_HEAT_PHASE_CHANGE_2D = 36), the scalar plane
mesh and the nodal forms, without a GPU: the C boundary (ids, tables, symbols), every host-side check of
``dxm_mesh_create_plane_scalar`` in its order, the Python classes, the value tables, the numpy restatement ``heat_plane_ref`` against
its own ``longdouble`` evaluation, the conditions the GPU tests rest on, and a ``QuadratureFieldMap`` run over the CPU double.

THE FIGURE THE GPU BOUND IS BUILT FROM (``test_restatement_is_held_to_its_longdouble_evaluation``): the largest float64-against-
longdouble error of ``heat_plane_ref.reference`` over every mesh and field of ``test_gpu_heat_plane_nodal.py``, in units of
``2^-53 S`` with ``S = sum_m |T_m| (|phi_m| + sum_d |(dphi_m Ji)_d|)`` per point.  Recorded: 0.070 (value) and 3.116 (gradient; the
random field on the distorted Q2 grid with 9 points -- S bounds the two sums, not the cancellation inside ``dphi Ji`` and ``det J``,
which is why the figure exceeds 1).  ``RECORDED_MULTIPLE = 3.2`` is that figure rounded up and is asserted here; the GPU bound is
4 x that, 12.8."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd import gradient as gm
from dolfinx_materials_amd.field_map import QuadratureFieldMap, evaluate_block
from dolfinx_materials_amd.jaxmat import JAXMaterial

import heat_plane_ref as hp
import heat_transfer_ref as ht
import plane_gradient_ref as pg
from fake_dxmat_heat_plane import FakeDxmatHeatPlane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dolfinx_materials_amd", "csrc")
#: float64 against longdouble of the restatement, in units of 2^-53 S: the bound asserted below; the GPU tests allow 4 x this
RECORDED_MULTIPLE = 3.2


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def test_ids_35_and_36_are_known_and_34_and_37_are_not():
    assert (_lib.LAW_HEAT_STATIONARY_2D, _lib.LAW_HEAT_PHASE_CHANGE_2D) == (35, 36)
    i = _lib.law_info(35)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (2, 2, 2, 0, 0, 64)
    i = _lib.law_info(36)
    assert (i.n_grad, i.n_flux, i.n_params, i.n_isv_fields, i.n_isv_total, i.algorithmic_bytes_per_point) == (2, 2, 7, 1, 1, 80)
    assert i.isv_name[0].decode() == "Enthalpy" and i.isv_dim[0] == 1
    for law in (34, 37):
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_info(law)
        with pytest.raises(_lib.DxmError, match=f"unknown law id {law}"):
            _lib.law_blocks(law)
    assert _lib.load().dxm_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "dxmat.h")).read()
    assert "DXM_LAW_HEAT_STATIONARY_2D = 35," in header and "DXM_LAW_HEAT_PHASE_CHANGE_2D = 36," in header and "DXM_LAW_COUNT = 37\n" in header
    assert "#define DXM_ABI_VERSION 6" in header


def test_law_blocks_of_the_two_laws():
    def blocks(law):
        b = _lib.law_blocks(law)
        return b, [(k.row_kind, k.row_index, k.col_kind, k.col_index, k.rows, k.cols) for k in list(b.block)[: b.n_blocks]]

    b, bl = blocks(35)
    assert (b.n_external, b.n_blocks, b.tangent_width) == (1, 2, 6) and b.external_name[0] == b"Temperature" and b.external_default[0] == 293.15
    assert bl == [(0, 0, 0, 0, 2, 2), (0, 0, 1, 0, 2, 1)]
    b, bl = blocks(36)
    assert (b.n_external, b.n_blocks, b.tangent_width) == (1, 3, 7) and b.external_name[0] == b"Temperature"
    assert bl == [(0, 0, 0, 0, 2, 2), (0, 0, 1, 0, 2, 1), (1, 0, 1, 0, 1, 1)]


def test_both_symbols_are_declared_bound_and_exported_and_the_launchers_hidden():
    hdr = open(os.path.join(ROOT, "include", "dxmat.h")).read()
    assert re.search(r"dxm_mesh\* dxm_mesh_create_plane_scalar\(const double\* coords, int64_t n_vertices, const int32_t\* geom_conn, int nv,", hdr)
    assert re.search(r"int dxm_mesh_scalar_gradient_device\(dxm_mesh\* mesh, const double\* t_dev, double\* grad_dev, double\* value_dev,", hdr)
    assert len(_lib.SYMBOLS["dxm_mesh_create_plane_scalar"][1]) == 13 and len(_lib.SYMBOLS["dxm_mesh_scalar_gradient_device"][1]) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dolfinx_materials_amd", "libdxmat.so")], capture_output=True, text=True).stdout
    for name in ("dxm_mesh_create_plane_scalar", "dxm_mesh_scalar_gradient_device"):
        assert re.search(rf"\sT\s+{name}$", out, flags=re.M), name
    exported = "\n".join(ln for ln in out.splitlines() if " T " in ln)
    for hidden in ("heat_plane_launch", "scalar_gradient_launch", "heat_plane_stationary_kernel_fn", "heat_plane_phase_change_kernel_fn"):
        assert hidden not in exported, hidden
    # the rows are the descriptor's, not an `if` on law ids; dxmat.hip names no kernel of the unit outside a string
    src = open(os.path.join(CSRC, "dxmat.hip")).read()
    assert "bool nodal_scalar;" in src[src.index("struct LawDesc {"):src.index("constexpr int ct_full_of")]
    assert src.count("d.nodal_scalar = true;") == 1 and "!kLaws[34].kernel" in src
    assert "law_ps_hosford(),\n    {}, law_heat_stationary_2d(), law_heat_phase_change_2d()," in src
    code = re.sub(r'"[^"]*"', "", src)
    assert "heat_plane_kernel<" not in code and "scalar_gradient_kernel" not in code and '#include "heat_plane.hpp"' in src
    body = src[src.index("static int integrate_nodal_host("):src.index("static int integrate_displacement_host(")]
    assert "DXM_LAW_" not in re.sub(r'"[^"]*"', "", body)


# ---- the constructor's host-side checks -------------------------------------------------------------------------------------------------
def _create(lib, case, **over):
    a = dict(coords=case["coords"], n_vertices=len(case["coords"]), conn=np.ascontiguousarray(case["cells"], dtype=np.int32),
             nv=case["cells"].shape[1], n_cells=len(case["cells"]), dofmap=case["dofmap"], nd=case["dofmap"].shape[1], n_dofs=case["n_dofs"],
             gd=case["geom_dphi"], phi=case["phi"], dphi=case["dphi"], nqp=case["dphi"].shape[0], device=0)
    a.update(over)
    keep = [np.ascontiguousarray(a[k]) for k in ("coords", "conn", "dofmap", "gd", "phi", "dphi")]
    ptr = [k.ctypes.data for k in keep]
    return lib.dxm_mesh_create_plane_scalar(ptr[0], a["n_vertices"], ptr[1], a["nv"], a["n_cells"], ptr[2], a["nd"], a["n_dofs"], ptr[3], ptr[4],
                                            ptr[5], a["nqp"], a["device"])


def test_host_side_checks_of_the_scalar_constructor_in_their_order():
    """arguments, then the tables, then indices, then det J, then the device: the sentences of dxm_mesh_create_plane, none needing a GPU"""
    lib = _lib.load()
    case = hp.quad_case("q1-x4")
    for nv in (2, 5, 8):
        assert not _create(lib, case, nv=nv) and "nv = 3 (triangles) or nv = 4 (bilinear quadrilaterals)" in err(lib), err(lib)
    for over in (dict(nd=3), dict(nd=65), dict(nqp=0), dict(nqp=65), dict(n_cells=0), dict(n_dofs=0), dict(n_vertices=0)):
        assert not _create(lib, case, **over) and "invalid plane mesh arguments" in err(lib), (over, err(lib))
    assert not lib.dxm_mesh_create_plane_scalar(None, 4, None, 4, 1, None, 4, 4, None, None, None, 1, 0) and "invalid plane mesh arguments" in err(lib)
    # a table entry that is not finite: after the arguments, before the indices
    bad = case["cells"].copy()
    bad[40, 2] = 100
    for name, key, at in (("phi", "phi", (2, 1)), ("dphi", "dphi", (1, 3, 0)), ("geom_dphi", "gd", (3, 0, 1))):
        tab = np.array(case["geom_dphi"] if key == "gd" else case[key])
        tab[at] = np.nan
        flat = int(np.ravel_multi_index(at, tab.shape))
        assert not _create(lib, case, conn=bad, **{key: tab}) and f"table {name}: entry {flat} is not finite" in err(lib), err(lib)
    # indices: the geometry's, then the field's; a bad cell after
    assert not _create(lib, case, conn=bad) and "geometry connectivity entry 162 out of range" in err(lib), err(lib)
    bad[40, 2] = -1
    assert not _create(lib, case, conn=bad) and "geometry connectivity entry 162 out of range" in err(lib), err(lib)
    dm = case["dofmap"].copy()
    dm[80, 3] = case["n_dofs"]
    assert not _create(lib, case, dofmap=dm) and "dofmap entry 323 out of range" in err(lib), err(lib)
    bow = case["cells"].copy()
    bow[17, [2, 3]] = bow[17, [3, 2]]                       # a bow-tie quadrilateral
    assert not _create(lib, case, dofmap=dm, conn=bow) and "dofmap entry 323 out of range" in err(lib)   # indices before det J
    assert not _create(lib, case, conn=bow) and "cell 17 is " in err(lib) and "det J" in err(lib), err(lib)
    flat = case["coords"].copy()
    flat[case["cells"][5]] = flat[case["cells"][5, 0]]       # a cell of zero area
    assert not _create(lib, case, coords=flat) and "cell 5 is degenerate" in err(lib), err(lib)
    nan = case["coords"].copy()
    nan[case["cells"][80, 3], 0] = np.nan
    assert not _create(lib, case, coords=nan) and "cell 80 is degenerate" in err(lib), err(lib)
    tri = hp.tri_case("p1tri", "deg2")
    flip = tri["cells"].copy()
    flip[::2] = flip[::2][:, [0, 2, 1]]
    have_gpu = _lib.device_count() > 0
    for c, over in ((case, {}), (tri, {}), (tri, dict(conn=flip, dofmap=flip))):
        h = _create(lib, c, **over)
        if have_gpu:
            assert h, err(lib)
            assert lib.dxm_mesh_npoints(h) == c["npoints"] and lib.dxm_mesh_displacement_size(h) == c["n_dofs"]     # ONE value per dof
            lib.dxm_mesh_destroy(h)
        else:
            assert not h and "no usable HIP device" in err(lib), err(lib)       # last: every check above came first


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def test_hypothesis_keyword_of_the_two_behaviours():
    s = jm.StationaryHeatTransfer(hypothesis="plane_strain")
    assert (s.law, s.ngrad, s.nflux, s.hypothesis) == (35, 2, 2, "plane_strain") and s.params() == [0.0375, 2.165e-4]
    p = jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0}, hypothesis="plane_strain")
    assert (p.law, p.ngrad, p.nflux) == (36, 2, 2) and p.params()[6] == 1.0
    assert jm.StationaryHeatTransfer.from_mfront_properties({"A": 1.0}, hypothesis="plane_strain").law == 35
    # the default is what it was
    d, e = jm.StationaryHeatTransfer(), jm.HeatTransferPhaseChange()
    assert (d.law, d.ngrad, d.nflux, e.law, e.ngrad, e.nflux) == (16, 3, 3, 17, 3, 3)
    assert jm.StationaryHeatTransfer.law == 16 and jm.HeatTransferPhaseChange.law == 17 and jm.HeatTransferBehavior.ngrad == 3
    assert d.flat_properties() == {"A": 0.0375, "B": 2.165e-4} and jm.StationaryHeatTransfer.from_mfront_properties().law == 16
    for cls in (jm.StationaryHeatTransfer, jm.HeatTransferPhaseChange):
        with pytest.raises(NotImplementedError, match="axisymmetric"):
            cls(hypothesis="axisymmetric")
        with pytest.raises(NotImplementedError, match="axisymmetric"):
            cls.from_mfront_properties({}, hypothesis="axisymmetric")
        with pytest.raises(ValueError, match="hypothesis must be one of"):
            cls(hypothesis="plane_stress")


def test_material_surface_of_the_plane_strain_hypothesis():
    m = JAXMaterial(jm.HeatTransferPhaseChange(hypothesis="plane_strain"))
    assert m.gradients == {"TemperatureGradient": 2} and m.fluxes == {"HeatFlux": 2} and m.internal_state_variables == {"Enthalpy": 1}
    assert m.external_state_variables == {"Temperature": 1}
    assert m.tangent_blocks == {("HeatFlux", "TemperatureGradient"): (2, 2), ("HeatFlux", "Temperature"): (2, 1), ("Enthalpy", "Temperature"): (1, 1)}
    assert list(m.tangent_blocks) == [("HeatFlux", "TemperatureGradient"), ("HeatFlux", "Temperature"), ("Enthalpy", "Temperature")]
    assert m.tangent_size == 7 and m.algorithmic_bytes_per_point == 80
    s = JAXMaterial(jm.StationaryHeatTransfer(hypothesis="plane_strain"))
    assert s.tangent_blocks == {("HeatFlux", "TemperatureGradient"): (2, 2), ("HeatFlux", "Temperature"): (2, 1)} and s.tangent_size == 6
    assert s.algorithmic_bytes_per_point == 64
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="no packed tangent record"):
            JAXMaterial(jm.StationaryHeatTransfer(hypothesis="plane_strain"), tangent_layout=layout)
    assert JAXMaterial(jm.StationaryHeatTransfer()).tangent_size == 12


def test_python_constructor_checks_and_the_mesh_surface():
    case = hp.quad_case("q2-x9")
    args = (case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"], case["phi"], case["dphi"])
    with pytest.raises(ValueError, match="phi must be"):
        gm.PlaneScalarMesh(*args[:5], case["phi"][:, :4], case["dphi"])
    with pytest.raises(ValueError, match="geom_dphi must be"):
        gm.PlaneScalarMesh(*args[:4], case["geom_dphi"][:4], case["phi"], case["dphi"])
    with pytest.raises(ValueError, match="dphi must be"):
        gm.PlaneScalarMesh(case["coords"], case["cells"], case["dofmap"][:, :4], case["n_dofs"], case["geom_dphi"], case["phi"], case["dphi"])
    xv, cells = pg.quad_grid()
    with pytest.raises(ValueError, match="degree 1 or 2"):
        gm.PlaneScalarMesh.lagrange(xv, cells, degree=3)
    assert gm.PlaneScalarMesh.tdim == 2 and gm.PlaneScalarMesh.nodal_variable == "Temperature" and not hasattr(gm.PlaneMesh, "nodal_variable")
    assert callable(gm.PlaneScalarMesh.from_dolfinx) and callable(gm.PlaneScalarMesh.scalar_gradient_device)
    if _lib.device_count() > 0:
        return          # a GPU is present: test_gpu_heat_plane_nodal.py builds these meshes
    bow = cells.copy()
    bow[3, [2, 3]] = bow[3, [3, 2]]
    with pytest.raises(_lib.DxmError, match="dxm_mesh_create_plane_scalar failed: cell 3 is "):
        gm.PlaneScalarMesh.lagrange(xv, bow, degree=2)
    with pytest.raises(_lib.DxmError, match="no usable HIP device"):
        gm.PlaneScalarMesh(*args)


# ---- the value tables ---------------------------------------------------------------------------------------------------------------------
def _quadratic(x):
    return 2.0 + 0.5 * x[:, 0] - 1.5 * x[:, 1] + 0.75 * x[:, 0] ** 2 - 0.25 * x[:, 0] * x[:, 1] + 1.25 * x[:, 1] ** 2


def test_value_tables_sum_to_one_their_derivatives_to_zero_and_reproduce_what_they_should():
    rng = np.random.default_rng(4)
    qpts = rng.uniform(0.0, 1.0, (11, 2))
    spts = pg.gr.interior_points_simplex(2, 11, seed=9)
    q2_nodes = np.array([[(0.0, 1.0, 0.5)[i], (0.0, 1.0, 0.5)[j]] for i, j in gm._Q2_NODES])
    p2_nodes = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0, 0.5], [0.5, 0]], dtype=float)       # vertices, then BASIX_EDGES midpoints
    bilinear = lambda x: 1.0 + 2.0 * x[:, 0] - 3.0 * x[:, 1] + 4.0 * x[:, 0] * x[:, 1]   # noqa: E731
    affine = lambda x: 1.0 + 2.0 * x[:, 0] - 3.0 * x[:, 1]                                # noqa: E731
    cases = [(gm.lagrange_quad_values(1, qpts), gm.lagrange_quad_table(1, qpts), q2_nodes[:4], qpts, bilinear),
             (gm.lagrange_quad_values(2, qpts), gm.lagrange_quad_table(2, qpts), q2_nodes, qpts, _quadratic),
             (gm.lagrange_simplex_values(2, 1, spts), gm.lagrange_simplex_table(2, 1, spts), p2_nodes[:3], spts, affine),
             (gm.lagrange_simplex_values(2, 2, spts), gm.lagrange_simplex_table(2, 2, spts), p2_nodes, spts, _quadratic)]
    for phi, dphi, nodes, pts, f in cases:
        assert phi.shape == dphi.shape[:2] == (len(pts), len(nodes))
        assert np.abs(phi.sum(axis=1) - 1.0).max() <= 4e-16 * len(nodes) and np.abs(dphi.sum(axis=1)).max() <= 2e-15 * len(nodes)
        assert np.abs(phi @ f(nodes) - f(pts)).max() <= 1e-14                        # Q1: bilinear; P1: affine; Q2, P2: a full quadratic
        # the Kronecker property at the nodes themselves
        at = gm.lagrange_quad_values(1 if len(nodes) == 4 else 2, nodes) if len(nodes) in (4, 9) else gm.lagrange_simplex_values(2, 1 if len(nodes) == 3 else 2, nodes)
        assert np.abs(at - np.eye(len(nodes))).max() <= 1e-15
    # what they must NOT reproduce: P1 / Q1 miss the quadratic
    assert np.abs(cases[0][0] @ _quadratic(q2_nodes[:4]) - _quadratic(qpts)).max() > 1e-3
    with pytest.raises(ValueError, match="degree 1 or 2"):
        gm.lagrange_quad_values(3, qpts)
    with pytest.raises(ValueError, match="degree 1 or 2"):
        gm.lagrange_simplex_values(2, 3, spts)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_held_to_its_longdouble_evaluation():
    worst = {"value": 0.0, "grad": 0.0}
    for tag, case in hp.all_cases():
        for name, t in zip(("random", "affine"), hp.nodal_fields(case)):
            v, g, S = hp.reference(case, t)
            vl, gl, Sl = hp.reference(case, t, np.longdouble)
            ev = float(np.max(np.abs(v - vl) / (hp.U * Sl)))
            eg = float(np.max(np.abs(g - gl).max(axis=1) / (hp.U * Sl)))
            print(f"heat_plane_ref {tag} {name}: value {ev:.3f}, gradient {eg:.3f} x 2^-53 S")
            worst["value"], worst["grad"] = max(worst["value"], ev), max(worst["grad"], eg)
            assert np.abs(S - Sl).max() <= 1e-13 * Sl.max()
            if name == "affine":      # grad(T) is the constant, T the field itself, to rounding
                assert np.abs(g - np.array(hp.AFFINE[1:])).max() <= 4 * RECORDED_MULTIPLE * hp.U * S.max()
                X = np.einsum("cva,qv->cqa", case["coords"][case["cells"]][:, :, :2], _geometry_values(case)).reshape(-1, 2)
                assert np.abs(v - (hp.AFFINE[0] + X @ np.array(hp.AFFINE[1:]))).max() <= 1e-12 * 1000.0
    print(f"heat_plane_ref: largest float64-vs-longdouble error {worst['value']:.3f} (value), {worst['grad']:.3f} (gradient) x 2^-53 S")
    assert max(worst.values()) <= RECORDED_MULTIPLE, worst


def _geometry_values(case):
    """values of the geometry's first-order shape functions at the case's points (the physical position of a Gauss point)"""
    nv = case["cells"].shape[1]
    nqp = case["phi"].shape[0]
    if nv == 4:
        tag = [t for t in hp.QUAD_TAGS if hp.quad_case(t) is case][0]
        return gm.lagrange_quad_values(1, pg._quad_points(pg.QUAD_CASES[tag][1]))
    (e, r), = [k for k in hp.TRI_TAGS if hp.tri_case(*k) is case]
    assert nqp == len(pg.gr.simplex_points(2, r))
    return gm.lagrange_simplex_values(2, 1, pg.gr.simplex_points(2, r))


def test_two_wide_restatement_is_the_three_wide_one_on_the_padded_gradient():
    for law in hp.LAWS_2D:
        g, T = hp.inputs(law, 257, seed=5)
        out, wide = hp.update(law, g, T, hp.PARAMS[law]), ht.update(hp.WIDE[law], hp.pad(g), T, hp.PARAMS[law])
        assert out["flux"].shape == (257, 2) and out["tangent"].shape == (257, hp.WIDTH[law]) and out["n_nan"] == 0
        assert np.array_equal(out["tangent"][:, 0], out["tangent"][:, 3]) and not out["tangent"][:, [1, 2]].any()
        assert np.array_equal(out["tangent"][:, 4:6], wide["tangent"][:, 9:11]) and not wide["tangent"][:, 11].any() and not wide["flux"][:, 2].any()


def test_conditions_the_gpu_tests_rest_on():
    """law 36: at least a tenth of the points solid, in the transition and liquid -- the array inputs at every size from 63 on, the
    interpolated nodal field on both law meshes; and the chunk plan of the chunked host case"""
    import tile_loop_cases as tl

    for n in (63, 64, 65, 257, tl.size_for(256, 1), tl.size_for(304, 1)):
        shares = hp.branch_shares(hp.inputs(hp.PHASE_CHANGE_2D, n, seed=100 + n)[1], hp.PARAMS[hp.PHASE_CHANGE_2D])
        assert min(shares) >= 0.1, (n, shares)
    for name in pg.LAW_MESHES:
        case = hp.law_mesh(name)
        for scale in (1.0, -1.0):       # the two updates of the nodal tests: the ramp and its mirror image
            t = 933.15 + scale * (hp.phase_field(case) - 933.15)
            T = hp.reference(case, t)[0]
            shares = hp.branch_shares(T, hp.PARAMS[hp.PHASE_CHANGE_2D])
            print(f"{name} x {scale}: solid / transition / liquid {shares}")
            assert min(shares) >= 0.1, (name, shares)


# ---- the map over the CPU double ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    lib = FakeDxmatHeatPlane(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    return lib


@pytest.mark.parametrize("subset", [False, True])
def test_map_update_through_the_nodal_form_blocks_and_enthalpy(fake, subset):
    case = hp.law_mesh("quad4x4")
    ncell, nqp = len(case["cells"]), case["phi"].shape[0]
    n = ncell * nqp
    cells = np.arange(0, ncell, 2, dtype=np.int32) if subset else None            # every second cell
    own = np.arange(ncell) if cells is None else cells
    rows = (own[:, None] * nqp + np.arange(nqp)[None]).ravel()
    rest = np.setdiff1d(np.arange(n), rows)
    m = JAXMaterial(jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0}, hypothesis="plane_strain"))
    q = QuadratureFieldMap(ncell, nqp, m, cells=cells)
    assert set(q.jacobians) == set(m.tangent_blocks) and q.jacobian_width == 7
    mesh = gm.PlaneScalarMesh(case["coords"], case["cells"][own], case["dofmap"][own], case["n_dofs"], case["geom_dphi"], case["phi"], case["dphi"])
    assert mesh.npoints == len(rows) and mesh.displacement_size == case["n_dofs"]
    t = [hp.phase_field(case)]
    q.register_device_gradient(mesh, lambda: t[0])
    q.register_external_state_variable("Temperature", 5000.0)                       # registered, and NOT uploaded by update()
    calls = list(fake.ext_calls)
    prm = hp.PARAMS[hp.PHASE_CHANGE_2D]
    for step in range(2):
        q.update()
        T, g, _ = hp.reference(case, t[0])
        ref = hp.update(hp.PHASE_CHANGE_2D, g[rows], T[rows], prm)
        flux = q.fluxes["HeatFlux"].x.array.reshape(n, 2)
        assert np.array_equal(flux[rows], ref["flux"]) and not flux[rest].any()
        jac = q.jacobian_flatten.x.array.reshape(n, 7)
        assert np.array_equal(jac[rows], ref["tangent"]) and not jac[rest].any()
        K = evaluate_block(q.jacobians[("HeatFlux", "TemperatureGradient")], rows)
        assert K.shape == (len(rows), 2, 2) and np.array_equal(K.reshape(-1, 4), ref["tangent"][:, :4])
        dj = evaluate_block(q.jacobians[("HeatFlux", "Temperature")], rows)
        assert dj.shape == (len(rows), 2, 1) and np.array_equal(dj[:, :, 0], ref["tangent"][:, 4:6])
        c = evaluate_block(q.jacobians[("Enthalpy", "Temperature")], rows)
        assert c.shape == (len(rows), 1, 1) and np.array_equal(c[:, 0, 0], ref["tangent"][:, 6])
        h = np.asarray(q.internal_state_variables["Enthalpy"].x.array)
        assert np.array_equal(h[rows], ref["enthalpy"]) and not h[rest].any() and ref["enthalpy"].any()
        assert m.last_stats["n_nan"] == 0
        q.advance()
        t[0] = 933.15 - (hp.phase_field(case) - 933.15)
    assert fake.nodal_calls == [("rows" if subset else "host", case["n_dofs"])] * 2
    assert fake.ext_calls == calls                                                  # the Temperature variable was not uploaded again
    q.close()
