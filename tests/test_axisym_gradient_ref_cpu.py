"""CPU: ``axisym_gradient_ref`` (the numpy restatement ``test_gpu_axisym_gradient.py`` compares the kernels with) held to its own
longdouble evaluation, to fields whose axisymmetric strain is known in closed form, and to ``plane_gradient_ref`` in the columns the two
share; the conditions the GPU tests' inputs rely on are asserted here."""
import numpy as np
import pytest

import axisym_gradient_ref as ag
import gradient_ref as gr
import plane_gradient_ref as pg
from dolfinx_materials_amd import gradient as gm
from plane_laws_2d import LAWS, increments

QUADS = [("quad", tag) for tag in pg.QUAD_CASES]
TRIS = [("tri", (e, r)) for e in ag.TRI_ELEMENTS for r in gr.SIMPLEX_RULES]


def _case(shape, key):
    return ag.quad_case(key) if shape == "quad" else ag.tri_case(*key)


def _ids(p):
    return f"{p[0]}-{p[1] if isinstance(p[1], str) else '-'.join(p[1])}"


def test_the_value_tables_belong_to_the_derivative_tables_of_the_cases():
    """the cases' ``dphi`` / ``geom_dphi`` are ``lagrange_*_table`` at the same points the value tables are taken at: exactly, for
    the two law meshes at the rules ``AxisymmetricMesh.lagrange`` would choose; every row of a value table sums to 1"""
    tri, quad = ag.law_mesh("tri6x3"), ag.law_mesh("quad4x4")
    pts = gm.simplex_quadrature(2, 2)
    assert np.array_equal(gm.lagrange_simplex_table(2, 2, pts), tri["dphi"]) and np.array_equal(gm.lagrange_simplex_table(2, 1, pts), tri["geom_dphi"])
    assert np.array_equal(gm.lagrange_simplex_values(2, 2, pts), tri["phi"]) and np.array_equal(gm.lagrange_simplex_values(2, 1, pts), tri["geom_phi"])
    pts = gm.quad_quadrature(2)
    assert np.array_equal(gm.lagrange_quad_table(1, pts), quad["dphi"]) and np.array_equal(gm.lagrange_quad_table(1, pts), quad["geom_dphi"])
    assert np.array_equal(gm.lagrange_quad_values(1, pts), quad["phi"]) and np.array_equal(gm.lagrange_quad_values(1, pts), quad["geom_phi"])
    assert np.array_equal(tri["dphi"], pg.law_mesh("tri6x3")["dphi"]) and np.array_equal(quad["dphi"], pg.law_mesh("quad4x4")["dphi"])
    for shape, key in QUADS + TRIS:
        case = _case(shape, key)
        assert case["phi"].shape == case["dphi"].shape[:2] and case["geom_phi"].shape == case["geom_dphi"].shape[:2]
        assert np.abs(case["phi"].sum(axis=1) - 1).max() < 1e-15 and np.abs(case["geom_phi"].sum(axis=1) - 1).max() < 1e-15
        assert np.array_equal(case["coords"][:, 1], (pg.quad_case(key) if shape == "quad" else pg.tri_case(*key))["coords"][:, 1])


@pytest.mark.parametrize("shape,key", QUADS + TRIS, ids=[_ids(p) for p in QUADS + TRIS])
def test_float64_against_longdouble_and_the_conditions_of_the_gpu_inputs(shape, key):
    case = _case(shape, key)
    worst = 0.0
    for name in ("random", "patch"):
        u = case["u_" + name]
        H, hoop, rad = ag.reference(case, u)
        Hl, hoopl, radl = ag.reference(case, u, np.longdouble)
        # the conditions test_gpu_axisym_gradient.py states its bound under
        assert np.abs(H).max() < 0.15 and np.abs(hoop).max() < 0.15 and rad.min() >= 1.0 and rad.max() <= 2.0
        assert float(np.abs(rad - radl).max() / radl.max()) < 1e-15
        for kind in range(4):
            e = float(np.abs(ag.rows(H, hoop, kind) - ag.rows(Hl, hoopl, kind)).max())
            worst = max(worst, e)
            assert e < 1e-14, (shape, key, name, kind, e)
        # what the axisymmetric rows share with the plane rows is the same bits
        assert np.array_equal(ag.rows(H, hoop, 0)[:, [0, 1, 3]], pg.rows(H, 2)[:, [0, 1, 3]])
        assert np.array_equal(ag.rows(H, hoop, 2)[:, [0, 1, 3, 4, 5]], pg.rows(H, 0)[:, [0, 1, 3, 4, 5]])
        assert np.array_equal(ag.rows(H, hoop, 3)[:, [0, 1, 3, 4, 5, 6, 7, 8]], pg.rows(H, 1)[:, [0, 1, 3, 4, 5, 6, 7, 8]])
        assert np.array_equal(ag.rows(H, hoop, 1), ag.rows(H, hoop, 3)[:, :5])
    print(f"axisym reference {shape} {key}: float64 against longdouble {worst:.3e} (bound 1e-14)")


@pytest.mark.parametrize("shape,key", [("quad", "q1-x4"), ("quad", "q1-x1"), ("tri", ("p1tri", "deg2")), ("tri", ("p1tri", "q5"))])
def test_a_linear_field_has_the_hoop_strain_of_its_radial_stretch(shape, key):
    """u = (a r, b z): eps = [a, b, a, 0], which P1 and Q1 represent"""
    case = _case(shape, key)
    a, b = 0.011, -0.023
    u = (case["xd"] * np.array([a, b])).ravel()
    got = ag.strain(case, u, 0)
    e = float(np.abs(got - np.array([a, b, a, 0.0])).max())
    print(f"u = (a r, b z) on {shape} {key}: {e:.3e}")
    assert e < 1e-14
    assert np.abs(ag.strain(case, u, 1) - np.array([1 + a, 1 + b, 1 + a, 0.0, 0.0])).max() < 1e-14


@pytest.mark.parametrize("shape,key", [("quad", "q2-x9"), ("quad", "q2-x5"), ("tri", ("p2tri", "deg2")), ("tri", ("p2tri", "q7"))])
def test_a_quadratic_radial_field_on_second_order_elements(shape, key):
    """u_r = r^2 (in the span of P2 on affine triangles and of Q2 on bilinear quadrilaterals): eps_rr = 2 r, eps_tt = r.  Bound: nodal
    values up to 4 carry 4.4e-16 each, the physical shape-function gradients are up to ~3 * 14 (reference gradient times 1 / h of the
    distorted 9 x 9 grid) over 9 dofs: 2e-13 at the very worst, asserted as 1e-12; the hoop term has no 1 / h: 1e-14."""
    case = _case(shape, key)
    xd = case["xd"]
    u = np.stack([xd[:, 0] ** 2, np.zeros(len(xd))], axis=1).ravel()
    H, hoop, rad = ag.reference(case, u)
    e_rr, e_tt = float(np.abs(H[:, 0, 0] - 2 * rad).max()), float(np.abs(hoop - rad).max())
    print(f"u_r = r^2 on {shape} {key}: eps_rr {e_rr:.3e} eps_tt {e_tt:.3e}")
    assert e_rr < 1e-12 and e_tt < 1e-14
    assert np.abs(H[:, 1, 1]).max() == 0.0 and np.abs(H[:, 1, 0]).max() == 0.0          # u_z = 0: exact


@pytest.mark.parametrize("shape,key", QUADS + TRIS, ids=[_ids(p) for p in QUADS + TRIS])
def test_an_axial_translation_strains_nothing(shape, key):
    """u = (0, c): u_r = 0 makes rr, tt and the H01 half of the shear exact zeros whatever the tables hold, and kind 1 has exactly
    1, 1 + 0 and 0 there.  The z derivatives of the constant c are sums of ``c * g_m`` over shape-function gradients that add up to zero
    only up to rounding (``plane_gradient_ref`` contracts the tables with the inverse Jacobian first), so zz and H10 are zeros at
    rounding level of c / h, not bit for bit: the figures are printed."""
    case = _case(shape, key)
    c = 0.37
    u = np.stack([np.zeros(len(case["xd"])), np.full(len(case["xd"]), c)], axis=1).ravel()
    H, hoop, _ = ag.reference(case, u)
    k0, k1 = ag.rows(H, hoop, 0), ag.rows(H, hoop, 1)
    assert np.all(k0[:, [0, 2]] == 0.0) and np.all(k1[:, [0, 2]] == 1.0) and np.all(k1[:, 3] == 0.0)
    rest = float(max(np.abs(k0[:, [1, 3]]).max(), np.abs(k1[:, 1] - 1).max(), np.abs(k1[:, 4]).max()))
    print(f"u = (0, c) on {shape} {key}: the z derivatives of a constant {rest:.3e}")
    assert rest < 1e-13
    H, hoop, _ = ag.reference(case, np.zeros_like(u))                  # c = 0: every entry exact
    assert np.all(ag.rows(H, hoop, 0) == 0.0) and np.all(ag.rows(H, hoop, 1) == np.array([1.0, 1.0, 1.0, 0.0, 0.0]))


@pytest.mark.parametrize("mesh_name", pg.LAW_MESHES)
def test_the_increments_of_the_displacement_form_tests_keep_the_conditions(mesh_name):
    case = ag.law_mesh(mesh_name)
    assert case["npoints"] == pg.law_mesh(mesh_name)["npoints"]
    for law in (26, 27, 28):
        for u in increments(law, mesh_name):
            H, hoop, rad = ag.reference(case, u)
            assert np.abs(H).max() < 0.15 and np.abs(hoop).max() < 0.15 and rad.min() >= 1.0, (law, mesh_name)
    assert LAWS[27]["kind"] == 2        # the plane kind of dxm_mesh_gradient_device; an axisymmetric mesh asks its own kind 0 for these rows
