"""No GPU: ``gradient_ref`` is fit to pin the gradient kernels, on every mesh, point set and displacement field that
``test_gpu_gradient_kernels.py`` uses.

* Reference accuracy: the float64 and the longdouble evaluation differ by at most 1e-14 absolute, in H and in both output layouts.
  The GPU tests compare at 1e-13: a factor of ten of that bound is the reference's, nine tenths are the kernels'.
* Patch test: ``u = A x + b`` at the nodes / dof positions gives ``H == A`` at every point of every element kind on the distorted
  meshes, and a rigid rotation about a centre gives ``F == R``.  The bound is the rounding of the contraction ``sum_m u_m g_m``
  itself, ``PATCH_ROUNDINGS eps max|u| max sum_m |g_m|_1``: the nodal values carry 3 roundings each (``A x + b``), the products
  one, the sum over up to 10 dofs up to 10, and the shape-function gradients g a relative error of some tens of eps from the cofactor
  inverse, which meets the same ``|u| |g|``.  64 eps covers them; the figures observed are printed.
* The restatement agrees with the two host evaluations the suite already has (``test_gpu_gradient.host_gradient`` with
  ``np.linalg.inv``, ``helpers.simplex_host_gradient``), its tables are derivatives of the shape functions (finite differences in
  longdouble) and sum to zero over the shape functions.
* The point sets are where the GPU tests say they are: inside the elements, away from the faces, and at the point counts whose
  256-point blocks start inside a cell; the chunked cases are cut into chunks that start inside a cell."""
import numpy as np
import pytest

import gradient_ref as gr
import tile_loop_cases as tc
from helpers import deformation_gradient9, mandel_strain, simplex_host_gradient

ACCURACY = 1e-14           # float64 against longdouble: a tenth of the GPU bound
PATCH_ROUNDINGS = 64
EPS = np.finfo(np.float64).eps
LD = np.longdouble


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps < 1e-3 * EPS          # x87 extended (64-bit mantissa) or better: else the accuracy test says nothing


def _patch_bound(u, g):
    return PATCH_ROUNDINGS * EPS * np.abs(u).max() * np.abs(np.asarray(g, dtype=np.float64)).sum(axis=(2, 3)).max()


@pytest.mark.parametrize("tag", list(gr.CASES) + list(gr.CHUNK_CASES))
def test_float64_reference_is_within_1e_14_of_longdouble(tag):
    if tag in gr.CHUNK_CASES:
        case = gr.chunk_case(tag)
        kind, us = case["kind"], {"u": case["u"]}
    else:
        kind, case = gr.get_case(tag)
        us = {"random": case["u_random"], "patch": case["u_patch"]}
    for name, u in us.items():
        H64, Hld = gr.reference(kind, case, u), gr.reference(kind, case, u, LD)
        assert H64.dtype == np.float64 and Hld.dtype == LD and H64.shape == Hld.shape
        eH = float(np.abs(H64 - Hld).max())
        ee = float(np.abs(mandel_strain(H64) - mandel_strain(Hld)).max())
        eF = float(np.abs(deformation_gradient9(H64) - deformation_gradient9(Hld)).max())
        print(f"gradient_ref {tag} {name}: {len(H64)} points, max|H| {np.abs(H64).max():.3f}, float64 - longdouble H {eH:.2e} strain {ee:.2e} F {eF:.2e} (bound {ACCURACY:.0e})")
        assert np.abs(H64).max() < 0.15                       # the magnitudes the 1e-13 of the GPU tests is meant for
        assert max(eH, ee, eF) <= ACCURACY


@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["float64", "longdouble"])
@pytest.mark.parametrize("tag", list(gr.CASES))
def test_patch_field_and_rigid_rotation(tag, dtype):
    kind, case = gr.get_case(tag)
    t = case["xd"].shape[1]
    A = np.zeros((3, 3))
    A[:t, :t] = gr.PATCH_A[:t, :t]
    H, g = gr.reference(kind, case, case["u_patch"], dtype, with_g=True)
    bound = _patch_bound(case["u_patch"], g)
    err = float(np.abs(H - A).max())
    print(f"gradient_ref {tag} patch ({np.dtype(dtype).name}): |H - A| {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    # rigid rotation by 0.6 rad about the axis (1, 2, 2) / 3 (tdim 2: in the plane) through the centre (0.4, 0.6, 0.5): F == R
    ax = np.array([1.0, 2.0, 2.0]) / 3.0 if t == 3 else np.array([0.0, 0.0, 1.0])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.6) * K + (1 - np.cos(0.6)) * K @ K
    c = np.array([0.4, 0.6, 0.5])[:t]
    u = ((case["xd"] - c) @ (R[:t, :t] - np.eye(t)).T).ravel()
    H = gr.reference(kind, case, u, dtype)
    F = deformation_gradient9(H)
    bound = _patch_bound(u, g)
    err = float(np.abs(F - deformation_gradient9((R - np.eye(3))[None])).max())
    print(f"gradient_ref {tag} rotation ({np.dtype(dtype).name}): |F - R| {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    if t == 2:        # plane strain: nothing out of the plane
        assert np.all(F[:, 2] == 1.0) and np.all(F[:, 5:] == 0.0) and np.all(mandel_strain(H)[:, [2, 4, 5]] == 0.0)


def test_cofactor_inverse_and_tables():
    rng = np.random.default_rng(0)
    for n in (2, 3):
        A = np.eye(n) + 0.3 * rng.uniform(-1, 1, (50, 4, n, n))
        assert np.abs(gr.cofactor_inverse(A) - np.linalg.inv(A)).max() < 1e-14
        assert np.abs(np.einsum("...ij,...jk->...ik", gr.cofactor_inverse(A.astype(LD)), A.astype(LD)) - np.eye(n)).max() < 1e-17
    # the hex8 table: derivative of N_m (central differences in longdouble), sums to zero, N_m is 1 at corner m and 0 at the others
    N = lambda p: np.prod(1 + gr.HEX_CORNERS.astype(LD)[None] * p[:, None, :], axis=2) / 8   # noqa: E731
    assert np.array_equal(N(gr.HEX_CORNERS.astype(LD)), np.eye(8))
    pts = gr.interior_points_hex(9, seed=1).astype(LD)
    dN = gr.hex8_table(pts, LD)
    step = LD(2.0) ** -24
    for d in range(3):
        e = np.zeros(3, dtype=LD)
        e[d] = step
        assert np.abs((N(pts + e) - N(pts - e)) / (2 * step) - dN[:, :, d]).max() < 1e-12    # (N is trilinear: the difference is exact up to rounding)
    assert np.abs(dN.sum(axis=1)).max() < 1e-18
    assert np.abs(gr.hex8_table(pts.astype(np.float64)) - gr.hex8_table(pts.astype(np.float64), LD)).max() < 4 * EPS
    for tdim in (2, 3):
        assert np.array_equal(gr.p1_table(tdim, 3).sum(axis=1), np.zeros((3, tdim)))
        from dolfinx_materials_amd.gradient import lagrange_simplex_table

        assert np.array_equal(gr.p1_table(tdim, 5), lagrange_simplex_table(tdim, 1, gr.interior_points_simplex(tdim, 5, seed=2)))


def test_agrees_with_the_host_evaluations_the_suite_already_has():
    from test_gpu_gradient import host_gradient

    for nqp in gr.HEX_DIRECT_NQP + gr.HEX_STAGED_NQP:
        c = gr.hex_case(nqp)
        old = host_gradient(c["coords"], c["conn"], c["u_random"], c["points"]).reshape(-1, 3, 3)
        assert np.abs(old - gr.reference("hex8", c, c["u_random"])).max() < 1e-14
    for e in gr.SIMPLEX_ELEMENTS:
        for r in gr.SIMPLEX_RULES:
            c = gr.simplex_case(e, r)
            old = simplex_host_gradient(c["coords"], c["cells"], c["dofmap"], c["u_random"], c["dphi"]).reshape(-1, 3, 3)
            assert np.abs(old - gr.reference("simplex", c, c["u_random"])).max() < 1e-14
    # tet4 == the P1 simplex with any table of that many points
    for nqp in gr.TET4_NQP:
        c = gr.tet4_case(nqp)
        old = simplex_host_gradient(c["coords"], c["conn"], c["conn"], c["u_random"], gr.p1_table(3, nqp)).reshape(-1, 3, 3)
        assert np.abs(old - gr.reference("tet4", c, c["u_random"])).max() < 1e-14


def test_point_sets_and_block_starts():
    for nqp in gr.HEX_DIRECT_NQP + gr.HEX_STAGED_NQP:
        c = gr.hex_case(nqp)
        assert c["points"].shape == (nqp, 3) and np.abs(c["points"]).max() < 0.9
        assert c["conn"].min() == 0 and c["conn"].max() == len(c["coords"]) - 1
        # every cell of the distorted grids keeps a positive Jacobian at its corners and points
        J = np.einsum("cma,qmd->cqad", c["coords"][c["conn"]], gr.hex8_table(np.concatenate([c["points"], gr.HEX_CORNERS])))
        assert np.linalg.det(J).min() > 0.3 * (0.5 * c["h"]) ** 3
    assert [len(gr.hex_case(q)["conn"]) * q for q in gr.HEX_DIRECT_NQP] == [343, 1029]          # several blocks, a ragged last one
    assert [len(gr.hex_case(q)["conn"]) * q for q in gr.HEX_STAGED_NQP] == [864, 1080, 1512, 5832]
    assert all(256 % q != 0 for q in (5, 7, 27)) and 256 % 4 == 0
    assert all((216 * q) % 256 != 0 for q in gr.HEX_STAGED_NQP)
    for tdim in (2, 3):
        for rule in gr.SIMPLEX_RULES:
            p = gr.simplex_points(tdim, rule)
            lam = np.concatenate([1 - p.sum(axis=1, keepdims=True), p], axis=1)
            assert lam.min() >= 0.05 - 1e-15 and len(p) == {"q1": 1, "q5": 5, "q7": 7, "deg2": tdim + 1}[rule]
    cells = gr.tet_mesh()[1]
    assert len(cells) == 162
    X = gr.tet_mesh()[0][cells]
    assert np.abs(np.linalg.det(X[:, 1:] - X[:, :1])).min() > 0.2 / 27                          # no sliver in the Kuhn split


@pytest.mark.parametrize("name", list(gr.CHUNK_CASES))
def test_the_chunked_cases_start_chunks_inside_a_cell(name):
    case = gr.chunk_case(name)
    n, nqp = case["npoints"], case["nqp"]
    assert n == {"tri6x3": 66_150, "tet4x5": 65_910}[name] and n >= 65_536 and n == len(case["cells"]) * nqp
    chunks = tc.host_chunks(n, 64, fused=True)
    print(f"chunked {name}: {n} points, chunks {chunks}, offsets mod nqp {[off % nqp for off, _ in chunks]}")
    assert len(chunks) >= 2 and sum(c for _, c in chunks) == n
    assert any(off % nqp != 0 for off, _ in chunks)
    assert len(tc.host_chunks(n, 64)) == 1            # the three-stream cap of the strain-driven form would not cut this batch at all
