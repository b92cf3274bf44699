"""Plain numpy restatement of the plane displacement gradient ``H[i][a] = du_i / dX_a`` on triangles and bilinear quadrilaterals, the
four row kinds ``dxm_mesh_gradient_device`` writes from it, and the meshes, point sets and displacement fields of
``test_gpu_plane_gradient.py``.  TEST INFRASTRUCTURE ONLY; no GPU.

Written from the element definitions, not from ``csrc/plane_gradient.hip``: the two shape-function derivative TABLES contracted with
einsum and ``gradient_ref.cofactor_inverse``, so that every function also runs in ``np.longdouble``:

1. ``J[c, q, a, d] = sum_v X[c, v, a] gdphi[q, v, d]`` from the geometry's table, ``Ji`` its inverse by cofactors;
2. ``g[c, q, m, a] = sum_d dphi[q, m, d] Ji[c, q, d, a]``, the physical gradients of the FIELD's shape functions;
3. ``H[c, q, i, a] = sum_m U[c, m, i] g[c, q, m, a]``.

``test_plane_gradient_ref_cpu.py`` holds the float64 evaluation to the longdouble one within 1e-14 on every input below, and both to
monomials, the patch test and a rigid rotation."""
import functools

import numpy as np

import gradient_ref as gr

R = np.sqrt(2.0) / 2.0
WIDTH = {0: 6, 1: 9, 2: 4, 3: 3}


def plane_gradient(coords, geom_conn, dofmap, u, geom_dphi, dphi, dtype=np.float64):
    """H (ncells, nqp, 2, 2)."""
    X = np.asarray(coords, dtype=dtype)[geom_conn][:, :, :2]
    J = np.einsum("cva,qvd->cqad", X, np.asarray(geom_dphi, dtype=dtype))
    g = np.einsum("qmd,cqda->cqma", np.asarray(dphi, dtype=dtype), gr.cofactor_inverse(J))
    U = np.asarray(u, dtype=dtype).reshape(-1, 2)[dofmap]
    return np.einsum("cmi,cqma->cqia", U, g)


def rows(H, kind):
    """(n, 2, 2) -> the (n, 6 | 9 | 4 | 3) rows of ``kind``; the components the plane does not have are exact zeros (ones on F's diagonal)."""
    H = H.reshape(-1, 2, 2)
    z = np.zeros(len(H), dtype=H.dtype)
    shear = np.asarray(R, dtype=H.dtype) * (H[:, 0, 1] + H[:, 1, 0])
    if kind == 0:
        cols = [H[:, 0, 0], H[:, 1, 1], z, shear, z, z]
    elif kind == 1:
        cols = [1 + H[:, 0, 0], 1 + H[:, 1, 1], 1 + z, H[:, 0, 1], H[:, 1, 0], z, z, z, z]
    elif kind == 2:
        cols = [H[:, 0, 0], H[:, 1, 1], z, shear]
    else:
        cols = [H[:, 0, 0], H[:, 1, 1], shear]
    return np.stack(cols, axis=1)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def quad_grid(n=9, distort=0.15, seed=11):
    """Unit square of n^2 quadrilaterals, vertices of a cell in basix's order (0,0),(1,0),(0,1),(1,1), every INTERIOR vertex moved by
    up to ``distort`` cell sizes: (coords (nv, 2), cells (nc, 4))."""
    xs = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    inner = (coords > 1e-12).all(axis=1) & (coords < 1 - 1e-12).all(axis=1)
    coords[inner] += distort / n * np.random.default_rng(seed).uniform(-1, 1, (int(inner.sum()), 2))
    i, j = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    idx = lambda a, b: (i + a) * (n + 1) + (j + b)   # noqa: E731
    cells = np.stack([idx(0, 0), idx(1, 0), idx(0, 1), idx(1, 1)], axis=1).astype(np.int32)
    return coords, cells


def interior_points_quad(nqp, seed):
    """Arbitrary points in (0.05, 0.95)^2."""
    return np.random.default_rng(seed).uniform(0.05, 0.95, (nqp, 2))


QUAD_CASES = {"q1-x1": (1, 1), "q1-x4": (1, 4), "q2-x5": (2, 5), "q2-x9": (2, 9)}   # tag -> (degree, nqp)


def _quad_points(nqp):
    from dolfinx_materials_amd.gradient import quad_quadrature

    if nqp == 1:
        return np.full((1, 2), 0.5)
    if nqp == 5:
        return interior_points_quad(5, seed=205)
    return quad_quadrature({4: 2, 9: 4}[nqp])


def _pad3(x):
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, 3 - x.shape[1]))))


@functools.lru_cache(maxsize=None)
def quad_case(tag):
    """dict(coords (nv, 3), cells, dofmap, n_dofs, geom_dphi, dphi, xd, h, u_random, u_patch) on the distorted 9 x 9 grid."""
    from dolfinx_materials_amd.gradient import lagrange_quad_table, q2_dofmap

    degree, nqp = QUAD_CASES[tag]
    xv, cells = quad_grid()
    pts = _quad_points(nqp)
    if degree == 1:
        dofmap, n_dofs, xd = cells, len(xv), xv.copy()
    else:
        dofmap, n_dofs, edges = q2_dofmap(cells)
        xd = np.concatenate([xv, 0.5 * (xv[edges[:, 0]] + xv[edges[:, 1]]), xv[cells].mean(axis=1)], axis=0)
    ur, up = gr.fields(xd, 1.0 / 9, seed=220 + 10 * degree + nqp, noise=1e-2 if degree == 1 else 4e-3)
    coords, gd, dphi = _pad3(xv), lagrange_quad_table(1, pts), lagrange_quad_table(degree, pts)
    gr._frozen(coords, cells, gd, dphi, xd)
    return dict(coords=coords, cells=cells, dofmap=np.ascontiguousarray(dofmap, dtype=np.int32), n_dofs=n_dofs, geom_dphi=gd, dphi=dphi,
                xd=xd, h=1.0 / 9, u_random=ur, u_patch=up)


@functools.lru_cache(maxsize=None)
def tri_case(element, rule):
    """``gr.simplex_case(element, rule)`` of a triangle element with the geometry table of the affine triangle added."""
    case = dict(gr.simplex_case(element, rule))
    assert case["tdim"] == 2
    case["geom_dphi"] = gr._frozen(gr.p1_table(2, case["dphi"].shape[0]))
    return case


def reference(case, u, dtype=np.float64):
    """H (npoints, 2, 2) of a case above."""
    return plane_gradient(case["coords"], case["cells"], case["dofmap"], u, case["geom_dphi"], case["dphi"], dtype).reshape(-1, 2, 2)


# ---- the meshes and the displacement of the displacement-form tests ----------------------------------------------------------------
LAW_MESHES = ("tri6x3", "quad4x4")
STRETCH = np.array([5e-3, -2e-3])     # the uniaxial stretch of gradient_ref.chunk_case: past the yield strain of the suite's J2 laws


@functools.lru_cache(maxsize=None)
def law_mesh(name):
    """dict(cells, coords, dofmap, n_dofs, geom_dphi, dphi, xd, h, npoints): tri6 with 3 Gauss points on ``triangle_grid(7)`` (294
    points) or quad4 with 4 on the distorted 9 x 9 grid (324 points)."""
    if name == "tri6x3":
        case = dict(tri_case("p2tri", "deg2"))
    else:
        case = dict(quad_case("q1-x4"))
    case["npoints"] = len(case["cells"]) * case["dphi"].shape[0]
    return case


def stretch_field(name, t=1.0, seed=5, noise=2.5e-3):
    """A uniaxial stretch past yield plus nodal noise of the same order in the gradient, as in ``gradient_ref.chunk_case``: elastic
    and yielded points mixed.  ``t`` scales the whole field (load steps)."""
    case = law_mesh(name)
    xd = case["xd"]
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((t * (xd * STRETCH + noise * case["h"] * rng.standard_normal(xd.shape))).ravel())
