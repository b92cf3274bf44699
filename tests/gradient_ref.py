"""Plain numpy restatement of the displacement gradient ``H[i][a] = du_i / dX_a`` at arbitrary reference points, and the meshes,
point sets and displacement fields of ``test_gpu_gradient_kernels.py``.  TEST INFRASTRUCTURE ONLY; no GPU.

Written from the element definitions, not from ``csrc/gradient.hpp``: shape-function derivative TABLES contracted with einsum and
an explicit cofactor inverse, so that every function also runs in ``np.longdouble`` (``np.linalg.inv`` does not).  Every evaluation
has the same three steps:

1. ``dN[q, m, d]``: reference derivatives of the shape functions at the points (trilinear hexahedron: built here from the corner
   signs; simplices: the constant barycentric table, or the caller's tabulated Lagrange basis);
2. ``J[c, q, a, d] = sum_m X[c, m, a] dN[q, m, d]`` and its inverse by cofactors: ``g[c, q, m, a] = sum_d dN[q, m, d] Ji[c, q, d, a]``,
   the physical gradients of the shape functions;
3. ``H[c, q, i, a] = sum_m U[c, m, i] g[c, q, m, a]``, embedded in 3 x 3 with zeros for triangles (plane strain).

``test_gradient_ref_cpu.py`` holds the float64 evaluation to the longdouble one within 1e-14 on every input below, and both to the
patch test and a rigid rotation."""
import functools

import numpy as np

#: corners of the trilinear hexahedron on [-1, 1]^3 in the order of ``Hex8Mesh``
HEX_CORNERS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)


def cofactor_inverse(A):
    """Inverse of (..., 2, 2) or (..., 3, 3) matrices from their cofactors, in the dtype of ``A``."""
    n = A.shape[-1]
    out = np.empty_like(A)
    if n == 2:
        det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
        out[..., 0, 0], out[..., 0, 1] = A[..., 1, 1] / det, -A[..., 0, 1] / det
        out[..., 1, 0], out[..., 1, 1] = -A[..., 1, 0] / det, A[..., 0, 0] / det
        return out
    assert n == 3
    cof = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            r, s = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            minor = A[..., r[0], s[0]] * A[..., r[1], s[1]] - A[..., r[0], s[1]] * A[..., r[1], s[0]]
            cof[..., i, j] = minor if (i + j) % 2 == 0 else -minor
    det = A[..., 0, 0] * cof[..., 0, 0] + A[..., 0, 1] * cof[..., 0, 1] + A[..., 0, 2] * cof[..., 0, 2]
    for i in range(3):
        for j in range(3):
            out[..., i, j] = cof[..., j, i] / det          # adjugate = transposed cofactors
    return out


def hex8_table(points, dtype=np.float64):
    """``dN[q, m, d]`` of ``N_m = (1 + s_m0 x)(1 + s_m1 y)(1 + s_m2 z) / 8`` at ``points`` (nqp, 3) in [-1, 1]^3."""
    xi = np.asarray(points, dtype=dtype).reshape(-1, 3)
    s = HEX_CORNERS.astype(dtype)
    f = 1 + s[None, :, :] * xi[:, None, :]                  # (q, m, axis): the three linear factors
    dN = np.empty((len(xi), 8, 3), dtype=dtype)
    for d in range(3):
        o = [a for a in range(3) if a != d]
        dN[:, :, d] = s[None, :, d] * f[:, :, o[0]] * f[:, :, o[1]] / 8
    return dN


def p1_table(tdim, nqp, dtype=np.float64):
    """``dN[q, m, d]`` of the barycentric coordinates ``l_0 = 1 - sum(xi), l_k = xi_k``: the same at every point."""
    d = np.concatenate([-np.ones((1, tdim)), np.eye(tdim)], axis=0).astype(dtype)
    return np.ascontiguousarray(np.broadcast_to(d, (nqp, tdim + 1, tdim)))


def shape_gradients(X, dN):
    """``g[c, q, m, a]``: physical gradients of the geometry's shape functions.  ``X`` (c, m, tdim) corner coordinates, ``dN`` (q, m, tdim)."""
    J = np.einsum("cma,qmd->cqad", X, dN)                   # dX_a / dxi_d
    return np.einsum("qmd,cqda->cqma", dN, cofactor_inverse(J))


def embed(H):
    """(c, q, tdim, tdim) -> (c, q, 3, 3), zeros outside the plane for tdim 2."""
    t = H.shape[-1]
    if t == 3:
        return H
    out = np.zeros(H.shape[:2] + (3, 3), dtype=H.dtype)
    out[:, :, :t, :t] = H
    return out


def hex8_gradient(coords, conn, u, points, dtype=np.float64, with_g=False):
    """Isoparametric trilinear hexahedra: H (ncells, nqp, 3, 3)."""
    X = np.asarray(coords, dtype=dtype)[conn]
    U = np.asarray(u, dtype=dtype).reshape(-1, 3)[conn]
    g = shape_gradients(X, hex8_table(points, dtype))
    H = np.einsum("cmi,cqma->cqia", U, g)
    return (H, g) if with_g else H


def tet4_gradient(coords, conn, u, nqp, dtype=np.float64, with_g=False):
    """Affine tetrahedra: the cell's constant gradient at each of its ``nqp`` points."""
    X = np.asarray(coords, dtype=dtype)[conn]
    U = np.asarray(u, dtype=dtype).reshape(-1, 3)[conn]
    g = shape_gradients(X, p1_table(3, nqp, dtype))
    H = np.einsum("cmi,cqma->cqia", U, g)
    return (H, g) if with_g else H


def simplex_gradient(coords, geom_conn, dofmap, u, dphi, dtype=np.float64, with_g=False):
    """Lagrange field with the tabulated basis ``dphi`` (nqp, nd, tdim) on straight-sided simplices (geometry from the vertices)."""
    tdim = geom_conn.shape[1] - 1
    dphi = np.asarray(dphi, dtype=dtype)
    X = np.asarray(coords, dtype=dtype)[geom_conn][:, :, :tdim]
    Jinv = cofactor_inverse(np.einsum("cma,qmd->cqad", X, p1_table(tdim, dphi.shape[0], dtype)))
    g = np.einsum("qmd,cqda->cqma", dphi, Jinv)             # the field's own basis through the affine map
    U = np.asarray(u, dtype=dtype).reshape(-1, tdim)[dofmap]
    H = embed(np.einsum("cmi,cqma->cqia", U, g))
    return (H, g) if with_g else H


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
KUHN = [(0, 1, 2, 6), (0, 2, 3, 6), (0, 3, 7, 6), (0, 7, 4, 6), (0, 4, 5, 6), (0, 5, 1, 6)]   # hex8 -> 6 tetrahedra along 0-6
#: the affine patch field u = A x + b: |A| <= 0.03
PATCH_A = np.array([[0.020, -0.013, 0.007], [0.011, -0.017, 0.023], [-0.019, 0.005, 0.029]])
PATCH_B = np.array([0.013, -0.021, 0.008])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)          # shared between tests: computed once, left unchanged
    return arrays[0] if len(arrays) == 1 else arrays


def hex_grid(n, distort, seed):
    """Unit cube of n^3 hexahedra (corner order of ``Hex8Mesh``), every node moved by up to ``distort`` cell sizes."""
    g = np.arange(n + 1) / n
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    coords = coords + distort / n * np.random.default_rng(seed).uniform(-1, 1, coords.shape)
    i, j, k = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"))
    node = lambda a, b, c: ((i + a) * (n + 1) + (j + b)) * (n + 1) + (k + c)   # noqa: E731
    conn = np.stack([node(*((HEX_CORNERS[m] + 1) / 2).astype(int)) for m in range(8)], axis=1).astype(np.int32)
    return coords, conn


def kuhn_split(conn):
    return np.ascontiguousarray(np.concatenate([conn[:, list(k)] for k in KUHN], axis=0).astype(np.int32))


def interior_points_hex(nqp, seed):
    """Arbitrary points in (-0.9, 0.9)^3."""
    return np.random.default_rng(seed).uniform(-0.9, 0.9, (nqp, 3))


def interior_points_simplex(tdim, nqp, seed):
    """Arbitrary points of the reference simplex with every barycentric coordinate >= 0.05."""
    lam = np.random.default_rng(seed).dirichlet(np.ones(tdim + 1), nqp)
    lam = 0.05 + (1.0 - 0.05 * (tdim + 1)) * lam
    return np.ascontiguousarray(lam[:, 1:])


def fields(xd, h, seed, noise=1e-2):
    """(random, patch) displacement vectors on the dof positions ``xd`` (n, tdim): a smooth part, a quadratic part and nodal noise of
    ``noise`` cell sizes (gradients of a few percent; second-order elements take 0.4 of it: their
    midside values weigh four times as much near a vertex), and ``PATCH_A x + PATCH_B``."""
    t = xd.shape[1]
    rng = np.random.default_rng(seed)
    rand = xd * np.array([8e-3, -3e-3, -3e-3][:t]) + 5e-3 * xd**2 + noise * h * rng.standard_normal(xd.shape)
    patch = xd @ PATCH_A[:t, :t].T + PATCH_B[:t]
    return _frozen(np.ascontiguousarray(rand.ravel()), np.ascontiguousarray(patch.ravel()))


HEX_DIRECT_NQP = (1, 3)            # hex8_gradient_kernel (nqp < 4) on 7^3 cells: 343 and 1029 points
HEX_STAGED_NQP = (4, 5, 7, 27)     # hex8_gradient_staged_kernel on 6^3 cells: 864, 1080, 1512 and 5832 points
TET4_NQP = (1, 4, 5)               # tet4_gradient_kernel on 162 cells
SIMPLEX_RULES = ("q1", "q5", "q7", "deg2")
SIMPLEX_ELEMENTS = ("p1tri", "p2tri", "p1tet", "p2tet")


@functools.lru_cache(maxsize=None)
def hex_case(nqp):
    """dict(coords, conn, points, xd, h, u_random, u_patch) of the hex8 cases."""
    n = 7 if nqp < 4 else 6
    coords, conn = hex_grid(n, 0.15, seed=20 + nqp)
    if nqp == 1:
        pts = np.zeros((1, 3))
    elif nqp == 27:
        from dolfinx_materials_amd.gradient import gauss_points_hex

        pts = np.ascontiguousarray(gauss_points_hex(4))
    else:
        pts = interior_points_hex(nqp, seed=40 + nqp)
    ur, up = fields(coords, 1.0 / n, seed=60 + nqp)
    _frozen(coords, conn, pts)
    return dict(coords=coords, conn=conn, points=pts, xd=coords, h=1.0 / n, u_random=ur, u_patch=up)


@functools.lru_cache(maxsize=None)
def tet_mesh():
    coords, conn = hex_grid(3, 0.2, seed=4)
    return _frozen(coords, kuhn_split(conn))


@functools.lru_cache(maxsize=None)
def tet4_case(nqp):
    coords, conn = tet_mesh()
    ur, up = fields(coords, 1.0 / 3, seed=80 + nqp)
    return dict(coords=coords, conn=conn, nqp=nqp, xd=coords, h=1.0 / 3, u_random=ur, u_patch=up)


def simplex_points(tdim, rule):
    from dolfinx_materials_amd.gradient import simplex_quadrature

    if rule == "deg2":
        return simplex_quadrature(tdim, 2)
    if rule == "q1":
        return np.full((1, tdim), 1.0 / (tdim + 1))
    return interior_points_simplex(tdim, int(rule[1:]), seed=100 + 10 * tdim + int(rule[1:]))


@functools.lru_cache(maxsize=None)
def simplex_case(element, rule):
    """dict(coords (nv, 3), cells, dofmap, n_dofs, dphi, xd, h, tdim, u_random, u_patch): ``element`` p1tri | p2tri | p1tet | p2tet,
    ``rule`` q1 (centroid) | q5 | q7 (arbitrary interior points) | deg2 (``simplex_quadrature``)."""
    from dolfinx_materials_amd.gradient import lagrange_simplex_table, p2_dofmap
    from helpers import triangle_grid

    degree, tdim = int(element[1]), 2 if element.endswith("tri") else 3
    if tdim == 2:
        xv, cells = triangle_grid(7, seed=3)              # 98 triangles
        h = 1.0 / 7
    else:
        xv, cells = tet_mesh()                            # 162 tetrahedra
        h = 1.0 / 3
    dphi = lagrange_simplex_table(tdim, degree, simplex_points(tdim, rule))
    if degree == 1:
        dofmap, n_dofs, xd = cells, len(xv), xv.copy()
    else:
        dofmap, n_dofs, edges = p2_dofmap(cells)
        xd = np.concatenate([xv, 0.5 * (xv[edges[:, 0]] + xv[edges[:, 1]])], axis=0)
    coords = np.ascontiguousarray(np.pad(xv, ((0, 0), (0, 3 - xv.shape[1]))))
    ur, up = fields(xd, h, seed=120 + 10 * tdim + degree, noise=1e-2 if degree == 1 else 4e-3)
    _frozen(coords, dphi, xd)
    return dict(coords=coords, cells=cells, dofmap=np.ascontiguousarray(dofmap, dtype=np.int32), n_dofs=n_dofs, dphi=dphi, xd=xd, h=h,
                tdim=tdim, u_random=ur, u_patch=up)


def reference(kind, case, u, dtype=np.float64, with_g=False):
    """H (npoints, 3, 3) of one of the cases above (``kind`` hex8 | tet4 | simplex) for the displacement vector ``u``."""
    if kind == "hex8":
        r = hex8_gradient(case["coords"], case["conn"], u, case["points"], dtype, with_g)
    elif kind == "tet4":
        r = tet4_gradient(case["coords"], case["conn"], u, case["nqp"], dtype, with_g)
    else:
        r = simplex_gradient(case["coords"], case["cells"], case["dofmap"], u, case["dphi"], dtype, with_g)
    if with_g:
        return r[0].reshape(-1, 3, 3), r[1]
    return r.reshape(-1, 3, 3)


CHUNK_CASES = {"tri6x3": 3, "tet4x5": 5}     # name -> nqp


@functools.lru_cache(maxsize=None)
def chunk_case(name):
    """The smallest meshes whose host-buffer displacement call is cut into chunks (from 65 536 points on), with an nqp that does not
    divide the chunk size: tri6 x 3 on ``triangle_grid(105)`` (22 050 cells, 66 150 points) and tet4 x 5 on the Kuhn split of 13^3
    hexahedra (13 182 cells, 65 910 points).  dict(kind, coords, cells, nqp, npoints, xd, u [, dofmap, n_dofs, dphi])."""
    from dolfinx_materials_amd.gradient import lagrange_simplex_table, p2_dofmap, simplex_quadrature
    from helpers import triangle_grid

    nqp = CHUNK_CASES[name]
    rng = np.random.default_rng(5)
    if name == "tri6x3":
        xv, cells = triangle_grid(105, seed=3)
        dofmap, n_dofs, edges = p2_dofmap(cells)
        xd = np.concatenate([xv, 0.5 * (xv[edges[:, 0]] + xv[edges[:, 1]])], axis=0)
        out = dict(kind="simplex", coords=np.ascontiguousarray(np.pad(xv, ((0, 0), (0, 1)))), cells=cells, dofmap=np.ascontiguousarray(dofmap, dtype=np.int32),
                   n_dofs=n_dofs, dphi=lagrange_simplex_table(2, 2, simplex_quadrature(2, 2)), h=1.0 / 105)
    else:
        xv, conn = hex_grid(13, 0.2, seed=7)
        xd = xv
        cells = kuhn_split(conn)
        out = dict(kind="tet4", coords=xv, cells=cells, conn=cells, h=1.0 / 13)
    # uniaxial stretch past the yield strain plus nodal noise of the same order in the gradient: elastic and plastic points mixed
    u = xd * np.array([5e-3, -2e-3, -2e-3][:xd.shape[1]]) + 2.5e-3 * out["h"] * rng.standard_normal(xd.shape)
    out.update(nqp=nqp, npoints=len(out["cells"]) * nqp, xd=xd, u=_frozen(np.ascontiguousarray(u.ravel())))
    return out


#: tag -> (kind, builder, arguments) of every mesh and point set ``test_gpu_gradient_kernels.py`` holds to this reference
CASES = {f"hex8-direct-x{q}": ("hex8", hex_case, (q,)) for q in HEX_DIRECT_NQP}
CASES.update({f"hex8-staged-x{q}": ("hex8", hex_case, (q,)) for q in HEX_STAGED_NQP})
CASES.update({f"tet4-x{q}": ("tet4", tet4_case, (q,)) for q in TET4_NQP})
CASES.update({f"{e}-{r}": ("simplex", simplex_case, (e, r)) for e in SIMPLEX_ELEMENTS for r in SIMPLEX_RULES})


def get_case(tag):
    """(kind, case) of ``CASES[tag]``"""
    kind, build, args = CASES[tag]
    return kind, build(*args)
