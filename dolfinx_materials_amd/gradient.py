"""Device-side gradient evaluation for first-order hexahedra / tetrahedra, for Lagrange elements of any order on
straight-sided simplices and for plane meshes of triangles or bilinear quadrilaterals (``dxm_mesh_*`` of ``include/dxmat.h``); a scalar
field on a plane mesh (:class:`PlaneScalarMesh`: the temperature and its gradient, for the two-dimensional heat-transfer laws); a
displacement on a meridian mesh (:class:`AxisymmetricMesh`: the gradients with the hoop term ``u_r / r`` of the axisymmetric hypothesis).

The step before the hot path in the reference is ``QuadratureExpression.eval`` ->
``fem.Expression.eval`` (``quadrature_function.py:45-51``): dolfinx tabulates the UFL gradient at
every Gauss point on the host.  ``Hex8Mesh`` keeps coordinates and connectivity on the GPU so that
the strain / deformation gradient array is produced directly in HBM from the displacement vector.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def gauss_points_hex(degree=2):
    """Tensor Gauss-Legendre points on [-1,1]^3, last coordinate fastest."""
    n = {0: 1, 1: 1, 2: 2, 3: 2, 4: 3, 5: 3}[degree]
    x, _ = np.polynomial.legendre.leggauss(n)
    return np.array([[a, b, c] for a in x for b in x for c in x])


class _DeviceMesh:
    #: topological dimension of the cells (``SimplexMesh``: 2 or 3, set per instance)
    tdim = 3

    def gradient_device(self, u_ptr, kind, grad_ptr, stream=0):
        """Device pointers, asynchronous on ``stream``.  With ``H[i][a] = du_i / dX_a`` and ``r = sqrt(2) / 2``, ``kind``

        * 0: Mandel strain (6);
        * 1: deformation gradient ``F = I + H`` (9);
        * 2: the plane-strain 4-vector ``[H00, H11, 0.0, r (H01 + H10)]`` of the ``hypothesis="plane_strain"`` laws;
        * 3: the in-plane 3-vector ``[H00, H11, r (H01 + H10)]`` of the plane-stress laws.

        Kinds 2 and 3 on two-dimensional meshes only (``tdim == 2``: :class:`PlaneMesh`, :class:`SimplexMesh` on triangles);
        ``grad_ptr`` holds ``npoints`` rows of 6, 9, 4 or 3 doubles."""
        _lib.check(self._lib.dxm_mesh_gradient_device(self._handle, int(u_ptr), int(kind), int(grad_ptr), int(stream) or None))

    @property
    def npoints(self):
        return self.n_cells * self.nqp

    @property
    def displacement_size(self):
        """Number of doubles of the displacement vector this mesh expects (``u.x.array.size``)."""
        return int(self._lib.dxm_mesh_displacement_size(self._handle))

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.dxm_mesh_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


#: our hex8 corner order (VTK / the order of ``dxm_mesh_create_hex8``) in terms of the tensor-product vertex order
#: of a dolfinx / basix first-order hexahedron ((0,0,0),(1,0,0),(0,1,0),(1,1,0),(0,0,1),(1,0,1),(0,1,1),(1,1,1))
DOLFINX_HEX_TO_VTK = (0, 1, 3, 2, 4, 5, 7, 6)


def _dolfinx_p1_layout(V):
    """Node coordinates and cell -> node table of a first-order vector Lagrange space ``V`` in the numbering of
    ``u.x.array.reshape(-1, 3)`` (owned + ghost dofs; all local cells, ghosts included, which is the cell set
    ``QuadratureMap`` integrates: ``quadrature_map.py:66-70``)."""
    element = V.ufl_element()
    degree = getattr(element, "degree", None)
    degree = degree() if callable(degree) else degree
    if degree not in (1, None) or V.dofmap.index_map_bs != 3:
        raise ValueError("device gradient evaluation needs a first-order vector Lagrange space with block size 3")
    coords = np.ascontiguousarray(V.tabulate_dof_coordinates()[:, :3], dtype=np.float64)
    conn = np.asarray(V.dofmap.list, dtype=np.int32)
    if conn.ndim == 1:   # older dolfinx: flat adjacency list
        conn = conn.reshape(-1, len(V.dofmap.cell_dofs(0)))
    return coords, conn


class Tet4Mesh(_DeviceMesh):
    """Linear tetrahedra: coords ``(n_nodes, 3)``, conn ``(n_cells, 4)``; the (constant) cell
    gradient is repeated at the cell's ``nqp`` Gauss points."""

    def __init__(self, coords, conn, nqp=1, device=0):
        self._lib = _lib.load()
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        self.n_nodes, self.n_cells, self.nqp = coords.shape[0], conn.shape[0], int(nqp)
        self.device = int(device)
        h = self._lib.dxm_mesh_create_tet4(coords.ctypes.data, self.n_nodes, conn.ctypes.data, self.n_cells, self.nqp, self.device)
        if not h:
            raise _lib.DxmError(f"dxm_mesh_create_tet4 failed: {_lib.last_error()}")
        self._handle = h

    @classmethod
    def from_dolfinx(cls, V, quadrature_degree, device=0, cells=None):
        """From a dolfinx P1 vector function space on tetrahedra: ``u.x.array`` is the displacement vector to hand to
        ``integrate_displacement``; ``quadrature_degree`` as given to ``QuadratureMap`` (the gradient of a P1 field is
        constant per cell and is repeated at the cell's points, point = cell * nqp + q: ``quadrature_map.py:255-260``).
        ``cells``: the cells of ONE ``QuadratureMap`` (``qmap.cells``, a multi-material problem) instead of all."""
        import basix

        coords, conn = _dolfinx_p1_layout(V)
        if conn.shape[1] != 4:
            raise ValueError("Tet4Mesh.from_dolfinx needs a tetrahedral mesh")
        pts, _ = basix.make_quadrature(basix.CellType.tetrahedron, int(quadrature_degree))
        return cls(coords, conn if cells is None else conn[np.asarray(cells)], nqp=len(pts), device=device)


class Hex8Mesh(_DeviceMesh):
    """coords ``(n_nodes, 3)``; conn ``(n_cells, 8)`` with the corner order
    ``(-,-,-)(+,-,-)(+,+,-)(-,+,-)(-,-,+)(+,-,+)(+,+,+)(-,+,+)``; Gauss point ``q`` of cell ``c``
    is point ``c * nqp + q``."""

    def __init__(self, coords, conn, qpoints=None, device=0):
        self._lib = _lib.load()
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        conn = np.ascontiguousarray(conn, dtype=np.int32)
        qp = np.ascontiguousarray(gauss_points_hex(2) if qpoints is None else qpoints, dtype=np.float64)
        self.n_nodes, self.n_cells, self.nqp = coords.shape[0], conn.shape[0], qp.shape[0]
        self.device = int(device)
        h = self._lib.dxm_mesh_create_hex8(
            coords.ctypes.data, self.n_nodes, conn.ctypes.data, self.n_cells, qp.ctypes.data, self.nqp, self.device
        )
        if not h:
            raise _lib.DxmError(f"dxm_mesh_create_hex8 failed: {_lib.last_error()}")
        self._handle = h

    @classmethod
    def from_dolfinx(cls, V, quadrature_degree, device=0, cells=None):
        """From a dolfinx P1 vector function space on hexahedra (``cells``: those of one ``QuadratureMap`` instead of all).  The Gauss points are basix's for
        ``quadrature_degree`` (what ``QuadratureMap`` uses: ``quadrature_map.py:239-243``, ``utils.py:89-94``), mapped
        from the reference cell [0,1]^3 to [-1,1]^3 in basix's own order, so Gauss point ``q`` of cell ``c`` is row
        ``c * nqp + q`` of the quadrature Functions; the cell's dofs come in the tensor-product vertex order of basix
        and are permuted to the corner order of the kernels (:data:`DOLFINX_HEX_TO_VTK`)."""
        import basix

        coords, conn = _dolfinx_p1_layout(V)
        if conn.shape[1] != 8:
            raise ValueError("Hex8Mesh.from_dolfinx needs a hexahedral mesh")
        pts, _ = basix.make_quadrature(basix.CellType.hexahedron, int(quadrature_degree))
        conn = conn if cells is None else conn[np.asarray(cells)]
        return cls(coords, conn[:, DOLFINX_HEX_TO_VTK], qpoints=2.0 * np.asarray(pts) - 1.0, device=device)


#: local vertex pairs of the edges of the reference triangle / tetrahedron in basix's edge numbering: the second-order
#: Lagrange element has its dofs at the vertices, then at the midpoints of these edges in this order
BASIX_EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}


def simplex_quadrature(tdim, degree):
    """Reference points (nqp, tdim) of a quadrature rule of the given degree (0..2) on the reference simplex with
    vertices 0, e_1, ..., e_tdim.  For stand-alone use and tests; with dolfinx take basix's points
    (:meth:`SimplexMesh.from_dolfinx` does), whose order defines the row order of the quadrature Functions."""
    if degree <= 1:
        return np.full((1, tdim), 1.0 / (tdim + 1))
    if degree != 2:
        raise ValueError("simplex_quadrature: degree 0, 1 or 2")
    if tdim == 2:
        return np.array([[1 / 6, 1 / 6], [2 / 3, 1 / 6], [1 / 6, 2 / 3]])
    a, b = (5 + 3 * 5**0.5) / 20, (5 - 5**0.5) / 20
    return np.array([[b, b, b], [a, b, b], [b, a, b], [b, b, a]])


def lagrange_simplex_table(tdim, degree, points):
    """Reference derivatives ``dphi[q, m, d] = d N_m / d xi_d`` of the Lagrange basis of the given degree (1 or 2) on the
    reference simplex at ``points`` (nqp, tdim), dofs in basix's order (vertices, then :data:`BASIX_EDGES` midpoints).
    With barycentric coordinates l_0 = 1 - sum(xi), l_k = xi_k: N_v = l_v (2 l_v - 1), N_(ij) = 4 l_i l_j."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, tdim)
    lam = np.concatenate([1.0 - pts.sum(axis=1, keepdims=True), pts], axis=1)          # (nqp, tdim+1)
    dlam = np.concatenate([-np.ones((1, tdim)), np.eye(tdim)], axis=0)                  # (tdim+1, tdim), constant
    if degree == 1:
        return np.ascontiguousarray(np.broadcast_to(dlam, (len(pts), tdim + 1, tdim)))
    if degree != 2:
        raise ValueError("lagrange_simplex_table: degree 1 or 2 (hand any other table to SimplexMesh directly)")
    cols = [(4.0 * lam[:, v, None] - 1.0) * dlam[v] for v in range(tdim + 1)]
    cols += [4.0 * (lam[:, i, None] * dlam[j] + lam[:, j, None] * dlam[i]) for i, j in BASIX_EDGES[tdim]]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def p2_dofmap(cells):
    """Second-order Lagrange dofmap of a simplex mesh given by its vertex table ``cells`` (n_cells, tdim+1): vertex dofs
    keep the vertex numbers, one more dof per unique edge.  Returns ``(dofmap (n_cells, nd), n_dofs, edge_vertices)``
    with ``edge_vertices`` (n_edges, 2) the end points of the edge dof ``n_vertices + k``."""
    cells = np.asarray(cells, dtype=np.int64)
    tdim = cells.shape[1] - 1
    nv = int(cells.max()) + 1
    pairs = np.stack([np.sort(cells[:, list(e)], axis=1) for e in BASIX_EDGES[tdim]], axis=1)   # (n_cells, n_e, 2)
    uniq, inv = np.unique(pairs.reshape(-1, 2), axis=0, return_inverse=True)
    dofmap = np.concatenate([cells, nv + inv.reshape(len(cells), -1)], axis=1).astype(np.int32)
    return dofmap, nv + len(uniq), uniq


class SimplexMesh(_DeviceMesh):
    """Lagrange displacement of any order on straight-sided simplices (``dxm_mesh_create_simplex``): the P2 spaces of the
    reference's demos (tet10 with 4 Gauss points, ``finite_strain_elastoplasticity.py:115-117``; tri6 with 3, embedded as
    plane strain, ``plane_elastoplasticity.py:96-100``).

    ``coords`` (n_vertices, 2|3) and ``geom_conn`` (n_cells, tdim+1) give the affine geometry; ``dofmap`` (n_cells, nd)
    indexes the ``n_dofs`` blocks of ``tdim`` displacement components; ``dphi`` (nqp, nd, tdim) are the reference
    derivatives of the nd shape functions at the Gauss points (:func:`lagrange_simplex_table`, or basix's tabulation).
    Gauss point ``q`` of cell ``c`` is point ``c * nqp + q``."""

    def __init__(self, coords, geom_conn, dofmap, n_dofs, dphi, device=0):
        self._lib = _lib.load()
        geom_conn = np.ascontiguousarray(geom_conn, dtype=np.int32)
        self.tdim = geom_conn.shape[1] - 1
        coords = np.asarray(coords, dtype=np.float64)
        if coords.shape[1] == 2:
            coords = np.concatenate([coords, np.zeros((len(coords), 1))], axis=1)
        coords = np.ascontiguousarray(coords)
        dofmap = np.ascontiguousarray(dofmap, dtype=np.int32)
        dphi = np.ascontiguousarray(dphi, dtype=np.float64)
        if dphi.ndim != 3 or dphi.shape[1] != dofmap.shape[1] or dphi.shape[2] != self.tdim or len(dofmap) != len(geom_conn):
            raise ValueError("dphi must be (nqp, nd, tdim) with nd = dofmap.shape[1]; one dofmap row per cell")
        self.n_nodes, self.n_cells, self.nqp = coords.shape[0], geom_conn.shape[0], dphi.shape[0]
        self.nd, self.n_dofs, self.device = dofmap.shape[1], int(n_dofs), int(device)
        h = self._lib.dxm_mesh_create_simplex(self.tdim, coords.ctypes.data, self.n_nodes, geom_conn.ctypes.data, self.n_cells,
                                              dofmap.ctypes.data, self.nd, self.n_dofs, dphi.ctypes.data, self.nqp, self.device)
        if not h:
            raise _lib.DxmError(f"dxm_mesh_create_simplex failed: {_lib.last_error()}")
        self._handle = h

    @classmethod
    def lagrange(cls, coords, cells, degree=2, quadrature_degree=None, device=0):
        """Stand-alone constructor (no dolfinx): P1 or P2 displacement on the vertex mesh ``(coords, cells)``; P2 dofs as
        numbered by :func:`p2_dofmap`.  Returns ``(mesh, dof_coords)`` with the (n_dofs, coords.shape[1]) dof positions."""
        coords, cells = np.asarray(coords, dtype=np.float64), np.asarray(cells)
        tdim = cells.shape[1] - 1
        qdeg = 2 * (degree - 1) if quadrature_degree is None else quadrature_degree
        dphi = lagrange_simplex_table(tdim, degree, simplex_quadrature(tdim, qdeg))
        if degree == 1:
            return cls(coords, cells, cells, len(coords), dphi, device=device), coords.copy()
        dofmap, n_dofs, edges = p2_dofmap(cells)
        dof_coords = np.concatenate([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]])], axis=0)
        return cls(coords, cells, dofmap, n_dofs, dphi, device=device), dof_coords

    @classmethod
    def from_dolfinx(cls, V, quadrature_degree, device=0, cells=None):
        """From a dolfinx vector Lagrange space (any order, block size = topological dimension; ``cells``: those of one
        ``QuadratureMap`` instead of all) on a first-order
        (straight-sided) triangle or tetrahedron mesh: geometry from ``mesh.geometry``, the dofmap of ``V`` as it is,
        Gauss points and tabulated derivatives from basix -- so point ``c * nqp + q`` is row ``c * nqp + q`` of the
        quadrature Functions (``quadrature_map.py:239-260``) and ``u.x.array`` is the vector to hand to
        ``integrate_displacement``."""
        import basix

        mesh = V.mesh
        tdim = mesh.topology.dim
        if tdim not in (2, 3) or V.dofmap.index_map_bs != tdim:
            raise ValueError("SimplexMesh.from_dolfinx needs a vector Lagrange space with block size = topological dimension")
        geom_conn = np.asarray(mesh.geometry.dofmap, dtype=np.int32)
        if geom_conn.ndim == 1:
            geom_conn = geom_conn.reshape(-1, tdim + 1)
        if geom_conn.shape[1] != tdim + 1:
            raise ValueError("SimplexMesh.from_dolfinx needs a first-order (affine) simplex geometry")
        dofmap = np.asarray(V.dofmap.list, dtype=np.int32)
        if dofmap.ndim == 1:
            dofmap = dofmap.reshape(len(geom_conn), -1)
        n_dofs = V.dofmap.index_map.size_local + V.dofmap.index_map.num_ghosts
        cell = basix.CellType.triangle if tdim == 2 else basix.CellType.tetrahedron
        pts, _ = basix.make_quadrature(cell, int(quadrature_degree))
        tab = np.asarray(V.element.basix_element.tabulate(1, np.asarray(pts)))
        if tab.ndim == 4:
            tab = tab[..., 0]
        if tab.shape[2] != dofmap.shape[1]:   # blocked element tabulated with its block: scalar basis is every bs-th
            tab = tab[:, :, ::tdim]
        dphi = np.ascontiguousarray(tab[1:1 + tdim].transpose(1, 2, 0))
        if cells is not None:
            geom_conn, dofmap = geom_conn[np.asarray(cells)], dofmap[np.asarray(cells)]
        return cls(np.asarray(mesh.geometry.x), geom_conn, dofmap, n_dofs, dphi, device=device)


# ---- plane meshes: triangles and bilinear quadrilaterals ---------------------------------------------------------------------------
#: local vertex pairs of the edges of the reference quadrilateral [0,1]^2 (vertices (0,0),(1,0),(0,1),(1,1)) in basix's edge numbering
BASIX_QUAD_EDGES = ((0, 1), (0, 2), (1, 3), (2, 3))
#: the 1-D node (0: x = 0, 1: x = 1, 2: x = 1/2) in each direction of the nine Q2 dofs in basix's order: vertices, edges, interior
_Q2_NODES = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (1, 2), (2, 1), (2, 2))


def quad_quadrature(degree):
    """Tensor Gauss-Legendre points (nqp, 2) on [0,1]^2 exact for polynomials of the given degree per direction (``degree // 2 + 1``
    points per direction), second coordinate fastest.  For stand-alone use and tests; with dolfinx take basix's points
    (:meth:`PlaneMesh.from_dolfinx` does), whose order defines the row order of the quadrature Functions."""
    n = int(degree) // 2 + 1
    x, _ = np.polynomial.legendre.leggauss(n)
    x = 0.5 * (x + 1.0)
    return np.array([[a, b] for a in x for b in x])


def lagrange_quad_table(degree, points):
    """Reference derivatives ``dphi[q, m, d] = d N_m / d xi_d`` of the tensor-product Lagrange basis Q1 or Q2 on [0,1]^2 at ``points``
    (nqp, 2), dofs in basix's order: vertices (0,0),(1,0),(0,1),(1,1), then the midpoints of the edges :data:`BASIX_QUAD_EDGES`, then
    the interior dof.  ``N = L_i(x) L_j(y)`` with the 1-D bases ``1 - t, t`` (Q1) and ``(1 - t)(1 - 2t), t (2t - 1), 4 t (1 - t)``."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if degree == 1:
        L = [np.stack([1.0 - pts[:, d], pts[:, d]], axis=1) for d in range(2)]
        dL = [np.stack([-np.ones(len(pts)), np.ones(len(pts))], axis=1) for d in range(2)]
        nodes = _Q2_NODES[:4]
    elif degree == 2:
        L = [np.stack([(1.0 - t) * (1.0 - 2.0 * t), t * (2.0 * t - 1.0), 4.0 * t * (1.0 - t)], axis=1) for t in (pts[:, 0], pts[:, 1])]
        dL = [np.stack([4.0 * t - 3.0, 4.0 * t - 1.0, 4.0 - 8.0 * t], axis=1) for t in (pts[:, 0], pts[:, 1])]
        nodes = _Q2_NODES
    else:
        raise ValueError("lagrange_quad_table: degree 1 or 2 (hand any other table to PlaneMesh directly)")
    cols = [np.stack([dL[0][:, i] * L[1][:, j], L[0][:, i] * dL[1][:, j]], axis=1) for i, j in nodes]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def q2_dofmap(cells):
    """Second-order Lagrange (Q2) dofmap of a quadrilateral mesh given by its vertex table ``cells`` (n_cells, 4), vertices in
    basix's order: vertex dofs keep the vertex numbers, then one dof per unique edge, then one per cell.  Returns
    ``(dofmap (n_cells, 9), n_dofs, edge_vertices)`` with ``edge_vertices`` (n_edges, 2) the end points of the edge dof
    ``n_vertices + k``; the interior dof of cell ``c`` is ``n_vertices + n_edges + c``."""
    cells = np.asarray(cells, dtype=np.int64)
    nv = int(cells.max()) + 1
    pairs = np.stack([np.sort(cells[:, list(e)], axis=1) for e in BASIX_QUAD_EDGES], axis=1)   # (n_cells, 4, 2)
    uniq, inv = np.unique(pairs.reshape(-1, 2), axis=0, return_inverse=True)
    inner = nv + len(uniq) + np.arange(len(cells))
    dofmap = np.concatenate([cells, nv + inv.reshape(len(cells), -1), inner[:, None]], axis=1).astype(np.int32)
    return dofmap, nv + len(uniq) + len(cells), uniq


class PlaneMesh(_DeviceMesh):
    """Lagrange displacement of any order on a two-dimensional mesh of triangles or bilinear quadrilaterals
    (``dxm_mesh_create_plane``): the N x N quadrilaterals of the reference's ``tests/uniaxial_tension.py`` and the tri6 mesh of
    ``plane_elastoplasticity.py``.  It answers the four kinds of :meth:`gradient_device`, so it serves the 4-wide plane-strain laws,
    the 3-wide plane-stress laws and, embedded, the 6-wide and 9-wide laws.

    ``coords`` (n_vertices, 2|3) and ``geom_conn`` (n_cells, 3|4) give the geometry, ``geom_dphi`` (nqp, nv, 2) the reference
    derivatives of ITS shape functions at the Gauss points (quadrilaterals: :func:`lagrange_quad_table` of degree 1, vertices in
    basix's order (0,0),(1,0),(0,1),(1,1)); ``dofmap`` (n_cells, nd) indexes the ``n_dofs`` blocks of two displacement components
    and ``dphi`` (nqp, nd, 2) are the derivatives of the field's shape functions at the same points.  Gauss point ``q`` of cell
    ``c`` is point ``c * nqp + q``.  The library checks every index and ``det J`` at every Gauss point before it touches a device."""

    tdim = 2

    def __init__(self, coords, geom_conn, dofmap, n_dofs, geom_dphi, dphi, device=0):
        self._lib = _lib.load()
        geom_conn = np.ascontiguousarray(geom_conn, dtype=np.int32)
        coords = np.asarray(coords, dtype=np.float64)
        if coords.shape[1] == 2:
            coords = np.concatenate([coords, np.zeros((len(coords), 1))], axis=1)
        coords = np.ascontiguousarray(coords)
        dofmap = np.ascontiguousarray(dofmap, dtype=np.int32)
        geom_dphi = np.ascontiguousarray(geom_dphi, dtype=np.float64)
        dphi = np.ascontiguousarray(dphi, dtype=np.float64)
        if dphi.ndim != 3 or dphi.shape[1] != dofmap.shape[1] or dphi.shape[2] != 2 or len(dofmap) != len(geom_conn):
            raise ValueError("dphi must be (nqp, nd, 2) with nd = dofmap.shape[1]; one dofmap row per cell")
        if geom_dphi.shape != (dphi.shape[0], geom_conn.shape[1], 2):
            raise ValueError("geom_dphi must be (nqp, nv, 2) with nv = geom_conn.shape[1] and the nqp of dphi")
        self.n_nodes, self.n_cells, self.nqp = coords.shape[0], geom_conn.shape[0], dphi.shape[0]
        self.nv, self.nd, self.n_dofs, self.device = geom_conn.shape[1], dofmap.shape[1], int(n_dofs), int(device)
        h = self._lib.dxm_mesh_create_plane(coords.ctypes.data, self.n_nodes, geom_conn.ctypes.data, self.nv, self.n_cells,
                                            dofmap.ctypes.data, self.nd, self.n_dofs, geom_dphi.ctypes.data, dphi.ctypes.data,
                                            self.nqp, self.device)
        if not h:
            raise _lib.DxmError(f"dxm_mesh_create_plane failed: {_lib.last_error()}")
        self._handle = h

    @classmethod
    def lagrange(cls, coords, cells, degree=1, quadrature_degree=None, device=0):
        """Stand-alone constructor (no dolfinx): first- or second-order displacement on the vertex mesh ``(coords, cells)`` of
        triangles (three columns; P2 dofs as numbered by :func:`p2_dofmap`, points of :func:`simplex_quadrature`, default degree
        ``2 (degree - 1)``) or quadrilaterals (four columns in basix's vertex order; Q2 dofs as numbered by :func:`q2_dofmap`,
        points of :func:`quad_quadrature`, default degree ``2 degree``).  Returns ``(mesh, dof_coords)`` with the
        (n_dofs, coords.shape[1]) dof positions."""
        coords, cells = np.asarray(coords, dtype=np.float64), np.asarray(cells)
        if degree not in (1, 2):
            raise ValueError("PlaneMesh.lagrange: degree 1 or 2 (hand any other table to PlaneMesh directly)")
        if cells.shape[1] == 3:
            pts = simplex_quadrature(2, 2 * (degree - 1) if quadrature_degree is None else quadrature_degree)
            geom_dphi, dphi = lagrange_simplex_table(2, 1, pts), lagrange_simplex_table(2, degree, pts)
            dofmap, n_dofs, edges = p2_dofmap(cells) if degree == 2 else (cells, len(coords), None)
            inner = np.empty((0, coords.shape[1]))
        elif cells.shape[1] == 4:
            pts = quad_quadrature(2 * degree if quadrature_degree is None else quadrature_degree)
            geom_dphi, dphi = lagrange_quad_table(1, pts), lagrange_quad_table(degree, pts)
            dofmap, n_dofs, edges = q2_dofmap(cells) if degree == 2 else (cells, len(coords), None)
            inner = coords[cells].mean(axis=1)            # the bilinear image of (1/2, 1/2)
        else:
            raise ValueError("PlaneMesh.lagrange: cells with 3 (triangles) or 4 (quadrilaterals) vertices")
        mesh = cls(coords, cells, dofmap, n_dofs, geom_dphi, dphi, device=device)
        if degree == 1:
            return mesh, coords.copy()
        return mesh, np.concatenate([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]]), inner], axis=0)

    @classmethod
    def from_dolfinx(cls, V, quadrature_degree, device=0, cells=None):
        """From a dolfinx vector Lagrange space (any order, block size 2; ``cells``: those of one ``QuadratureMap`` instead of all)
        on a first-order triangle or quadrilateral mesh: geometry from ``mesh.geometry`` with the table of basix's first-order
        coordinate element, the dofmap of ``V`` as it is, Gauss points and the field's tabulated derivatives from basix -- so point
        ``c * nqp + q`` is row ``c * nqp + q`` of the quadrature Functions and ``u.x.array`` is the vector to hand to
        ``integrate_displacement``.  UNTESTED without dolfinx."""
        import basix

        mesh = V.mesh
        if mesh.topology.dim != 2 or V.dofmap.index_map_bs != 2:
            raise ValueError("PlaneMesh.from_dolfinx needs a vector Lagrange space with block size 2 on a two-dimensional mesh")
        dofmap = np.asarray(V.dofmap.list, dtype=np.int32)
        n_cells = dofmap.shape[0] if dofmap.ndim == 2 else len(dofmap) // len(V.dofmap.cell_dofs(0))
        dofmap = dofmap.reshape(n_cells, -1)
        geom_conn = np.asarray(mesh.geometry.dofmap, dtype=np.int32).reshape(n_cells, -1)
        nv = geom_conn.shape[1]
        if nv not in (3, 4):
            raise ValueError("PlaneMesh.from_dolfinx needs a first-order triangle or quadrilateral geometry (no curved cells)")
        cell = basix.CellType.triangle if nv == 3 else basix.CellType.quadrilateral
        pts, _ = basix.make_quadrature(cell, int(quadrature_degree))
        pts = np.asarray(pts)

        def table(element, nd):
            tab = np.asarray(element.tabulate(1, pts))
            if tab.ndim == 4:
                tab = tab[..., 0]
            if tab.shape[2] != nd:      # blocked element tabulated with its block: the scalar basis is every second function
                tab = tab[:, :, ::2]
            return np.ascontiguousarray(tab[1:3].transpose(1, 2, 0))

        geom_dphi = table(basix.create_element(basix.ElementFamily.P, cell, 1), nv)
        dphi = table(V.element.basix_element, dofmap.shape[1])
        n_dofs = V.dofmap.index_map.size_local + V.dofmap.index_map.num_ghosts
        if cells is not None:
            geom_conn, dofmap = geom_conn[np.asarray(cells)], dofmap[np.asarray(cells)]
        return cls(np.asarray(mesh.geometry.x), geom_conn, dofmap, n_dofs, geom_dphi, dphi, device=device)


# ---- a scalar field on a plane mesh: the temperature of the two-dimensional heat-transfer laws -------------------------------------
def lagrange_simplex_values(tdim, degree, points):
    """Values ``phi[q, m] = N_m(xi_q)`` of the Lagrange basis of the given degree (1 or 2) on the reference simplex at ``points``
    (nqp, tdim): the table beside :func:`lagrange_simplex_table`, dofs in the same order."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, tdim)
    lam = np.concatenate([1.0 - pts.sum(axis=1, keepdims=True), pts], axis=1)          # (nqp, tdim+1)
    if degree == 1:
        return np.ascontiguousarray(lam)
    if degree != 2:
        raise ValueError("lagrange_simplex_values: degree 1 or 2 (hand any other table to PlaneScalarMesh directly)")
    cols = [lam[:, v] * (2.0 * lam[:, v] - 1.0) for v in range(tdim + 1)]
    cols += [4.0 * lam[:, i] * lam[:, j] for i, j in BASIX_EDGES[tdim]]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def lagrange_quad_values(degree, points):
    """Values ``phi[q, m] = N_m(xi_q)`` of the tensor-product Lagrange basis Q1 or Q2 on [0,1]^2 at ``points`` (nqp, 2): the table
    beside :func:`lagrange_quad_table`, dofs in the same order."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if degree == 1:
        L = [np.stack([1.0 - pts[:, d], pts[:, d]], axis=1) for d in range(2)]
        nodes = _Q2_NODES[:4]
    elif degree == 2:
        L = [np.stack([(1.0 - t) * (1.0 - 2.0 * t), t * (2.0 * t - 1.0), 4.0 * t * (1.0 - t)], axis=1) for t in (pts[:, 0], pts[:, 1])]
        nodes = _Q2_NODES
    else:
        raise ValueError("lagrange_quad_values: degree 1 or 2 (hand any other table to PlaneScalarMesh directly)")
    return np.ascontiguousarray(np.stack([L[0][:, i] * L[1][:, j] for i, j in nodes], axis=1))


class PlaneScalarMesh(_DeviceMesh):
    """A scalar Lagrange field of any order -- a temperature -- on a two-dimensional mesh of triangles or bilinear quadrilaterals
    (``dxm_mesh_create_plane_scalar``): what the reference's heat-transfer demos differentiate (``ufl.grad(T)``, 2 wide, with ``T``
    itself as the external state variable).  Arguments as for :class:`PlaneMesh`, with ONE value per dof and the table ``phi``
    (nqp, nd) of the field's shape functions at the Gauss points beside their derivatives ``dphi`` (nqp, nd, 2).

    With a heat-transfer material of ``hypothesis="plane_strain"`` the mesh goes where a displacement mesh goes
    (``HIPMaterial.integrate_displacement*``, ``QuadratureMap.register_device_gradient``) and the nodal temperature where the
    displacement goes: the update kernel interpolates ``T`` and ``grad(T)`` at its own points.  :meth:`gradient_device` refuses:
    :meth:`scalar_gradient_device` is this mesh's stand-alone evaluation."""

    tdim = 2
    #: the external state variable the nodal forms interpolate themselves (a ``QuadratureMap`` does not upload it then)
    nodal_variable = "Temperature"

    def __init__(self, coords, geom_conn, dofmap, n_dofs, geom_dphi, phi, dphi, device=0):
        self._lib = _lib.load()
        geom_conn = np.ascontiguousarray(geom_conn, dtype=np.int32)
        coords = np.asarray(coords, dtype=np.float64)
        if coords.shape[1] == 2:
            coords = np.concatenate([coords, np.zeros((len(coords), 1))], axis=1)
        coords = np.ascontiguousarray(coords)
        dofmap = np.ascontiguousarray(dofmap, dtype=np.int32)
        geom_dphi = np.ascontiguousarray(geom_dphi, dtype=np.float64)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        dphi = np.ascontiguousarray(dphi, dtype=np.float64)
        if dphi.ndim != 3 or dphi.shape[1] != dofmap.shape[1] or dphi.shape[2] != 2 or len(dofmap) != len(geom_conn):
            raise ValueError("dphi must be (nqp, nd, 2) with nd = dofmap.shape[1]; one dofmap row per cell")
        if phi.shape != dphi.shape[:2]:
            raise ValueError("phi must be (nqp, nd), the values beside the derivatives dphi (nqp, nd, 2)")
        if geom_dphi.shape != (dphi.shape[0], geom_conn.shape[1], 2):
            raise ValueError("geom_dphi must be (nqp, nv, 2) with nv = geom_conn.shape[1] and the nqp of dphi")
        self.n_nodes, self.n_cells, self.nqp = coords.shape[0], geom_conn.shape[0], dphi.shape[0]
        self.nv, self.nd, self.n_dofs, self.device = geom_conn.shape[1], dofmap.shape[1], int(n_dofs), int(device)
        h = self._lib.dxm_mesh_create_plane_scalar(coords.ctypes.data, self.n_nodes, geom_conn.ctypes.data, self.nv, self.n_cells,
                                                   dofmap.ctypes.data, self.nd, self.n_dofs, geom_dphi.ctypes.data, phi.ctypes.data,
                                                   dphi.ctypes.data, self.nqp, self.device)
        if not h:
            raise _lib.DxmError(f"dxm_mesh_create_plane_scalar failed: {_lib.last_error()}")
        self._handle = h

    def scalar_gradient_device(self, t_ptr, grad_ptr, value_ptr=0, stream=0):
        """Device pointers, asynchronous on ``stream``: ``grad(T)`` into ``grad_ptr`` (npoints, 2) and, unless ``value_ptr`` is 0,
        ``T`` into ``value_ptr`` (npoints) at the Gauss points from the ``n_dofs`` nodal values at ``t_ptr``."""
        _lib.check(self._lib.dxm_mesh_scalar_gradient_device(self._handle, int(t_ptr), int(grad_ptr), int(value_ptr) or None,
                                                             int(stream) or None))

    @classmethod
    def lagrange(cls, coords, cells, degree=1, quadrature_degree=None, device=0):
        """Stand-alone constructor (no dolfinx), the mirror of :meth:`PlaneMesh.lagrange`: a first- or second-order scalar field on
        the vertex mesh ``(coords, cells)`` of triangles or quadrilaterals, the same dof numbering, points and default quadrature
        degrees.  Returns ``(mesh, dof_coords)``."""
        coords, cells = np.asarray(coords, dtype=np.float64), np.asarray(cells)
        if degree not in (1, 2):
            raise ValueError("PlaneScalarMesh.lagrange: degree 1 or 2 (hand any other table to PlaneScalarMesh directly)")
        if cells.shape[1] == 3:
            pts = simplex_quadrature(2, 2 * (degree - 1) if quadrature_degree is None else quadrature_degree)
            geom_dphi, dphi, phi = lagrange_simplex_table(2, 1, pts), lagrange_simplex_table(2, degree, pts), lagrange_simplex_values(2, degree, pts)
            dofmap, n_dofs, edges = p2_dofmap(cells) if degree == 2 else (cells, len(coords), None)
            inner = np.empty((0, coords.shape[1]))
        elif cells.shape[1] == 4:
            pts = quad_quadrature(2 * degree if quadrature_degree is None else quadrature_degree)
            geom_dphi, dphi, phi = lagrange_quad_table(1, pts), lagrange_quad_table(degree, pts), lagrange_quad_values(degree, pts)
            dofmap, n_dofs, edges = q2_dofmap(cells) if degree == 2 else (cells, len(coords), None)
            inner = coords[cells].mean(axis=1)            # the bilinear image of (1/2, 1/2)
        else:
            raise ValueError("PlaneScalarMesh.lagrange: cells with 3 (triangles) or 4 (quadrilaterals) vertices")
        mesh = cls(coords, cells, dofmap, n_dofs, geom_dphi, phi, dphi, device=device)
        if degree == 1:
            return mesh, coords.copy()
        return mesh, np.concatenate([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]]), inner], axis=0)

    @classmethod
    def from_dolfinx(cls, V, quadrature_degree, device=0, cells=None):
        """From a dolfinx SCALAR Lagrange space (any order, block size 1; ``cells``: those of one ``QuadratureMap`` instead of all)
        on a first-order triangle or quadrilateral mesh, as :meth:`PlaneMesh.from_dolfinx` does for a vector space: point
        ``c * nqp + q`` is row ``c * nqp + q`` of the quadrature Functions and ``T.x.array`` is the vector to hand to
        ``integrate_displacement``.  UNTESTED without dolfinx."""
        import basix

        mesh = V.mesh
        if mesh.topology.dim != 2 or V.dofmap.index_map_bs != 1:
            raise ValueError("PlaneScalarMesh.from_dolfinx needs a scalar Lagrange space (block size 1) on a two-dimensional mesh")
        dofmap = np.asarray(V.dofmap.list, dtype=np.int32)
        n_cells = dofmap.shape[0] if dofmap.ndim == 2 else len(dofmap) // len(V.dofmap.cell_dofs(0))
        dofmap = dofmap.reshape(n_cells, -1)
        geom_conn = np.asarray(mesh.geometry.dofmap, dtype=np.int32).reshape(n_cells, -1)
        nv = geom_conn.shape[1]
        if nv not in (3, 4):
            raise ValueError("PlaneScalarMesh.from_dolfinx needs a first-order triangle or quadrilateral geometry (no curved cells)")
        cell = basix.CellType.triangle if nv == 3 else basix.CellType.quadrilateral
        pts, _ = basix.make_quadrature(cell, int(quadrature_degree))
        pts = np.asarray(pts)

        def tables(element):
            tab = np.asarray(element.tabulate(1, pts))
            if tab.ndim == 4:
                tab = tab[..., 0]
            return np.ascontiguousarray(tab[0]), np.ascontiguousarray(tab[1:3].transpose(1, 2, 0))

        _, geom_dphi = tables(basix.create_element(basix.ElementFamily.P, cell, 1))
        phi, dphi = tables(V.element.basix_element)
        n_dofs = V.dofmap.index_map.size_local + V.dofmap.index_map.num_ghosts
        if cells is not None:
            geom_conn, dofmap = geom_conn[np.asarray(cells)], dofmap[np.asarray(cells)]
        return cls(np.asarray(mesh.geometry.x), geom_conn, dofmap, n_dofs, geom_dphi, phi, dphi, device=device)


# ---- axisymmetric meshes: the meridian half plane (r, z) ----------------------------------------------------------------------------
def axisymmetric_radii(coords, geom_conn, geom_phi):
    """``r = sum_v r_v geom_phi[q, v]`` at the Gauss points of a meridian mesh, (n_cells * nqp), summed in the table's local order
    from 0.0 as the library's check and the kernel do: what :meth:`AxisymmetricMesh.radii` returns.  No GPU."""
    r = np.asarray(coords, dtype=np.float64)[np.asarray(geom_conn), 0]
    geom_phi = np.asarray(geom_phi, dtype=np.float64)
    rad = np.zeros((r.shape[0], geom_phi.shape[0]))
    for v in range(r.shape[1]):
        rad = rad + r[:, v, None] * geom_phi[None, :, v]
    return rad.reshape(-1)


class AxisymmetricMesh(_DeviceMesh):
    """Lagrange displacement ``(u_r, u_z)`` of any order on a MERIDIAN mesh of triangles or bilinear quadrilaterals
    (``dxm_mesh_create_axisymmetric``): column 0 of ``coords`` is ``r``, column 1 is ``z``.  This is the reference's
    ``hypothesis="axisymmetric"``.  Under MGIS that hypothesis has the slots of the plane-strain one -- ``[rr, zz, tt, sqrt(2) rz]`` for a
    symmetric tensor, ``[F_rr, F_zz, F_tt, F_rz, F_zr]`` for ``F`` -- and an isotropic behaviour does nothing different; what changes is
    the caller's gradient, ``eps_tt = u_r / r`` and ``F_tt = 1 + u_r / r``.  So the hypothesis lives on the MESH: a behaviour built with
    ``hypothesis="plane_strain"`` (or a ``"3d"`` one) on this mesh IS the axisymmetric law; the string ``"axisymmetric"`` itself is
    still refused by the behaviours.

    Arguments as for :class:`PlaneMesh`, plus the VALUES of the shape functions at the Gauss points: ``geom_phi`` (nqp, nv) of the
    geometry's (for ``r``) and ``phi`` (nqp, nd) of the field's (for ``u_r``).  The library checks, before it touches a device, every
    index, ``det J``, every table entry and ``r > 0`` at every Gauss point: the mesh lies on one side of the axis.

    The mesh goes where a :class:`PlaneMesh` goes (``HIPMaterial.integrate_displacement*``,
    ``QuadratureMap.register_device_gradient``): the 4-wide plane-strain laws, the 6-wide and the 9-wide laws.  The 5-wide laws (Ogden and
    logarithmic-strain plasticity under plane strain) take kind 1 of :meth:`axisymmetric_gradient_device` followed by the array form;
    the plane-stress and heat-transfer laws are refused.  :meth:`gradient_device` refuses.  :meth:`radii` gives ``r`` at the Gauss
    points for the measure ``2 pi r w |det J|`` (assembly is the caller's)."""

    tdim = 2
    #: the gradients of this mesh carry the hoop term: :meth:`axisymmetric_gradient_device`, not :meth:`gradient_device`
    axisymmetric = True

    def __init__(self, coords, geom_conn, dofmap, n_dofs, geom_phi, geom_dphi, phi, dphi, device=0):
        self._lib = _lib.load()
        geom_conn = np.ascontiguousarray(geom_conn, dtype=np.int32)
        coords = np.asarray(coords, dtype=np.float64)
        if coords.shape[1] == 2:
            coords = np.concatenate([coords, np.zeros((len(coords), 1))], axis=1)
        coords = np.ascontiguousarray(coords)
        dofmap = np.ascontiguousarray(dofmap, dtype=np.int32)
        geom_phi = np.ascontiguousarray(geom_phi, dtype=np.float64)
        geom_dphi = np.ascontiguousarray(geom_dphi, dtype=np.float64)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        dphi = np.ascontiguousarray(dphi, dtype=np.float64)
        if dphi.ndim != 3 or dphi.shape[1] != dofmap.shape[1] or dphi.shape[2] != 2 or len(dofmap) != len(geom_conn):
            raise ValueError("dphi must be (nqp, nd, 2) with nd = dofmap.shape[1]; one dofmap row per cell")
        if phi.shape != dphi.shape[:2]:
            raise ValueError("phi must be (nqp, nd), the values beside the derivatives dphi (nqp, nd, 2)")
        if geom_dphi.shape != (dphi.shape[0], geom_conn.shape[1], 2):
            raise ValueError("geom_dphi must be (nqp, nv, 2) with nv = geom_conn.shape[1] and the nqp of dphi")
        if geom_phi.shape != geom_dphi.shape[:2]:
            raise ValueError("geom_phi must be (nqp, nv), the values beside the derivatives geom_dphi (nqp, nv, 2)")
        self.n_nodes, self.n_cells, self.nqp = coords.shape[0], geom_conn.shape[0], dphi.shape[0]
        self.nv, self.nd, self.n_dofs, self.device = geom_conn.shape[1], dofmap.shape[1], int(n_dofs), int(device)
        h = self._lib.dxm_mesh_create_axisymmetric(coords.ctypes.data, self.n_nodes, geom_conn.ctypes.data, self.nv, self.n_cells,
                                                   dofmap.ctypes.data, self.nd, self.n_dofs, geom_phi.ctypes.data, geom_dphi.ctypes.data,
                                                   phi.ctypes.data, dphi.ctypes.data, self.nqp, self.device)
        if not h:
            raise _lib.DxmError(f"dxm_mesh_create_axisymmetric failed: {_lib.last_error()}")
        self._handle = h
        self._radii = axisymmetric_radii(coords, geom_conn, geom_phi)

    def gradient_device(self, u_ptr, kind, grad_ptr, stream=0):
        """Refused with the library's sentence: no kind of ``dxm_mesh_gradient_device`` holds the hoop term.  Use
        :meth:`axisymmetric_gradient_device`."""
        super().gradient_device(u_ptr, kind, grad_ptr, stream)

    def axisymmetric_gradient_device(self, u_ptr, kind, grad_ptr, radius_ptr=0, stream=0):
        """Device pointers, asynchronous on ``stream``.  With ``H[i][a] = du_i / dX_a`` in ``(r, z)``, ``hoop = u_r / r`` and
        ``s = sqrt(2) / 2``, ``kind`` (numbered by this entry point alone)

        * 0: ``[H00, H11, hoop, s (H01 + H10)]``, the strain of the ``hypothesis="plane_strain"`` laws (4);
        * 1: ``[1 + H00, 1 + H11, 1 + hoop, H01, H10]``, the ``F`` of the 5-wide laws (5);
        * 2: ``[H00, H11, hoop, s (H01 + H10), 0, 0]``, the Mandel strain of the 6-wide laws (6);
        * 3: ``[1 + H00, 1 + H11, 1 + hoop, H01, H10, 0, 0, 0, 0]``, the ``F`` of the 9-wide laws (9).

        ``grad_ptr`` holds ``npoints`` rows (16-byte aligned for kinds 0 and 2); unless ``radius_ptr`` is 0, ``r`` at the Gauss points
        goes into its ``npoints`` doubles."""
        _lib.check(self._lib.dxm_mesh_axisymmetric_gradient_device(self._handle, int(u_ptr), int(kind), int(grad_ptr),
                                                                   int(radius_ptr) or None, int(stream) or None))

    def radii(self):
        """``r`` at the Gauss points, host array (npoints), from the tables alone (no GPU): the measure of the hypothesis is
        ``2 pi r w |det J|``."""
        return self._radii.copy()

    @classmethod
    def lagrange(cls, coords, cells, degree=1, quadrature_degree=None, device=0):
        """Stand-alone constructor (no dolfinx), the mirror of :meth:`PlaneMesh.lagrange`: a first- or second-order displacement on
        the vertex mesh ``(coords, cells)`` of triangles or quadrilaterals in the ``(r, z)`` half plane, the same dof numbering, points
        and default quadrature degrees.  Returns ``(mesh, dof_coords)``."""
        coords, cells = np.asarray(coords, dtype=np.float64), np.asarray(cells)
        if degree not in (1, 2):
            raise ValueError("AxisymmetricMesh.lagrange: degree 1 or 2 (hand any other table to AxisymmetricMesh directly)")
        if cells.shape[1] == 3:
            pts = simplex_quadrature(2, 2 * (degree - 1) if quadrature_degree is None else quadrature_degree)
            geom_phi, geom_dphi = lagrange_simplex_values(2, 1, pts), lagrange_simplex_table(2, 1, pts)
            phi, dphi = lagrange_simplex_values(2, degree, pts), lagrange_simplex_table(2, degree, pts)
            dofmap, n_dofs, edges = p2_dofmap(cells) if degree == 2 else (cells, len(coords), None)
            inner = np.empty((0, coords.shape[1]))
        elif cells.shape[1] == 4:
            pts = quad_quadrature(2 * degree if quadrature_degree is None else quadrature_degree)
            geom_phi, geom_dphi = lagrange_quad_values(1, pts), lagrange_quad_table(1, pts)
            phi, dphi = lagrange_quad_values(degree, pts), lagrange_quad_table(degree, pts)
            dofmap, n_dofs, edges = q2_dofmap(cells) if degree == 2 else (cells, len(coords), None)
            inner = coords[cells].mean(axis=1)            # the bilinear image of (1/2, 1/2)
        else:
            raise ValueError("AxisymmetricMesh.lagrange: cells with 3 (triangles) or 4 (quadrilaterals) vertices")
        mesh = cls(coords, cells, dofmap, n_dofs, geom_phi, geom_dphi, phi, dphi, device=device)
        if degree == 1:
            return mesh, coords.copy()
        return mesh, np.concatenate([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]]), inner], axis=0)

    @classmethod
    def from_dolfinx(cls, V, quadrature_degree, device=0, cells=None):
        """From a dolfinx vector Lagrange space (any order, block size 2; ``cells``: those of one ``QuadratureMap`` instead of all)
        on a first-order triangle or quadrilateral mesh whose ``x`` is ``r`` and whose ``y`` is ``z``, as
        :meth:`PlaneMesh.from_dolfinx`: point ``c * nqp + q`` is row ``c * nqp + q`` of the quadrature Functions and ``u.x.array`` is
        the vector to hand to ``integrate_displacement``.  UNTESTED without dolfinx."""
        import basix

        mesh = V.mesh
        if mesh.topology.dim != 2 or V.dofmap.index_map_bs != 2:
            raise ValueError("AxisymmetricMesh.from_dolfinx needs a vector Lagrange space with block size 2 on a two-dimensional mesh")
        dofmap = np.asarray(V.dofmap.list, dtype=np.int32)
        n_cells = dofmap.shape[0] if dofmap.ndim == 2 else len(dofmap) // len(V.dofmap.cell_dofs(0))
        dofmap = dofmap.reshape(n_cells, -1)
        geom_conn = np.asarray(mesh.geometry.dofmap, dtype=np.int32).reshape(n_cells, -1)
        nv = geom_conn.shape[1]
        if nv not in (3, 4):
            raise ValueError("AxisymmetricMesh.from_dolfinx needs a first-order triangle or quadrilateral geometry (no curved cells)")
        cell = basix.CellType.triangle if nv == 3 else basix.CellType.quadrilateral
        pts, _ = basix.make_quadrature(cell, int(quadrature_degree))
        pts = np.asarray(pts)

        def tables(element, nd):
            tab = np.asarray(element.tabulate(1, pts))
            if tab.ndim == 4:
                tab = tab[..., 0]
            if tab.shape[2] != nd:      # blocked element tabulated with its block: the scalar basis is every second function
                tab = tab[:, :, ::2]
            return np.ascontiguousarray(tab[0]), np.ascontiguousarray(tab[1:3].transpose(1, 2, 0))

        geom_phi, geom_dphi = tables(basix.create_element(basix.ElementFamily.P, cell, 1), nv)
        phi, dphi = tables(V.element.basix_element, dofmap.shape[1])
        n_dofs = V.dofmap.index_map.size_local + V.dofmap.index_map.num_ghosts
        if cells is not None:
            geom_conn, dofmap = geom_conn[np.asarray(cells)], dofmap[np.asarray(cells)]
        return cls(np.asarray(mesh.geometry.x), geom_conn, dofmap, n_dofs, geom_phi, geom_dphi, phi, dphi, device=device)
