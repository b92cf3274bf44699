"""Tensor <-> vector conventions at the boundary (reference ``dolfinx_materials/utils.py:146-212``,
``docs/intro.md:134-175``) and the host-side state conversion the FeFp law needs."""
from __future__ import annotations

import numpy as np

SQ2 = np.sqrt(2.0)
#: (row, col) of each entry of the non-symmetric 9-vector [11,22,33,12,21,13,31,23,32]
NSYM_IDX = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))


def mandel_to_tensor(v):
    v = np.asarray(v, dtype=np.float64)
    T = np.empty(v.shape[:-1] + (3, 3))
    T[..., 0, 0], T[..., 1, 1], T[..., 2, 2] = v[..., 0], v[..., 1], v[..., 2]
    T[..., 0, 1] = T[..., 1, 0] = v[..., 3] / SQ2
    T[..., 0, 2] = T[..., 2, 0] = v[..., 4] / SQ2
    T[..., 1, 2] = T[..., 2, 1] = v[..., 5] / SQ2
    return T


def tensor_to_mandel(T):
    T = np.asarray(T, dtype=np.float64)
    v = np.empty(T.shape[:-2] + (6,))
    v[..., 0], v[..., 1], v[..., 2] = T[..., 0, 0], T[..., 1, 1], T[..., 2, 2]
    v[..., 3] = SQ2 * T[..., 0, 1]
    v[..., 4] = SQ2 * T[..., 0, 2]
    v[..., 5] = SQ2 * T[..., 1, 2]
    return v


def nsym_to_tensor(v):
    v = np.asarray(v, dtype=np.float64)
    T = np.empty(v.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(NSYM_IDX):
        T[..., i, j] = v[..., k]
    return T


def tensor_to_nsym(T):
    T = np.asarray(T, dtype=np.float64)
    v = np.empty(T.shape[:-2] + (9,))
    for k, (i, j) in enumerate(NSYM_IDX):
        v[..., k] = T[..., i, j]
    return v


def cp_bar_inv_from_be_bar(F9, be_bar6):
    """Hidden FeFp state from the user-visible pair (F_n, be_bar_n):
    ``Cp_bar^-1 = J^(2/3) F^-1 be_bar F^-T`` (Mandel in, Mandel out).

    Rows whose ``be_bar`` is not positive definite (e.g. the all-zero initial value of a dolfinx
    quadrature Function handed over by ``QuadratureMap.initialize_state``,
    ``quadrature_map.py:281-295``) are replaced by the identity, the natural unstressed state the
    reference documents (``finite_strain_elastoplasticity.py:181``).
    """
    F = nsym_to_tensor(F9)
    be = mandel_to_tensor(be_bar6)
    bad = ~(np.linalg.det(be) > 0.0) | ~(be[..., 0, 0] > 0.0)
    if bad.any():
        be = be.copy()
        be[bad] = np.eye(3)
    J = np.linalg.det(F)
    Finv = np.linalg.inv(F)
    G = (J ** (2.0 / 3.0))[..., None, None] * (Finv @ be @ np.swapaxes(Finv, -1, -2))
    return tensor_to_mandel(0.5 * (G + np.swapaxes(G, -1, -2))), tensor_to_mandel(be)


def hencky_strain(F9):
    """Hencky strain ``E = 1/2 log(F^T F)`` of every row of ``F9`` (N, 9), Mandel (N, 6): what the hidden plastic strain of
    logarithmic-strain plasticity is rebuilt from, ``Ep_n = E(F_n) - ElasticStrain_n``.

    Rows that are not a deformation gradient (``det F <= 0`` or not finite, e.g. the all-zero initial value of a dolfinx quadrature
    Function handed over by ``QuadratureMap.initialize_state``) count as ``F = I``: zero strain."""
    F = nsym_to_tensor(np.asarray(F9, dtype=np.float64).reshape(-1, 9))
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~(np.isfinite(F).all(axis=(1, 2)) & (np.linalg.det(np.where(np.isfinite(F), F, 0.0)) > 0.0))
    if bad.any():
        F = F.copy()
        F[bad] = np.eye(3)
    c, V = np.linalg.eigh(np.swapaxes(F, -1, -2) @ F)
    E = (V * (0.5 * np.log(c))[:, None, :]) @ np.swapaxes(V, -1, -2)
    return tensor_to_mandel(0.5 * (E + np.swapaxes(E, -1, -2)))


#: (i, j) of the 21 entries of the symmetric-packed 6x6 tangent (upper triangle, row-major)
SYM_IDX = tuple((i, j) for i in range(6) for j in range(i, 6))


def pack_sym_tangent(ct):
    """(N,6,6) symmetric -> (N,21)."""
    ct = np.asarray(ct, dtype=np.float64).reshape(-1, 6, 6)
    ii, jj = np.array([p[0] for p in SYM_IDX]), np.array([p[1] for p in SYM_IDX])
    return ct[:, ii, jj]


def unpack_sym_tangent(ct21):
    """(N,21) -> (N,6,6) symmetric (what ``jacobian_flatten`` of quadrature_map.py:83-105 holds)."""
    ct21 = np.asarray(ct21, dtype=np.float64).reshape(-1, 21)
    out = np.empty((ct21.shape[0], 6, 6))
    for t, (i, j) in enumerate(SYM_IDX):
        out[:, i, j] = ct21[:, t]
        out[:, j, i] = ct21[:, t]
    return out


def tangent_from_coefficients(coef):
    """(N,9) ``(c1, c2, c3, n[6])`` -> (N,6,6): ``Ct = c1 1x1 + c2 I + c3 n x n`` (the ``"coef"`` tangent layout)."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 9)
    one = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    n = coef[:, 3:]
    return (coef[:, 0, None, None] * np.outer(one, one)[None] + coef[:, 1, None, None] * np.eye(6)[None]
            + coef[:, 2, None, None] * n[:, :, None] * n[:, None, :])


def tangent_from_pack4(stress, pack):
    """(N,6) stress and (N,4) ``(c1, c2, c3, w)`` of the same update -> (N,6,6) (the ``"pack4"`` tangent layout): the flow
    direction is ``n = dev(stress) w``, formed with the kernel's own three operations (``small_strain.hpp`` step 5), then
    ``Ct = c1 1x1 + c2 I + c3 n x n`` entry by entry as ``fma(c3, n_i n_j, t0)`` would (numpy rounds the product and the sum
    separately: equal to the kernel's block to 1 ulp of the ``c3`` term, not to the bit)."""
    stress = np.asarray(stress, dtype=np.float64).reshape(-1, 6)
    pack = np.asarray(pack, dtype=np.float64).reshape(-1, 4)
    third = (stress[:, 0] + stress[:, 1] + stress[:, 2]) * (1.0 / 3.0)
    n = stress * pack[:, 3:4]
    n[:, :3] = (stress[:, :3] - third[:, None]) * pack[:, 3:4]
    return tangent_from_coefficients(np.concatenate([pack[:, :3], n], axis=1))


def plane_stress_stiffness(E, nu):
    """The plane-stress stiffness on ``[xx, yy, sqrt(2) xy]`` (Kelvin-Mandel), formed as the reference forms it
    (``demos/cvxpy/cvxpy_materials.py:16-18``): ``E / (1 - nu^2) [[1, nu, 0], [nu, 1, 0], [0, 0, 1 - nu]]``."""
    return (E / (1 - nu**2)) * np.array([[1.0, nu, 0.0], [nu, 1.0, 0.0], [0.0, 0.0, (1.0 - nu)]])


def plane_stress_compliance(E, nu):
    """Its inverse in closed form: ``1 / E [[1, -nu, 0], [-nu, 1, 0], [0, 0, 1 + nu]]``."""
    return np.array([[1.0, -nu, 0.0], [-nu, 1.0, 0.0], [0.0, 0.0, 1.0 + nu]]) / E


#: positions, in the 6-wide Mandel vector, of the four components [xx, yy, zz, sqrt(2) xy] of a plane-strain state
PLANE_STRAIN_IDX = (0, 1, 2, 3)


def embed_plane_strain(v4):
    """(..., 4) ``[xx, yy, zz, sqrt(2) xy]`` (the 4-vector ``utils.py:146-150`` builds from a 2x2 tensor under the reference's
    ``hypothesis="plane_strain"``) -> (..., 6) Mandel with zero out-of-plane shears."""
    v4 = np.asarray(v4, dtype=np.float64)
    if v4.shape[-1] != 4:
        raise ValueError(f"a plane-strain vector has 4 components [xx, yy, zz, sqrt(2) xy], got shape {v4.shape}")
    out = np.zeros(v4.shape[:-1] + (6,))
    out[..., list(PLANE_STRAIN_IDX)] = v4
    return out


def restrict_plane_strain(v6):
    """(..., 6) Mandel -> (..., 4) ``[xx, yy, zz, sqrt(2) xy]``: the components a plane-strain state has (the other two are
    zero in such a state and are dropped, whatever they hold)."""
    v6 = np.asarray(v6, dtype=np.float64)
    if v6.shape[-1] != 6:
        raise ValueError(f"a Mandel vector has 6 components, got shape {v6.shape}")
    return np.ascontiguousarray(v6[..., list(PLANE_STRAIN_IDX)])


def restrict_plane_strain_tangent(C66):
    """(..., 6, 6) -> (..., 4, 4): rows and columns ``[0, 1, 2, 3]`` of a 6-wide tangent block, the block of a plane-strain law."""
    C66 = np.asarray(C66, dtype=np.float64)
    if C66.shape[-2:] != (6, 6):
        raise ValueError(f"a 6-wide tangent block is (..., 6, 6), got shape {C66.shape}")
    idx = list(PLANE_STRAIN_IDX)
    return np.ascontiguousarray(C66[..., idx, :][..., :, idx])


#: positions, in the non-symmetric 9-vector, of the five components [00, 11, 22, 01, 10] a plane deformation gradient has
#: (``utils.py:168-172``: ``nonsymmetric_tensor_to_vector`` of a 2x2 tensor with its ``T22``)
PLANE_F_IDX = (0, 1, 2, 3, 4)


def embed_plane_F(v5):
    """(..., 5) ``[F00, F11, F22, F01, F10]`` -> (..., 9) ``[11, 22, 33, 12, 21, 13, 31, 23, 32]`` with zero out-of-plane shears: the
    deformation gradient ``[[F00, F01, 0], [F10, F11, 0], [0, 0, F22]]`` of a plane-strain state."""
    v5 = np.asarray(v5, dtype=np.float64)
    if v5.shape[-1] != 5:
        raise ValueError(f"a plane deformation gradient has 5 components [F00, F11, F22, F01, F10], got shape {v5.shape}")
    out = np.zeros(v5.shape[:-1] + (9,))
    out[..., list(PLANE_F_IDX)] = v5
    return out


def restrict_plane_F(v9):
    """(..., 9) -> (..., 5) ``[00, 11, 22, 01, 10]``: the components a plane non-symmetric tensor has (the other four are zero in
    such a state and are dropped, whatever they hold)."""
    v9 = np.asarray(v9, dtype=np.float64)
    if v9.shape[-1] != 9:
        raise ValueError(f"a non-symmetric 9-vector has 9 components, got shape {v9.shape}")
    return np.ascontiguousarray(v9[..., list(PLANE_F_IDX)])


def restrict_plane_F_tangent(A99):
    """(..., 9, 9) -> (..., 5, 5): rows and columns ``[0, 1, 2, 3, 4]`` of a 9-wide ``dP/dF``, the block of the plane-strain law."""
    A99 = np.asarray(A99, dtype=np.float64)
    if A99.shape[-2:] != (9, 9):
        raise ValueError(f"a 9-wide tangent block is (..., 9, 9), got shape {A99.shape}")
    idx = list(PLANE_F_IDX)
    return np.ascontiguousarray(A99[..., idx, :][..., :, idx])


def hencky_strain_plane(F5):
    """Hencky strain of every row of ``F5`` (N, 5) ``[F00, F11, F22, F01, F10]`` as (N, 4) ``[xx, yy, zz, sqrt(2) xy]``:
    :func:`hencky_strain` of the embedded ``F``, restricted (its out-of-plane shears are zero for such an ``F``).  What the hidden
    plastic strain of plane-strain logarithmic-strain plasticity is rebuilt from.  Rows that are no deformation gradient count as
    ``F = I``, as there."""
    return restrict_plane_strain(hencky_strain(embed_plane_F(np.asarray(F5, dtype=np.float64).reshape(-1, 5))))


def plane_stress_axial_strain(E, nu, stress, epsp):
    """The out-of-plane strain of a plane-stress state from the outputs of plane-stress J2 plasticity (``[xx, yy, sqrt(2) xy]``):
    ``eps_zz = -nu / E (s_xx + s_yy) - (epsp_xx + epsp_yy)`` -- the elastic part from ``sig_zz = 0``, the plastic part from the
    trace-free flow.  The field the reference's ``_plane_stress_elastoplasticity.py`` carries as an unknown of the global problem."""
    stress, epsp = np.asarray(stress, dtype=np.float64).reshape(-1, 3), np.asarray(epsp, dtype=np.float64).reshape(-1, 3)
    return -nu / E * (stress[:, 0] + stress[:, 1]) - (epsp[:, 0] + epsp[:, 1])
