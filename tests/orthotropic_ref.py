"""Numpy restatement of orthotropic elasticity in a material frame (``DXM_LAW_ORTHOTROPIC_ELASTIC``), written from the equations of
``include/dxmat.h`` / DESIGN.md:

* :func:`update` is float64 in the Mandel form of the kernel's convention, ``eps_m = Q eps``, ``sigma = Q^T C Q eps``, with plain
  matrix products (``numpy.linalg.inv`` for the normal block, ``einsum`` for the products -- none of the kernel's fma chains);
* :func:`update_mp` is the same law in ``mpmath`` at 50 digits in the fourth-order tensor form ``C_ijkl = R_pi R_qj R_rk R_sl Cm_pqrs``,
  ``sigma_ij = C_ijkl eps_kl``: it never forms ``Q`` and shares no algebra with it.

:func:`host_stiffness` repeats the closed-form adjugate of ``csrc/dxmat.hip::build_orthotropic`` operation by operation (what the
no-frame kernel's tangent is compared with bit for bit).  TEST INFRASTRUCTURE ONLY.

Convention: ``R`` is 3x3 and its ROWS are the material axes in global coordinates: ``eps_m = R eps R^T``, ``sigma = R^T sigma_m R``."""
import numpy as np

SQ2 = np.sqrt(2.0)
NAMES = ("E1", "E2", "E3", "nu12", "nu23", "nu13", "G12", "G23", "G13")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # tensor indices of the Mandel components
#: parameter sets [E1, E2, E3, nu12, nu23, nu13, G12, G23, G13]
PARAMETER_SETS = {
    "isotropic": [70e3, 70e3, 70e3, 0.3, 0.3, 0.3, 70e3 / 2.6, 70e3 / 2.6, 70e3 / 2.6],
    "cubic": [208e3, 208e3, 208e3, 0.3, 0.3, 0.3, 120e3, 120e3, 120e3],          # G != E / (2 (1 + nu)) = 80e3
    # the StandardElasticity brick of tests/mfront/MericCailletaudSingleCrystalViscoPlasticity.mfront:18-28 (E1 = 208000)
    "brick": [208e3, 208e3, 208e3, 0.3, 0.3, 0.3, 80e3, 80e3, 80e3],
    "strong": [200e3, 40e3, 10e3, 0.25, 0.3, 0.2, 12e3, 4e3, 7e3],               # E1 / E3 = 20
}
FRAME_CLASSES = ("identity", "quarter_x", "quarter_y", "quarter_z", "z_0", "z_pi4", "z_pi3", "z_pi2", "random", "near_identity")


def to_tensor(v):
    v = np.asarray(v)
    t = np.empty(v.shape[:-1] + (3, 3))
    for I, (i, j) in enumerate(PAIRS):
        t[..., i, j] = t[..., j, i] = v[..., I] / (1.0 if I < 3 else SQ2)
    return t


def to_mandel(t):
    return np.stack([t[..., i, j] * (1.0 if I < 3 else SQ2) for I, (i, j) in enumerate(PAIRS)], axis=-1)


def compliance(p):
    E1, E2, E3, nu12, nu23, nu13 = p[:6]
    return np.array([[1 / E1, -nu12 / E1, -nu13 / E1], [-nu12 / E1, 1 / E2, -nu23 / E2], [-nu13 / E1, -nu23 / E2, 1 / E3]])


def stiffness(p):
    """the 6x6 Mandel stiffness in the material frame"""
    C = np.zeros((6, 6))
    C[:3, :3] = np.linalg.inv(compliance(p))
    C[3, 3], C[4, 4], C[5, 5] = 2 * p[6], 2 * p[8], 2 * p[7]   # 2 G12, 2 G13, 2 G23
    return C


def host_stiffness(p):
    """the same 6x6 with the arithmetic of dxmat.hip::build_orthotropic, every operation individually rounded"""
    E1, E2, E3, nu12, nu23, nu13, G12, G23, G13 = (np.float64(x) for x in p)
    one = np.float64(1.0)
    s11, s22, s33, s12, s13, s23 = one / E1, one / E2, one / E3, -nu12 / E1, -nu13 / E1, -nu23 / E2
    c11, c12, c13 = s22 * s33 - s23 * s23, s13 * s23 - s12 * s33, s12 * s23 - s13 * s22
    c22, c23, c33 = s11 * s33 - s13 * s13, s12 * s13 - s11 * s23, s11 * s22 - s12 * s12
    det = s11 * c11 + s12 * c12 + s13 * c13
    C = np.zeros((6, 6))
    C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2] = c11 / det, c12 / det, c13 / det, c22 / det, c23 / det, c33 / det
    C[1, 0], C[2, 0], C[2, 1] = C[0, 1], C[0, 2], C[1, 2]
    C[3, 3], C[4, 4], C[5, 5] = 2.0 * G12, 2.0 * G13, 2.0 * G23
    return C


def mandel_rotation(R):
    """Q (..., 6, 6) of R (..., 3, 3): eps_m = Q eps for eps_m = R eps R^T; orthogonal"""
    R = np.asarray(R, dtype=np.float64)
    Q = np.empty(R.shape[:-2] + (6, 6))
    for I, (i, j) in enumerate(PAIRS):
        for K, (k, l) in enumerate(PAIRS):
            if K < 3:
                v = R[..., i, k] * R[..., j, k]
            else:
                v = (R[..., i, k] * R[..., j, l] + R[..., i, l] * R[..., j, k]) / SQ2
            Q[..., I, K] = v * (1.0 if I < 3 else SQ2)
    return Q


def update(eps, p, R=None):
    """(sigma (N, 6), Ct (N, 6, 6)) of strains eps (N, 6); R: None, (3, 3) or (N, 3, 3)"""
    eps = np.asarray(eps, dtype=np.float64)
    C = stiffness(p)
    n = len(eps)
    if R is None:
        return eps @ C.T, np.broadcast_to(C, (n, 6, 6)).copy()
    Q = mandel_rotation(np.broadcast_to(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), (n, 3, 3)))
    Ct = np.einsum("nai,ab,nbj->nij", Q, C, Q)
    return np.einsum("nij,nj->ni", Ct, eps), Ct


def update_reference_cadence(eps, p, R):
    """What the reference's QuadratureMap.update() does around a law without a frame (quadrature_map.py:315-330): rotate the gradients
    into the material frame, run the law there, rotate flux and tangent back -- in tensors, point by point."""
    eps = np.asarray(eps, dtype=np.float64)
    n = len(eps)
    R = np.broadcast_to(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), (n, 3, 3))
    em = to_mandel(np.einsum("nik,nkl,njl->nij", R, to_tensor(eps), R))
    sm, Cm = update(em, p)
    sig = to_mandel(np.einsum("nki,nkl,nlj->nij", R, to_tensor(sm), R))
    Q = mandel_rotation(R)
    return sig, np.einsum("nai,nab,nbj->nij", Q, Cm, Q)


# ---- frames and inputs ---------------------------------------------------------------------------------------------------
def axis_rotation(axis, angle):
    """rows = material axes turned by +angle about `axis` (0, 1, 2); about z: the matrix of tests/uniaxial_tension.py:61-66"""
    c, s = np.cos(angle), np.sin(angle)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[a, a], R[a, b], R[b, a], R[b, b] = c, s, -s, c
    return R


def random_rotations(rng, n):
    """proper rotations from unit quaternions"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], axis=1)


def frames(n, seed=0):
    """(labels (n,), R (n, 3, 3)): the frame classes in turn"""
    rng = np.random.default_rng(seed)
    rnd = random_rotations(rng, n)
    tiny = random_rotations(rng, n)
    out, labels = np.empty((n, 3, 3)), []
    for i in range(n):
        c = FRAME_CLASSES[i % len(FRAME_CLASSES)]
        labels.append(c)
        if c == "identity" or c == "z_0":
            out[i] = np.eye(3)
        elif c.startswith("quarter_"):
            out[i] = axis_rotation("xyz".index(c[-1]), np.pi / 2)
        elif c.startswith("z_pi"):
            out[i] = axis_rotation(2, np.pi / int(c[4:]))
        elif c == "random":
            out[i] = rnd[i]
        else:   # within 1e-9 of the identity: a rotation by 5e-10 rad about a random axis
            ax = tiny[i, 0]
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            t = 5e-10
            out[i] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    return np.array(labels), out


def strains(n, seed=1, scale=1e-3):
    return np.random.default_rng(seed).standard_normal((n, 6)) * scale


# ---- 50 digits, fourth-order tensor form ---------------------------------------------------------------------------------------
def update_mp(eps, p, R, digits=50):
    """one point: (sigma (6,), Ct (6, 6)) as float64 roundings of the 50-digit values, through C_ijkl = R_pi R_qj R_rk R_sl Cm_pqrs"""
    import mpmath as mp

    mp.mp.dps = digits
    P = [mp.mpf(float(x)) for x in p]
    E1, E2, E3, nu12, nu23, nu13, G12, G23, G13 = P
    S = mp.matrix([[1 / E1, -nu12 / E1, -nu13 / E1], [-nu12 / E1, 1 / E2, -nu23 / E2], [-nu13 / E1, -nu23 / E2, 1 / E3]])
    A = S ** -1
    G = {(0, 1): G12, (0, 2): G13, (1, 2): G23}
    Cm = {}
    for a in range(3):
        for b in range(3):
            Cm[(a, a, b, b)] = A[a, b]
    for (a, b), g in G.items():   # sigma_ab = 2 G eps_ab: minor-symmetric C_abab = C_abba = G
        for idx in ((a, b, a, b), (a, b, b, a), (b, a, a, b), (b, a, b, a)):
            Cm[idx] = g
    Rm = [[mp.mpf(float(R[i][j])) for j in range(3)] for i in range(3)]
    rng3 = range(3)
    Cg = [[[[mp.mpf(0) for _ in rng3] for _ in rng3] for _ in rng3] for _ in rng3]
    for (a, b, c, d), v in Cm.items():
        for i in rng3:
            for j in rng3:
                for k in rng3:
                    for l in rng3:
                        Cg[i][j][k][l] += Rm[a][i] * Rm[b][j] * Rm[c][k] * Rm[d][l] * v
    sq2 = mp.sqrt(2)
    w = [mp.mpf(1)] * 3 + [sq2] * 3
    et = [[mp.mpf(0)] * 3 for _ in rng3]
    for I, (i, j) in enumerate(PAIRS):
        et[i][j] = et[j][i] = mp.mpf(float(eps[I])) / w[I]
    sig = np.empty(6)
    Ct = np.empty((6, 6))
    for I, (i, j) in enumerate(PAIRS):
        sig[I] = float(w[I] * sum(Cg[i][j][k][l] * et[k][l] for k in rng3 for l in rng3))
        for K, (k, l) in enumerate(PAIRS):
            # d (w_I sigma_ij) / d (w_K eps_kl): both (k, l) and (l, k) carry eps_K / w_K when k != l
            v = Cg[i][j][k][l] if k == l else Cg[i][j][k][l] + Cg[i][j][l][k]
            Ct[I, K] = float(w[I] * v / w[K])
    return sig, Ct
