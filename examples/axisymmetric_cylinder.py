#!/usr/bin/env python3
"""A thick-walled cylinder under internal pressure on an axisymmetric mesh: what a reference user with
``hypothesis="axisymmetric"`` runs here.  The behaviour is built with ``hypothesis="plane_strain"`` -- MGIS gives an axisymmetric state
the slots of a plane-strain one, ``[rr, zz, tt, sqrt(2) rz]`` -- and the hypothesis lives on the mesh:
:class:`~dolfinx_materials_amd.gradient.AxisymmetricMesh` evaluates ``eps_tt = u_r / r`` where a ``PlaneMesh`` writes 0.

The meridian section ``a <= r <= b``, ``0 <= z <= 1`` is meshed with Q2 quadrilaterals and fed the NODAL INTERPOLANT of Lame's
displacement for a long cylinder (``eps_zz = 0``), ``u_r = (1 + nu) / E [(1 - 2 nu) C r + C b^2 / r]`` with ``C = p a^2 / (b^2 - a^2)``;
the stresses at the Gauss points are compared with ``sigma_rr = C (1 - b^2 / r^2)``, ``sigma_tt = C (1 + b^2 / r^2)`` at two mesh
sizes (the interpolant's gradient converges with h^2).  No equilibrium solve: assembly is the caller's, with the measure
``2 pi r w |det J|`` from ``mesh.radii()``.

    python examples/axisymmetric_cylinder.py [n_coarse]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd.gradient import AxisymmetricMesh
from dolfinx_materials_amd.jaxmat import JAXMaterial


def section(n, a, b):
    """n x n quadrilaterals on [a, b] x [0, 1], vertices of a cell in basix's order (0,0),(1,0),(0,1),(1,1)"""
    R, Z = np.meshgrid(np.linspace(a, b, n + 1), np.linspace(0.0, 1.0, n + 1), indexing="ij")
    i, j = (x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    idx = lambda p, q: (i + p) * (n + 1) + (j + q)   # noqa: E731
    return np.stack([R.ravel(), Z.ravel()], axis=1), np.stack([idx(0, 0), idx(1, 0), idx(0, 1), idx(1, 1)], axis=1).astype(np.int32)


def run(n, E=70e3, nu=0.3, a=1.0, b=2.0, p=100.0, verbose=True):
    C = p * a**2 / (b**2 - a**2)
    mesh, xd = AxisymmetricMesh.lagrange(*section(n, a, b), degree=2)
    r_dof = xd[:, 0]
    u = np.stack([(1 + nu) / E * ((1 - 2 * nu) * C * r_dof + C * b**2 / r_dof), np.zeros(len(xd))], axis=1).ravel()
    material = JAXMaterial(jm.ElasticBehavior(jm.LinearElasticIsotropic(E=E, nu=nu), hypothesis="plane_strain"))
    material.set_data_manager(mesh.npoints)
    sig, _, _ = material.integrate_displacement(mesh, u)
    r = mesh.radii()
    lame = np.stack([C * (1 - b**2 / r**2), C * (1 + b**2 / r**2)], axis=1)
    err = np.abs(sig[:, [0, 2]] - lame).max(axis=0) / p
    if verbose:
        print(f"{n} x {n} Q2 cells, {mesh.npoints} Gauss points, p = {p}")
        print("        r     sigma_rr        Lame     sigma_tt        Lame")
        for k in np.argsort(r)[:: max(mesh.npoints // 6, 1)]:
            print(f"  {r[k]:.4f}  {sig[k, 0]:11.5f} {lame[k, 0]:11.5f}  {sig[k, 2]:11.5f} {lame[k, 1]:11.5f}")
        print(f"  largest error / p: sigma_rr {err[0]:.3e}  sigma_tt {err[1]:.3e};  |sigma_rz| / p <= {np.abs(sig[:, 3]).max() / p:.1e}")
    material.close()
    mesh.close()
    return err


def main(n=8):
    coarse, fine = run(n), run(2 * n)
    print(f"error at h / 2 over error at h: sigma_rr {fine[0] / coarse[0]:.3f}  sigma_tt {fine[1] / coarse[1]:.3f}  (h^2: 0.25)")
    return coarse, fine


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
