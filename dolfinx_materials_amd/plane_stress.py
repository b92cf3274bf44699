"""The plane-stress laws of the reference's ``demos/cvxpy/cvxpy_materials.py`` under their own names and constructor signatures, as
:class:`HIPMaterial` s: where the demo solves one conic program per Gauss point and call, these run one fused kernel over the batch
(``csrc/plane_stress.hip``: a scalar Newton on one multiplier for the quadratic set, a closed form for the polygonal ones;
``csrc/plane_stress_hosford.hip``: one bracketed root in a polar angle for the Hosford set, at any exponent from 2 to 100).

    from dolfinx_materials_amd.plane_stress import PlaneStressvonMises, Rankine, L1Rankine, PlaneStressHosford
    material = Rankine(E=70e3, nu=0.2, fc=30.0, ft=10.0)       # demos/cvxpy/cvxpy_return_mapping.py
    material.set_data_manager(N); sig, isv, Ct = material.integrate(eps); material.data_manager.update()

Strain and stress are ``[xx, yy, sqrt(2) xy]``; ``gradients == {"Strain": 3}``, ``fluxes == {"Stress": 3}``, no internal state variable;
the state dictionaries carry ``Strain`` and ``Stress`` like the reference's.  ``PlaneStressHosford(E=E, nu=nu, sig0=sig0, a=10)`` is the demo's fourth law (``cvxpy_return_mapping.py:179-207``).

:class:`PlaneStressvonMisesHardening` is von Mises plasticity with linear or Voce hardening in the same three components
(``csrc/plane_stress_j2.hip``), the law of ``demos/jax/elastoplasticity/_plane_stress_elastoplasticity.py`` without its extra
unknown ``eps_zz``; its internal state variables are ``p`` (1) and ``epsp`` (3)."""
from . import materials as _m
from .hip_material import HIPMaterial


class _PlaneStressMaterial(HIPMaterial):
    @property
    def C(self):
        """``cvxpy_materials.py:16-18``"""
        from .conventions import plane_stress_stiffness

        return plane_stress_stiffness(self.behavior.E, self.behavior.nu)

    @property
    def E(self):
        return self.behavior.E

    @property
    def nu(self):
        return self.behavior.nu


class PlaneStressvonMises(_PlaneStressMaterial):
    """``cvxpy_materials.py:89-93``: ``sigma^T Q sigma <= sig0^2`` with ``Q = [[1, -1/2, 0], [-1/2, 1, 0], [0, 0, shear_weight]]``.
    ``shear_weight=1`` is the reference's matrix, which is not von Mises in the ``sqrt(2) xy`` component; ``shear_weight=1.5`` is.
    ``tangent="elastic"`` hands back ``C`` as the reference does, ``"consistent"`` the algorithmic tangent of the yielded points."""

    def __init__(self, E, nu, sig0, shear_weight=1.0, tangent="elastic", **kwargs):
        if tangent not in ("elastic", "consistent"):
            raise ValueError(f"PlaneStressvonMises: tangent must be 'elastic' or 'consistent', got {tangent!r}")
        super().__init__(_m.PlaneStressQuadraticYield(E, nu, sig0, q=shear_weight, tangent=int(tangent == "consistent")), **kwargs)

    @property
    def sig0(self):
        return self.behavior.sig0


class PlaneStressHosford(_PlaneStressMaterial):
    """``cvxpy_materials.py:96-110``: ``(|sigma_I|^a + |sigma_II|^a + |sigma_I - sigma_II|^a) / 2 <= sig0^a`` on the principal stresses,
    ``2 <= a <= 100``.  ``tangent="elastic"`` hands back ``C`` as the reference does, ``"consistent"`` the algorithmic tangent of the
    yielded points."""

    def __init__(self, E, nu, sig0, a, tangent="elastic", **kwargs):
        if tangent not in ("elastic", "consistent"):
            raise ValueError(f"PlaneStressHosford: tangent must be 'elastic' or 'consistent', got {tangent!r}")
        super().__init__(_m.PlaneStressHosfordYield(E, nu, sig0, a, tangent=int(tangent == "consistent")), **kwargs)

    @property
    def sig0(self):
        return self.behavior.sig0

    @property
    def a(self):
        return self.behavior.a


class PlaneStressvonMisesHardening(_PlaneStressMaterial):
    """von Mises plasticity with isotropic hardening in plane stress (``csrc/plane_stress_j2.hip``): the law of the reference's
    ``demos/jax/elastoplasticity/_plane_stress_elastoplasticity.py`` without its extra unknown ``eps_zz``.  ``yield_stress`` is a
    ``materials.LinearHardening`` or ``materials.VoceHardening``.  ``gradients == {"Strain": 3}``, ``fluxes == {"Stress": 3}``,
    ``internal_state_variables == {"p": 1, "epsp": 3}``; the tangent is the consistent one.  The out-of-plane strain is
    ``conventions.plane_stress_axial_strain(E, nu, stress, epsp)``."""

    def __init__(self, E, nu, yield_stress, **kwargs):
        super().__init__(_m.PlaneStressJ2(_m.LinearElasticIsotropic(E=E, nu=nu), yield_stress), **kwargs)

    @property
    def yield_stress(self):
        return self.behavior.yield_stress


class PlaneStressPolygon(_PlaneStressMaterial):
    """A polygonal yield set ``n_k . (sigma_I, sigma_II) <= d_k`` in the plane of the principal stresses: ``planes`` is a list of at
    most four ``(n1, n2, d)``, ``d > 0``, closed under the exchange of the two principal stresses."""

    def __init__(self, E, nu, planes, tangent="elastic", **kwargs):
        if tangent != "elastic":
            raise ValueError(f"{type(self).__name__}: tangent={tangent!r} is not served: a consistent tangent of the polygonal law has "
                             "eigen-derivative limits at equal principal stresses and at the vertices and is out of scope; the "
                             "tangent handed back is the elastic C, as the reference's")
        super().__init__(_m.PlaneStressPolygonYield(E, nu, planes), **kwargs)


def _strengths(name, ft, fc):
    ft, fc = float(ft), float(fc)
    if not (0.0 < ft < float("inf") and 0.0 < fc < float("inf")):
        raise ValueError(f"{name}: the strengths ft and fc must be finite and > 0, got ft={ft}, fc={fc}")
    return ft, fc


class Rankine(PlaneStressPolygon):
    """``cvxpy_materials.py:54-65``: ``-fc <= sigma_I, sigma_II <= ft``."""

    def __init__(self, E, nu, ft, fc, **kwargs):
        self.ft, self.fc = _strengths("Rankine", ft, fc)
        super().__init__(E, nu, [(1.0, 0.0, self.ft), (0.0, 1.0, self.ft), (-1.0, 0.0, self.fc), (0.0, -1.0, self.fc)], **kwargs)


class L1Rankine(PlaneStressPolygon):
    """``cvxpy_materials.py:68-86``: ``-fc <= tr sigma <= ft`` and ``a tr sigma + b |sigma_I - sigma_II| <= 1`` with
    ``a = (1/ft - 1/fc)/2``, ``b = (1/ft + 1/fc)/2``."""

    def __init__(self, E, nu, ft, fc, **kwargs):
        self.ft, self.fc = _strengths("L1Rankine", ft, fc)
        a, b = (1 / self.ft - 1 / self.fc) / 2, (1 / self.ft + 1 / self.fc) / 2
        super().__init__(E, nu, [(1.0, 1.0, self.ft), (-1.0, -1.0, self.fc), (a + b, a - b, 1.0), (a - b, a + b, 1.0)], **kwargs)
