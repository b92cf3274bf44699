"""Behaviour descriptors with the constructor surface of ``jaxmat.materials`` as the reference
uses it (``tests/test_FeFp_jax.py:17-19``, ``demos/jax/elastoplasticity/plane_elastoplasticity.py:67-71``,
``demos/jax/finite_strain_elastoplasticity/finite_strain_elastoplasticity.py:165-169``).

A descriptor only carries parameters and names; it selects one fused HIP kernel (a law id of
``include/dxmat.h``).  Hardening is one of the closed-form laws below, a :class:`CustomHardening`
(C expressions) or -- as in the reference, ``tests/test_FeFp_jax.py:14-19`` -- any Python callable
``yield_stress(p)`` written with arithmetic operators and numpy ufuncs: it is traced once
(``tracing.py``), differentiated symbolically and compiled into the kernel on first use.
"""
from __future__ import annotations

from dataclasses import dataclass

from . import _lib


@dataclass
class LinearElasticIsotropic:
    """``jm.LinearElasticIsotropic(E=, nu=)``; Lame constants as ``python_materials/elasticity.py:12-13``."""

    E: float
    nu: float

    @property
    def mu(self):
        return self.E / 2 / (1 + self.nu)

    @property
    def lmbda(self):
        return self.E * self.nu / (1 + self.nu) / (1 - 2 * self.nu)

    @property
    def kappa(self):
        return self.lmbda + 2 * self.mu / 3


@dataclass
class LinearHardening:
    """R(p) = sig0 + H p (``tests/mfront/IsotropicPlasticMisesFlow.mfront:7-11``)."""

    sig0: float
    H: float


@dataclass
class VoceHardening:
    """R(p) = sig0 + (sigu - sig0)(1 - exp(-b p)) (``tests/test_FeFp_jax.py:14-15``)."""

    sig0: float
    sigu: float
    b: float


class CustomHardening:
    """An arbitrary isotropic hardening law given as C expressions, compiled into the fused kernels
    on first use (the role a Python ``yield_stress(p)`` callable plays for jaxmat,
    ``tests/test_FeFp_jax.py:14-19``)::

        jm.CustomHardening("sig0 + K * pow(p + 1e-12, n)", "K * n * pow(p + 1e-12, n - 1)",
                           sig0=250.0, K=600.0, n=0.3)

    ``R`` is R(p), ``dR`` its derivative, both in the variable ``p``, ``sig0`` and up to six named
    parameters; R(0) must equal ``sig0`` and R must be non-decreasing (the local Newton relies on
    it, as with the built-in laws)."""

    #: names that mean something else inside the generated C expression
    _RESERVED = {"p", "sig0", "c", "exp", "expm1", "log", "log1p", "log2", "log10", "pow", "sqrt", "cbrt", "tanh", "sinh",
                 "cosh", "sin", "cos", "tan", "atan", "asin", "acos", "fabs", "fmax", "fmin", "fma", "erf", "double", "float",
                 "int", "const", "return", "if", "else", "for", "while", "prm"}

    def __init__(self, R: str, dR: str, sig0: float, **params):
        import re

        if len(params) > 6:
            raise ValueError("at most 6 named parameters")
        bad = self._RESERVED & set(params)
        if bad:
            raise ValueError(f"parameter names {sorted(bad)} are reserved")
        self.sig0 = float(sig0)
        self.names = list(params)
        self.values = [float(v) for v in params.values()]
        self.R_source, self.dR_source = R, dR

        def sub(expr):
            for i, name in enumerate(self.names):
                expr = re.sub(rf"\b{re.escape(name)}\b", f"c[{i}]", expr)
            return "(" + expr + ")"

        self.expr_R, self.expr_dR = sub(R), sub(dR)

    @classmethod
    def from_callable(cls, func):
        """Trace a Python ``yield_stress(p)`` (operators + numpy ufuncs) into the two C expressions; numbers the
        callable closes over become literals, ``sig0 = yield_stress(0)``."""
        from .tracing import TracedLaw

        law = TracedLaw(func)
        self = cls(law.expr_R, law.expr_dR, sig0=law.sig0)
        self.traced = law
        return self

    def coefficients(self):
        return self.values + [0.0] * (6 - len(self.values))

    # named parameters read and written like attributes (update_material_property("yield_stress.K", ...))
    def __getattr__(self, name):
        names = self.__dict__.get("names", [])
        if name in names:
            return self.__dict__["values"][names.index(name)]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        names = self.__dict__.get("names", [])
        if name in names:
            self.__dict__["values"][names.index(name)] = float(value)
        else:
            object.__setattr__(self, name, value)


class Behavior:
    """Common part: law id, parameter vector, field names and sizes."""

    law: int = -1
    gradient_name = "strain"
    flux_name = "stress"

    def params(self):
        raise NotImplementedError

    def flat_properties(self):
        raise NotImplementedError


class SmallStrainBehavior(Behavior):
    """gradient ``strain`` (6), flux ``stress`` (6): ``jaxmat.py:166-169, :177-180``."""

    gradient_name = "strain"
    flux_name = "stress"
    ngrad = 6
    nflux = 6


class FiniteStrainBehavior(Behavior):
    """gradient ``F`` (9), flux ``PK1`` (9): ``jaxmat.py:170-171, :181-182``."""

    gradient_name = "F"
    flux_name = "PK1"
    ngrad = 9
    nflux = 9


def _check_hardening(yield_stress):
    if isinstance(yield_stress, (LinearHardening, VoceHardening, CustomHardening)):
        return yield_stress
    if callable(yield_stress):   # what the reference passes (tests/test_FeFp_jax.py:14-19)
        return CustomHardening.from_callable(yield_stress)
    raise TypeError(
        "yield_stress must be a callable yield_stress(p) (arithmetic operators and numpy ufuncs), or a "
        "materials.LinearHardening / VoceHardening / CustomHardening instance"
    )


def _hardening_params(e, y):
    if isinstance(y, LinearHardening):
        return [e.E, e.nu, y.sig0, y.H]
    if isinstance(y, CustomHardening):
        return [e.E, e.nu, y.sig0] + y.coefficients()
    return [e.E, e.nu, y.sig0, y.sigu, y.b]


def _hardening_properties(y):
    if isinstance(y, CustomHardening):
        return {"yield_stress.sig0": y.sig0, **{f"yield_stress.{n}": v for n, v in zip(y.names, y.values)}}
    return {f"yield_stress.{k}": v for k, v in vars(y).items()}


#: the modelling hypotheses served, the reference's strings (``dolfinx_materials/mfront.py:33-37``)
HYPOTHESES = ("3d", "plane_strain")


def _check_hypothesis(hypothesis):
    if hypothesis == "axisymmetric":
        raise NotImplementedError('hypothesis="axisymmetric" is not served yet (a follow-up: its 4-wide strain [rr, zz, tt, sqrt(2) rz] '
                                  'needs a gradient of its own); "3d" and "plane_strain" are')
    if hypothesis not in HYPOTHESES:
        raise ValueError(f"hypothesis must be one of {list(HYPOTHESES)}, got {hypothesis!r}")
    return hypothesis


def _set_hypothesis(behavior, hypothesis):
    """``"plane_strain"``: strain, stress and plastic strain are the 4-vectors ``[xx, yy, zz, sqrt(2) xy]`` of a 2x2 tensor
    (``utils.py:146-150``), the tangent block is ``(4, 4)``."""
    behavior.hypothesis = _check_hypothesis(hypothesis)
    if hypothesis == "plane_strain":
        behavior.ngrad = behavior.nflux = 4


class ElasticBehavior(SmallStrainBehavior):
    """Linear isotropic elasticity as a small-strain behaviour; ``hypothesis="plane_strain"``: in the four components
    ``[xx, yy, zz, sqrt(2) xy]``."""

    law = _lib.LAW_ELASTIC_ISO

    def __init__(self, elasticity: LinearElasticIsotropic, hypothesis: str = "3d"):
        self.elasticity = elasticity
        _set_hypothesis(self, hypothesis)
        if hypothesis == "plane_strain":
            self.law = _lib.LAW_PE_ELASTIC_ISO

    def params(self):
        return [self.elasticity.E, self.elasticity.nu]

    def flat_properties(self):
        return {"elasticity.E": self.elasticity.E, "elasticity.nu": self.elasticity.nu}


class vonMisesIsotropicHardening(SmallStrainBehavior):
    """Small-strain J2 plasticity with isotropic hardening (``plane_elastoplasticity.py:67-71``).  ``hypothesis="plane_strain"``
    (what the reference's ``MFrontMaterial(..., hypothesis="plane_strain")`` asks for): strain, stress and ``epsp`` are the
    4-vectors ``[xx, yy, zz, sqrt(2) xy]``, the tangent block is ``(4, 4)``; stock hardening laws only."""

    def __init__(self, elasticity: LinearElasticIsotropic, yield_stress, hypothesis: str = "3d"):
        self.elasticity = elasticity
        _set_hypothesis(self, hypothesis)
        if hypothesis == "plane_strain" and not isinstance(yield_stress, (LinearHardening, VoceHardening)):
            raise TypeError('hypothesis="plane_strain" is served with the stock hardening laws only: yield_stress must be a '
                            "materials.LinearHardening or materials.VoceHardening, not a CustomHardening or a traced callable "
                            f"(got {type(yield_stress).__name__}); use the \"3d\" hypothesis with an embedded strain for those")
        self.yield_stress = _check_hardening(yield_stress)
        linear = isinstance(self.yield_stress, LinearHardening)
        if hypothesis == "plane_strain":
            self.law = _lib.LAW_PE_J2_LINEAR if linear else _lib.LAW_PE_J2_VOCE
        else:
            self.law = _lib.LAW_J2_LINEAR if linear else _lib.LAW_J2_VOCE
        self.custom_hardening = self.yield_stress if isinstance(self.yield_stress, CustomHardening) else None

    def params(self):
        return _hardening_params(self.elasticity, self.yield_stress)

    def flat_properties(self):
        out = {"elasticity.E": self.elasticity.E, "elasticity.nu": self.elasticity.nu}
        out.update(_hardening_properties(self.yield_stress))
        return out


class FeFpJ2Plasticity(FiniteStrainBehavior):
    """Finite-strain FeFp J2 plasticity (``tests/test_FeFp_jax.py:17-19``); Voce hardening."""

    def __init__(self, elasticity: LinearElasticIsotropic, yield_stress):
        self.elasticity = elasticity
        self.yield_stress = _check_hardening(yield_stress)
        self.law = _lib.LAW_FEFP_J2_LINEAR if isinstance(self.yield_stress, LinearHardening) else _lib.LAW_FEFP_J2_VOCE
        self.custom_hardening = self.yield_stress if isinstance(self.yield_stress, CustomHardening) else None

    def params(self):
        return _hardening_params(self.elasticity, self.yield_stress)

    def flat_properties(self):
        out = {"elasticity.E": self.elasticity.E, "elasticity.nu": self.elasticity.nu}
        out.update(_hardening_properties(self.yield_stress))
        return out


class RambergOsgoodNonLinearElasticity(SmallStrainBehavior):
    """Small-strain Ramberg-Osgood nonlinear elasticity, no internal state
    (``tests/mfront/RambergOsgoodNonLinearElasticity.mfront``): the equivalent strain is
    ``eps_e = sig_e / (3 mu) + beta (sig_e / sig0)^n`` with ``beta = alpha sig0 / E``; ``sig0 > 0``, ``alpha > 0``, ``n >= 1``.

    ``JAXMaterial(RambergOsgoodNonLinearElasticity(...), gradient_name="Strain", flux_name="Stress")`` stands where the
    reference uses ``MFrontMaterial(lib, "RambergOsgoodNonLinearElasticity", material_properties=...)``
    (``tests/mfront/test_nonlinear_elasticity.py``); :meth:`from_mfront_properties` takes that dictionary."""

    law = _lib.LAW_RAMBERG_OSGOOD

    def __init__(self, elasticity: LinearElasticIsotropic, sig0: float, alpha: float, n: float):
        self.elasticity = elasticity
        self.sig0 = float(sig0)
        self.alpha = float(alpha)
        self.n = float(n)

    @classmethod
    def from_mfront_properties(cls, props: dict):
        """The ``material_properties`` of the reference's MFront test: ``YoungModulus``, ``PoissonRatio``,
        ``YieldStrength``, ``alpha``, ``n``."""
        known = {"YoungModulus", "PoissonRatio", "YieldStrength", "alpha", "n"}
        missing, extra = known - set(props), set(props) - known
        if missing or extra:
            raise ValueError(f"Ramberg-Osgood material properties: missing {sorted(missing)}, unknown {sorted(extra)}")
        el = LinearElasticIsotropic(E=float(props["YoungModulus"]), nu=float(props["PoissonRatio"]))
        return cls(el, sig0=props["YieldStrength"], alpha=props["alpha"], n=props["n"])

    def params(self):
        return [self.elasticity.E, self.elasticity.nu, self.sig0, self.alpha, self.n]

    def flat_properties(self):
        return {"elasticity.E": self.elasticity.E, "elasticity.nu": self.elasticity.nu, "sig0": self.sig0, "alpha": self.alpha,
                "n": self.n}


class OgdenHyperelasticity(FiniteStrainBehavior):
    """Finite-strain Ogden hyperelasticity (``demos/mfront/hyperelasticity/Ogden.mfront``): stored energy
    ``W(F) = (mu / alpha) (J^(-alpha/3) sum_i c_i^(alpha/2) - 3) + K/2 (J - 1)^2`` with ``c_i`` the eigenvalues of ``C = F^T F``
    and ``J = det F``; ``alpha != 0``, ``mu > 0``, ``K > 0`` (the file's defaults: 28.8, 27778, 69444444).  One internal state
    variable, ``PK2Stress`` (6): the isochoric part of the second Piola-Kirchhoff stress.

    ``JAXMaterial(OgdenHyperelasticity(...))`` stands where the reference's hyperelasticity demo uses
    ``MFrontMaterial(lib, "Ogden")``: gradient ``DeformationGradient`` (9), flux ``FirstPiolaKirchhoffStress`` (9), tangent block
    ``(9, 9)``; :meth:`from_mfront_properties` takes the ``material_properties`` dictionary of that call.  Full tangent only; the
    displacement forms need option ``fused_gradient`` off (no fused kernel for this law).

    ``hypothesis="plane_strain"`` (``MFrontMaterial(lib, "Ogden", hypothesis="plane_strain")``): the gradient is the 5-vector
    ``[F00, F11, F22, F01, F10]`` of a 2x2 tensor with its out-of-plane stretch (``utils.py:168-172``), the flux the 5-wide PK1 in the
    same order, the tangent block ``(5, 5)`` and ``PK2Stress`` the 4-vector ``[xx, yy, zz, sqrt(2) xy]``: the 9-wide law on the embedded
    ``F``, restricted (``conventions.embed_plane_F`` / ``restrict_plane_F`` / ``restrict_plane_F_tangent``).  ``F22`` is read, not
    assumed to be 1.  F is passed as an array: the displacement forms are not served under this hypothesis."""

    law = _lib.LAW_OGDEN
    gradient_name = "DeformationGradient"
    flux_name = "FirstPiolaKirchhoffStress"
    MFRONT_DEFAULTS = {"alpha": 28.8, "mu": 27778.0, "K": 69444444.0}

    def __init__(self, mu: float = MFRONT_DEFAULTS["mu"], alpha: float = MFRONT_DEFAULTS["alpha"], K: float = MFRONT_DEFAULTS["K"],
                 hypothesis: str = "3d"):
        if _check_hypothesis(hypothesis) == "plane_strain":
            self.hypothesis = hypothesis
            self.law = _lib.LAW_OGDEN_PE
            self.ngrad = self.nflux = 5
        self.mu = float(mu)
        self.alpha = float(alpha)
        self.K = float(K)
        if not (self.alpha != 0.0 and self.mu > 0.0 and self.K > 0.0 and all(map(_isfinite, (self.alpha, self.mu, self.K)))):
            raise ValueError(f"Ogden: alpha must be non-zero, mu and K > 0 (all finite); got alpha={alpha}, mu={mu}, K={K}")

    @classmethod
    def from_mfront_properties(cls, props: dict | None = None, hypothesis: str = "3d"):
        """``material_properties`` of ``MFrontMaterial(..., "Ogden", material_properties=...)``: any of ``alpha``, ``mu``, ``K``;
        what is absent keeps the behaviour file's default, as MFront parameters do.  ``hypothesis``: that of the same call."""
        props = dict(props or {})
        extra = set(props) - set(cls.MFRONT_DEFAULTS)
        if extra:
            raise ValueError(f"Ogden material properties: unknown {sorted(extra)} (the behaviour has alpha, mu, K)")
        return cls(**{**cls.MFRONT_DEFAULTS, **{k: float(v) for k, v in props.items()}}, hypothesis=hypothesis)

    def params(self):
        return [self.alpha, self.mu, self.K]

    def flat_properties(self):
        return {"alpha": self.alpha, "mu": self.mu, "K": self.K}


class HosfordIsotropicHardening(SmallStrainBehavior):
    """Small-strain Hosford plasticity with linear isotropic hardening (the reference's ``IsotropicPlasticHosfordFlowLinear``
    MFront behaviour, the matrix material of ``demos/multimaterials/multimaterials.py``): Hooke's law, associated flow on
    ``seq = (1/2 (|s1-s2|^a + |s1-s3|^a + |s2-s3|^a))^(1/a)`` of the principal stresses, ``R(p) = R0 + H p``; ``R0 > 0``,
    ``H >= 0``, ``a >= 2`` (the behaviour file fixes ``a = 10``; ``a = 2`` and ``a = 4`` are von Mises).  Internal state variables
    ``ElasticStrain`` (6) and ``EquivalentPlasticStrain`` (1), MFront's names.

    ``JAXMaterial(HosfordIsotropicHardening(...))`` stands where the demo uses ``MFrontMaterial(lib, "IsotropicPlasticHosfordFlowLinear",
    material_properties=...)``: gradient ``Strain``, flux ``Stress``; :meth:`from_mfront_properties` takes that dictionary.  Tangent
    layouts ``"full"`` and ``"sym"`` (a general symmetric 6x6: no ``"coef"`` / ``"pack4"``); uniform properties only; the displacement
    forms need option ``fused_gradient`` off.

    ``hypothesis="plane_strain"`` (the demo's plane mesh; ``MFrontMaterial(..., hypothesis="plane_strain")``): strain, stress and
    ``ElasticStrain`` are the 4-vectors ``[xx, yy, zz, sqrt(2) xy]``, the tangent block is a general symmetric ``(4, 4)``: the 6-wide law
    on the embedded strain, restricted (``conventions.embed_plane_strain`` / ``restrict_plane_strain`` /
    ``restrict_plane_strain_tangent``).  ``eps_zz`` is read, not assumed to be 0.  Full tangent only; on a ``PlaneMesh`` the
    displacement forms evaluate the 4-wide strain themselves."""

    law = _lib.LAW_HOSFORD_LINEAR
    gradient_name = "Strain"
    flux_name = "Stress"
    MFRONT_NAMES = ("young_modulus", "poisson_ratio", "R0", "hardening_slope")

    def __init__(self, elasticity: LinearElasticIsotropic, yield_stress, a: float = 10.0, hypothesis: str = "3d"):
        if _check_hypothesis(hypothesis) == "plane_strain":
            self.hypothesis = hypothesis
            self.law = _lib.LAW_PE_HOSFORD_LINEAR
            self.ngrad = self.nflux = 4
        if not isinstance(yield_stress, LinearHardening):
            raise TypeError("Hosford plasticity is served with linear hardening only: yield_stress must be a materials.LinearHardening(R0, H), "
                            f"got {type(yield_stress).__name__}")
        self.elasticity = elasticity
        self.yield_stress = yield_stress
        self.a = float(a)
        R0, H = float(yield_stress.sig0), float(yield_stress.H)
        if not (R0 > 0.0 and H >= 0.0 and self.a >= 2.0 and all(map(_isfinite, (R0, H, self.a)))):
            raise ValueError(f"Hosford: R0 must be > 0, H >= 0 and the exponent a >= 2 (all finite); got R0={R0}, H={H}, a={a}")

    @classmethod
    def from_mfront_properties(cls, props: dict, hypothesis: str = "3d"):
        """The ``material_properties`` of the multi-material demo: ``young_modulus``, ``poisson_ratio``, ``R0``, ``hardening_slope``,
        and optionally the exponent ``a`` (10, the behaviour file's value, when absent).  ``hypothesis``: that of the same call."""
        need, known = set(cls.MFRONT_NAMES), set(cls.MFRONT_NAMES) | {"a"}
        missing, extra = need - set(props), set(props) - known
        if missing or extra:
            raise ValueError(f"Hosford material properties: missing {sorted(missing)}, unknown {sorted(extra)}")
        el = LinearElasticIsotropic(E=float(props["young_modulus"]), nu=float(props["poisson_ratio"]))
        return cls(el, LinearHardening(float(props["R0"]), float(props["hardening_slope"])), a=float(props.get("a", 10.0)),
                   hypothesis=hypothesis)

    def params(self):
        return [self.elasticity.E, self.elasticity.nu, self.yield_stress.sig0, self.yield_stress.H, self.a]

    def flat_properties(self):
        return {"elasticity.E": self.elasticity.E, "elasticity.nu": self.elasticity.nu, "yield_stress.sig0": self.yield_stress.sig0,
                "yield_stress.H": self.yield_stress.H, "a": self.a}


class LogarithmicStrainPlasticity(FiniteStrainBehavior):
    """Finite-strain J2 plasticity in logarithmic strains with linear isotropic hardening (the reference's
    ``demos/mfront/finite_strain_elastoplasticity/LogarithmicStrainPlasticity.mfront``): the Hencky strain ``E = 1/2 log(F^T F)``
    goes through the small-strain radial return (Hooke, Mises, ``R(p) = s0 + H0 p``) and the stress ``T`` is mapped back to the first
    Piola-Kirchhoff stress by the derivatives of the tensor logarithm.  ``s0 > 0``, ``H0 >= 0``; ``E`` and ``nu`` default to the
    values the behaviour file writes in (210e9, 0.3).  Internal state variables ``ElasticStrain`` (6) and
    ``EquivalentPlasticStrain`` (1), MFront's names.

    ``JAXMaterial(LogarithmicStrainPlasticity.from_mfront_properties({"YieldStrength": 250e6, "HardeningSlope": 1e6}))`` stands
    where the demo uses ``MFrontMaterial(lib, "LogarithmicStrainPlasticity", material_properties=...)``: gradient
    ``DeformationGradient`` (9), flux ``FirstPiolaKirchhoffStress`` (9), tangent block ``(9, 9)``.  Full tangent only; uniform
    properties only; the displacement forms need option ``fused_gradient`` off.

    ``hypothesis="plane_strain"`` (``MFrontMaterial(lib, "LogarithmicStrainPlasticity", hypothesis="plane_strain")``): the gradient is
    the 5-vector ``[F00, F11, F22, F01, F10]`` of a 2x2 tensor with its out-of-plane stretch (``utils.py:168-172``), the flux the 5-wide
    PK1 in the same order, the tangent block ``(5, 5)``, ``ElasticStrain`` the 4-vector ``[xx, yy, zz, sqrt(2) xy]``: the 9-wide law on
    the embedded ``F``, restricted (``conventions.embed_plane_F`` / ``restrict_plane_F`` / ``restrict_plane_F_tangent`` /
    ``restrict_plane_strain``).  ``F22`` is read, not assumed to be 1.  F is passed as an array: the displacement forms are not served
    under this hypothesis."""

    law = _lib.LAW_LOG_STRAIN_J2
    gradient_name = "DeformationGradient"
    flux_name = "FirstPiolaKirchhoffStress"

    def __init__(self, s0: float, H0: float, E: float = 210e9, nu: float = 0.3, hypothesis: str = "3d"):
        if _check_hypothesis(hypothesis) == "plane_strain":
            self.hypothesis = hypothesis
            self.law = _lib.LAW_LOG_STRAIN_PE
            self.ngrad = self.nflux = 5
        self.s0 = float(s0)
        self.H0 = float(H0)
        self.E = float(E)
        self.nu = float(nu)
        if not (self.E > 0.0 and -1.0 < self.nu < 0.5 and self.s0 > 0.0 and self.H0 >= 0.0
                and all(map(_isfinite, (self.E, self.nu, self.s0, self.H0)))):
            raise ValueError("logarithmic-strain plasticity: E > 0, -1 < nu < 0.5, s0 > 0 and H0 >= 0 (all finite); "
                             f"got E={E}, nu={nu}, s0={s0}, H0={H0}")

    @classmethod
    def from_mfront_properties(cls, props: dict, hypothesis: str = "3d"):
        """The ``material_properties`` of the demo: ``HardeningSlope`` and ``YieldStrength`` (the demo's key; ``YieldStress``, the
        glossary name, is taken too).  ``E`` and ``nu`` are written into the behaviour file and are no material properties.
        ``hypothesis``: that of the same call."""
        props = dict(props)
        extra = set(props) - {"HardeningSlope", "YieldStrength", "YieldStress"}
        if extra:
            raise ValueError(f"logarithmic-strain plasticity material properties: unknown {sorted(extra)} (the behaviour has YieldStrength, "
                             "HardeningSlope)")
        if "YieldStrength" in props and "YieldStress" in props:
            raise ValueError("logarithmic-strain plasticity material properties: YieldStrength and YieldStress name the same property, pass one")
        missing = [k for k, ok in (("YieldStrength", "YieldStrength" in props or "YieldStress" in props),
                                   ("HardeningSlope", "HardeningSlope" in props)) if not ok]
        if missing:
            raise ValueError(f"logarithmic-strain plasticity material properties: missing {missing}")
        return cls(s0=float(props.get("YieldStrength", props.get("YieldStress"))), H0=float(props["HardeningSlope"]), hypothesis=hypothesis)

    def params(self):
        return [self.E, self.nu, self.s0, self.H0]

    def flat_properties(self):
        return {"E": self.E, "nu": self.nu, "s0": self.s0, "H0": self.H0}


class OrthotropicElasticity(SmallStrainBehavior):
    """Small-strain orthotropic elasticity in a material frame (the orthotropic form of MFront's ``StandardElasticity`` brick, as
    ``tests/mfront/MericCailletaudSingleCrystalViscoPlasticity.mfront:18-28`` sets it up): nine constants ``E1, E2, E3, nu12,
    nu23, nu13, G12, G23, G13``; all finite, ``E_i > 0``, ``G_ij > 0`` and a positive definite compliance.  No internal state.

    ``JAXMaterial(OrthotropicElasticity(...))`` is the one material here whose ``rotation_matrix`` can be set: a constant 3x3
    array, or anything else for the quadrature map to evaluate per point (``mfront.py:83``).  The ROWS of the matrix are the
    material axes in global coordinates -- the matrix ``tests/uniaxial_tension.py:61-66`` builds.  The rotation happens inside the
    kernel: gradients, fluxes and tangents of every call are global.  Tangent layouts ``"full"`` and ``"sym"``; uniform
    properties only; the displacement forms need option ``fused_gradient`` off."""

    law = _lib.LAW_ORTHOTROPIC_ELASTIC
    gradient_name = "Strain"
    flux_name = "Stress"
    NAMES = ("E1", "E2", "E3", "nu12", "nu23", "nu13", "G12", "G23", "G13")
    #: the MFront glossary names of the nine constants, in the order of the parameter vector
    MFRONT_NAMES = ("YoungModulus1", "YoungModulus2", "YoungModulus3", "PoissonRatio12", "PoissonRatio23", "PoissonRatio13",
                    "ShearModulus12", "ShearModulus23", "ShearModulus13")

    def __init__(self, E1, E2, E3, nu12, nu23, nu13, G12, G23, G13):
        for name, v in zip(self.NAMES, (E1, E2, E3, nu12, nu23, nu13, G12, G23, G13)):
            object.__setattr__(self, name, float(v))
        self.validate()

    def validate(self):
        """The rules the library applies in ``dxm_create`` / ``dxm_set_params``, with the offending value in the message."""
        p = dict(zip(self.NAMES, self.params()))
        for k, v in p.items():
            if not _isfinite(v):
                raise ValueError(f"orthotropic elasticity: {k} must be finite, got {v}")
        for k in ("E1", "E2", "E3", "G12", "G23", "G13"):
            if not p[k] > 0.0:
                raise ValueError(f"orthotropic elasticity: {k} must be > 0, got {p[k]}")
        # leading minors of the compliance, scaled
        m2 = 1.0 - p["nu12"] ** 2 * p["E2"] / p["E1"]
        m3 = (m2 - p["nu23"] ** 2 * p["E3"] / p["E2"] - p["nu13"] ** 2 * p["E3"] / p["E1"]
              - 2.0 * p["nu12"] * p["nu23"] * p["nu13"] * p["E3"] / p["E1"])
        if not (m2 > 0.0 and m3 > 0.0):
            raise ValueError("orthotropic elasticity: the compliance is not positive definite: 1 - nu12^2 E2/E1 = "
                             f"{m2:g}, det(S) E1 E2 E3 = {m3:g}")

    @classmethod
    def from_mfront_properties(cls, props: dict):
        """``material_properties`` keyed by the glossary names (``YoungModulus1`` ... ``ShearModulus13``), all nine."""
        missing, extra = set(cls.MFRONT_NAMES) - set(props), set(props) - set(cls.MFRONT_NAMES)
        if missing or extra:
            raise ValueError(f"orthotropic elasticity material properties: missing {sorted(missing)}, unknown {sorted(extra)}")
        return cls(*(float(props[k]) for k in cls.MFRONT_NAMES))

    # the properties are read and written under their glossary names (update_material_property("YoungModulus1", ...))
    def __getattr__(self, name):
        if name in type(self).MFRONT_NAMES:
            return getattr(self, self.NAMES[self.MFRONT_NAMES.index(name)])
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in self.MFRONT_NAMES:
            name = self.NAMES[self.MFRONT_NAMES.index(name)]
        object.__setattr__(self, name, float(value) if name in self.NAMES else value)

    def params(self):
        return [getattr(self, k) for k in self.NAMES]

    def flat_properties(self):
        return {g: getattr(self, k) for g, k in zip(self.MFRONT_NAMES, self.NAMES)}


class MericCailletaudSingleCrystalViscoPlasticity(OrthotropicElasticity):
    """Small-strain FCC single-crystal viscoplasticity (the reference's ``MericCailletaudSingleCrystalViscoPlasticity`` MFront
    behaviour, ``tests/mfront/test_elastoplasticity.py::test_mfront_single_cristal``): the orthotropic elasticity of
    :class:`OrthotropicElasticity`, twelve ``{111}<01-1>`` slip systems with Norton flow ``(f/K)^n``, nonlinear isotropic hardening
    ``tau0 + Q sum_j h_ij (1 - exp(-b p_j))`` through the six-coefficient interaction matrix ``h = [self, coplanar, Hirth,
    collinear, glissile, Lomer]``, and Armstrong-Frederick kinematic hardening ``x = C a``.  Rate-dependent: the time increment is
    ``material.dt`` (or the ``dt`` of the call).  Internal state variables, all in the material frame: ``ElasticStrain`` (6),
    ``ViscoplasticSlip`` (12), ``EquivalentViscoplasticSlip`` (12), ``BackStrain`` (12); the systems are numbered plane-major over
    (1,1,1), (-1,1,1), (1,-1,1), (1,1,-1), which is this library's order, not necessarily MFront's.

    ``rotation_matrix`` and ``set_frame`` as for :class:`OrthotropicElasticity` (rows = material axes); the frame must not change
    while slip has accumulated.  Tangent layout ``"full"`` only (the tangent is not symmetric); uniform properties only; the
    displacement forms need option ``fused_gradient`` off."""

    law = _lib.LAW_SINGLE_CRYSTAL_FCC
    FLOW_NAMES = ("n", "K", "tau0", "Q", "b", "d", "C")
    #: the constants of the behaviour file next to the one material property it declares (``YoungModulus1``)
    MFRONT_DEFAULTS = {"YoungModulus2": 208000.0, "YoungModulus3": 208000.0, "PoissonRatio12": 0.3, "PoissonRatio23": 0.3,
                       "PoissonRatio13": 0.3, "ShearModulus12": 80000.0, "ShearModulus23": 80000.0, "ShearModulus13": 80000.0}
    MFRONT_FLOW = {"n": 10.0, "K": 25.0, "tau0": 66.62, "Q": 11.43, "b": 2.1, "d": 494.0, "C": 14363.0}
    #: the published copper values, [self, coplanar, Hirth, collinear, glissile, Lomer]
    INTERACTION = (1.0, 1.0, 0.6, 12.3, 1.6, 1.8)

    def __init__(self, E1, E2, E3, nu12, nu23, nu13, G12, G23, G13, n=10.0, K=25.0, tau0=66.62, Q=11.43, b=2.1, d=494.0, C=14363.0,
                 interaction=INTERACTION):
        for name, v in zip(self.FLOW_NAMES, (n, K, tau0, Q, b, d, C)):
            object.__setattr__(self, name, float(v))
        h = tuple(float(v) for v in interaction)
        if len(h) != 6:
            raise ValueError(f"single-crystal viscoplasticity: the interaction matrix takes six coefficients, got {len(h)}")
        object.__setattr__(self, "interaction", h)
        super().__init__(E1, E2, E3, nu12, nu23, nu13, G12, G23, G13)

    def validate(self):
        super().validate()
        for k in self.FLOW_NAMES:
            if not _isfinite(getattr(self, k)):
                raise ValueError(f"single-crystal viscoplasticity: {k} must be finite, got {getattr(self, k)}")
        for k, v in zip(("h_self", "h_coplanar", "h_Hirth", "h_collinear", "h_glissile", "h_Lomer"), self.interaction):
            if not _isfinite(v):
                raise ValueError(f"single-crystal viscoplasticity: {k} must be finite, got {v}")
        if not self.n >= 1.0:
            raise ValueError(f"single-crystal viscoplasticity: the Norton exponent n must be >= 1, got {self.n}")
        if not self.K > 0.0:
            raise ValueError(f"single-crystal viscoplasticity: K must be > 0, got {self.K}")
        for k in ("tau0", "b", "d", "C"):
            if not getattr(self, k) >= 0.0:
                raise ValueError(f"single-crystal viscoplasticity: {k} must be >= 0, got {getattr(self, k)}")

    @classmethod
    def from_mfront_properties(cls, props: dict):
        """``material_properties`` of the reference test: ``{"YoungModulus1": ...}``; the other elastic constants, the flow and
        hardening parameters and the interaction matrix are those of the behaviour file unless given (glossary names for the
        elastic constants, ``n, K, tau0, Q, b, d, C``, ``interaction``)."""
        known = set(cls.MFRONT_NAMES) | set(cls.FLOW_NAMES) | {"interaction"}
        extra = set(props) - known
        if "YoungModulus1" not in props or extra:
            raise ValueError(f"single-crystal material properties: YoungModulus1 is required, unknown {sorted(extra)}")
        el = {**cls.MFRONT_DEFAULTS, **{k: props[k] for k in cls.MFRONT_NAMES if k in props}}
        flow = {k: float(props.get(k, v)) for k, v in cls.MFRONT_FLOW.items()}
        return cls(*(float(el[k]) for k in cls.MFRONT_NAMES), interaction=props.get("interaction", cls.INTERACTION), **flow)

    def __setattr__(self, name, value):
        if name in self.FLOW_NAMES:
            object.__setattr__(self, name, float(value))
        else:
            super().__setattr__(name, value)

    def params(self):
        return super().params() + [getattr(self, k) for k in self.FLOW_NAMES] + list(self.interaction)

    def flat_properties(self):
        return {**super().flat_properties(), **{k: getattr(self, k) for k in self.FLOW_NAMES},
                **{f"interaction.{i}": v for i, v in enumerate(self.interaction)}}


class FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity(FiniteStrainBehavior):
    """Finite-strain FCC single-crystal viscoplasticity (the reference's
    ``mfront_materials/FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity.mfront``): multiplicative ``F = Fe Fp``, cubic
    elasticity of ``E, nu, G`` between the Green-Lagrange strain of ``Fe`` and its second Piola-Kirchhoff stress, the twelve
    ``{111}<01-1>`` systems, Norton flow, interaction hardening and Armstrong-Frederick back strain of
    :class:`MericCailletaudSingleCrystalViscoPlasticity` driven by the Mandel stress on the non-symmetrised ``m_i x n_i``.  The
    file's interaction matrix is self-hardening only, which is the default here.  Rate-dependent: the time increment is
    ``material.dt`` (or the ``dt`` of the call).

    Gradient ``DeformationGradient`` (9), flux ``FirstPiolaKirchhoffStress`` (9), tangent block ``(9, 9)``.  Internal state
    variables, all in the material frame: ``PlasticSlip`` (12), ``EquivalentViscoplasticSlip`` (12), ``BackStrain`` (12),
    ``PlasticPartOfTheDeformationGradient`` (9, the identity at the start).  MFront's other variables are functions of ``F`` and
    this state: :meth:`derived_state` returns them under MFront's names.  The systems are numbered as for the small-strain law,
    which is this library's order, not necessarily MFront's.

    ``rotation_matrix`` and ``set_frame`` as for :class:`OrthotropicElasticity` (rows = material axes).  Tangent layout ``"full"``
    only; uniform properties only; ``F`` is passed as an array (no displacement forms)."""

    law = _lib.LAW_FS_SINGLE_CRYSTAL_FCC
    gradient_name = "DeformationGradient"
    flux_name = "FirstPiolaKirchhoffStress"
    #: the ten material properties of the behaviour file, in the order of the parameter vector
    NAMES = ("E", "nu", "G", "n", "K", "tau0", "Q", "b", "d", "C")
    #: the file's interaction matrix, [self, coplanar, Hirth, collinear, glissile, Lomer]
    INTERACTION = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)

    def __init__(self, E, nu, G, n, K, Q, b, tau0, d, C, interaction=INTERACTION):
        for name, v in zip(("E", "nu", "G", "n", "K", "Q", "b", "tau0", "d", "C"), (E, nu, G, n, K, Q, b, tau0, d, C)):
            object.__setattr__(self, name, float(v))
        h = tuple(float(v) for v in interaction)
        if len(h) != 6:
            raise ValueError(f"finite-strain single-crystal viscoplasticity: the interaction matrix takes six coefficients, got {len(h)}")
        object.__setattr__(self, "interaction", h)
        self.validate()

    def validate(self):
        """The rules the library applies in ``dxm_create`` / ``dxm_set_params``, with the offending value in the message."""
        for k in self.NAMES:
            if not _isfinite(getattr(self, k)):
                raise ValueError(f"finite-strain single-crystal viscoplasticity: {k} must be finite, got {getattr(self, k)}")
        for k, v in zip(("h_self", "h_coplanar", "h_Hirth", "h_collinear", "h_glissile", "h_Lomer"), self.interaction):
            if not _isfinite(v):
                raise ValueError(f"finite-strain single-crystal viscoplasticity: {k} must be finite, got {v}")
        for k in ("E", "G", "K"):
            if not getattr(self, k) > 0.0:
                raise ValueError(f"finite-strain single-crystal viscoplasticity: {k} must be > 0, got {getattr(self, k)}")
        if not -1.0 < self.nu < 0.5:
            raise ValueError(f"finite-strain single-crystal viscoplasticity: nu must lie in (-1, 0.5), got {self.nu}")
        if not self.n >= 1.0:
            raise ValueError(f"finite-strain single-crystal viscoplasticity: the Norton exponent n must be >= 1, got {self.n}")
        for k in ("tau0", "b", "d", "C"):
            if not getattr(self, k) >= 0.0:
                raise ValueError(f"finite-strain single-crystal viscoplasticity: {k} must be >= 0, got {getattr(self, k)}")

    @classmethod
    def from_mfront_properties(cls, props: dict):
        """``material_properties`` keyed by the file's names, all ten: it gives no defaults.  ``interaction`` may be added."""
        missing, extra = set(cls.NAMES) - set(props), set(props) - set(cls.NAMES) - {"interaction"}
        if missing or extra:
            raise ValueError(f"finite-strain single-crystal material properties: missing {sorted(missing)}, unknown {sorted(extra)}")
        return cls(**{k: float(props[k]) for k in cls.NAMES}, interaction=props.get("interaction", cls.INTERACTION))

    def __setattr__(self, name, value):
        object.__setattr__(self, name, float(value) if name in self.NAMES else value)

    def params(self):
        return [getattr(self, k) for k in self.NAMES] + list(self.interaction)

    def flat_properties(self):
        return {**{k: getattr(self, k) for k in self.NAMES}, **{f"interaction.{i}": v for i, v in enumerate(self.interaction)}}

    def derived_state(self, F, state, rotation=None):
        """MFront's variables that are functions of ``F`` and the state, on the host: ``ElasticStrain`` (N, 6) -- the
        Green-Lagrange strain of ``Fe``, tensor components [11, 22, 33, 12, 13, 23] --, ``ElasticPartOfTheDeformationGradient``
        (N, 9) and ``ResolvedShearStress`` (N, 12), all in the material frame.  ``F`` (N, 9); ``state`` maps
        ``PlasticPartOfTheDeformationGradient`` to (N, 9); ``rotation``: None, (3, 3) or (N, 3, 3), rows = material axes."""
        import numpy as np

        TI, TJ = (0, 1, 2, 0, 1, 0, 2, 1, 2), (0, 1, 2, 1, 0, 2, 0, 2, 1)   # the order of the 9-vectors

        F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
        N = F.shape[0]
        Fp = np.asarray(state["PlasticPartOfTheDeformationGradient"], dtype=np.float64).reshape(N, 9)

        def mat(v):
            m = np.empty((N, 3, 3))
            for t in range(9):
                m[:, TI[t], TJ[t]] = v[:, t]
            return m

        Fm = mat(F)
        if rotation is not None:
            R = np.broadcast_to(np.asarray(rotation, dtype=np.float64).reshape(-1, 3, 3), (N, 3, 3))
            Fm = R @ Fm @ np.swapaxes(R, 1, 2)
        Fe = Fm @ np.linalg.inv(mat(Fp))
        Eel = 0.5 * (np.swapaxes(Fe, 1, 2) @ Fe - np.eye(3))
        # the cubic stiffness: the normal block is the inverse of the compliance block
        S3 = np.full((3, 3), -self.nu / self.E)
        np.fill_diagonal(S3, 1.0 / self.E)
        A = np.linalg.inv(S3)
        S = 2.0 * self.G * Eel
        tr = Eel[:, 0, 0] + Eel[:, 1, 1] + Eel[:, 2, 2]
        for i in range(3):
            S[:, i, i] = (A[0, 0] - A[0, 1]) * Eel[:, i, i] + A[0, 1] * tr
        M = (np.swapaxes(Fe, 1, 2) @ Fe) @ S
        planes = ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1))
        dirs = ((0, 1, -1), (1, 0, -1), (1, -1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0))
        mu = np.array([np.outer(d, p) / np.sqrt(6.0) for p in planes for d in dirs if np.dot(p, d) == 0])
        return {"ElasticStrain": np.stack([Eel[:, 0, 0], Eel[:, 1, 1], Eel[:, 2, 2], Eel[:, 0, 1], Eel[:, 0, 2], Eel[:, 1, 2]], axis=1),
                "ElasticPartOfTheDeformationGradient": np.stack([Fe[:, TI[t], TJ[t]] for t in range(9)], axis=1),
                "ResolvedShearStress": np.einsum("nkl,ikl->ni", M, mu)}


class HeatTransferBehavior(Behavior):
    """Base of the heat-transfer laws: gradient ``TemperatureGradient`` (3), flux ``HeatFlux`` (3) and one external state variable,
    ``Temperature``, the value at the end of the step (``HIPMaterial.update_external_state_variable``).  The gradient is 3 wide
    under the default hypothesis: a 2-D caller pads ``grad(T)`` with a zero.  ``hypothesis="plane_strain"`` (what the reference's
    heat-transfer demos load their law with, ``MFrontMaterial(..., hypothesis="plane_strain")``): gradient and flux are 2 wide,
    ``[d/dx, d/dy]``, the tangent blocks ``(2, 2)``, ``(2, 1)`` [``(1, 1)``]; with a :class:`gradient.PlaneScalarMesh` such a
    material is updated from the nodal temperature (``HIPMaterial.integrate_displacement*``)."""

    gradient_name = "TemperatureGradient"
    flux_name = "HeatFlux"
    ngrad = 3
    nflux = 3
    external_state_variables = {"Temperature": 1}
    NAMES = ()

    #: the law of ``hypothesis="plane_strain"``
    law_2d = None

    def _set_hypothesis(self, hypothesis):
        self.hypothesis = _check_hypothesis(hypothesis)
        if hypothesis == "plane_strain":
            self.ngrad = self.nflux = 2
            self.law = self.law_2d

    def validate(self):
        for k in self.NAMES:
            if not _isfinite(getattr(self, k)):
                raise ValueError(f"{type(self).__name__}: {k} must be finite, got {getattr(self, k)}")

    def __setattr__(self, name, value):
        object.__setattr__(self, name, float(value) if name in self.NAMES else value)

    def get_parameter(self, name):
        """``mgis.behaviour.getParameterDefaultValue`` as the demos use it (``material.get_parameter("A")``): the current value."""
        if name not in self.NAMES:
            raise ValueError(f"{type(self).__name__} has no parameter {name!r} (it has {list(self.NAMES)})")
        return getattr(self, name)

    def params(self):
        return [getattr(self, k) for k in self.NAMES]

    def flat_properties(self):
        return {k: getattr(self, k) for k in self.NAMES}


class StationaryHeatTransfer(HeatTransferBehavior):
    """``demos/mfront/heat_transfer/StationaryHeatTransfer.mfront``: ``k = 1 / (A + B T)``, ``j = -k grad(T)``; tangent blocks
    ``(HeatFlux, TemperatureGradient) = -k I`` and ``(HeatFlux, Temperature) = B k^2 grad(T)``.  ``A + B T <= 0`` is not refused
    (MFront does not refuse it either)."""

    law = _lib.LAW_HEAT_STATIONARY
    law_2d = _lib.LAW_HEAT_STATIONARY_2D
    NAMES = ("A", "B")
    MFRONT_DEFAULTS = {"A": 0.0375, "B": 2.165e-4}

    def __init__(self, A: float = MFRONT_DEFAULTS["A"], B: float = MFRONT_DEFAULTS["B"], hypothesis: str = "3d"):
        self._set_hypothesis(hypothesis)
        self.A, self.B = A, B
        self.validate()

    @classmethod
    def from_mfront_properties(cls, props: dict | None = None, hypothesis: str = "3d"):
        props = dict(props or {})
        extra = set(props) - set(cls.NAMES)
        if extra:
            raise ValueError(f"stationary heat transfer parameters: unknown {sorted(extra)}")
        return cls(**{**cls.MFRONT_DEFAULTS, **props}, hypothesis=hypothesis)


class HeatTransferPhaseChange(HeatTransferBehavior):
    """``demos/mfront/heat_transfer/HeatTransferPhaseChange.mfront`` (its lines 41-56, not the demo's prose: the transition's heat
    capacity is ``(cs + cl) / 2 + dhsl / Tsmooth``): conductivity and enthalpy of a solid / liquid with a transition of width
    ``Tsmooth`` around the melting temperature.  One internal state variable, ``Enthalpy`` (1), and three tangent blocks:
    ``(HeatFlux, TemperatureGradient)``, ``(HeatFlux, Temperature)``, ``(Enthalpy, Temperature)``.  The parameters carry the file's
    entry names."""

    law = _lib.LAW_HEAT_PHASE_CHANGE
    law_2d = _lib.LAW_HEAT_PHASE_CHANGE_2D
    NAMES = ("MeltingTemperature", "SolidConductivity", "SolidHeatCapacity", "LiquidConductivity", "LiquidHeatCapacity", "FusionEnthalpy",
             "Tsmooth")
    MFRONT_DEFAULTS = {"MeltingTemperature": 933.15, "SolidConductivity": 210.0, "SolidHeatCapacity": 3.0e6, "LiquidConductivity": 95.0,
                       "LiquidHeatCapacity": 2.58e6, "FusionEnthalpy": 1.08048e9, "Tsmooth": 0.1}

    def __init__(self, MeltingTemperature=MFRONT_DEFAULTS["MeltingTemperature"], SolidConductivity=MFRONT_DEFAULTS["SolidConductivity"],
                 SolidHeatCapacity=MFRONT_DEFAULTS["SolidHeatCapacity"], LiquidConductivity=MFRONT_DEFAULTS["LiquidConductivity"],
                 LiquidHeatCapacity=MFRONT_DEFAULTS["LiquidHeatCapacity"], FusionEnthalpy=MFRONT_DEFAULTS["FusionEnthalpy"],
                 Tsmooth=MFRONT_DEFAULTS["Tsmooth"], hypothesis: str = "3d"):
        self._set_hypothesis(hypothesis)
        for k, v in zip(self.NAMES, (MeltingTemperature, SolidConductivity, SolidHeatCapacity, LiquidConductivity, LiquidHeatCapacity,
                                     FusionEnthalpy, Tsmooth)):
            setattr(self, k, v)
        self.validate()

    def validate(self):
        super().validate()
        if not self.Tsmooth > 0.0:
            raise ValueError(f"HeatTransferPhaseChange: Tsmooth must be > 0, got {self.Tsmooth}")

    @classmethod
    def from_mfront_properties(cls, props: dict | None = None, hypothesis: str = "3d"):
        """Parameters keyed by the file's entry names; those not given keep the file's defaults."""
        props = dict(props or {})
        extra = set(props) - set(cls.NAMES)
        if extra:
            raise ValueError(f"heat transfer with phase change parameters: unknown {sorted(extra)}")
        return cls(**{**cls.MFRONT_DEFAULTS, **props}, hypothesis=hypothesis)


class PlaneStressBehavior(Behavior):
    """Base of the plane-stress return mappings (the reference's ``demos/cvxpy/cvxpy_materials.py``): gradient ``Strain`` (3), flux
    ``Stress`` (3), both ``[xx, yy, sqrt(2) xy]``; perfectly plastic; no internal state variable (the state of the reference is the
    strain and the stress of the last accepted increment, which the material keeps as the gradient and the flux of ``s0``)."""

    gradient_name = "Strain"
    flux_name = "Stress"
    ngrad = 3
    nflux = 3

    def _check_elastic(self):
        if not (_isfinite(self.E) and _isfinite(self.nu) and self.E > 0.0 and -1.0 < self.nu < 1.0):
            raise ValueError(f"{type(self).__name__}: E must be > 0 and -1 < nu < 1 (both finite); got E={self.E}, nu={self.nu}")


class PlaneStressQuadraticYield(PlaneStressBehavior):
    """Closest-point projection, in the elastic energy norm, of the trial stress onto ``{s^T Q s <= sig0^2}`` with
    ``Q = [[1, -1/2, 0], [-1/2, 1, 0], [0, 0, q]]``.  ``q = 1`` is the matrix of the reference's ``PlaneStressvonMises``
    (``cvxpy_materials.py:89-93``) -- NOT von Mises in Kelvin-Mandel components, where the third component is ``sqrt(2) s_xy``;
    ``q = 3/2`` is von Mises.  ``tangent`` 0 hands back the elastic ``C`` like the reference, 1 the algorithmic tangent of the
    yielded points."""

    law = _lib.LAW_PS_QUADRATIC

    def __init__(self, E, nu, sig0, q=1.0, tangent=0):
        self.E, self.nu, self.sig0, self.q = float(E), float(nu), float(sig0), float(q)
        self.tangent = int(tangent)
        self._check_elastic()
        if not (_isfinite(self.sig0) and self.sig0 > 0.0):
            raise ValueError(f"{type(self).__name__}: sig0 must be finite and > 0, got {sig0}")
        if not (_isfinite(self.q) and self.q > 0.0):
            raise ValueError(f"{type(self).__name__}: the shear weight q must be finite and > 0, got {q}")
        if tangent not in (0, 1):
            raise ValueError(f"{type(self).__name__}: tangent must be 0 (elastic) or 1 (algorithmic), got {tangent!r}")

    def params(self):
        return [self.E, self.nu, self.sig0, self.q, float(self.tangent)]

    def flat_properties(self):
        return {"E": self.E, "nu": self.nu, "sig0": self.sig0, "q": self.q}


class PlaneStressPolygonYield(PlaneStressBehavior):
    """Closest-point projection onto ``{n_k . (s_I, s_II) <= d_k}``: at most four half-planes ``(n1, n2, d)`` in the unordered plane
    of the two principal stresses, ``d > 0``, no zero normal, and the list closed under the exchange of the principal stresses (the
    mirror ``(n2, n1, d)`` of every row is a row).  The tangent handed back is the elastic ``C``."""

    law = _lib.LAW_PS_POLYGON
    MAX_PLANES = 4

    def __init__(self, E, nu, planes):
        self.E, self.nu = float(E), float(nu)
        self._check_elastic()
        try:
            rows = [tuple(float(v) for v in r) for r in planes]
        except TypeError:
            raise ValueError(f"{type(self).__name__}: planes must be a list of (n1, n2, d) rows, got {planes!r}") from None
        if not 1 <= len(rows) <= self.MAX_PLANES or any(len(r) != 3 for r in rows):
            raise ValueError(f"{type(self).__name__}: between 1 and {self.MAX_PLANES} half-planes (n1, n2, d), got {planes!r}")
        for k, (n1, n2, d) in enumerate(rows):
            if not all(map(_isfinite, (n1, n2, d))):
                raise ValueError(f"{type(self).__name__}: half-plane {k} {rows[k]} must be finite")
            if not d > 0.0:
                raise ValueError(f"{type(self).__name__}: half-plane {k} has d = {d}: d must be > 0, the origin lies strictly inside the set")
            if n1 == 0.0 and n2 == 0.0:
                raise ValueError(f"{type(self).__name__}: half-plane {k} has a zero normal")
        for k, (n1, n2, d) in enumerate(rows):
            if (n2, n1, d) not in rows:
                raise ValueError(f"{type(self).__name__}: the half-planes are not symmetric under the exchange of the principal stresses: "
                                 f"the mirror {(n2, n1, d)} of half-plane {k} is not in the list")
        self.planes = rows

    def params(self):
        flat = [v for r in self.planes for v in r]
        return [self.E, self.nu, float(len(self.planes))] + flat + [0.0] * (3 * self.MAX_PLANES - len(flat))

    def flat_properties(self):
        return {"E": self.E, "nu": self.nu}


class PlaneStressHosfordYield(PlaneStressBehavior):
    """Closest-point projection, in the elastic energy norm, of the trial stress onto ``{phi(s) <= sig0}`` with the Hosford function
    ``phi = ((|s_I|^a + |s_II|^a + |s_I - s_II|^a) / 2)^(1/a)`` of the principal stresses (the reference's ``PlaneStressHosford``,
    ``cvxpy_materials.py:96-110``).  ``2 <= a <= 100``, not necessarily an integer; ``a = 2`` is von Mises.  ``tangent`` 0 hands
    back the elastic ``C`` like the reference, 1 the algorithmic tangent of the yielded points."""

    law = _lib.LAW_PS_HOSFORD
    A_MIN, A_MAX = 2.0, 100.0

    def __init__(self, E, nu, sig0, a, tangent=0):
        self.E, self.nu, self.sig0, self.a = float(E), float(nu), float(sig0), float(a)
        self.tangent = int(tangent)
        self._check_elastic()
        if not (_isfinite(self.sig0) and self.sig0 > 0.0):
            raise ValueError(f"{type(self).__name__}: sig0 must be finite and > 0, got {sig0}")
        if not _isfinite(self.a):
            raise ValueError(f"{type(self).__name__}: the exponent a must be finite, got {a}")
        if not self.a >= self.A_MIN:
            raise ValueError(f"{type(self).__name__}: the exponent a must be >= 2 (below 2 the Hessian of the yield function is "
                             f"unbounded on the axes), got {a}")
        if not self.a <= self.A_MAX:
            raise ValueError(f"{type(self).__name__}: the exponent a must be <= 100 (the largest exponent at which the accuracy was "
                             f"measured), got {a}")
        if tangent not in (0, 1):
            raise ValueError(f"{type(self).__name__}: tangent must be 0 (elastic) or 1 (algorithmic), got {tangent!r}")

    def params(self):
        return [self.E, self.nu, self.sig0, self.a, float(self.tangent)]

    def flat_properties(self):
        return {"E": self.E, "nu": self.nu, "sig0": self.sig0, "a": self.a}


class PlaneStressJ2(PlaneStressBehavior):
    """Small-strain J2 plasticity with isotropic hardening under plane stress (``sig_zz = sig_xz = sig_yz = 0``): the law of
    :class:`vonMisesIsotropicHardening` on ``[xx, yy, sqrt(2) xy]``, what the reference's
    ``demos/jax/elastoplasticity/_plane_stress_elastoplasticity.py`` obtains with ``eps_zz`` as an extra unknown.  Internal state
    variables ``p`` (1) and ``epsp`` (3, in-plane; ``epsp_zz = -(epsp_xx + epsp_yy)``); the tangent is the consistent 3x3 block.
    Stock hardening laws only."""

    def __init__(self, elasticity: LinearElasticIsotropic, yield_stress):
        if not isinstance(yield_stress, (LinearHardening, VoceHardening)):
            raise TypeError("plane-stress J2 plasticity is served with the stock hardening laws only: yield_stress must be a "
                            "materials.LinearHardening or materials.VoceHardening, not a CustomHardening or a traced callable "
                            f"(got {type(yield_stress).__name__})")
        self.elasticity = elasticity
        self.yield_stress = yield_stress
        self.law = _lib.LAW_PS_J2_LINEAR if isinstance(yield_stress, LinearHardening) else _lib.LAW_PS_J2_VOCE

    @property
    def E(self):
        return self.elasticity.E

    @property
    def nu(self):
        return self.elasticity.nu

    def params(self):
        return _hardening_params(self.elasticity, self.yield_stress)

    def flat_properties(self):
        out = {"elasticity.E": self.elasticity.E, "elasticity.nu": self.elasticity.nu}
        out.update(_hardening_properties(self.yield_stress))
        return out


def _isfinite(x):
    return x == x and abs(x) != float("inf")
