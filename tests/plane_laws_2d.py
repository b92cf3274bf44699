"""The eight two-dimensional laws as the displacement-form tests drive them: parameters, the gradient kind a two-dimensional mesh is
asked for, the state fields, the numpy restatement of each family behind one call, and the two displacement increments (a uniaxial
stretch past yield plus nodal noise, ``plane_gradient_ref.stretch_field``, scaled by the law's yield strain).  TEST INFRASTRUCTURE ONLY;
no GPU."""
import numpy as np

import plane_gradient_ref as pg
import plane_strain_ref as pe
import plane_stress_hosford_ref as psh
import plane_stress_j2_ref as pj
import plane_stress_ref as ps

E = 70e3
_PS = dict(kind=3, width=3, fields=(3,), yields=True)
_PE = dict(kind=2, width=4, fields=(1, 4), yields=True)
_PJ = dict(kind=3, width=3, fields=(1, 3), yields=True)
#: law id -> kind (of dxm_mesh_gradient_device), width of strain and stress, dims of the state fields dxm_get_state addresses,
#: parameters, yield stress (the scale of the displacement)
LAWS = {
    23: dict(_PS, prm=[E, 0.2, 30.0, 1.5, 1.0], sig0=30.0, family="plane_stress"),
    24: dict(_PS, prm=ps.polygon_params(E, 0.2, ps.rankine_planes(10.0, 30.0)), sig0=10.0, family="plane_stress"),
    26: dict(_PE, prm=[E, 0.3], sig0=250.0, fields=(), yields=False, family="plane_strain"),
    27: dict(_PE, prm=[E, 0.3, 250.0, 5e3], sig0=250.0, family="plane_strain"),
    28: dict(_PE, prm=[E, 0.3, 350.0, 500.0, 1e3], sig0=350.0, family="plane_strain"),
    30: dict(_PJ, prm=[E, 0.3, 250.0, 5e3], sig0=250.0, family="plane_stress_j2"),
    31: dict(_PJ, prm=[E, 0.3, 350.0, 500.0, 1e3], sig0=350.0, family="plane_stress_j2"),
    33: dict(_PS, prm=[E, 0.2, 30.0, 10.0, 1.0], sig0=30.0, family="plane_stress_hosford"),
}
#: one law per family is also held to its numpy restatement on the reference gradient
PARITY_LAWS = (23, 27, 30, 33)
#: the stretch of ``plane_gradient_ref.STRETCH`` (5e-3 axial) is written for sig0 / E = 250 / 70e3; the two load steps, chosen so that
#: on both meshes between a tenth and nine tenths of the points yield in each (test_plane_gradient_cpu.py asserts it on the CPU):
#: the nodal noise, not the stretch, decides which
STEPS = (0.42, 0.56)


def increments(law, mesh_name):
    """the displacement vectors of the two load steps: the stretch field scaled to the law's yield strain"""
    scale = LAWS[law]["sig0"] / 250.0
    return [pg.stretch_field(mesh_name, t=t * scale) for t in STEPS]


def reference_update(law, eps, carry=None):
    """One increment of the law's numpy restatement from the state ``carry`` of the last call (None: the initial state).
    dict(stress (n, w), tangent (n, w w), state (n, sum of the fields), plastic, carry)."""
    spec = LAWS[law]
    n, prm = len(eps), spec["prm"]
    if spec["family"] == "plane_strain":
        epsp, p = (np.zeros((n, 4)), np.zeros(n)) if carry is None else carry
        r = pe.update(law, eps, epsp, p, prm)
        state = np.zeros((n, 0)) if law == pe.ELASTIC else np.concatenate([r["p"][:, None], r["epsp"]], axis=1)
        return dict(stress=r["stress"], tangent=r["tangent"], state=state, plastic=r["plastic"], carry=(r["epsp"], r["p"]))
    if spec["family"] == "plane_stress_j2":
        epsp, p = (np.zeros((n, 3)), np.zeros(n)) if carry is None else carry
        r = pj.update(law, eps, epsp, p, prm)
        return dict(stress=r["stress"], tangent=r["tangent"], state=np.concatenate([r["p"][:, None], r["epsp"]], axis=1), plastic=r["plastic"],
                    carry=(r["epsp"], r["p"]))
    epn = np.zeros((n, 3)) if carry is None else carry
    r = ps.update(law, eps, epn, prm) if spec["family"] == "plane_stress" else psh.update(eps, epn, prm)
    return dict(stress=r["stress"], tangent=r["tangent"], state=r["state"], plastic=r["plastic"], carry=r["state"])


def parity_bounds(law):
    """(stress / sig0, tangent / E, state / (sig0 / E)): the tolerance the family's own GPU test file uses against this restatement"""
    family = LAWS[law]["family"]
    if family == "plane_strain":
        return (1e-12, 1e-12, 1e-12)            # TIGHT of test_gpu_plane_strain.py, of the field scale
    if family == "plane_stress":
        return ps.gpu_bounds(law)
    if family == "plane_stress_j2":
        return pj.gpu_bounds(law)
    return psh.gpu_bounds(LAWS[law]["prm"][4])
