"""CPU: the Python layer above the C ABI for single-crystal viscoplasticity, over the test double ``fake_dxmat_single_crystal``: the
``dt`` route (``material.dt`` when the call names none), the four state fields through ``integrate`` and the state dictionaries, and
``AcceleratedUpdate`` over the stand-in map with per-point frames (``frame_fused``), whole-mesh and subset (rows) maps, the frames
handed over once, ``update_material_rotation_matrix()``."""
import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial

import single_crystal_ref as sc
from fake_dxmat_single_crystal import FakeDxmatSingleCrystal

NCELL, NQP = 37, 4
N = NCELL * NQP
PRM = sc.param_vector()
NAMES = {"ElasticStrain": "eel", "ViscoplasticSlip": "g", "EquivalentViscoplasticSlip": "p", "BackStrain": "a"}


@pytest.fixture
def fake(monkeypatch):
    lib = FakeDxmatSingleCrystal(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    return lib


def behaviour():
    return jm.MericCailletaudSingleCrystalViscoPlasticity.from_mfront_properties({"YoungModulus1": 208000.0})


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 6)) * np.array([1, 1, 1, 0.7, 0.7, 0.7])
    d[np.arange(n), np.arange(n) % 3] += 1.5
    d /= np.linalg.norm(d, axis=1)[:, None]
    R = np.array([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(n)])
    return d, R


def history(d, R, steps, dt=0.1):
    st = sc.zero_state(len(d))
    for k in range(1, steps + 1):
        out = sc.update(k * 1e-4 * d, st, PRM, dt, R=R)
        assert (out["status"] == 0).all()
        st = sc.next_state(out)
    return out


def test_integrate_uses_material_dt_when_the_call_names_none_and_dt_zero_is_elastic(fake):
    n = 11
    d, R = inputs(n, 3)
    m = JAXMaterial(behaviour())
    m.set_data_manager(n)
    m.set_frame(R)
    pre = history(d, R, 14)
    m.set_initial_state_dict({k: pre[v] for k, v in NAMES.items()})
    eps = 15e-4 * d
    m.dt = 0.1
    S1, isv1, C1 = (np.array(x) for x in m.integrate(eps))
    S2, isv2, C2 = (np.array(x) for x in m.integrate(eps, 0.1))
    assert fake.dt_calls == [0.1, 0.1]
    assert np.array_equal(S1, S2) and np.array_equal(isv1, isv2) and np.array_equal(C1, C2)
    ref = sc.update(eps, sc.next_state(pre), PRM, 0.1, R=R)
    assert ref["plastic"].all() and np.array_equal(S1, ref["stress"]) and np.array_equal(C1.reshape(n, 6, 6), ref["tangent"])
    assert isv1.shape == (n, 42) and np.array_equal(isv1, np.concatenate([ref[k] for k in ("eel", "g", "p", "a")], axis=1))
    # dt = 0: the elastic response, whatever material.dt says
    S0, isv0, C0 = (np.array(x) for x in m.integrate(eps, 0))
    assert fake.dt_calls[-1] == 0.0
    D, Q = sc.stiffness(PRM), sc.mandel_rotation(R)
    assert np.allclose(C0.reshape(n, 6, 6), np.einsum("nri,rs,nsk->nik", Q, D, Q), rtol=0, atol=1e-9)
    assert np.array_equal(isv0[:, 6:18], pre["g"]) and np.array_equal(isv0[:, 18:30], pre["p"])
    assert m.last_stats["n_plastic"] == n and m.last_stats["n_not_converged"] == 0
    with pytest.raises(_lib.DxmError, match="dt must be finite and >= 0"):
        m.integrate(eps, -1.0)


@pytest.mark.parametrize("subset", [False, True])
def test_map_update_advance_and_frames_over_the_double(fake, subset):
    d, R = inputs(N, 9)
    cells = np.sort(np.random.default_rng(5).permutation(NCELL)[: 2 * NCELL // 3]).astype(np.int32) if subset else None
    rows = np.arange(N) if cells is None else (cells[:, None] * NQP + np.arange(NQP)[None]).ravel()
    rest = np.setdiff1d(np.arange(N), rows)
    m = JAXMaterial(behaviour())
    m.rotation_matrix = R
    m.dt = 0.1                                               # the map never passes dt (quadrature_map.py:321)
    q = QuadratureFieldMap(NCELL, NQP, m, cells=cells)
    assert np.array_equal(q.rotation_func.x.array.reshape(N, 9), R.reshape(N, 9))
    scale = [0.0]
    q.register_gradient("Strain", lambda c: (scale[0] * d).reshape(NCELL, NQP, 6)[c].reshape(-1, 6))
    st = sc.zero_state(len(rows))
    for k in range(1, 16):
        scale[0] = k * 1e-4
        q.update()
        out = sc.update(scale[0] * d[rows], st, PRM, 0.1, R=R[rows])
        assert (out["status"] == 0).all()
        if k in (1, 12, 15):
            sig = q.fluxes["Stress"].x.array.reshape(N, 6)
            jac = q.jacobian_flatten.x.array.reshape(N, 36)
            assert np.abs(sig[rows] - out["stress"]).max() <= 1e-13 * np.abs(out["stress"]).max(), k
            assert np.abs(jac[rows] - out["tangent"].reshape(-1, 36)).max() <= 1e-13 * np.abs(out["tangent"]).max(), k
            assert not sig[rest].any() and not jac[rest].any()
        q.advance()
        st = sc.next_state(out)
    assert out["plastic"].any() and set(fake.dt_calls) == {0.1}
    assert [k for k, _ in fake.frame_calls] == ["field"]    # handed over once, not per update
    assert m.kernel_name == "single_crystal_kernel<2" and m.algorithmic_bytes_per_point == 1080
    for name, key in NAMES.items():
        got = np.asarray(q.internal_state_variables[name].x.array).reshape(N, -1)[rows]
        assert np.abs(got - st[key]).max() <= 1e-13 * max(np.abs(st[key]).max(), 1e-30), name
    q.update_material_rotation_matrix(sc.rot_z(np.pi / 3))   # a constant: the uniform form
    assert [k for k, _ in fake.frame_calls] == ["field", "uniform"] and m.kernel_name == "single_crystal_kernel<1"
