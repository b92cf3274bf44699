"""GPU: randomised parity sweep of the Hosford, Ogden and Ramberg-Osgood kernels over the PARAMETER space, what ``test_gpu_fuzz.py``
is for J2 and FeFp: elastic constants over 2.5 decades with nu up to 0.49, yield strains from 1e-4 to 1e-2, hardening from none to
H ~ E, every Hosford exponent of ``law_fuzz.HOSFORD_EXPONENTS`` over four increments with unloading, re-yielding on the other side
and non-proportional steps (the 13-slot state advanced three times); Ogden exponents of either sign with stretches up to 2 under
rotation; Ramberg-Osgood with E, nu and sig0 drawn.  Everything goes through ``JAXMaterial`` -> ctypes -> C ABI, at N = 4099 (64
full tiles and a ragged tail of 3).

References and bounds: the float64 restatements, which ``test_law_fuzz_cpu.py`` pins against their high-precision versions over
these very inputs; ``tests/golden/law_fuzz_bounds.npz`` holds 8 x the largest deviation found there, never less than the bound of the
law's fixed-parameter GPU tests -- which is what all five come to (1e-12 Hosford, 3.2e-12 Ogden, 1e-12 / 1e-11 Ramberg-Osgood)."""
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd.conventions import unpack_sym_tangent
from dolfinx_materials_amd.jaxmat import JAXMaterial

import law_fuzz as lf
import ogden_ref as og
import ramberg_osgood_ref as ro
import test_gpu_hosford as gh
import test_gpu_ramberg_osgood as gro

pytestmark = pytest.mark.gpu
BOUNDS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "law_fuzz_bounds.npz"))
N = lf.N_POINTS
SYM_SEED = 5          # a = 10, H ~ E, nu = 0.47: also run in the "sym" tangent layout


@pytest.mark.parametrize("seed", lf.HOSFORD_SEEDS)
def test_hosford_random_parameters_unloading_and_reyielding(seed):
    prm = lf.draw_hosford(seed)
    E, nu, R0, H, a = prm
    props = dict(E=E, nu=nu, R0=R0, H=H)
    b_state, b_tangent = float(BOUNDS["bound_hosford_state"]), float(BOUNDS["bound_hosford_tangent"])
    hist = lf.hosford_history(seed, N, prm)
    mats = [gh.material(a, N, np.array(hist["ep0"]), np.array(hist["p0"]), props=props)]
    if seed == SYM_SEED:
        mats.append(gh.material(a, N, np.array(hist["ep0"]), np.array(hist["p0"]), props=props, tangent_layout="sym"))
    assert mats[0].kernel_name.startswith("hosford_kernel")
    for inc in range(lf.HOSFORD_INCREMENTS):
        ref, skip, eps = hist["ref"][inc], hist["skip"][inc], np.array(hist["eps"][inc])
        tag = f"seed {seed} (E, nu, R0, H, a) = {prm} increment {inc + 1}"
        assert ref["converged"].all() and skip.mean() <= lf.KINK_CAP, (tag, int(skip.sum()))
        sig, isv, Ct = (np.array(x) for x in mats[0].integrate(eps))
        st = dict(mats[0].last_stats)
        keep = ~skip
        print(f"hosford sweep {tag}: skipped {int(skip.sum())} of {N}, plastic {st['n_plastic']}, iterations {st['max_local_iters']} (reference {int(ref['iters'].max())})")
        gh.compare(tag, sig[keep], isv[keep], Ct.reshape(N, 36)[keep], {q: ref[q][keep] for q in ("sig", "eel", "p", "Ct")},
                   props=props, b_state=b_state, b_tangent=b_tangent)
        assert st["n_not_converged"] == 0 and st["n_nan"] == 0, (tag, st)
        assert st["max_local_iters"] <= int(ref["iters"].max(initial=0)) + 2, (tag, st, int(ref["iters"].max(initial=0)))
        assert abs(st["n_plastic"] - int(ref["plastic"].sum())) <= int(skip.sum()), (tag, st, int(ref["plastic"].sum()))
        for ms in mats[1:]:
            sig_s, isv_s, C21 = (np.array(x) for x in ms.integrate(eps))
            assert C21.reshape(N, -1).shape[1] == 21, tag
            assert np.array_equal(sig_s, sig) and np.array_equal(isv_s, isv) and np.array_equal(unpack_sym_tangent(C21).reshape(N, 36), Ct.reshape(N, 36)), tag
            assert {k: ms.last_stats[k] for k in ("n_plastic", "n_not_converged", "max_local_iters")} == {k: st[k] for k in ("n_plastic", "n_not_converged", "max_local_iters")}, tag
        if inc + 1 < lf.HOSFORD_INCREMENTS:
            for m in mats:
                m.data_manager.update()
    last, keep = hist["ref"][-1], ~hist["skip"][-1]
    fin = mats[0].get_final_state_dict()
    sc = np.maximum(np.abs(last["sig"]).max(axis=1), R0)[keep]
    ee = (E * np.abs(np.array(fin["ElasticStrain"]).reshape(N, 6) - last["eel"]).max(axis=1)[keep] / sc).max()
    ep = (E * np.abs(np.array(fin["EquivalentPlasticStrain"]).reshape(N) - last["p"])[keep] / sc).max()
    print(f"hosford sweep seed {seed}: final state eel {ee:.3e} p {ep:.3e} (bound {b_state:.2e})")
    assert ee <= b_state and ep <= b_state, (prm, ee, ep)
    for m in mats:
        m.close()


@pytest.mark.parametrize("seed", lf.OGDEN_SEEDS)
def test_ogden_random_parameters_large_stretches_with_rotation(seed):
    prm = lf.draw_ogden(seed)
    amp = lf.OGDEN_AMPS[seed % len(lf.OGDEN_AMPS)]
    bound = float(BOUNDS["bound_ogden"])
    F = lf.ogden_F(seed, N, amp)
    tag = f"seed {seed} {prm} stretches up to {amp}"
    series, quotient = lf.ogden_paths(F, prm["alpha"])
    assert series.mean() >= 0.05 and quotient.mean() >= 0.05, (tag, series.mean(), quotient.mean())   # both forms of the divided difference run
    m = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
    m.set_data_manager(N)
    assert m.kernel_name.startswith("ogden_kernel")
    P, isv, A = m.integrate(F)
    st = m.last_stats
    assert st["n_nan"] == 0 and st["n_not_converged"] == 0, (tag, st)
    eP, eA, eI = (float(e.max()) for e in lf.ogden_errors((P, A, isv), og.closed_form(F, **prm)))
    print(f"ogden sweep {tag}: series rows {series.mean():.2f} quotient rows {quotient.mean():.2f}  P {eP:.3e} A {eA:.3e} PK2Stress {eI:.3e} (bound {bound:.1e})")
    assert eP <= bound and eA <= bound and eI <= bound, (tag, eP, eA, eI)
    m.close()


@pytest.mark.parametrize("seed", lf.RO_SEEDS)
def test_ramberg_osgood_random_parameters(seed):
    prm, eps = lf.ramberg_osgood_inputs(seed, N)
    E, nu, sig0, alpha, n_exp = prm
    tag = f"seed {seed} (E, nu, sig0, alpha, n) = {prm}"
    assert float(BOUNDS["bound_ro_stress"]) == 1e-12 and float(BOUNDS["bound_ro_tangent"]) == 1e-11      # what check_against_ref applies
    m = JAXMaterial(jm.RambergOsgoodNonLinearElasticity(jm.LinearElasticIsotropic(E=E, nu=nu), sig0=sig0, alpha=alpha, n=n_exp))
    m.set_data_manager(N)
    assert m.kernel_name.startswith("small_strain_kernel<3")
    sig, isv, ct = m.integrate(eps)
    st = m.last_stats
    r = ro.update(eps, *prm)
    es, ec = (float(e.max()) for e in lf.ramberg_osgood_errors(np.array(sig), ct, r["sig"], r["Ct_mfront"]))
    print(f"ramberg-osgood sweep {tag}: stress {es:.3e} (bound 1e-12) tangent {ec:.3e} (bound 1e-11) iterations {st['max_local_iters']} (reference {int(r['iters'].max())})")
    r = gro.check_against_ref(np.array(sig), ct, eps, prm, st, tag=tag)
    assert r["converged"].all(), tag
    assert st["n_not_converged"] == 0 and st["max_local_iters"] <= 12, (tag, st)
    assert st["max_local_iters"] <= r["iters"].max() + 2, (tag, st, int(r["iters"].max()))
    m.close()
