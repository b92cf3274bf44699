"""GPU: randomised parity sweep of the two plane-strain kernels that are not their 3-D law with fewer columns, over the PARAMETER space --
what ``test_gpu_fuzz_laws.py`` is for laws 10 and 7.  Plane-strain Hosford (law 40, ``hosford_plane_kernel``: one closed-form
rotation, one divided difference of three, the point's record parked in LDS across the local Newton): the ten draws of
``law_fuzz.draw_hosford`` -- every exponent of ``law_fuzz.HOSFORD_EXPONENTS``, nu from 0 to 0.49, yield strains from 1e-4 to 1e-2,
hardening from none to H ~ E -- over four increments with unloading, re-yielding on the other side and non-proportional plane steps,
the nine-slot state advanced three times.  Plane-strain Ogden (law 38, ``ogden_plane_kernel``): the eight draws of
``law_fuzz.draw_ogden`` -- alpha of either sign, K / mu over 2.4 decades -- at stretches up to 2 under in-plane rotation.  Everything
goes through ``JAXMaterial`` with ``hypothesis="plane_strain"`` -> ctypes -> C ABI, at N = 4099 (64 full tiles and a ragged tail of 3).

References and bounds: the laws' definitions (law 10 / law 7 restated in numpy on the embedding, restricted), which
``test_plane_law_fuzz_cpu.py`` pins against their high-precision versions over these very inputs, together with the branches of the two
kernels the inputs reach; ``tests/golden/plane_law_fuzz_bounds.npz`` holds 8 x the largest deviation found there, never less than the
bound of the law's fixed-parameter GPU tests -- which is what all three come to (1e-12 Hosford state and tangent, 3.2e-12 Ogden).
Every test prints its figures before it asserts."""
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import conventions as cv
from dolfinx_materials_amd.jaxmat import JAXMaterial

import ogden_plane_ref as op
import plane_law_fuzz as pf
import test_gpu_hosford_plane as ghp
import test_gpu_ogden_plane as gop

pytestmark = pytest.mark.gpu
BOUNDS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_law_fuzz_bounds.npz"))
N = pf.N_POINTS
LAW_10_SEED = 5                  # a = 10, H ~ E, nu = 0.47: also run through law 10 on the embedded strains and state
LAW_7_SEEDS = (4, 5)             # alpha = 15.4 and alpha = -23.5: also run through law 7 on the embedded F


@pytest.mark.parametrize("seed", pf.HOSFORD_SEEDS)
def test_plane_hosford_random_parameters_unloading_and_reyielding(seed):
    prm = pf.draw_hosford(seed)
    E, nu, R0, H, a = prm
    props = dict(E=E, nu=nu, R0=R0, H=H)
    b_state, b_tangent = float(BOUNDS["bound_hosford_state"]), float(BOUNDS["bound_hosford_tangent"])
    hist = pf.plane_hosford_history(seed, N, prm)
    m = ghp.material(a, N, np.array(hist["ep0"]), np.array(hist["p0"]), props=props)
    assert m.kernel_name == "hosford_plane_kernel"
    w = None
    if seed == LAW_10_SEED:
        assert a == 10.0 and H > 0.25 * E
        w = ghp.material(a, N, cv.embed_plane_strain(hist["ep0"]), np.array(hist["p0"]), props=props, hypothesis="3d")
        assert w.kernel_name.startswith("hosford_kernel")
    for inc in range(pf.HOSFORD_INCREMENTS):
        ref, skip, eps = hist["ref"][inc], hist["skip"][inc], np.array(hist["eps"][inc])
        tag = f"seed {seed} (E, nu, R0, H, a) = {prm} increment {inc + 1}"
        assert ref["converged"].all() and skip.mean() <= pf.KINK_CAP, (tag, int(skip.sum()))
        sig, isv, Ct = (np.array(x) for x in m.integrate(eps))
        st = dict(m.last_stats)
        keep = ~skip
        print(f"plane hosford sweep {tag}: skipped {int(skip.sum())} of {N}, plastic {st['n_plastic']} (reference {int(ref['plastic'].sum())}), "
              f"iterations {st['max_local_iters']} (reference {int(ref['iters'].max())})")
        ghp.compare(tag, sig[keep], isv[keep], Ct.reshape(N, 16)[keep], {q: ref[q][keep] for q in ("sig", "eel", "p", "Ct")},
                    props=props, b_state=b_state, b_tangent=b_tangent)
        assert st["n_not_converged"] == 0 and st["n_nan"] == 0, (tag, st)
        assert st["max_local_iters"] <= int(ref["iters"].max(initial=0)) + 2, (tag, st, int(ref["iters"].max(initial=0)))
        assert abs(st["n_plastic"] - int(ref["plastic"].sum())) <= int(skip.sum()), (tag, st, int(ref["plastic"].sum()))
        T = Ct.reshape(N, 4, 4)
        assert np.array_equal(ghp.bits(T), ghp.bits(T.transpose(0, 2, 1))), tag                       # exactly symmetric
        if w is not None:
            s6, i7, C6 = (np.array(x) for x in w.integrate(cv.embed_plane_strain(eps)))
            C6 = C6.reshape(N, 6, 6)
            sw = dict(w.last_stats)
            want = dict(sig=cv.restrict_plane_strain(s6), eel=cv.restrict_plane_strain(i7[:, :6]), p=i7[:, 6], Ct=cv.restrict_plane_strain_tangent(C6))
            ghp.compare(f"{tag} vs law 10 restricted", sig[keep], isv[keep], Ct.reshape(N, 16)[keep], {q: v[keep] for q, v in want.items()},
                        props=props, b_state=2 * b_state, b_tangent=2 * b_tangent)                    # each is within the bounds of the same reference
            assert abs(st["n_plastic"] - sw["n_plastic"]) <= int(skip.sum()) and sw["n_not_converged"] == 0, (tag, st, sw)
        if inc + 1 < pf.HOSFORD_INCREMENTS:
            m.data_manager.update()
            if w is not None:
                w.data_manager.update()
    last, keep = hist["ref"][-1], ~hist["skip"][-1]
    fin = m.get_final_state_dict()
    sc = np.maximum(np.abs(last["sig"]).max(axis=1), R0)[keep]
    ee = (E * np.abs(np.array(fin["ElasticStrain"]).reshape(N, 4) - last["eel"]).max(axis=1)[keep] / sc).max()
    ep = (E * np.abs(np.array(fin["EquivalentPlasticStrain"]).reshape(N) - last["p"])[keep] / sc).max()
    print(f"plane hosford sweep seed {seed}: final state eel {ee:.3e} p {ep:.3e} (bound {b_state:.2e})")
    assert ee <= b_state and ep <= b_state, (prm, ee, ep)
    m.close()
    if w is not None:
        w.close()


@pytest.mark.parametrize("seed", pf.OGDEN_SEEDS)
def test_plane_ogden_random_parameters_large_stretches_with_rotation(seed):
    prm = pf.draw_ogden(seed)
    amp = pf.plane_ogden_amp(seed)
    bound = float(BOUNDS["bound_ogden"])
    F = np.array(pf.plane_ogden_F(seed, N, amp))
    tag = f"sweep seed {seed} K/mu={prm['K'] / prm['mu']:.0f} stretches up to {amp}"
    series, quotient = pf.plane_ogden_paths(F, prm["alpha"])
    print(f"plane ogden {tag}: series rows {series.mean():.2f} quotient rows {quotient.mean():.2f}")
    assert series.mean() >= 0.05 and quotient.mean() >= 0.05, (tag, series.mean(), quotient.mean())   # both forms of the divided difference run
    m = gop.material(N, **prm)
    assert m.kernel_name == "ogden_plane_kernel"
    P, isv, A = (np.array(x) for x in m.integrate(F))
    st = m.last_stats
    assert st["n_nan"] == 0 and st["n_plastic"] == 0 and st["n_not_converged"] == 0, (tag, st)
    gop.check(tag, P, A, isv, F, prm, bound=bound)
    if seed in LAW_7_SEEDS:
        assert (prm["alpha"] > 0.0) == (seed == LAW_7_SEEDS[0])
        w = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
        w.set_data_manager(N)
        assert w.kernel_name.startswith("ogden_kernel")
        P9, isv6, A9 = (np.array(x) for x in w.integrate(cv.embed_plane_F(F)))
        want = (cv.restrict_plane_F(P9), cv.restrict_plane_F_tangent(A9.reshape(N, 9, 9)), cv.restrict_plane_strain(isv6))
        e = op.errors((P, A.reshape(N, 5, 5), isv), want)
        print(f"plane ogden {tag} vs law 7 restricted alpha={prm['alpha']}: P {e[0]:.3e} A {e[1]:.3e} PK2Stress {e[2]:.3e} (bound {2 * bound:.1e})")
        assert max(e) <= 2 * bound, (tag, e)                                                          # each is within the bound of the same reference
        w.close()
    m.close()
