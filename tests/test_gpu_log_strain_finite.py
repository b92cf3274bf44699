"""GPU: logarithmic-strain J2 plasticity (``log_strain_kernel``) at finite stretches, over ten parameter sets and six-increment
histories (``log_strain_cases``): against the eigen-free 100-digit values of ``golden/log_strain_finite.npz`` directly, against the
numpy restatement ``log_strain_ref.update`` on batches of 4099 points whose stretches reach 3 and on histories carried on the
device, against itself under the two rotations that bypass both references (the cyclic permutations on the right hand the same
physical point to a different one of the kernel's three quotients), and a re-parameterised handle against fresh ones.

Every bound is ``BOUNDS`` of ``test_log_strain_finite_cpu.py``: 16 x the measured floor of the restatement against mpmath in the
stratum (``amp``, or the special rows), scaled as ``log_strain_ref.scaled_errors`` with the draw's own s0 and E.  The rules the inputs
obey (plastic share, kink cap, every branch of every divided difference taken) are asserted there, by the references alone.
Measured on an MI355X: see DESIGN.md, section "Logarithmic-strain J2 plasticity"."""
import ctypes as C
import functools

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp

import log_strain_cases as lc
import log_strain_ref as ls
from test_log_strain_finite_cpu import BOUNDS, HISTORY_STRATUM, batch_of, stratum_of

pytestmark = pytest.mark.gpu

FIELD_DIMS = (6, 1, 6)      # ElasticStrain, EquivalentPlasticStrain, the hidden PlasticStrain
KEYS = ("P", "A", "eel", "p", "Ep")
TI, TJ = ls.TI, ls.TJ


def material(N, prm):
    m = JAXMaterial(jm.LogarithmicStrainPlasticity(prm["s0"], prm["H0"], E=prm["E"], nu=prm["nu"]), lazy_isv=False)
    m.set_data_manager(N)
    assert m.kernel_name.startswith("log_strain_kernel")
    return m


def state_of(m, which=_lib.S1):
    out = []
    for f, dim in enumerate(FIELD_DIMS):
        a = np.empty((m._n, dim))
        m._chk(m._lib.dxm_get_state(m._require(), which, f, a.ctypes.data))
        out.append(a)
    return out


def results(m, P, A):
    eel, p, Ep = state_of(m)
    return dict(P=np.array(P), A=np.array(A).reshape(-1, 9, 9), eel=eel, p=p[:, 0].copy(), Ep=Ep)


def run(m, F, Ep_n, p_n):
    """One update of all points from the old state (Ep_n, p_n), set as ``test_degenerate_set_matches_mpmath_directly`` sets it."""
    n = len(F)
    m._set_state(1, np.ascontiguousarray(np.asarray(p_n).reshape(n, 1)))
    m._set_state(2, np.ascontiguousarray(Ep_n))
    P, isv, A = m.integrate(np.ascontiguousarray(F))
    st = m.last_stats
    assert st["n_points"] == n and st["n_nan"] == 0 and st["n_not_converged"] == 0, st
    got = results(m, P, A)
    assert np.array_equal(np.asarray(isv)[:, :6], got["eel"]) and np.array_equal(np.asarray(isv)[:, 6], got["p"])
    assert all(np.isfinite(got[q]).all() for q in KEYS)
    return got


def held(tag, got, want, prm, strata, keep=None):
    """Assert ``got`` within each stratum's bound of ``want``; ``strata``: {name: row mask}."""
    keep = np.ones(len(want["P"]), dtype=bool) if keep is None else keep
    bad = {}
    for name, mask in strata.items():
        if not (mask & keep).any():
            continue
        e = ls.scaled_errors(got, want, s0=prm["s0"], E=prm["E"], keep=mask & keep)
        print(f"log-strain finite {tag}, {name}: " + " ".join(f"{q} {v:.3e}" for q, v in e.items()) + f" (bound {BOUNDS[name]:.1e})")
        if not max(e.values()) <= BOUNDS[name]:
            bad[name] = e
    assert not bad, (tag, bad)


@functools.lru_cache(maxsize=None)
def fixture():
    return lc.load_fixture()


@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_fixture_matches_mpmath_directly(k):
    fx = fixture()
    rows = fx["draw"] == k
    prm = lc.draw(k)
    m = material(int(rows.sum()), prm)
    got = run(m, fx["F"][rows], fx["Ep_n"][rows], fx["p_n"][rows])
    assert m.last_stats["n_plastic"] == int(fx["plastic"][rows].sum())
    want = {q: fx[q][rows] for q in KEYS}
    held(f"vs mpmath, draw {k}", got, want, prm, {name: mask[rows] for name, mask in lc.strata(fx).items()})
    m.close()


@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_batch_matches_the_reference(k):
    amp, (F, Ep, p) = batch_of(k)
    prm = lc.draw(k)
    ref = ls.update(F, Ep, p, **prm)
    m = material(lc.N_BATCH, prm)
    got = run(m, F, Ep, p)
    assert abs(m.last_stats["n_plastic"] - int(ref["plastic"].sum())) <= int(ref["skip"].sum())
    held(f"batch, draw {k}", got, ref, prm, {stratum_of(amp): np.ones(lc.N_BATCH, dtype=bool)}, keep=~ref["skip"])
    m.close()


@functools.lru_cache(maxsize=None)
def mixed():
    F, Ep, p, special = lc.mixed_prm_batch()
    strata = {stratum_of(amp): ~special & (np.arange(lc.N_BATCH) % len(lc.AMPS) == q) for q, amp in enumerate(lc.AMPS)}
    strata["special"] = special
    return F, Ep, p, strata


def test_mixed_batch_with_the_special_rows_at_the_tile_boundaries():
    F, Ep, p, strata = mixed()
    ref = ls.update(F, Ep, p)
    assert strata["special"][[0, 63, 64, lc.N_BATCH - 3, lc.N_BATCH - 1]].all()
    m = material(lc.N_BATCH, ls.PRM)
    got = run(m, F, Ep, p)
    assert abs(m.last_stats["n_plastic"] - int(ref["plastic"].sum())) <= int(ref["skip"].sum())
    held("mixed batch", got, ref, ls.PRM, strata, keep=~ref["skip"])
    m.close()


@pytest.mark.parametrize("k", lc.HISTORY_DRAWS)
def test_history_carried_on_the_device(k):
    h = lc.history(k)
    prm = lc.draw(k)
    n = lc.N_HISTORY
    m = material(n, prm)
    everything = {HISTORY_STRATUM: np.ones(n, dtype=bool)}
    for inc, (F, ref, out) in enumerate(zip(h["F"], h["ref"], h["out"])):
        if inc:
            m.data_manager.update()
        P, isv, A = m.integrate(F)
        st = m.last_stats
        assert st["n_points"] == n and st["n_nan"] == 0
        assert abs(st["n_plastic"] - int(ref["plastic"].sum())) <= int(out.sum())
        held(f"history draw {k} increment {inc + 1}", results(m, P, A), ref, prm, everything, keep=~out)
    m.close()


# ---- symmetries that bypass both references ------------------------------------------------------------------------------------
def _tangent4(A):
    A4 = np.empty((len(A), 3, 3, 3, 3))
    A4[:, TI[:, None], TJ[:, None], TI[None, :], TJ[None, :]] = A
    return A4


def _tangent9(A4):
    return np.ascontiguousarray(A4[:, TI, TJ][:, :, TI, TJ])


def _mandel_rotated(X6, Q0):
    """Q0^T X Q0 of Mandel vectors."""
    return onp.tensor_to_mandel(np.einsum("ai,nab,bj->nij", Q0, onp.mandel_to_tensor(X6), Q0))


@pytest.fixture(scope="module")
def plain():
    F, Ep, p, strata = mixed()
    m = material(lc.N_BATCH, ls.PRM)
    got = run(m, F, Ep, p)
    m.close()
    return got


def test_rotation_on_the_left(plain):
    """F -> Q0 F: C is the same matrix up to rounding, so P -> Q0 P, the tangent turns on its first index pair and the state stays."""
    F, Ep, p, strata = mixed()
    Q0 = ls._rotation([0.3, -1.0, 0.5], 1.1)
    m = material(lc.N_BATCH, ls.PRM)
    got = run(m, ls.to_vector(Q0 @ ls.to_matrix(F)), Ep, p)
    m.close()
    want = dict(plain, P=ls.to_vector(Q0 @ ls.to_matrix(plain["P"])), A=_tangent9(np.einsum("ia,kc,naJcL->niJkL", Q0, Q0, _tangent4(plain["A"]))))
    held("rotation on the left", got, want, ls.PRM, strata)


@pytest.mark.parametrize("q", (1, 2))
def test_cyclic_permutation_on_the_right(plain, q):
    """F -> F Q0 with Ep_n -> Q0^T Ep_n Q0: the same physical point in axes renamed cyclically.  C' = Q0^T C Q0 holds the same
    numbers in other places, Jacobi delivers its eigenvalues in another order, and the (0, 1, 2) call is handed another of f0 / f1
    / f2.  The renaming itself is exact (a permutation of entries), so this pits the kernel's selections against each other."""
    F, Ep, p, strata = mixed()
    Q0 = lc.CYCLIC[q]
    F2, Ep2 = ls.to_vector(ls.to_matrix(F) @ Q0), _mandel_rotated(Ep, Q0)
    moved = lc.classify(F2)["f"] != lc.classify(F)["f"]
    assert moved.mean() > 0.3
    m = material(lc.N_BATCH, ls.PRM)
    got = run(m, F2, Ep2, p)
    m.close()
    want = dict(P=ls.to_vector(ls.to_matrix(plain["P"]) @ Q0), A=_tangent9(np.einsum("niMkN,MJ,NL->niJkL", _tangent4(plain["A"]), Q0, Q0)),
                eel=_mandel_rotated(plain["eel"], Q0), Ep=_mandel_rotated(plain["Ep"], Q0), p=plain["p"])
    held(f"cyclic permutation {q} on the right", got, want, ls.PRM, strata)
    held(f"cyclic permutation {q} on the right, points handed another quotient", got, want, ls.PRM, strata, keep=moved)


# ---- parameters travel --------------------------------------------------------------------------------------------------------
def test_one_handle_reparameterised_answers_like_fresh_handles():
    n = 1000
    m = material(n, ls.PRM)
    for k in (5, 3, 1):
        prm = lc.draw(k)
        F, Ep, p = lc.stretch_case(k, n, 2.0, seed=3)
        m._chk(m._lib.dxm_set_params(m._require(), (C.c_double * 4)(prm["E"], prm["nu"], prm["s0"], prm["H0"]), 4))
        got = run(m, F, Ep, p)
        fresh = material(n, prm)
        want = run(fresh, F, Ep, p)
        assert fresh.last_stats["n_plastic"] == m.last_stats["n_plastic"] > 0
        fresh.close()
        for key in KEYS:
            assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), (k, key)
    m.close()
