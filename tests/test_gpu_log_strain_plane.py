"""GPU: plane-strain logarithmic-strain J2 plasticity (DXM_LAW_LOG_STRAIN_PE = 42, ``log_strain_plane_kernel``) through ``HIPMaterial``
(ctypes -> C ABI) against the law's definition ``log_strain_plane_ref.restricted`` -- law 19's numpy restatement on the embedded F and
state, restricted: the formulation the kernel does NOT use (LAPACK's 3x3 eigen-solver, every divided difference, the 9 x 9 block) -- on
the families ``test_log_strain_plane_cpu.py`` pins; against the 100-digit fixture directly; against law 19 of the same process; the
special rows at the tile boundaries; histories carried on the device; a diagonal known answer that bypasses the restatement; the tile
loop past its first pass; the routes of the library against each other bit for bit; every refusal on a live handle.

Every bound is ``BOUNDS`` of ``test_log_strain_plane_cpu.py``: 16 x the measured floor of the restatement against mpmath in the stratum
(``amp``, or the special rows), scaled as ``log_strain_ref.scaled_errors`` with the draw's own s0 and E.  Every test prints its figures
before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions as cv
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp

import log_strain_cases as lc
import log_strain_plane_ref as lp
import log_strain_ref as ls
import tile_loop_cases as tlc
from helpers import to_device, to_host
from test_log_strain_plane_cpu import BOUNDS, HISTORY_STRATUM

pytestmark = pytest.mark.gpu

FIELD_DIMS = (4, 1, 4)      # ElasticStrain, EquivalentPlasticStrain, the hidden PlasticStrain
KEYS = lp.KEYS
NLOOP = 206_147             # blocks_per_cu = 1: three full passes of the tile loop on 256 CUs and a ragged fourth (tile_loop_cases.size_for)
NCHUNK = 264_600            # the host path takes two chunks: full-layout laws cross in chunks of 131 072 points


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def behaviour(prm):
    return jm.LogarithmicStrainPlasticity(prm["s0"], prm["H0"], E=prm["E"], nu=prm["nu"], hypothesis="plane_strain")


def material(N, prm=ls.PRM, **kw):
    m = JAXMaterial(behaviour(prm), lazy_isv=False, **kw)
    m.set_data_manager(N)
    assert m.kernel_name == "log_strain_plane_kernel"
    return m


def law19(N, prm=ls.PRM):
    m = JAXMaterial(jm.LogarithmicStrainPlasticity(prm["s0"], prm["H0"], E=prm["E"], nu=prm["nu"]), lazy_isv=False)
    m.set_data_manager(N)
    return m


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def state_of(m, which=_lib.S1, dims=FIELD_DIMS):
    out = []
    for f, dim in enumerate(dims):
        a = np.empty((m._n, dim))
        m._chk(m._lib.dxm_get_state(m._require(), which, f, a.ctypes.data))
        out.append(a)
    return out


def results(m, P, A):
    eel, p, Ep = state_of(m)
    return dict(P=np.array(P), A=np.array(A).reshape(-1, 5, 5), eel=eel, p=p[:, 0].copy(), Ep=Ep)


def set_old_state(m, Ep_n, p_n):
    n = m._n
    m._set_state(1, np.ascontiguousarray(np.asarray(p_n, dtype=np.float64).reshape(n, 1)))
    m._set_state(2, np.ascontiguousarray(Ep_n))


def run(m, F, Ep_n, p_n):
    """One update of all points from the old state (Ep_n, p_n)."""
    n = len(F)
    set_old_state(m, Ep_n, p_n)
    P, isv, A = m.integrate(np.ascontiguousarray(F))
    st = m.last_stats
    assert st["n_points"] == n and st["n_nan"] == 0 and st["n_not_converged"] == 0 and st["max_local_iters"] == 0, st
    got = results(m, P, A)
    assert np.array_equal(np.asarray(isv)[:, :4], got["eel"]) and np.array_equal(np.asarray(isv)[:, 4], got["p"])
    assert all(np.isfinite(got[q]).all() for q in KEYS)
    return got


def held(tag, got, want, prm, strata, keep=None, factor=1.0):
    """Assert ``got`` within ``factor`` x each stratum's bound of ``want``; ``strata``: {name: row mask}."""
    keep = np.ones(len(want["P"]), dtype=bool) if keep is None else keep
    bad = {}
    for name, mask in strata.items():
        if not (mask & keep).any():
            continue
        e = ls.scaled_errors(got, want, s0=prm["s0"], E=prm["E"], keep=mask & keep)
        print(f"plane log-strain {tag}, {name}: " + " ".join(f"{q} {v:.3e}" for q, v in e.items()) + f" (bound {factor * BOUNDS[name]:.1e})")
        if not max(e.values()) <= factor * BOUNDS[name]:
            bad[name] = e
    assert not bad, (tag, bad)


@functools.lru_cache(maxsize=None)
def batch(k):
    """(amp, F, Ep, p, the reference) of draw k's batch: computed once, shared, left unchanged."""
    amp, (F, Ep, p) = lp.batch_of(k)
    ref = lp.restricted(F, Ep, p, **lc.draw(k))
    assert ref["dropped"] == 0.0 and not ref["skip"].any()
    for a in (F, Ep, p, *[ref[q] for q in KEYS], ref["plastic"]):
        a.setflags(write=False)
    return amp, F, Ep, p, ref


@functools.lru_cache(maxsize=None)
def mixed():
    F, Ep, p, special = lp.mixed_batch()
    strata = {lp.stratum_of(amp): ~special & (np.arange(lp.N_BATCH) % len(lc.AMPS) == q) for q, amp in enumerate(lc.AMPS)}
    strata["special"] = special
    ref = lp.restricted(F, Ep, p)
    assert ref["dropped"] == 0.0 and not ref["skip"].any()
    return F, Ep, p, strata, ref


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, lp.N_BATCH])
@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_update_matches_the_restricted_reference(N, k):
    amp, F, Ep, p, ref = batch(k)
    prm = lc.draw(k)
    m = material(N, prm)
    assert m.gradients == {"DeformationGradient": 5} and m.fluxes == {"FirstPiolaKirchhoffStress": 5}
    assert m.internal_state_variables == {"ElasticStrain": 4, "EquivalentPlasticStrain": 1}
    assert m.tangent_blocks == {("FirstPiolaKirchhoffStress", "DeformationGradient"): (5, 5)}
    assert m.tangent_size == 25 and m.algorithmic_bytes_per_point == 392
    got = run(m, F[:N], Ep[:N], p[:N])
    assert got["P"].shape == (N, 5) and got["A"].shape == (N, 5, 5)
    want = {q: ref[q][:N] for q in KEYS}
    print(f"draw {k} N={N}: n_plastic {m.last_stats['n_plastic']} (reference {int(ref['plastic'][:N].sum())})")
    assert m.last_stats["n_plastic"] == int(ref["plastic"][:N].sum())
    held(f"parity, draw {k} N={N}", got, want, prm, {lp.stratum_of(amp): np.ones(N, dtype=bool)})
    m.close()


@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_fixture_matches_mpmath_directly(k):
    fx = lp.load_fixture()
    rows = fx["draw"] == k
    prm = lc.draw(k)
    m = material(int(rows.sum()), prm)
    got = run(m, fx["F"][rows], fx["Ep_n"][rows], fx["p_n"][rows])
    assert m.last_stats["n_plastic"] == int(fx["plastic"][rows].sum())
    held(f"vs mpmath, draw {k}", got, {q: fx[q][rows] for q in KEYS}, prm, {name: mask[rows] for name, mask in lp.strata(fx).items()})
    m.close()


def test_identity_from_the_natural_state_is_stress_free_with_the_elastic_block():
    N = 130
    m = material(N)
    F = np.tile([1.0, 1.0, 1.0, 0.0, 0.0], (N, 1))
    P, isv, A = m.integrate(F)
    got = results(m, P, A)
    st = m.last_stats
    assert st["n_plastic"] == 0 and st["n_nan"] == 0 and st["n_not_converged"] == 0 and st["max_local_iters"] == 0
    assert not got["P"].any() and not got["eel"].any() and not got["p"].any() and not got["Ep"].any()          # exactly zero
    # at F = I the tangent is Hooke's on the symmetric part: A[(i,J),(k,L)] = lam d_iJ d_kL + mu (d_ik d_JL + d_iL d_Jk)
    lam, mu = onp.lame(ls.PRM["E"], ls.PRM["nu"])
    RI, RJ = (0, 1, 2, 0, 1), (0, 1, 2, 1, 0)
    want = np.array([[lam * (RI[r] == RJ[r]) * (RI[c] == RJ[c]) + mu * ((RI[r] == RI[c]) * (RJ[r] == RJ[c]) + (RI[r] == RJ[c]) * (RJ[r] == RI[c]))
                      for c in range(5)] for r in range(5)])
    e = np.abs(got["A"] - want[None]).max() / np.abs(want).max()
    print(f"F = I: tangent against the elastic plane block {e:.3e} (bound {BOUNDS['special']:.1e})")
    assert e <= BOUNDS["special"] and (got["A"] == got["A"][0]).all()
    m.close()


@pytest.mark.parametrize("k", range(lc.N_DRAWS))
def test_law_19_of_the_same_process_on_the_embedded_gradient_and_state(k):
    amp, F, Ep, p, ref = batch(k)
    prm = lc.draw(k)
    N = lp.N_BATCH
    m = material(N, prm)
    got = run(m, F, Ep, p)
    w = law19(N, prm)
    w._set_state(1, np.ascontiguousarray(p.reshape(N, 1)))
    w._set_state(2, cv.embed_plane_strain(Ep))
    P9, isv7, A9 = (np.array(x) for x in w.integrate(cv.embed_plane_F(F)))
    eel6, p19, Ep6 = state_of(w, dims=(6, 1, 6))
    A9 = A9.reshape(N, 9, 9)
    print(f"law 19 on the embedding, draw {k}: largest dropped entry of P {np.abs(P9[:, 5:]).max():.1e}, cross blocks "
          f"{max(np.abs(A9[:, :5, 5:]).max(), np.abs(A9[:, 5:, :5]).max()):.1e}, strains {max(np.abs(eel6[:, 4:]).max(), np.abs(Ep6[:, 4:]).max()):.1e}")
    want = dict(P=cv.restrict_plane_F(P9), A=cv.restrict_plane_F_tangent(A9), eel=cv.restrict_plane_strain(eel6), p=p19[:, 0],
                Ep=cv.restrict_plane_strain(Ep6))
    assert w.last_stats["n_plastic"] == m.last_stats["n_plastic"] == int(ref["plastic"].sum())
    held(f"vs law 19 restricted, draw {k}", got, want, prm, {lp.stratum_of(amp): np.ones(N, dtype=bool)}, factor=2.0)   # each within the bound of one reference
    m.close()
    w.close()


# ---- special rows ---------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_with_the_special_rows_at_the_tile_boundaries():
    F, Ep, p, strata, ref = mixed()
    assert strata["special"][[0, 63, 64, lp.N_BATCH - 3, lp.N_BATCH - 1]].all()
    m = material(lp.N_BATCH)
    got = run(m, F, Ep, p)
    assert m.last_stats["n_plastic"] == int(ref["plastic"].sum())
    held("mixed batch", got, {q: ref[q] for q in KEYS}, ls.PRM, strata)
    # c2 equal to c0 or to c1 changes nothing: the same row with another F22 keeps its in-plane rotation and divided differences, so
    # the 2 x 2 in-plane stress differs by the pressure term alone; here the rows are held to the reference like every other
    Fs, labels = lp.special_F5()
    for lab in ("c2 equals c0", "c2 equals c1", "c2 equals c1 rotated swapped"):
        k = labels.index(lab)
        e = ls.scaled_errors({q: got[q][k:k + 1] for q in KEYS}, {q: ref[q][k:k + 1] for q in KEYS}, s0=ls.PRM["s0"], E=ls.PRM["E"])
        print(f"{lab}: " + " ".join(f"{q} {v:.3e}" for q, v in e.items()))
        assert max(e.values()) <= BOUNDS["special"]
    m.close()


def test_a_diagonal_gradient_passes_through_the_rotation_exactly():
    """c01 == 0: the rotation is the no-op, so from the natural state P01 = P10 = 0 and the xy strains are zero exactly, and the
    shear rows and columns of the tangent couple to nothing."""
    N = 200
    rng = np.random.default_rng(3)
    lam = np.exp(rng.uniform(-0.3, 0.3, (N, 3)))
    F = np.concatenate([lam, np.zeros((N, 2))], axis=1)
    m = material(N)
    P, isv, A = m.integrate(F)
    got = results(m, P, A)
    assert m.last_stats["n_nan"] == 0
    assert not got["P"][:, 3:].any() and not got["eel"][:, 3].any() and not got["Ep"][:, 3].any()
    assert not got["A"][:, :3, 3:].any() and not got["A"][:, 3:, :3].any()
    ref = lp.restricted(F, *lp.natural_state(N))
    held("diagonal F", got, {q: ref[q] for q in KEYS}, ls.PRM, {"amp 1.3": np.ones(N, dtype=bool)}, keep=~ref["skip"])
    m.close()


def test_invalid_points_are_counted_and_leave_their_neighbours_alone():
    N = 200
    amp, F0, Ep0, p0, _ = batch(0)
    F, Ep, p = F0[:N].copy(), Ep0[:N], p0[:N]
    bad = F.copy()
    bad[[3, 64, 129], 2] *= -1.0           # F22 < 0
    bad[63, 2] = 0.0                       # F22 = 0
    bad[70] = [0.1, 0.1, 1.0, 2.0, 2.0]    # in-plane determinant < 0
    bad[191] = [0.0, 0.0, 1.0, 0.0, 0.0]   # a zero in-plane block: J = 0
    bad[N - 1, [0, 3]] *= -1.0             # the last point: the first row of F reversed, an inverted in-plane block
    where = np.array([3, 63, 64, 70, 129, 191, N - 1])
    assert (bad[where, 2] * (bad[where, 0] * bad[where, 1] - bad[where, 3] * bad[where, 4]) <= 0.0).all()
    m = material(N)
    set_old_state(m, Ep, p)
    P, isv, A = m.integrate(F)
    base = [np.array(P), np.array(A).reshape(N, 25)] + state_of(m)
    assert m.last_stats["n_nan"] == 0
    n_plastic = m.last_stats["n_plastic"]
    P, isv, A = m.integrate(bad)
    got = [np.array(P), np.array(A).reshape(N, 25)] + state_of(m)
    assert m.last_stats["n_nan"] == len(where)
    ok = np.setdiff1d(np.arange(N), where)
    ref = lp.restricted(F, Ep, p)
    assert m.last_stats["n_plastic"] == n_plastic - int(ref["plastic"][where].sum())
    for a, b in zip(got, base):
        assert np.isnan(a[where]).all()                                       # every output of the point
        assert np.array_equal(bits(a[ok]), bits(b[ok]))
    nonfinite = F.copy()
    nonfinite[17, 0] = np.inf
    nonfinite[64, 2] = -np.inf
    nonfinite[130, 4] = np.nan
    P, isv, A = m.integrate(nonfinite)
    assert m.last_stats["n_nan"] == 3
    got = [np.array(P), np.array(A).reshape(N, 25)] + state_of(m)
    ok = np.setdiff1d(np.arange(N), [17, 64, 130])
    for a, b in zip(got, base):
        assert np.isnan(a[[17, 64, 130]]).all() and np.array_equal(bits(a[ok]), bits(b[ok]))
    m.close()


# ---- histories --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", lc.HISTORY_DRAWS)
def test_history_carried_on_the_device_with_a_revert_in_the_middle(k):
    h = lp.history(k)
    prm = lc.draw(k)
    n = lp.N_HISTORY
    m = material(n, prm)
    everything = {HISTORY_STRATUM: np.ones(n, dtype=bool)}
    for inc, (F, ref, out) in enumerate(zip(h["F"], h["ref"], h["out"])):
        if inc:
            m.data_manager.update()
        if inc == 3:
            # an increment that is thrown away: the state at the beginning of the increment is what it was
            before = state_of(m, _lib.S0)
            m.integrate(h["F"][5])
            m.data_manager.revert()
            for a, b, c in zip(state_of(m, _lib.S0), state_of(m, _lib.S1), before):
                assert np.array_equal(bits(a), bits(c)) and np.array_equal(bits(b), bits(c))
        P, isv, A = m.integrate(F)
        st = m.last_stats
        assert st["n_points"] == n and st["n_nan"] == 0 and st["n_not_converged"] == 0
        assert abs(st["n_plastic"] - int(ref["plastic"].sum())) <= int(out.sum())
        held(f"history draw {k} increment {inc + 1}", results(m, P, A), {q: ref[q] for q in KEYS}, prm, everything, keep=~out)
    m.close()


def test_diagonal_load_and_unload_against_the_small_strain_radial_return():
    """A known answer that bypasses the restatement: for a diagonal F the Hencky strain is diag(ln lam) in the global axes, so
    T = the small-strain J2 stress of [ln lam0, ln lam1, ln lam2, 0] and P_ii = T_ii / lam_i.  T from the oracle's radial return and
    from law 27 (plane-strain J2, linear hardening) of the same process; loading far past yield, then unloading by half a yield stress."""
    N = 300
    prm = ls.PRM
    lam_, mu = onp.lame(prm["E"], prm["nu"])
    rng = np.random.default_rng(17)
    h1 = rng.uniform(-np.log(1.3), np.log(1.3), (N, 3))
    h1 -= h1.mean(axis=1, keepdims=True)
    dev = np.linalg.norm(h1, axis=1)
    h2 = h1 * (1.0 - 0.5 * prm["s0"] / (2.0 * mu * np.sqrt(1.5) * dev))[:, None]
    steps = [h1, h2]
    hard = onp.LinearHardening(prm["s0"], prm["H0"])
    m = material(N, prm)
    j2 = JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=prm["E"], nu=prm["nu"]), jm.LinearHardening(prm["s0"], prm["H0"]),
                                                   hypothesis="plane_strain"), lazy_isv=False)
    j2.set_data_manager(N)
    ep, p = np.zeros((N, 6)), np.zeros(N)
    for inc, h in enumerate(steps):
        if inc:
            m.data_manager.update()
            j2.data_manager.update()
        F = np.concatenate([np.exp(h), np.zeros((N, 2))], axis=1)
        P = np.array(m.integrate(F)[0])
        r = onp.j2_update(np.concatenate([h, np.zeros((N, 3))], axis=1), ep, p, prm["E"], prm["nu"], hard)
        ep, p = r["epsp"], r["p"]
        assert r["plastic"].all() if inc == 0 else not r["plastic"].any()
        assert m.last_stats["n_plastic"] == int(r["plastic"].sum()) and m.last_stats["n_nan"] == 0
        T27 = np.array(j2.integrate(np.concatenate([h, np.zeros((N, 1))], axis=1))[0])
        scale = np.maximum(np.abs(P).max(axis=1), prm["s0"])
        for name, T in (("the oracle", r["sig"][:, :3]), ("law 27", T27[:, :3])):
            e = (np.abs(P[:, :3] - T / np.exp(h)).max(axis=1) / scale).max()
            print(f"diagonal {'load' if inc == 0 else 'unload'}: P_ii against T_ii / lam_i of {name} {e:.3e} (bound {BOUNDS['amp 1.3']:.1e})")
            assert e <= BOUNDS["amp 1.3"]
        assert not P[:, 3:].any()
    m.close()
    j2.close()


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------------
def test_tile_loop_at_one_workgroup_per_cu_equals_the_default_grid_bit_for_bit():
    torch = pytest.importorskip("torch")
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert NLOOP == tlc.size_for(256)
    print(f"tile loop: {num_cu} CUs, {tlc.passes(NLOOP, num_cu, 1)} passes at blocks_per_cu = 1, {tlc.passes(NLOOP, num_cu, 256)} at 256")
    assert tlc.passes(NLOOP, num_cu, 1) >= 4 and NLOOP % 64 != 0
    F, Ep, p = lp.stretch_case(0, NLOOP, 2.0, seed=8)
    g = to_device(F)
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for bpc in (None, 1):
        m = material(NLOOP)
        set_old_state(m, Ep, p)
        if bpc is not None:
            m.set_option("blocks_per_cu", bpc)
        f = torch.full((NLOOP + 3, 5), float("nan"), dtype=torch.float64, device="cuda:0")
        c = torch.full((NLOOP + 3, 25), float("nan"), dtype=torch.float64, device="cuda:0")
        m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), st)
        torch.cuda.synchronize()
        out.append((to_host(f), to_host(c), *state_of(m), m.stats()[1]))
        m.close()
    a, b = out
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(bits(x), bits(y))
    assert a[5]["n_nan"] == b[5]["n_nan"] == 0 and a[5]["n_plastic"] == b[5]["n_plastic"] > 0
    assert np.isnan(b[0][NLOOP:]).all() and np.isnan(b[1][NLOOP:]).all()               # nothing past 5 n / 25 n doubles
    idx = tlc.reference_sample(NLOOP, num_cu)
    ref = lp.restricted(F[idx], Ep[idx], p[idx])
    got = dict(P=b[0][idx], A=b[1][idx].reshape(-1, 5, 5), eel=b[2][idx], p=b[3][idx, 0], Ep=b[4][idx])
    held("tile loop sample", got, {q: ref[q] for q in KEYS}, ls.PRM, {"amp 2": np.ones(len(idx), dtype=bool)}, keep=~ref["skip"])
    assert ref["skip"].mean() <= ls.KINK_CAP and ls.SHARE[0] <= ref["plastic"].mean() <= ls.SHARE[1]


# ---- routes -----------------------------------------------------------------------------------------------------------------------------
def test_routes_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    N = NCHUNK
    assert tlc.plan_chunks(N, False, True, 64)[0] == 2
    F, Ep, p = lp.stretch_case(0, N, 1.3, seed=4)
    m = material(N)
    set_old_state(m, Ep, p)
    P, isv, A = m.integrate(F)                                  # host buffers, two chunks
    P, isv, A = np.array(P), np.array(isv), np.array(A).reshape(N, 25)
    st2 = dict(m.last_stats)
    S = state_of(m)
    assert st2["n_nan"] == 0 and st2["n_plastic"] > 0
    idx = np.r_[0:300, 131072 - 300:131072 + 300, N - 300:N]     # both chunks and their seam
    ref = lp.restricted(F[idx], Ep[idx], p[idx])
    held("host path sample", dict(P=P[idx], A=A[idx].reshape(-1, 5, 5), eel=S[0][idx], p=S[1][idx, 0], Ep=S[2][idx]), {q: ref[q] for q in KEYS},
         ls.PRM, {"amp 1.3": np.ones(len(idx), dtype=bool)}, keep=~ref["skip"])
    # host buffers in one chunk
    m.set_option("max_chunks", 1)
    P1, isv1, A1 = m.integrate(F)
    assert np.array_equal(bits(P1), bits(P)) and np.array_equal(bits(np.array(A1).reshape(N, 25)), bits(A)) and np.array_equal(bits(isv1), bits(isv))
    assert all(m.last_stats[q] == st2[q] for q in ("n_plastic", "n_nan", "n_not_converged", "max_local_iters"))
    for a, b in zip(state_of(m), S):
        assert np.array_equal(bits(a), bits(b))
    m.set_option("max_chunks", 64)
    # option packed_transfer has nothing to pack for this law: same bytes either way
    m.set_option("packed_transfer", 0)
    P0, _, A0 = m.integrate(F)
    assert np.array_equal(bits(P0), bits(P)) and np.array_equal(bits(np.array(A0).reshape(N, 25)), bits(A))
    m.set_option("packed_transfer", 2)
    # the device-pointer form
    dev = torch.device("cuda:0")
    g = to_device(F)
    f = torch.empty((N, 5), dtype=torch.float64, device=dev)
    c = torch.empty((N, 25), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(bits(to_host(f)), bits(P)) and np.array_equal(bits(to_host(c)), bits(A))
    fin = m.get_final_state_dict()
    assert np.array_equal(bits(np.array(fin["ElasticStrain"])), bits(isv[:, :4])) and np.array_equal(bits(np.array(fin["EquivalentPlasticStrain"]).reshape(N)), bits(isv[:, 4]))
    for a, b in zip(state_of(m), S):
        assert np.array_equal(bits(a), bits(b))
    # rows form over a permuted subset of a larger array: the named rows get the values, the others keep their fill
    M = N + 500
    rows = np.ascontiguousarray(np.random.default_rng(0).permutation(M)[:N], dtype=np.int64)
    flux, tang = np.full((M, 5), -7.0), np.full((M, 25), -9.0)
    m.integrate_rows(F, rows, flux, tang)
    assert np.array_equal(bits(flux[rows]), bits(P)) and np.array_equal(bits(tang[rows]), bits(A))
    rest = np.setdiff1d(np.arange(M), rows)
    assert np.all(flux[rest] == -7.0) and np.all(tang[rest] == -9.0)
    m.close()


def test_state_routes_set_get_and_the_elastic_strain_rebuild():
    """``dxm_set_state`` / ``dxm_get_state`` of all three fields, and the hidden plastic strain rebuilt from (F_n, ElasticStrain_n):
    a handle whose state is set through the public dictionary answers like one whose hidden field is set directly."""
    N = 1003
    F1 = lp.stretch_case(0, N, 1.3, seed=21)[0]
    F2, Ep, p = lp.stretch_case(0, N, 1.3, seed=22)
    lib = _lib.load()
    m = material(N)
    h = m._parts[0][0]
    rng = np.random.default_rng(5)
    for which in (_lib.S0, _lib.S1):
        for f, dim in enumerate(FIELD_DIMS):
            a = np.ascontiguousarray(rng.standard_normal((N, dim)))
            b = np.empty_like(a)
            assert lib.dxm_set_state(h, which, f, a.ctypes.data) == 0 and lib.dxm_get_state(h, which, f, b.ctypes.data) == 0, err(lib)
            assert np.array_equal(bits(a), bits(b)), (which, f)
    bad = np.zeros((N, 4))
    assert lib.dxm_get_state(h, _lib.S0, 3, bad.ctypes.data) < 0 and lib.dxm_get_state(h, _lib.S0, 2, bad.ctypes.data) == 0      # three fields
    m.close()
    # the rebuild: Ep_n = E(F_n) - ElasticStrain_n
    E1 = cv.hencky_strain_plane(F1)
    eel_n = E1 - Ep
    hidden = E1 - eel_n                    # what the Python layer hands over, in its own rounding
    a = material(N)
    a.set_initial_state_dict({"DeformationGradient": F1, "ElasticStrain": eel_n, "EquivalentPlasticStrain": p})
    got = state_of(a, _lib.S0)
    assert np.array_equal(bits(got[2]), bits(hidden)) and np.array_equal(bits(got[1][:, 0]), bits(p)) and np.array_equal(bits(got[0]), bits(eel_n))
    Pa, isva, Aa = (np.array(x) for x in a.integrate(F2))
    b = material(N)
    set_old_state(b, hidden, p)
    Pb, isvb, Ab = (np.array(x) for x in b.integrate(F2))
    assert np.array_equal(bits(Pa), bits(Pb)) and np.array_equal(bits(Aa), bits(Ab)) and np.array_equal(bits(isva), bits(isvb))
    assert a.last_stats["n_plastic"] == b.last_stats["n_plastic"] > 0
    ref = lp.restricted(F2, hidden, p)
    held("after the rebuild", results(b, Pb, Ab), {q: ref[q] for q in KEYS}, ls.PRM, {"amp 1.3": np.ones(N, dtype=bool)}, keep=~ref["skip"])
    # the natural state is F = I
    s0 = material(5).get_initial_state_dict()
    assert np.array_equal(np.array(s0["DeformationGradient"]), np.tile([1.0, 1, 1, 0, 0], (5, 1)))
    a.close()
    b.close()


@pytest.mark.parametrize("ncell,nqp", [(41, 4), (2001, 4)])
def test_two_maps_on_disjoint_cells_equal_one_map_over_all(ncell, nqp):
    """The reference's test_multimaterials property through the accelerated field map (rows forms for the subsets), over two
    increments with an advance between: the second one starts from the plastic strain the first one left."""
    n = ncell * nqp
    rng = np.random.default_rng(2)
    perm = rng.permutation(ncell)
    parts = [np.sort(perm[: ncell // 3]).astype(np.int32), np.sort(perm[ncell // 3:]).astype(np.int32)]
    hist = [lp.stretch_case(0, n, 1.1, seed=31)[0], lp.stretch_case(0, n, 1.3, seed=32)[0]]
    now = {"g": np.tile([1.0, 1.0, 1.0, 0.0, 0.0], (n, 1))}     # the state is initialised at F = I, as the demo's is
    ev = lambda c: now["g"].reshape(ncell, nqp, 5)[c].reshape(-1, 5)   # noqa: E731
    whole = QuadratureFieldMap(ncell, nqp, JAXMaterial(behaviour(ls.PRM)))
    subs = [QuadratureFieldMap(ncell, nqp, JAXMaterial(behaviour(ls.PRM)), cells=c) for c in parts]
    for q in [whole] + subs:
        q.register_gradient("DeformationGradient", ev)
        q.initialize_state()
    fields = lambda q: {"flux": q.fluxes["FirstPiolaKirchhoffStress"].x.array, "eel": q.internal_state_variables["ElasticStrain"].x.array,   # noqa: E731
                        "p": q.internal_state_variables["EquivalentPlasticStrain"].x.array, "jac": q.jacobian_flatten.x.array}
    width = {"flux": 5, "eel": 4, "p": 1, "jac": 25}
    Ep, p = lp.natural_state(n)
    for g in hist:
        now["g"] = g
        for q in [whole] + subs:
            q.update()
            q.advance()
        ref = lp.restricted(g, Ep, p)
        Ep, p = ref["Ep"], ref["p"]
        got = {name: fields(whole)[name].reshape(n, w) for name, w in width.items()}
        held("field map", dict(P=got["flux"], A=got["jac"].reshape(n, 5, 5), eel=got["eel"], p=got["p"][:, 0], Ep=ref["Ep"]), {q: ref[q] for q in KEYS},
             ls.PRM, {"amp 1.3": np.ones(n, dtype=bool)}, keep=~ref["skip"])
        for name, w in width.items():
            for q, cells in zip(subs, parts):
                mine = fields(q)[name].reshape(n, w)
                rows = (cells[:, None] * nqp + np.arange(nqp)[None]).ravel()
                assert np.array_equal(bits(mine[rows]), bits(got[name][rows])), name
                rest = np.setdiff1d(np.arange(n), rows)
                assert not mine[rest].any(), name          # the other cells' rows are not this map's to write
    for q in [whole] + subs:
        q.close()
        q.material.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle_each_with_its_own_sentence():
    import plane_gradient_ref as pg
    from dolfinx_materials_amd.gradient import PlaneMesh

    lib = _lib.load()
    case = pg.quad_case("q1-x4")
    mesh = PlaneMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"], case["dphi"])
    n = mesh.npoints
    F, Ep, p = lp.stretch_case(0, n, 1.3, seed=3)
    m = material(n)
    set_old_state(m, Ep, p)
    P, isv, A = m.integrate(F)
    before = [np.array(P), np.array(A)] + state_of(m)
    h = m._parts[0][0]
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h, layout) < 0 and "the plane-strain logarithmic-strain plasticity tangent dP/dF is a 5x5 block of 25 entries" in err(lib)
    assert lib.dxm_tangent_size(h) == 25
    field = np.full(n, 1.0)
    assert lib.dxm_set_param_field(h, 1, field.ctypes.data) < 0
    assert "per-point parameter fields are not served for plane-strain logarithmic-strain plasticity" in err(lib)
    frame = np.eye(3)
    assert lib.dxm_set_frame(h, frame.ctypes.data) < 0 and "plane-strain logarithmic-strain plasticity is isotropic" in err(lib)
    frames = np.tile(np.eye(3).reshape(9), (n, 1))
    assert lib.dxm_set_frame_field(h, frames.ctypes.data) < 0 and "plane-strain logarithmic-strain plasticity is isotropic" in err(lib)
    for badp, word in (((210e9, 0.3, -1.0, 1e6), "s0 must be > 0"), ((210e9, 0.3, 250e6, -1.0), "H0 must be >= 0"), ((210e9, 0.5, 250e6, 1e6), "invalid elastic constants"),
                       ((210e9, 0.3, float("nan"), 1e6), "s0 must be finite")):
        assert lib.dxm_set_params(h, (C.c_double * 4)(*badp), 4) < 0 and word in err(lib), err(lib)
    assert lib.dxm_set_params(h, (C.c_double * 3)(210e9, 0.3, 250e6), 3) < 0 and "expects 4 parameters" in err(lib), err(lib)
    assert lib.dxm_set_external_state_uniform(h, 0, 300.0) < 0 and "law 42 has no external state variable" in err(lib), err(lib)
    u, fl, ct = np.zeros(mesh.displacement_size), np.zeros((n, 5)), np.zeros((n, 25))
    rows, st = np.arange(n, dtype=np.int64), _lib.Stats()
    for fused in (1, 0):
        m.set_option("fused_gradient", fused)
        rcs = (lib.dxm_integrate_displacement(h, mesh._handle, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_rows(h, mesh._handle, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_device(h, mesh._handle, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
        for rc in rcs:
            assert rc < 0 and "plane-strain logarithmic-strain plasticity takes the 5-wide deformation gradient [F00, F11, F22, F01, F10]" in err(lib), err(lib)
            assert "[1 + H00, 1 + H11, 1, H01, H10]" in err(lib)
    m.set_option("fused_gradient", 1)
    assert not fl.any() and not ct.any()
    with pytest.raises(ValueError, match="5x5 block of 25 entries"):
        JAXMaterial(behaviour(ls.PRM), tangent_layout="sym")
    good = (C.c_double * 4)(210e9, 0.3, 250e6, 1e6)
    for unknown in (41, 43):
        assert not lib.dxm_create(unknown, good, 4, 8, 0) and f"unknown law id {unknown}" in err(lib)
    assert not lib.dxm_create(42, (C.c_double * 4)(210e9, 0.3, -1.0, 1e6), 4, 8, 0) and "s0 must be > 0" in err(lib)
    # the handle is what it was
    set_old_state(m, Ep, p)
    P, isv, A = m.integrate(F)
    after = [np.array(P), np.array(A)] + state_of(m)
    for a, b in zip(after, before):
        assert np.array_equal(bits(a), bits(b))
    assert lib.dxm_kernel_name(h) == b"log_strain_plane_kernel" and lib.dxm_tangent_size(h) == 25
    m.close()
    mesh.close()


def test_a_custom_hardening_build_refuses_the_law_with_its_own_sentence():
    """(the expressions are those of tests/test_custom_hardening.py: one build in the cache serves every file that asks)"""
    hd = jm.CustomHardening("sig0 + K * (pow(p + p0, n) - pow(p0, n))", "K * n * pow(p + p0, n - 1.0)", sig0=250.0, K=600.0, n=0.3, p0=1e-3)
    lib = _lib.load_custom(hd.expr_R, hd.expr_dR)
    assert lib.dxm_has_custom_hardening() == 1
    assert not lib.dxm_create(42, (C.c_double * 4)(210e9, 0.3, 250e6, 1e6), 4, 64, 0)
    msg = (lib.dxm_last_error() or b"").decode()
    assert "plane-strain logarithmic-strain plasticity takes linear hardening only" in msg and "not by a custom-hardening build" in msg, msg
