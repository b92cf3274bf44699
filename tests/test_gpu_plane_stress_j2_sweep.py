"""GPU: plane-stress J2 plasticity with isotropic hardening (laws 30 and 31, ``plane_stress_j2_kernel<hard>``) over the seeded
parameter draws, histories and closed-form rows of ``plane_stress_j2_cases``, through the C ABI (ctypes, the ``Handle`` of
``test_gpu_plane_stress_j2``): the kernel against the 50-digit sweep fixture per draw and over six increments carried on the device,
against the closed forms, against the restatement at 4099 random trials per draw, and the counted point without a bracket.

Bounds on stress (in sig0), tangent (in E) and state (p and epsp, in sig0 / E): 16 x what the restatement deviates from the fixture
by (``plane_stress_j2_cases.MEASURED_SWEEP``, pinned by ``tests/test_plane_stress_j2_sweep_cpu.py``), floored at 2e-14 -- linear
1.1e-9 / 7.4e-14 / 1.3e-9, Voce 5.1e-14 / 3.7e-13 / 3.7e-10; the closed-form rows: ``plane_stress_j2_cases.special_bounds``.  The
softening draws (10 and 11 of each law) are held to the same bounds as the others.

Measured on an MI355X: see DESIGN.md, "Plane-stress J2 plasticity with isotropic hardening"."""
import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import plane_stress_j2_cases as cs
import plane_stress_j2_ref as pj
from helpers import to_device
from test_gpu_plane_stress_j2 import Handle as BaseHandle, err

pytestmark = pytest.mark.gpu

DRAWS = [(law, k) for law in cs.LAWS for k in range(cs.N_DRAWS)]
HISTORIES = [(law, k) for law in cs.LAWS for k in cs.HISTORY_DRAWS[law]]
IDS = lambda lk: cs.tag(*lk)      # noqa: E731
N_PARITY = 4099                   # 64 tiles and a ragged one of 3
N_SPECIAL = 4 * 64 + 7


class Handle(BaseHandle):
    def set_state(self, p, epsp, which=_lib.S0):
        p, epsp = np.ascontiguousarray(p, dtype=np.float64).reshape(self.n, 1), np.ascontiguousarray(epsp, dtype=np.float64).reshape(self.n, 3)
        assert self.lib.dxm_set_state(self.h, which, 0, p.ctypes.data) == 0, err(self.lib)
        assert self.lib.dxm_set_state(self.h, which, 1, epsp.ctypes.data) == 0, err(self.lib)


_fixture = []


def fixture():
    if not _fixture:
        _fixture.append(cs.load_fixture())
    return _fixture[0]


def deviations(prm, got, want):
    s, Em = prm[2], prm[0]
    return np.array([np.abs(got[0] - want["stress"]).max() / s, np.abs(got[1] - want["tangent"]).max() / Em,
                     np.abs(got[2] - cs.state_of(want)).max() / (s / Em)])


WORST = {}      # (law, against what) -> the largest deviations the tests of this run have seen


def check(tag, law, prm, got, want, kind="fixture"):
    dev, bound = deviations(prm, got, want), cs.gpu_bounds(law)
    w = WORST[(law, kind)] = np.maximum(WORST.get((law, kind), np.zeros(3)), dev)
    print(f"plane-stress J2 sweep {tag}: stress {dev[0]:.3e} (bound {bound[0]:.2e})  tangent {dev[1]:.3e} ({bound[1]:.2e})  "
          f"state {dev[2]:.3e} ({bound[2]:.2e});  {cs.NAME[law]} against the {kind}, largest so far: {w[0]:.3e} / {w[1]:.3e} / {w[2]:.3e}")
    assert all(d <= b for d, b in zip(dev, bound)), (tag, dev, bound)
    return dev


def symmetric(ct):
    ct = ct.reshape(-1, 3, 3)
    return np.array_equal(ct, np.swapaxes(ct, 1, 2))


def take(d, idx):
    return {q: d[q][idx] for q in ("stress", "tangent", "p", "epsp", "plastic")}


# ---- the kernel against the fixture, per draw ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 321])          # one tile and a point; five tiles and a point
@pytest.mark.parametrize("lk", DRAWS, ids=IDS)
def test_the_kernel_against_the_fixture_from_the_drawn_old_state(lk, N):
    law, k = lk
    d = cs.fixture_draw(fixture(), law, k)
    prm = d["prm"]
    idx = np.arange(N) % len(d["eps"])
    ref = pj.update(law, d["eps"], d["epsp_n"], d["p_n"], prm)
    h = Handle(law, N, prm)
    h.set_state(d["p_n"][idx], d["epsp_n"][idx])
    got = h.device(to_device(d["eps"][idx]))
    check(f"{cs.tag(law, k)} N={N}", law, prm, got, take(d, idx))
    st = got[3]
    assert st["n_plastic"] == int(d["plastic"][idx].sum()) and st["n_not_converged"] == 0 and st["n_nan"] == 0 and st["n_points"] == N
    assert symmetric(got[1])
    assert abs(st["max_local_iters"] - int(ref["iters"].max())) <= 1, (st, int(ref["iters"].max()))
    # an elastic point keeps the bits of the state it read
    el = ~d["plastic"][idx]
    old = np.concatenate([d["p_n"][idx, None], d["epsp_n"][idx]], axis=1)
    assert np.array_equal(got[2][el].view(np.uint64), old[el].view(np.uint64))
    h.close()


# ---- histories carried on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", HISTORIES, ids=IDS)
def test_six_increments_carried_on_the_device_against_the_fixture(lk):
    law, k = lk
    prm, incs = cs.fixture_history(fixture(), law, k)
    N = 65
    idx = np.arange(N) % len(incs[0]["eps"])
    h = Handle(law, N, prm)
    rested = 0
    for q, inc in enumerate(incs):
        got = h.device(to_device(inc["eps"][idx]))
        check(f"history {cs.tag(law, k)} increment {q}", law, prm, got, take(inc, idx), kind="fixture over histories")
        st = got[3]
        assert st["n_plastic"] == int(inc["plastic"][idx].sum()) and st["n_not_converged"] == 0 and st["n_nan"] == 0
        assert symmetric(got[1])
        before = h.state(_lib.S0)
        el = ~inc["plastic"][idx]
        assert np.array_equal(got[2][el].view(np.uint64), before[el].view(np.uint64))
        rested += int((el & (before[:, 0] > 0)).sum())
        assert (got[2][:, 0] >= before[:, 0]).all()
        h.advance()
    assert rested >= 40            # the elastic points met states that are not zero
    h.close()


# ---- rows with a closed form, across the tile edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", DRAWS, ids=IDS)
def test_special_rows_at_the_head_of_a_batch_follow_the_closed_forms(lk):
    law, k = lk
    prm = cs.draw(law, k)
    sp = cs.special_rows(law, prm, cs.softening(law, k))
    m = len(sp["labels"])
    eps, ep, p, _ = cs.points(law, k)
    idx = np.arange(N_SPECIAL) % len(eps)
    eps, ep, p = eps[idx].copy(), ep[idx].copy(), p[idx].copy()
    # the rows at the head of the batch, and again across the edge of tiles 0 and 1 and in the ragged tail
    places = [0, 64 - m // 2, N_SPECIAL - m]
    for at in places:
        eps[at:at + m], ep[at:at + m], p[at:at + m] = sp["eps"], sp["epsp_n"], sp["p_n"]
    h = Handle(law, N_SPECIAL, prm)
    h.set_state(p, ep)
    got = h.device(to_device(eps))
    ref = pj.update(law, eps, ep, p, prm)
    bs, be = cs.special_bounds(prm, sp["eps"])
    either = sum(1 for x in sp["plastic"] if x is None) * len(places)
    assert abs(got[3]["n_plastic"] - int(ref["plastic"].sum())) <= either and got[3]["n_not_converged"] == 0 and got[3]["n_nan"] == 0
    worst = np.zeros(2)
    for at in places:
        stress, state = got[0][at:at + m], got[2][at:at + m]
        for i, label in enumerate(sp["labels"]):
            slack = 2e-12 if sp["plastic"][i] is None else 0.0          # either branch: the two answers differ by 1e-12 sig0
            es = np.abs(stress[i] - sp["stress"][i]).max() / prm[2]
            ee = max(abs(state[i, 0] - sp["p"][i]), np.abs(state[i, 1:] - sp["epsp"][i]).max()) / (prm[2] / prm[0])
            worst = np.maximum(worst, [es / (bs[i] + slack), ee / (be[i] + slack)])
            assert es <= bs[i] + slack and ee <= be[i] + slack, (cs.tag(law, k), label, at, es, bs[i], ee, be[i])
            if sp["plastic"][i] is not None:     # on the branch its label says: a yielded point moves p, an elastic one keeps its bits
                assert (state[i, 0] > sp["p_n"][i]) == sp["plastic"][i], (label, at)
            # symmetry makes these exact zeros
            if label.startswith("equibiaxial"):
                assert stress[i, 2] == 0.0 and state[i, 3] == 0.0 and stress[i, 0] == stress[i, 1] and state[i, 1] == state[i, 2], (label, at)
            if label.startswith("pure shear"):
                assert not stress[i, :2].any() and not state[i, 1:3].any(), (label, at)
            if label == "zero strain":
                assert not stress[i].any() and not state[i].any(), (label, at)
    print(f"plane-stress J2 sweep special rows {cs.tag(law, k)}: largest share of the closed-form bound, stress {worst[0]:.2f} state {worst[1]:.2f}")
    assert symmetric(got[1])
    h.close()


# ---- the restatement as a witness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", DRAWS, ids=IDS)
def test_restatement_parity_at_4099_random_trials(lk):
    law, k = lk
    prm = cs.draw(law, k)
    top = cs.OVER_SOFT if cs.softening(law, k) else cs.OVER_HARD
    eps = pj.random_trials(prm, N_PARITY, seed=400 + k, lo=0.2, hi=top)
    want = pj.update(law, eps, np.zeros_like(eps), np.zeros(N_PARITY), prm)
    h = Handle(law, N_PARITY, prm)
    got = h.device(to_device(eps))
    check(f"restatement parity {cs.tag(law, k)}", law, prm, got, want, kind="restatement")
    near = np.abs(want["overshoot"] - 1.0) < 1e-9                     # on the surface: either side may count
    ref = pj.stats(want)
    assert abs(got[3]["n_plastic"] - ref["n_plastic"]) <= int(near.sum()) and 0.5 * N_PARITY < ref["n_plastic"] < N_PARITY
    assert got[3]["n_not_converged"] == 0 == ref["n_not_converged"] and got[3]["n_nan"] == 0
    assert abs(got[3]["max_local_iters"] - ref["max_local_iters"]) <= 1
    assert symmetric(got[1])
    h.close()


# ---- no bracket: counted, not silently wrong ------------------------------------------------------------------------------------------------------
def test_a_point_without_a_bracket_is_counted_and_its_neighbours_are_untouched():
    """H = -E / 70 at overshoot 1e3: the lower bound of R over the step is negative and no bracket exists"""
    law, prm = pj.J2_LINEAR, cs.draw(pj.J2_LINEAR, 10)
    n = 64 + 9
    eps = pj.random_trials(prm, n, seed=5, lo=2.0, hi=4.0)
    h = Handle(law, n, prm)
    base = h.device(to_device(eps))
    over = pj.update(law, eps, np.zeros_like(eps), np.zeros(n), prm)["overshoot"]
    bad = eps.copy()
    bad[70] *= 1e3 / over[70]
    want = pj.update(law, bad, np.zeros_like(eps), np.zeros(n), prm)
    assert want["not_converged"].sum() == 1 and want["not_converged"][70] and want["iters"][70] == 0
    got = h.device(to_device(bad))
    assert base[3]["n_not_converged"] == 0 and got[3]["n_not_converged"] == 1 and got[3]["n_nan"] == 0 and got[3]["n_plastic"] == n
    keep = np.arange(n) != 70
    assert all(np.array_equal(a[keep].view(np.uint64), b[keep].view(np.uint64)) for a, b in zip(got[:3], base[:3]))
    # the point writes the start of its iteration: finite, and the restatement's to rounding
    assert np.isfinite(got[0][70]).all() and np.isfinite(got[2][70]).all()
    assert np.abs(got[0][70] - want["stress"][70]).max() <= 1e-12 * np.abs(want["stress"][70]).max()
    h.close()
