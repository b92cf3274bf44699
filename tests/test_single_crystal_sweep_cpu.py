"""No GPU: the inputs, references and bounds of the single-crystal sweep (``single_crystal_cases.py``,
``golden/single_crystal_sweep.npz``) pinned with the references alone, and the driver code of ``test_gpu_single_crystal_sweep.py`` run
on the CPU double ``fake_dxmat_single_crystal.py``.

Narrowed: the increment norm of the histories of seeds 2, 6 and 9 (``STEP_NORM``: 3.125e-6, 5e-5, 2.5e-5 instead of 1e-4).  At
n = 2 and n = 6 with dt = 1e3 and at seed 6 the Newton from dg = 0 needs more than the shipped 25 iterations for more than 1 % of
the points at 1e-4; the guard at dg = 0 trips at no seed."""
import json
import os

import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import single_crystal_cases as cs
import single_crystal_ref as sc
from fake_dxmat_single_crystal import FakeDxmatSingleCrystal

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_crystal_sweep.npz"))
META = json.loads(str(GOLD["meta"]))
HV = {k[3:]: GOLD[k] for k in GOLD.files if k.startswith("hv_")}
GROUPS = ("stress", "tangent", "state")
N_CPU = 257                            # the histories of the CPU runs of the driver


def make(prm, n):
    return cs.Handle(FakeDxmatSingleCrystal(_lib.load()), _lib.LAW_SINGLE_CRYSTAL_FCC, prm, n)


def test_the_draws_cover_their_ranges():
    prm = np.array([cs.draw(s)[0] for s in cs.SEEDS])
    dts = [cs.draw(s)[1] for s in cs.SEEDS]
    assert np.array_equal(prm[0], sc.param_vector()) and np.array_equal(prm[1], GOLD_KAT["params"][1]) and dts[:2] == [0.1, 0.1]
    assert np.array_equal(prm[0], GOLD_KAT["params"][0])
    assert set(prm[:, 9]) == {2.0, 4.0, 6.0, 10.0, 20.0} and set(dts) == {1e-3, 0.1, 10.0, 1e3}
    eighth = lambda col, lo, hi: (prm[2:, col].min() <= lo + (hi - lo) / 8 and prm[2:, col].max() >= hi - (hi - lo) / 8  # noqa: E731
                                  and prm[2:, col].min() >= lo and prm[2:, col].max() <= hi)
    for col, lo, hi in ((10, 10.0, 80.0), (11, 20.0, 200.0), (12, 0.0, 200.0), (13, 1.0, 50.0), (14, 0.0, 3e3), (0, 1e5, 2.5e5), (1, 1e5, 2.5e5),
                        (2, 1e5, 2.5e5), (3, 0.15, 0.35), (4, 0.15, 0.35), (5, 0.15, 0.35), (6, 4e4, 1e5), (7, 4e4, 1e5), (8, 4e4, 1e5)) + tuple(
                            (c, 0.5, 15.0) for c in range(16, 22)):
        assert eighth(col, lo, hi), col
    lc = np.log(prm[2:, 15])
    assert lc.min() <= np.log(1e3) + np.log(200.0) / 8 and lc.max() >= np.log(2e5) - np.log(200.0) / 8 and lc.min() >= np.log(1e3)
    assert (prm[:, 12] == 0.0).sum() == 1 and (prm[:, 14] == 0.0).sum() == 1
    for p in prm:      # positive definite, and independent moduli
        assert np.linalg.eigvalsh(sc.stiffness(p)).min() > 0
    assert len(set(prm[2:, 0])) == len(set(prm[2:, 1])) == len(set(prm[2:, 8])) == 8 and not np.array_equal(prm[2:, 0], prm[2:, 1])


GOLD_KAT = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_crystal_kat.npz"))


@pytest.mark.parametrize("seed", cs.SEEDS)
def test_every_history_meets_its_conditions(seed):
    """at the size of the GPU sweep: the shares, the cap of the count tolerance, and that the path is what it is said to be"""
    hist = cs.history(seed, cs.N_SWEEP)
    n = cs.N_SWEEP
    assert len(hist["eps"]) == cs.N_INC >= 40 and hist["h"] == META["step_norm"][seed]
    assert (hist["first_fail"] != 2).all()                                    # the guard at dg = 0 trips nowhere
    for inc, ref in enumerate(hist["ref"]):
        assert (ref["status"] == 0).sum() >= cs.STATUS0_SHARE * n, inc
        assert hist["kink"][inc].sum() <= cs.KINK_CAP * n, inc
    assert cs.history_ok(hist)
    pl = [int(r["plastic"].sum()) for r in hist["ref"]]
    assert pl[0] == 0 and pl[cs.REVERSAL] < n // 50                           # the two jumps are elastic (but where another system takes over at once)
    assert pl[1] < n // 100 and pl[4] > 0.9 * n and pl[cs.REVERSAL - 1] == n  # first yield, then developed flow
    assert pl[cs.REVERSAL + 1] < n // 50 and pl[cs.N_INC - cs.TURN - 1] == n  # yields again on the other side
    g_up, g_end = hist["ref"][cs.REVERSAL - 1]["g"], hist["ref"][cs.N_INC - cs.TURN - 1]["g"]
    moved = np.abs(g_end - g_up).max(axis=1) > 0
    assert moved[hist["first_fail"] == 0].all()
    assert hist["n_frozen"] == int((hist["first_fail"] != 0).sum()) <= n // 100
    print(f"seed {seed}: dt {hist['dt']:g} n {hist['prm'][9]:g} h {hist['h']:g} frozen {hist['n_frozen']} iterations <= {max(int(r['iters'].max()) for r in hist['ref'])}")


def test_the_step_norm_of_a_narrowed_seed_is_the_first_that_meets_the_conditions():
    assert not cs.history_ok(cs.history(6, cs.N_SWEEP, h=1e-4)) and cs.STEP_NORM[6] == 5e-5


def test_every_harvested_case_still_has_its_class():
    cs.check_harvest(HV)
    assert cs.mixing_corners(HV)
    for corner, (name, prm, dt) in enumerate(cs.CORNERS):
        m = HV["corner"] == corner
        eps, R, state = cs.harvest_inputs(HV, m)
        out = sc.update(eps, state, prm, dt, R=R)
        assert np.array_equal(out["status"], HV["status"][m]) and np.array_equal(out["halvings"], HV["halvings"][m]), name
        assert np.array_equal(out["iters"], HV["iters"][m]) and np.array_equal(cs.classify(out), HV["cls"][m]), name
    c = HV["cls"]
    assert ((c == 0) & (HV["iters"] >= 3) & (HV["iters"] <= 5)).sum() >= 8 and ((c == 1) & (HV["iters"] >= 15)).sum() >= 8
    assert ((c == 2) & (HV["status"] == 0) & (HV["halvings"] > 0)).sum() >= 8 and ((c == 2) & (HV["halvings"] >= 2)).sum() >= 2
    assert ((c == 3) & (HV["status"] == 1)).sum() >= 8 and ((c == 4) & (HV["status"] == 2)).sum() >= 8
    assert np.isfinite(HV["stress"][HV["status"] == 0]).all() and np.isnan(HV["stress"][HV["status"] != 0]).all()


def test_stored_bounds_are_eight_times_the_stored_deviations_floored_at_the_existing_bounds():
    assert META["digits"] == 50 and META["mp_sample"] == cs.MP_SAMPLE >= 3 and META["groups"] == list(GROUPS)
    floor = np.array([cs.EXISTING_BOUND[g] for g in GROUPS])
    assert floor.tolist() == [1e-12, 3.8e-11, 1e-12]
    assert np.array_equal(GOLD["hist_bound"], np.maximum(floor, 8 * GOLD["hist_dev_all"]))
    assert np.array_equal(GOLD["hv_corner_bound"], np.maximum(floor, 8 * GOLD["hv_corner_dev"]))
    assert (GOLD["hist_dev_last"] <= GOLD["hist_dev_all"]).all() and (GOLD["hist_dev_reversal"] <= GOLD["hist_dev_all"]).all()
    for c in range(len(cs.CORNERS)):
        m = (HV["corner"] == c) & (HV["status"] == 0)
        if m.any():
            assert np.array_equal(GOLD["hv_corner_dev"][c], HV["dev"][m].max(axis=0))
    print("history deviations:", GOLD["hist_dev_all"].max(axis=0), "harvest deviations:", GOLD["hv_corner_dev"].max(axis=0))
    # one conditioning finding, kept with its measured bound: the tangent of the n = 2, dt = 10 corner.  The restatement (and the kernel)
    # take the tangent from the Jacobian of the last-but-one iterate; at n = 2 the overstress term (f / K)^2 has a vanishing slope at
    # f = 0, the Newton closes in on barely yielded systems at a linear rate, and that iterate is 1e-9 of the slip away, not 1e-14
    over = GOLD["hv_corner_dev"] > 1e-9
    assert GOLD["hist_dev_all"].max() <= 1e-9 and over.sum() == 1 and over[4, 1] and GOLD["hv_corner_dev"][4, 1] <= 1e-8


def test_deviations_rederived_for_one_seed_and_two_harvested_cases():
    seed = 5
    hist = cs.history(seed, cs.N_SWEEP)
    idx = GOLD["hist_sample"][seed]
    assert (hist["first_fail"][idx] == 0).all()
    for tag, inc in (("last", cs.N_INC - 1), ("reversal", cs.REVERSAL + 1)):
        V = GOLD[f"hist_{tag}_state"][seed]
        ref = {"stress": GOLD[f"hist_{tag}_stress"][seed], "tangent": GOLD[f"hist_{tag}_tangent"][seed], "eel": V[:, :6], "g": V[:, 6:18],
               "p": V[:, 18:30], "a": V[:, 30:42]}
        out = hist["ref"][inc]
        for j, i in enumerate(idx):      # per point, as the generator measured it
            one = {k: v[j:j + 1] for k, v in ref.items()}
            dev = cs.deviations(out["stress"][i:i + 1], out["tangent"][i:i + 1], {k: out[k][i:i + 1] for k in cs.FIELDS}, one)
            for g, k in enumerate(GROUPS):
                assert dev[k] <= GOLD[f"hist_dev_{tag}"][seed, g] * (1 + 1e-12) and 8 * dev[k] <= GOLD["hist_bound"][seed, g], (tag, k)
    # two harvested cases, a halved one among them, through the 50-digit Newton itself
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_single_crystal_sweep as gen

    halved = int(np.nonzero((HV["cls"] == 2) & (HV["halvings"] >= 2))[0][0])
    slow = int(np.nonzero(HV["cls"] == 1)[0][0])
    for i in (halved, slow):
        _, prm, dt = cs.CORNERS[HV["corner"][i]]
        eps, R, st = cs.harvest_inputs(HV, i)
        dev, S, T, V = gen.solve_case((prm, dt, eps, R, st))      # raises unless the residual falls below 1e-45 from the restatement's root
        assert np.array_equal(S, HV["stress"][i]) and np.array_equal(T, HV["tangent"][i]) and np.array_equal(V, HV["state"][i])
        for g, k in enumerate(GROUPS):
            assert dev[k] == HV["dev"][i, g] and 8 * dev[k] <= GOLD["hv_corner_bound"][HV["corner"][i], g]


# ---- the driver code of the GPU tests on the CPU double ------------------------------------------------------------------------
def test_driver_walks_a_history_on_the_cpu_double():
    hist = cs.history(3, N_CPU)
    h = make(hist["prm"], N_CPU).frame(hist["R"])
    worst = cs.walk_history(h, hist, dict(zip(GROUPS, GOLD["hist_bound"][3])))
    assert max(worst.values()) == 0.0      # the double is the restatement
    h.close()


def test_driver_revert_on_the_cpu_double():
    ra, rb = cs.revert_inside_history(make, cs.history(1, N_CPU))
    assert cs.bit_equal(ra, rb) and ra[3] == rb[3]


def test_driver_harvest_checks_on_the_cpu_double():
    corner = cs.mixing_corners(HV)[0]
    dev, bound = cs.harvest_against_50_digits(make, GOLD, corner)
    assert all(dev[k] <= bound[k] for k in GROUPS)
    assert sum(cs.failed_cases(make, HV, c) for c in range(len(cs.CORNERS))) == int((HV["status"] != 0).sum())
    capped, ok = cs.lowered_cap(make, GOLD, corner)
    assert capped > 0 and ok > 0


def test_driver_caps_on_halved_cases_on_the_cpu_double():
    """and that the halving branch is what stops the iteration at some cap of enough cases for the GPU test to mean something"""
    hit = sum(cs.caps_on_a_halved_case(make, HV, int(i)) for i in np.nonzero(HV["cls"] == 2)[0])
    assert hit >= 8, hit


def test_driver_placements_on_the_cpu_double():
    corner = cs.mixing_corners(HV)[0]
    for c in range(5):
        x = np.nonzero((HV["corner"] == corner) & (HV["cls"] == c))[0]
        if x.size:
            cs.check_placements(make, HV, int(x[0]), same=lambda a, b: np.allclose(a, b, rtol=1e-7, atol=1e-12))
