"""GPU: ``single_crystal_kernel`` (law id 14) through the C ABI over parameters, time steps, GPU-carried histories and every branch of
its local Newton -- step halving, the iteration cap, the guard at dg = 0, rounds whose four points finish at different times.  Inputs,
references and driver code are ``single_crystal_cases.py`` (run on the CPU double by ``test_single_crystal_sweep_cpu.py``); every bound
is read from ``golden/single_crystal_sweep.npz``: max(the field's existing bound, 8 x the deviation of the float64 restatement from
the 50-digit law), per field group and per seed or harvest corner.  No point is left out of a value comparison but those the
restatement itself reports as not converged (they are counted); the yield-surface tolerance touches the n_plastic count only.

Sizes: 1027 points (16 full tiles and a ragged one of 3) for the sweeps, 71 for the constructed tiles; the grid comparison runs at
``tile_loop_cases.size_for(num_cu)`` (206 147 points on 256 compute units: 7 ms of kernel time)."""
import json
import os

import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import single_crystal_cases as cs
import tile_loop_cases as tl
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_crystal_sweep.npz"))
META = json.loads(str(GOLD["meta"]))
HV = {k[3:]: GOLD[k] for k in GOLD.files if k.startswith("hv_")}
GROUPS = ("stress", "tangent", "state")
LAW = _lib.LAW_SINGLE_CRYSTAL_FCC
ROUTE_SEED, ROUTE_INC = 4, 15          # dt = 10, developed flow on the way up


class DeviceArrays:
    @staticmethod
    def up(a):
        return to_device(np.ascontiguousarray(a, dtype=np.float64))

    @staticmethod
    def zeros(n, k):
        import torch

        return torch.zeros((n, k), dtype=torch.float64, device="cuda")

    @staticmethod
    def ptr(t):
        return t.data_ptr()

    @staticmethod
    def down(t):
        return to_host(t)

    @staticmethod
    def sync():
        import torch

        torch.cuda.synchronize()


def make(prm, n):
    return cs.Handle(_lib.load(), LAW, prm, n, arrays=DeviceArrays)


def line(tag, dev, bound):
    print(f"single crystal sweep parity {tag}: " + " ".join(f"{k} {dev[k]:.3e} (bound {bound[k]:.1e})" for k in GROUPS))


# ---- a. parameters and time steps, histories carried by the kernel's own stores ---------------------------------------------------
@pytest.mark.parametrize("seed", cs.SEEDS)
def test_history_carried_on_the_device(seed):
    """create, frame field, then 44 x (dxm_integrate_device, compare, dxm_advance): the state is never set from the host"""
    hist = cs.history(seed, cs.N_SWEEP)
    bound = dict(zip(GROUPS, GOLD["hist_bound"][seed]))
    h = make(hist["prm"], cs.N_SWEEP).frame(hist["R"])
    worst = cs.walk_history(h, hist, bound)
    h.close()
    line(f"history seed {seed} dt {hist['dt']:g} n {hist['prm'][9]:g}", worst, bound)


# ---- b. revert inside a history ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1, 4))
def test_revert_at_the_reversal_leaves_no_trace(seed):
    ra, rb = cs.revert_inside_history(make, cs.history(seed, cs.N_SWEEP))
    assert cs.bit_equal(ra, rb) and ra[3] == rb[3]


# ---- c. harvested cases against the 50-digit values ----------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", range(len(cs.CORNERS)))
def test_harvested_status_0_cases_against_50_digits(corner):
    """quick, slow and halved cases of one parameter set and dt: the halved iteration lands on the root the 50-digit Newton confirms"""
    dev, bound = cs.harvest_against_50_digits(make, GOLD, corner)
    line(f"harvest {cs.CORNERS[corner][0]}", dev, bound)


def test_status_0_cases_alone_against_50_digits():
    """every status-0 case once more without company: its own iteration count is what max_local_iters reports, so a wrong halving or a
    wrong first step cannot hide behind the corner's slowest case"""
    for i in np.nonzero(HV["status"] == 0)[0]:
        _, prm, dt = cs.CORNERS[HV["corner"][i]]
        eps, R, state = cs.harvest_inputs(HV, [i])
        S, T, new, st = cs.run_cases(make, prm, dt, eps, R, state)
        V = HV["state"][[i]]
        ref = {"stress": HV["stress"][[i]], "tangent": HV["tangent"][[i]], "eel": V[:, :6], "g": V[:, 6:18], "p": V[:, 18:30], "a": V[:, 30:42]}
        dev = cs.deviations(S, T, new, ref)
        bound = dict(zip(GROUPS, GOLD["hv_corner_bound"][HV["corner"][i]]))
        if HV["cls"][i] == 2:
            line(f"halved case {i} ({HV['halvings'][i]} halvings, {HV['iters'][i]} iterations)", dev, bound)
        assert all(dev[k] <= bound[k] for k in GROUPS), (int(i), dev)
        assert st["n_not_converged"] == 0 and abs(st["max_local_iters"] - int(HV["iters"][i])) <= 1, (int(i), st, int(HV["iters"][i]))


# ---- d. the law's own failures: the iteration cap and the guard at dg = 0 -----------------------------------------------------------
def test_capped_and_guard_failed_cases():
    n = sum(cs.failed_cases(make, HV, corner) for corner in range(len(cs.CORNERS)))
    assert n == int((HV["status"] != 0).sum()) >= 16


def test_capped_cases_alone_report_the_cap():
    """one at a time: status 1, finite outputs, and the shipped cap in max_local_iters: 25, or 26 where the last pass halved a step
    (the restatement's own count; an iteration that never converges may halve once more or less on other arithmetic)"""
    for i in np.nonzero(HV["status"] == 1)[0]:
        _, prm, dt = cs.CORNERS[HV["corner"][i]]
        eps, R, state = cs.harvest_inputs(HV, [i])
        S, T, new, st = cs.run_cases(make, prm, dt, eps, R, state)
        assert st["n_not_converged"] == 1 and 25 <= st["max_local_iters"] <= 26 and 25 <= int(HV["iters"][i]) <= 26, (int(i), st)
        assert np.isfinite(S).all() and np.isfinite(T).all()


def test_every_cap_on_the_halved_cases():
    """dxm_set_newton(h, m, 1e-14) for every m below a halved case's own count: the cap of the halving branch (`it >= maxit` after
    `step *= 0.5`) is reached at exactly the pass the restatement reaches it"""
    hit = sum(cs.caps_on_a_halved_case(make, HV, int(i)) for i in np.nonzero(HV["cls"] == 2)[0])
    assert hit >= 8, hit


@pytest.mark.parametrize("corner", range(len(cs.CORNERS)))
def test_lowered_iteration_cap(corner):
    """dxm_set_newton(h, 3, 1e-14) on the well-behaved cases: the restatement's count at maxit = 3"""
    got = cs.lowered_cap(make, GOLD, corner)
    if got is not None:
        print(f"lowered cap {cs.CORNERS[corner][0]}: {got[0]} capped, {got[1]} converged")
    assert got is not None or not ((HV["corner"] == corner) & (HV["cls"] <= 1)).any()


# ---- e. round-mates do not matter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", range(len(cs.CORNERS)))
def test_round_mates_do_not_matter(corner):
    """every harvested point of the corner alone among elastic points, as rank 0 to 3 of a round of the other classes, in a fully
    yielded tile and in the ragged tail: its own numbers and what it adds to the counts bit for bit the same, the other points
    untouched by it"""
    for x in np.nonzero(HV["corner"] == corner)[0]:
        cs.check_placements(make, HV, int(x))


def test_a_corner_mixes_quick_slow_and_halved_or_capped():
    assert cs.mixing_corners(HV)


# ---- f. routes at a time step that is not the default ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route():
    hist = cs.history(ROUTE_SEED, cs.N_SWEEP)
    assert hist["dt"] != 0.1 and hist["ref"][ROUTE_INC]["plastic"].all()
    state = {k: hist["ref"][ROUTE_INC - 1][k] for k in cs.FIELDS}
    h = make(hist["prm"], cs.N_SWEEP).frame(hist["R"]).set_state(state)
    base = h.device(hist["eps"][ROUTE_INC], hist["dt"])
    h.close()
    return hist, state, hist["eps"][ROUTE_INC], base


def test_routes_host_buffer_form_in_one_chunk_and_in_three(route):
    hist, state, eps, (S, T, new, st) = route
    isv_ref = np.concatenate([new[k] for k in cs.FIELDS], axis=1)
    h = make(hist["prm"], cs.N_SWEEP).frame(hist["R"])
    for chunks in (1, 3):
        h.set_state(state).option("max_chunks", chunks)
        S2, T2, isv, st2 = h.host(eps, hist["dt"])
        assert np.array_equal(S2, S) and np.array_equal(T2, T) and np.array_equal(isv, isv_ref) and st2 == st, chunks
    h.close()


def test_routes_rows_form(route):
    hist, state, eps, (S, T, new, st) = route
    rows = 2 * np.arange(cs.N_SWEEP)
    h = make(hist["prm"], cs.N_SWEEP).frame(hist["R"]).set_state(state)
    F, Ct, st2 = h.rows(eps, hist["dt"], rows)
    assert np.array_equal(F[rows], S) and np.array_equal(Ct[rows], T) and np.all(F[1::2] == -7.0) and np.all(Ct[1::2] == -9.0) and st2 == st
    assert cs.bit_equal((S, T, h.get_state()), (S, T, new))
    h.close()


def test_routes_device_form_on_a_stream(route):
    import torch

    hist, state, eps, base = route
    h = make(hist["prm"], cs.N_SWEEP).frame(hist["R"]).set_state(state)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = h.device(eps, hist["dt"], stream=s.cuda_stream)
    assert cs.bit_equal(got, base) and got[3] == base[3]
    h.close()


def test_routes_one_workgroup_per_cu(route):
    """at 1027 points and at tile_loop_cases.size_for(num_cu): three full passes of the tile loop and a ragged fourth"""
    import torch

    hist, state, eps, base = route
    h = make(hist["prm"], cs.N_SWEEP).frame(hist["R"]).set_state(state).option("blocks_per_cu", 1)
    got = h.device(eps, hist["dt"])
    assert cs.bit_equal(got, base) and got[3] == base[3]
    h.close()
    N = tl.size_for(int(torch.cuda.get_device_properties(0).multi_processor_count))
    idx = np.arange(N) % cs.N_SWEEP
    big = []
    for bpc in (None, 1):
        h = make(hist["prm"], N).frame(hist["R"][idx]).set_state({k: v[idx] for k, v in state.items()})
        if bpc:
            h.option("blocks_per_cu", bpc)
        big.append(h.device(eps[idx], hist["dt"]))
        h.close()
    assert cs.bit_equal(big[0], big[1]) and big[0][3] == big[1][3]
    assert np.array_equal(big[0][0], base[0][idx]) and np.array_equal(big[0][1], base[1][idx])
    assert big[0][3]["n_plastic"] == N and big[0][3]["n_not_converged"] == 0
