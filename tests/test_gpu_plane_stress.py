"""GPU: the two plane-stress return mappings (DXM_LAW_PS_QUADRATIC = 23, DXM_LAW_PS_POLYGON = 24; ``plane_stress_kernel<surface,
tangent>``) through the C ABI (ctypes): against the committed 50-digit values and the numpy restatement ``plane_stress_ref``, the grids
and the routes of the library against each other bit for bit, constructed tiles, histories, the projection's own variational
inequality on the kernel's output, the demo's stress paths through ``HIPMaterial``, the status record and every refusal.

Bound on stress (in s* = sig0 / the largest d_k), tangent (in E) and state (in s* / E): 16 x what the restatement deviates from the
50-digit values by (``plane_stress_ref.MEASURED``, pinned by ``tests/test_plane_stress_cpu.py``), floored at 2e-14 --
quadratic 8.3e-12 / 5.6e-12 / 3.4e-11, polygon 2.1e-12 / 2e-14 / 2.1e-12.  The far overshoots set the figures; the margin is for the
kernel's own division and square-root sequences."""
import ctypes as C

import numpy as np
import pytest

from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.plane_stress import L1Rankine, PlaneStressvonMises, Rankine

import plane_stress_ref as ps
import tile_loop_cases as tc
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

E, NU, SIG0, FC, FT = 70e3, 0.2, 30.0, 30.0, 10.0
KINDS = {"quadratic_c": (ps.QUADRATIC, [E, NU, SIG0, 1.0, 0.0]), "quadratic_alg": (ps.QUADRATIC, [E, NU, SIG0, 1.5, 1.0]),
         "rankine": (ps.POLYGON, ps.polygon_params(E, NU, ps.rankine_planes(FT, FC))),
         "l1rankine": (ps.POLYGON, ps.polygon_params(E, NU, ps.l1rankine_planes(FT, FC)))}
GUARD, SENTINEL = 64, -7.25


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


class Handle:
    """one dxm_material of a plane-stress law, driven through ctypes alone"""

    def __init__(self, law, n, prm):
        p = [float(v) for v in prm]
        self.lib, self.n, self.law, self.prm = _lib.load(), n, law, p
        self.h = self.lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        assert self.lib.dxm_tangent_size(self.h) == 9 and self.lib.dxm_algorithmic_bytes(self.h) == 168
        self.tangent = law == ps.QUADRATIC and p[4] != 0

    def stats(self):
        st = _lib.Stats()
        rc = self.lib.dxm_get_stats(self.h, C.byref(st))
        assert rc >= 0, err(self.lib)
        return st.as_dict()

    def state(self, which=_lib.S1):
        a = np.full((self.n, 3), np.nan)
        assert self.lib.dxm_get_state(self.h, which, 0, a.ctypes.data) == 0, err(self.lib)
        return a

    def set_state(self, a, which=_lib.S0):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.n, 3) and self.lib.dxm_set_state(self.h, which, 0, a.ctypes.data) == 0, err(self.lib)

    def device(self, eps_dev):
        """(stress, tangent, state of s1, stats); the output arrays end in guard cells that must keep their sentinel"""
        import torch

        f = torch.full((self.n * 3 + GUARD,), SENTINEL, dtype=torch.float64, device=eps_dev.device)
        c = torch.full((self.n * 9 + GUARD,), SENTINEL, dtype=torch.float64, device=eps_dev.device)
        assert self.lib.dxm_integrate_device(self.h, eps_dev.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        f, c = to_host(f), to_host(c)
        assert (f[self.n * 3:] == SENTINEL).all() and (c[self.n * 9:] == SENTINEL).all()
        return f[: self.n * 3].reshape(self.n, 3), c[: self.n * 9].reshape(self.n, 9), self.state(), self.stats()

    def host(self, eps):
        f, c, st = np.full((self.n, 3), np.nan), np.full((self.n, 9), np.nan), _lib.Stats()
        rc = self.lib.dxm_integrate(self.h, eps.ctypes.data, 0.0, f.ctypes.data, None, c.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()

    def advance(self):
        assert self.lib.dxm_advance(self.h) == 0, err(self.lib)

    def revert(self):
        assert self.lib.dxm_revert(self.h) == 0, err(self.lib)

    def newton(self, maxit=25, rtol=1e-14):
        assert self.lib.dxm_set_newton(self.h, maxit, rtol) == 0, err(self.lib)

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def close(self):
        self.lib.dxm_destroy(self.h)


def same(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def deviations(law, prm, got, want):
    s, Em = ps.scale(law, prm), prm[0]
    return (np.abs(got[0] - want["stress"]).max() / s, np.abs(got[1] - want["tangent"]).max() / Em, np.abs(got[2] - want["state"]).max() / (s / Em))


def check(tag, law, prm, got, want):
    dev, bound = deviations(law, prm, got, want), ps.gpu_bounds(law)
    print(f"plane stress {tag}: stress {dev[0]:.3e} (bound {bound[0]:.2e})  tangent {dev[1]:.3e} ({bound[1]:.2e})  state {dev[2]:.3e} ({bound[2]:.2e})")
    assert all(d <= b for d, b in zip(dev, bound)), (tag, dev, bound)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4161])
@pytest.mark.parametrize("inst", ["quadratic_c", "quadratic_alg", "polygon"])
def test_fixture_parity_over_both_increments(inst, N):
    kat = ps.load_kat()
    law = ps.POLYGON if inst == "polygon" else ps.QUADRATIC
    ran = 0
    for tag, claw, prm, eps, incs in ps.kat_cases(kat):
        if claw != law:
            continue
        prm = prm.copy()
        if law == ps.QUADRATIC:
            prm[4] = float(inst == "quadratic_alg")
        idx = np.arange(N) % len(eps[0])
        h = Handle(law, N, prm)
        for k in range(2):
            got = h.device(to_device(eps[k][idx]))
            tangent = incs[k]["tangent"] if inst == "quadratic_alg" else np.tile(kat[tag + "_elastic"], (len(eps[k]), 1))
            want = dict(stress=incs[k]["stress"][idx], tangent=tangent[idx], state=incs[k]["state"][idx])
            check(f"fixture {tag} {inst} N={N} increment {k + 1}", law, prm, got, want)
            st = got[3]
            assert st["n_plastic"] == int(incs[k]["plastic"][idx].sum()) and st["n_not_converged"] == 0 and st["n_nan"] == 0 and st["n_points"] == N
            assert st["max_local_iters"] <= 25 and (law == ps.QUADRATIC or st["max_local_iters"] == 0)
            if law == ps.QUADRATIC and N >= 63:
                assert st["max_local_iters"] >= 2
            h.advance()
        h.close()
        ran += 1
    assert ran == (4 if law == ps.POLYGON else 6)


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quadratic_c", "quadratic_alg", "rankine"])
def test_tile_loop_at_one_workgroup_per_cu_equals_the_shipped_grid(kind):
    import torch

    law, prm = KINDS[kind]
    N = tc.size_for(int(torch.cuda.get_device_properties(0).multi_processor_count))
    eps = ps.random_trials(law, prm, N, seed=21, lo=0.3, hi=50.0)
    eps2 = eps * np.random.default_rng(22).uniform(0.2, 1.6, (N, 1))
    a, b = Handle(law, N, prm), Handle(law, N, prm)
    b.option("blocks_per_cu", 1)
    for k, e in enumerate((eps, eps2)):
        e_dev = to_device(e)
        ga, gb = a.device(e_dev), b.device(e_dev)
        assert same(ga, gb), (kind, k)
        assert 0.2 * N < ga[3]["n_plastic"] < 0.95 * N and ga[3]["n_nan"] == 0 and ga[3]["n_not_converged"] == 0
        if k == 0:   # a sample of the late passes against the restatement
            idx = tc.reference_sample(N, int(torch.cuda.get_device_properties(0).multi_processor_count))
            want = ps.update(law, e[idx], np.zeros((len(idx), 3)), prm)
            check(f"tile loop {kind}", law, prm, tuple(x[idx] for x in ga[:3]), want)
        a.advance()
        b.advance()
    a.close()
    b.close()


# ---- constructed tiles --------------------------------------------------------------------------------------------------------------------
def constructed(law, prm, seed):
    """tiles of 64: wholly elastic | wholly yielded | alternating lanes | one yielded lane, lane 0 | one yielded lane, lane 63 | a ragged
    tile of 17, mixed.  The yielded points overshoot by 1.01 ... 1e4: the Newton trip counts diverge within a wave"""
    pattern = np.concatenate([np.zeros(64, bool), np.ones(64, bool), np.arange(64) % 2 == 1, np.arange(64) == 0, np.arange(64) == 63,
                              np.arange(17) % 3 == 0])
    n = len(pattern)
    el = ps.random_trials(law, prm, n, seed, lo=0.05, hi=0.95)
    pl = ps.random_trials(law, prm, n, seed + 1, lo=1.01, hi=1e4)
    return np.where(pattern[:, None], pl, el), pattern


@pytest.mark.parametrize("kind", list(KINDS))
def test_constructed_tiles_and_the_guard_cells(kind):
    law, prm = KINDS[kind]
    eps, pattern = constructed(law, prm, seed=31)
    n = len(eps)
    assert n == 5 * 64 + 17
    h = Handle(law, n, prm)
    got = h.device(to_device(eps))                      # (the guard cells are checked by Handle.device)
    want = ps.update(law, eps, np.zeros_like(eps), prm)
    assert np.array_equal(want["plastic"], pattern)
    check(f"constructed tiles {kind}", law, prm, got, want)
    ref = ps.stats(want, h.tangent)
    assert got[3]["n_plastic"] == int(pattern.sum()) and got[3]["n_nan"] == 0 and got[3]["n_not_converged"] == 0
    if law == ps.QUADRATIC:
        assert abs(got[3]["max_local_iters"] - ref["max_local_iters"]) <= 1 and got[3]["max_local_iters"] >= 4
    else:
        assert got[3]["max_local_iters"] == 0
    # an elastic point's state: the zero bits it read; its stress: the trial; its tangent: C
    el = ~pattern
    assert not got[2][el].any() and np.array_equal(got[1][el], want["tangent"][el])
    h.close()


# ---- histories ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_load_unload_reload_and_the_bits_of_points_that_stay_elastic(kind):
    law, prm = KINDS[kind]
    n = 1000
    load = ps.random_trials(law, prm, n, seed=41, lo=0.4, hi=6.0)
    steps = [load, 0.55 * load, 1.4 * load + ps.random_trials(law, prm, n, seed=42, lo=0.1, hi=0.5)]
    h = Handle(law, n, prm)
    state = np.zeros((n, 3))
    for k, eps in enumerate(steps):
        got = h.device(to_device(eps))
        want = ps.update(law, eps, state, prm)
        check(f"history {kind} step {k}", law, prm, got, want)
        near = np.abs(ps.violation(law, want["stress"], prm)) < 1e-9 * ps.scale(law, prm)       # on the surface: either side may count
        assert abs(got[3]["n_plastic"] - int(want["plastic"].sum())) <= int((near & ~want["plastic"]).sum())
        # points that stay elastic keep the PlasticStrain bits they had
        before = h.state(_lib.S0)
        el = ~want["plastic"] & ~near
        assert el.sum() > 50 and np.array_equal(got[2][el].view(np.uint64), before[el].view(np.uint64))
        if k == 1:   # the unloading step: most points stay elastic (the far ones yield in reverse), many from a plastic strain that is not zero
            assert el.sum() > 0.6 * n and (np.abs(before[el]).max(axis=1) > 0).sum() > 0.3 * n
        h.advance()
        state = got[2]                       # the kernel's own state carries on, as the handle's does
    h.close()


# ---- no oracle --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_feasibility_and_the_variational_inequality_on_the_kernels_own_output(kind):
    law, prm = KINDS[kind]
    n = 4096
    eps = ps.random_trials(law, prm, n, seed=51, lo=0.2, hi=8.0)
    h = Handle(law, n, prm)
    got = h.device(to_device(eps))
    trial = eps @ ps.stiffness(prm[0], prm[1]).T
    plastic = np.abs(got[0] - trial).max(axis=1) > 1e-9 * ps.scale(law, prm)
    assert abs(int(plastic.sum()) - got[3]["n_plastic"]) <= 4 and plastic.sum() > 2000
    ps.check_projection(law, prm, trial, got[0], plastic, np.random.default_rng(52))
    h.close()


# ---- the demo, through the Python classes -----------------------------------------------------------------------------------------------------
MATERIALS = {"vonmises": lambda: PlaneStressvonMises(E=E, nu=NU, sig0=SIG0), "rankine": lambda: Rankine(E=E, nu=NU, fc=FC, ft=FT),
             "l1rankine": lambda: L1Rankine(E=E, nu=NU, fc=FC, ft=FT)}


@pytest.mark.parametrize("name", list(MATERIALS))
def test_the_demos_stress_paths(name):
    """``plot_stress_paths`` of demos/cvxpy/cvxpy_return_mapping.py: 21 radial strain paths x 19 increments"""
    m = MATERIALS[name]()
    law, prm = m.behavior.law, m.behavior.params()
    theta = np.linspace(0, 2 * np.pi, 21)
    Eps = np.vstack([np.array([1e-3 * np.cos(t), 1e-3 * np.sin(t), 0]) for t in theta])
    m.set_data_manager(len(Eps))
    state = m.get_initial_state_dict()
    assert set(state) == {"Strain", "Stress"}
    ref_state = np.zeros((21, 3))
    for t in np.linspace(0, 1, 20)[1:]:
        sig, isv, Ct = m.integrate(t * Eps)
        want = ps.update(law, t * Eps, ref_state, prm)
        got = (np.asarray(sig), np.asarray(Ct).reshape(21, 9), want["state"])
        check(f"demo {name} t={t:.3f}", law, prm, got, want)
        m.data_manager.update()
        ref_state = want["state"]
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.asarray(s0["Strain"]), Eps) and np.array_equal(np.asarray(s0["Stress"]), np.asarray(sig))
    # every yielded path ends on its surface
    v = ps.violation(law, np.asarray(sig), prm)
    assert want["plastic"].sum() >= 15 and np.abs(v[want["plastic"]]).max() <= 1e-12 * ps.scale(law, prm) and v.max() <= 1e-12 * ps.scale(law, prm)
    m.close()


# ---- host forms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quadratic_alg", "l1rankine"])
def test_host_buffer_form_equals_the_device_form_bit_for_bit(kind):
    law, prm = KINDS[kind]
    n = 100_003
    eps = ps.random_trials(law, prm, n, seed=61, lo=0.3, hi=20.0)
    h = Handle(law, n, prm)
    base = h.device(to_device(eps))
    assert same(h.host(eps), base)
    h.option("max_chunks", 3)
    assert same(h.host(eps), base)
    h.option("pipeline", 0)
    assert same(h.host(eps), base)
    h.close()


@pytest.mark.parametrize("name", list(MATERIALS))
def test_prestress_through_set_initial_state_dict_and_revert(name):
    m = MATERIALS[name]()
    law, prm = m.behavior.law, m.behavior.params()
    n = 500
    m.set_data_manager(n)
    pre = ps.sample_admissible(law, prm, n, np.random.default_rng(71)) * 0.8
    m.set_initial_state_dict({"Stress": pre})                       # a zero strain
    epsp = -(pre @ ps.compliance(E, NU).T)
    eps = ps.random_trials(law, prm, n, seed=72, lo=0.2, hi=3.0)
    sig, _, Ct = m.integrate(eps)
    want = ps.update(law, eps, epsp, prm)
    check(f"prestress {name}", law, prm, (np.asarray(sig), np.asarray(Ct).reshape(n, 9), want["state"]), want)
    first = np.asarray(sig).copy()
    m.data_manager.revert()                                          # the increment is rejected: s1 <- s0
    back = m.get_final_state_dict()
    assert np.array_equal(np.asarray(back["Stress"]), pre) and not np.asarray(back["Strain"]).any()
    sig2, _, _ = m.integrate(eps)
    assert np.array_equal(np.asarray(sig2), first)
    m.data_manager.update()
    sig3, _, _ = m.integrate(eps)                                    # from the accepted state: the same strain again changes nothing
    assert np.abs(np.asarray(sig3) - first).max() <= ps.gpu_bounds(law)[0] * ps.scale(law, prm) and m.last_stats["n_plastic"] <= int(want["plastic"].sum())
    m.close()


# ---- the status record ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_nan_strain_counts_once_and_leaves_its_neighbours_alone(kind):
    law, prm = KINDS[kind]
    n = 777
    eps = ps.random_trials(law, prm, n, seed=81, lo=0.3, hi=5.0)
    h = Handle(law, n, prm)
    base = h.device(to_device(eps))
    bad = eps.copy()
    bad[300, 1] = np.nan
    got = h.device(to_device(bad))
    ok = np.delete(np.arange(n), 300)
    assert got[3]["n_nan"] == 1 and base[3]["n_nan"] == 0 and np.isnan(got[0][300]).any()
    assert all(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)) for a, b in zip(got[:3], base[:3]))
    assert not got[2][300].any()             # the state of the point: the bits it read
    bad[300, 1] = np.inf
    got = h.device(to_device(bad))
    assert got[3]["n_nan"] == 1 and got[3]["n_not_converged"] == 0
    h.close()


def test_a_capped_newton_counts_its_points():
    law, prm = KINDS["quadratic_alg"]
    n = 640
    eps = ps.random_trials(law, prm, n, seed=91, lo=50.0, hi=1e4)
    h = Handle(law, n, prm)
    h.newton(maxit=1)
    got = h.device(to_device(eps))
    want = ps.update(law, eps, np.zeros_like(eps), prm, maxit=1)
    assert want["not_converged"].sum() >= n // 2
    assert abs(got[3]["n_not_converged"] - int(want["not_converged"].sum())) <= 2 and got[3]["max_local_iters"] == 1 and got[3]["n_plastic"] == n
    h.newton()
    got = h.device(to_device(eps))
    assert got[3]["n_not_converged"] == 0 and 2 <= got[3]["max_local_iters"] <= 25
    check("after the cap is lifted", law, prm, got, ps.update(law, eps, np.zeros_like(eps), prm))
    h.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_library_refuses():
    lib = _lib.load()

    def refused(law, p, words):
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 8, 0)
        assert words in err(lib), (words, err(lib))

    good = [E, NU, SIG0, 1.0, 0.0]
    for k, v, words in ((0, 0.0, "E must be > 0"), (1, 1.0, "nu must lie in (-1, 1)"), (2, 0.0, "sig0 must be > 0"), (3, 0.0, "the shear weight q must be > 0"),
                        (4, 0.5, "tangent must be 0"), (2, float("nan"), "sig0 must be finite")):
        p = list(good)
        p[k] = v
        refused(23, p, words)
    refused(23, good[:4], "expects 5 parameters")
    rk = ps.rankine_planes(FT, FC)
    refused(24, ps.polygon_params(E, NU, [rk[0], rk[3]]), "not symmetric under the exchange of the principal stresses")
    refused(24, ps.polygon_params(E, NU, [(1.0, 1.0, 0.0)]), "d must be > 0")
    refused(24, ps.polygon_params(E, NU, [(0.0, 0.0, 1.0)]), "has a zero normal")
    p = ps.polygon_params(E, NU, rk)
    p[2] = 5.0
    refused(24, p, "the number of half-planes M must be an integer")
    from dolfinx_materials_amd.gradient import gauss_points_hex

    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    for kind in ("quadratic_c", "rankine"):
        law, prm = KINDS[kind]
        h = Handle(law, 8, prm)
        # the displacement forms: the mesh gradient kernels evaluate 6-wide strains or F, never this law's 3-wide strain
        u, fl, ct = np.zeros(24), np.zeros((8, 3)), np.zeros((8, 9))
        rows, st = np.arange(8, dtype=np.int64), _lib.Stats()
        for fused in (1, 0):
            h.option("fused_gradient", fused)
            rcs = (lib.dxm_integrate_displacement(h.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
                   lib.dxm_integrate_displacement_rows(h.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
                   lib.dxm_integrate_displacement_device(h.h, mesh, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
            for rc in rcs:
                assert rc < 0 and "3-wide strain" in err(lib), err(lib)
        for layout in (1, 2, 3):
            assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and "3x3 block of 9 entries" in err(lib)
        frame = np.eye(3)
        assert lib.dxm_set_frame(h.h, frame.ctypes.data) < 0 and "a material frame changes nothing" in err(lib)
        field = np.full(8, 1.0)
        assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "per-point parameter fields" in err(lib)
        assert lib.dxm_kernel_name(h.h) == f"plane_stress_kernel<{law - 23}".encode()
        ep = h.state(_lib.S0)
        assert not ep.any()
        assert lib.dxm_get_state(h.h, _lib.S0, 1, ep.ctypes.data) < 0      # one field, the hidden one
        h.close()
    lib.dxm_mesh_destroy(mesh)
