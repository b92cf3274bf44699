"""GPU: plane-stress J2 plasticity with isotropic hardening (DXM_LAW_PS_J2_LINEAR = 30, DXM_LAW_PS_J2_VOCE = 31;
``plane_stress_j2_kernel<hard>``) through the C ABI (ctypes): against the committed 50-digit values and the numpy restatement
``plane_stress_j2_ref``, the grids and the routes of the library against each other bit for bit, constructed tiles, histories, a
law-23 handle at ``H = 0``, the status record and every refusal.

Bound on stress (in sig0), tangent (in E) and state (p and epsp, in sig0 / E): 16 x what the restatement deviates from the 50-digit
values by (``plane_stress_j2_ref.MEASURED``, pinned by ``tests/test_plane_stress_j2_cpu.py``), floored at 2e-14 -- linear
2.1e-11 / 1.8e-13 / 3.2e-11, Voce 7.7e-12 / 3.9e-12 / 6.9e-11.  The far overshoots set the figures; the margin is for the kernel's own
division and square-root sequences, its ``exp`` and the one FMA of the linear ``R``.

Measured on an MI355X (kernel against the fixture, largest over N, cases and both increments): see DESIGN.md, "Plane-stress J2
plasticity with isotropic hardening"."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd.plane_stress import PlaneStressvonMisesHardening

import plane_stress_j2_ref as pj
import tile_loop_cases as tc
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

E, NU = pj.E, pj.NU
GUARD, SENTINEL = 64, -7.25


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


class Handle:
    """one dxm_material of law 30 / 31 (or of law 23, for the comparison at H = 0), driven through ctypes alone"""

    def __init__(self, law, n, prm):
        p = [float(v) for v in prm]
        self.lib, self.n, self.law, self.prm = _lib.load(), n, law, p
        self.h = self.lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        self.mine = law in (pj.J2_LINEAR, pj.J2_VOCE)
        assert self.lib.dxm_tangent_size(self.h) == 9 and self.lib.dxm_algorithmic_bytes(self.h) == (184 if self.mine else 168)

    def stats(self):
        st = _lib.Stats()
        rc = self.lib.dxm_get_stats(self.h, C.byref(st))
        assert rc >= 0, err(self.lib)
        return st.as_dict()

    def state(self, which=_lib.S1):
        """(n, 4): p, epsp -- or the (n, 3) hidden plastic strain of a law-23 handle"""
        if not self.mine:
            a = np.full((self.n, 3), np.nan)
            assert self.lib.dxm_get_state(self.h, which, 0, a.ctypes.data) == 0, err(self.lib)
            return a
        p, ep = np.full((self.n, 1), np.nan), np.full((self.n, 3), np.nan)
        assert self.lib.dxm_get_state(self.h, which, 0, p.ctypes.data) == 0, err(self.lib)
        assert self.lib.dxm_get_state(self.h, which, 1, ep.ctypes.data) == 0, err(self.lib)
        return np.concatenate([p, ep], axis=1)

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
        f, c, isv, st = np.full((self.n, 3), np.nan), np.full((self.n, 9), np.nan), np.full((self.n, 4), np.nan), _lib.Stats()
        rc = self.lib.dxm_integrate(self.h, eps.ctypes.data, 0.0, f.ctypes.data, isv.ctypes.data, c.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        state = self.state()
        assert np.array_equal(isv.view(np.uint64), state.view(np.uint64))      # the state array of the call is the state of s1
        return f, c, state, st.as_dict()

    def advance(self):
        assert self.lib.dxm_advance(self.h) == 0, err(self.lib)

    def newton(self, maxit=25, rtol=1e-14):
        assert self.lib.dxm_set_newton(self.h, maxit, rtol) == 0, err(self.lib)

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def close(self):
        self.lib.dxm_destroy(self.h)


def same(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def wanted(r):
    return dict(stress=r["stress"], tangent=r["tangent"], state=np.concatenate([r["p"][:, None], r["epsp"]], axis=1))


def deviations(prm, got, want):
    s, Em = prm[2], prm[0]
    return (np.abs(got[0] - want["stress"]).max() / s, np.abs(got[1] - want["tangent"]).max() / Em, np.abs(got[2] - want["state"]).max() / (s / Em))


def check(tag, law, prm, got, want):
    dev, bound = deviations(prm, got, want), pj.gpu_bounds(law)
    print(f"plane-stress J2 {tag}: stress {dev[0]:.3e} (bound {bound[0]:.2e})  tangent {dev[1]:.3e} ({bound[1]:.2e})  state {dev[2]:.3e} ({bound[2]:.2e})")
    assert all(d <= b for d, b in zip(dev, bound)), (tag, dev, bound)
    return dev


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4161])
@pytest.mark.parametrize("law", [pj.J2_LINEAR, pj.J2_VOCE], ids=["linear", "voce"])
def test_fixture_parity_over_both_increments_carried_on_the_device(law, N):
    kat = pj.load_kat()
    ran, worst = 0, np.zeros(3)
    for tag, claw, prm, eps, incs in pj.kat_cases(kat):
        if claw != law:
            continue
        idx = np.arange(N) % len(eps[0])
        h = Handle(law, N, prm)
        for k in range(2):
            got = h.device(to_device(eps[k][idx]))
            want = dict(stress=incs[k]["stress"][idx], tangent=incs[k]["tangent"][idx],
                        state=np.concatenate([incs[k]["p"][idx, None], incs[k]["epsp"][idx]], axis=1))
            worst = np.maximum(worst, check(f"fixture {tag} N={N} increment {k + 1}", law, prm, got, want))
            st = got[3]
            assert st["n_plastic"] == int(incs[k]["plastic"][idx].sum()) and st["n_not_converged"] == 0 and st["n_nan"] == 0 and st["n_points"] == N
            assert st["max_local_iters"] <= 9
            if N >= 63:
                assert st["max_local_iters"] >= 2
            ct = got[1].reshape(N, 3, 3)
            assert np.array_equal(ct, np.swapaxes(ct, 1, 2))           # six distinct numbers per point
            h.advance()
        h.close()
        ran += 1
    print(f"plane-stress J2 law {law} N={N}: kernel against the fixture, largest: stress {worst[0]:.3e}  tangent {worst[1]:.3e}  state {worst[2]:.3e}")
    assert ran == (3 if law == pj.J2_LINEAR else 1)


# ---- the tile loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["linear_H5e3", "voce"])
def test_tile_loop_at_one_workgroup_per_cu_equals_the_shipped_grid(case):
    import torch

    law, prm = pj.CASES[case]
    num_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    N = tc.size_for(num_cu)
    eps = pj.random_trials(prm, N, seed=21, lo=0.3, hi=50.0)
    eps2 = eps * np.random.default_rng(22).uniform(0.2, 1.6, (N, 1))
    a, b = Handle(law, N, prm), Handle(law, N, prm)
    b.option("blocks_per_cu", 1)
    assert tc.passes(N, num_cu, 1) == 4 and N % 64 != 0          # four passes, the last ragged
    for k, e in enumerate((eps, eps2)):
        e_dev = to_device(e)
        ga, gb = a.device(e_dev), b.device(e_dev)
        assert same(ga, gb), (case, k)
        assert 0.2 * N < ga[3]["n_plastic"] < 0.95 * N and ga[3]["n_nan"] == 0 and ga[3]["n_not_converged"] == 0
        if k == 0:   # a sample of the late passes against the restatement
            idx = tc.reference_sample(N, num_cu)
            want = pj.update(law, e[idx], np.zeros((len(idx), 3)), np.zeros(len(idx)), prm)
            check(f"tile loop {case}", law, prm, tuple(x[idx] for x in ga[:3]), wanted(want))
        a.advance()
        b.advance()
    a.close()
    b.close()


# ---- constructed tiles --------------------------------------------------------------------------------------------------------------------
def constructed(prm, seed):
    """tiles of 64: wholly elastic | wholly yielded | alternating lanes | one yielded lane, lane 0 | one yielded lane, lane 63 | a ragged
    tile of 17, mixed.  The yielded points overshoot by 1.01 ... 1e4: the Newton trip counts diverge within a wave"""
    pattern = np.concatenate([np.zeros(64, bool), np.ones(64, bool), np.arange(64) % 2 == 1, np.arange(64) == 0, np.arange(64) == 63,
                              np.arange(17) % 3 == 0])
    n = len(pattern)
    el = pj.random_trials(prm, n, seed, lo=0.05, hi=0.95)
    pl = pj.random_trials(prm, n, seed + 1, lo=1.01, hi=1e4)
    return np.where(pattern[:, None], pl, el), pattern


@pytest.mark.parametrize("case", list(pj.CASES))
def test_constructed_tiles_and_the_guard_cells(case):
    law, prm = pj.CASES[case]
    eps, pattern = constructed(prm, seed=31)
    n = len(eps)
    assert n == 5 * 64 + 17
    h = Handle(law, n, prm)
    got = h.device(to_device(eps))                      # (the guard cells are checked by Handle.device)
    want = pj.update(law, eps, np.zeros_like(eps), np.zeros(n), prm)
    assert np.array_equal(want["plastic"], pattern)
    check(f"constructed tiles {case}", law, prm, got, wanted(want))
    ref = pj.stats(want)
    assert got[3]["n_plastic"] == int(pattern.sum()) and got[3]["n_nan"] == 0 and got[3]["n_not_converged"] == 0
    assert abs(got[3]["max_local_iters"] - ref["max_local_iters"]) <= 1 and got[3]["max_local_iters"] >= 3
    # an elastic point's state: the zero bits it read; its tangent: C
    el = ~pattern
    assert not got[2][el].any() and np.array_equal(got[1][el], want["tangent"][el])
    h.close()


# ---- histories ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pj.CASES))
def test_load_unload_reload_and_the_bits_of_points_that_stay_elastic(case):
    law, prm = pj.CASES[case]
    R, _ = pj.hardening(law, prm)
    n = 1000
    load = pj.random_trials(prm, n, seed=41, lo=0.4, hi=6.0)
    steps = [load, 0.55 * load, 1.4 * load + pj.random_trials(prm, n, seed=42, lo=0.1, hi=0.5)]
    h = Handle(law, n, prm)
    state = np.zeros((n, 4))
    for k, eps in enumerate(steps):
        got = h.device(to_device(eps))
        want = pj.update(law, eps, state[:, 1:], state[:, 0], prm)
        check(f"history {case} step {k}", law, prm, got, wanted(want))
        near = np.abs(want["overshoot"] - 1.0) < 1e-9                       # on the surface: either side may count
        assert abs(got[3]["n_plastic"] - int(want["plastic"].sum())) <= int(near.sum())
        # points that stay elastic keep the bits of p and epsp they had
        before = h.state(_lib.S0)
        el = ~want["plastic"] & ~near
        assert el.sum() > 50 and np.array_equal(got[2][el].view(np.uint64), before[el].view(np.uint64))
        if k == 1:   # the unloading step: most points stay elastic, many from a plastic strain that is not zero
            assert el.sum() > 0.6 * n and (before[el, 0] > 0).sum() > 0.3 * n
        # the yielded points end on their surface, p never decreases
        seq = pj.seq_of(got[0])
        pl = want["plastic"] & ~near
        assert np.abs(seq[pl] - R(got[2][pl, 0])).max(initial=0.0) <= 1e-11 * prm[2] * max(1.0, want["overshoot"].max())
        assert (got[2][:, 0] >= before[:, 0]).all()
        h.advance()
        state = got[2]                       # the kernel's own state carries on, as the handle's does
    h.close()


# ---- host forms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["linear_H5e3", "voce"])
def test_host_buffer_form_equals_the_device_form_bit_for_bit(case):
    law, prm = pj.CASES[case]
    n = 100_003
    eps = pj.random_trials(prm, n, seed=61, lo=0.3, hi=20.0)
    h = Handle(law, n, prm)
    base = h.device(to_device(eps))
    assert same(h.host(eps), base)
    h.option("max_chunks", 3)
    assert same(h.host(eps), base)
    h.option("pipeline", 0)
    assert same(h.host(eps), base)
    h.close()


# ---- the status record ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["linear_H5e3", "voce"])
def test_one_nan_strain_counts_once_and_leaves_its_neighbours_alone(case):
    law, prm = pj.CASES[case]
    n = 777
    eps = pj.random_trials(prm, n, seed=81, lo=0.3, hi=5.0)
    h = Handle(law, n, prm)
    first = h.device(to_device(0.8 * eps))               # a state that is not zero
    h.advance()
    base = h.device(to_device(eps))
    bad = eps.copy()
    bad[300, 1] = np.nan
    got = h.device(to_device(bad))
    ok = np.delete(np.arange(n), 300)
    assert got[3]["n_nan"] == 1 and base[3]["n_nan"] == 0 and np.isnan(got[0][300]).any()
    assert all(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)) for a, b in zip(got[:3], base[:3]))
    assert np.array_equal(got[2][300].view(np.uint64), first[2][300].view(np.uint64))      # the state of the point: the bits it read
    bad[300, 1] = np.inf
    got = h.device(to_device(bad))
    assert got[3]["n_nan"] == 1 and got[3]["n_not_converged"] == 0
    assert first[3]["n_plastic"] > 100 and first[2][:, 0].max() > 0
    h.close()


def test_a_capped_newton_counts_its_points():
    law, prm = pj.CASES["voce"]
    n = 640
    eps = pj.random_trials(prm, n, seed=91, lo=50.0, hi=1e4)
    h = Handle(law, n, prm)
    h.newton(maxit=1)
    got = h.device(to_device(eps))
    want = pj.update(law, eps, np.zeros_like(eps), np.zeros(n), prm, maxit=1)
    assert want["not_converged"].sum() >= n // 2
    # (a point whose residual after its one step sits at the tolerance may fall on either side)
    assert abs(got[3]["n_not_converged"] - int(want["not_converged"].sum())) <= 2 and got[3]["max_local_iters"] == 1 and got[3]["n_plastic"] == n
    h.newton()
    got = h.device(to_device(eps))
    assert got[3]["n_not_converged"] == 0 and 2 <= got[3]["max_local_iters"] <= 9
    check("after the cap is lifted", law, prm, got, wanted(pj.update(law, eps, np.zeros_like(eps), np.zeros(n), prm)))
    h.close()


# ---- H = 0: the quadratic yield set with q = 3/2 ---------------------------------------------------------------------------------------------------
def test_at_h_zero_the_kernel_agrees_with_a_law_23_handle():
    law, prm = pj.CASES["linear_H0"]
    n = 2000
    a, b = Handle(law, n, prm), Handle(_lib.LAW_PS_QUADRATIC, n, [E, NU, prm[2], 1.5, 1.0])
    for k, eps in enumerate(pj.increments(prm, n, seed=95)):
        e_dev = to_device(eps)
        ga, gb = a.device(e_dev), b.device(e_dev)
        want = dict(stress=gb[0], tangent=gb[1], state=gb[2])
        check(f"H = 0 against law 23, step {k}", law, prm, (ga[0], ga[1], ga[2][:, 1:]), want)
        assert ga[3]["n_plastic"] == gb[3]["n_plastic"] > (n // 4 if k != 1 else 0)       # (step 1 unloads: few points re-yield)
        a.advance()
        b.advance()
    a.close()
    b.close()


# ---- through the Python class ---------------------------------------------------------------------------------------------------------------------
def test_the_material_class_and_the_axial_strain():
    law, prm = pj.CASES["voce"]
    m = PlaneStressvonMisesHardening(E, NU, jm.VoceHardening(*prm[2:]))
    n = 300
    m.set_data_manager(n)
    assert m.kernel_name.startswith("plane_stress_j2_kernel<2") and m.internal_state_variables == {"p": 1, "epsp": 3}
    state = np.zeros((n, 4))
    for k, e in enumerate(pj.increments(prm, n, seed=120)):
        sig, isv, Ct = m.integrate(e)
        want = pj.update(law, e, state[:, 1:], state[:, 0], prm)
        got = (np.asarray(sig), np.asarray(Ct).reshape(n, 9), np.asarray(isv))
        check(f"material, increment {k + 1}", law, prm, got, wanted(want))
        m.data_manager.update()
        s0 = m.get_initial_state_dict()
        assert np.array_equal(np.asarray(s0["Strain"]), e) and np.array_equal(np.asarray(s0["Stress"]), got[0])
        assert np.array_equal(np.asarray(s0["epsp"]), got[2][:, 1:])
        ezz = conventions.plane_stress_axial_strain(E, NU, got[0], got[2][:, 1:])
        assert np.abs(ezz - pj.axial_strain(E, NU, want["stress"], want["epsp"])).max() <= 2 * pj.gpu_bounds(law)[2] * prm[2] / E
        state = got[2]
    m.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_library_refuses():
    lib = _lib.load()
    from dolfinx_materials_amd.gradient import gauss_points_hex

    for law, p, words in ((30, [E, 0.5, 250.0, 5e3], "invalid elastic constants"), (30, [E, NU, 250.0], "expects 4 parameters"),
                          (31, [-1.0, NU, 350.0, 500.0, 1e3], "invalid elastic constants"), (31, [E, NU, 350.0, 500.0], "expects 5 parameters")):
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 8, 0) and words in err(lib), err(lib)
    for law in (29, 32):
        assert not lib.dxm_create(law, (C.c_double * 4)(E, NU, 250.0, 5e3), 4, 8, 0) and f"unknown law id {law}" in err(lib), err(lib)
    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    for case in ("linear_H5e3", "voce"):
        law, prm = pj.CASES[case]
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
            assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and "3x3 block of 9 entries" in err(lib), err(lib)
        assert lib.dxm_set_tangent_layout(h.h, 0) == 0
        frame = np.eye(3)
        assert lib.dxm_set_frame(h.h, frame.ctypes.data) < 0 and "this law is isotropic: a material frame changes nothing" in err(lib), err(lib)
        field = np.full(8, 1.0)
        assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "not served for plane-stress J2 plasticity" in err(lib), err(lib)
        assert lib.dxm_set_external_state_uniform(h.h, 0, 300.0) < 0 and "has no external state variable" in err(lib), err(lib)
        assert lib.dxm_set_external_state(h.h, 0, field.ctypes.data) < 0 and "has no external state variable" in err(lib), err(lib)
        assert lib.dxm_kernel_name(h.h) == f"plane_stress_j2_kernel<{law - 29}".encode()
        assert not h.state(_lib.S0).any()
        bad = np.zeros((8, 3))
        assert lib.dxm_get_state(h.h, _lib.S0, 2, bad.ctypes.data) < 0          # two fields
        h.close()
    lib.dxm_mesh_destroy(mesh)


def test_a_custom_hardening_build_refuses_the_two_laws_with_their_own_sentence():
    """(the expressions are those of tests/test_custom_hardening.py: one build in the cache serves every file that asks)"""
    hd = jm.CustomHardening("sig0 + K * (pow(p + p0, n) - pow(p0, n))", "K * n * pow(p + p0, n - 1.0)", sig0=250.0, K=600.0, n=0.3, p0=1e-3)
    lib = _lib.load_custom(hd.expr_R, hd.expr_dR)
    assert lib.dxm_has_custom_hardening() == 1
    for law, p in ((30, [E, NU, 250.0, 5e3]), (31, [E, NU, 350.0, 500.0, 1e3])):
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 64, 0)
        msg = err(lib)
        assert "plane-stress J2 plasticity takes the stock hardening laws only" in msg and "not by a custom-hardening build" in msg, msg
        assert _lib.law_blocks(law, lib).tangent_width == 9
