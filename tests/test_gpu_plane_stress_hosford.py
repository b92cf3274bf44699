"""GPU: plane-stress Hosford plasticity (DXM_LAW_PS_HOSFORD = 33; ``plane_stress_hosford_kernel<tangent>``) through the C ABI (ctypes):
against the committed 50-digit values and the numpy restatement ``plane_stress_hosford_ref``, an a = 2 handle against a law-23 handle,
the tile loop past its first pass on tiles built from fixture rows, a capped iteration, the Python class over two increments and from a
prestress, the host forms against the device form bit for bit, and every refusal on a live handle.

Bound on stress (in sig0), tangent (in E) and state (in sig0 / E), per tangent mode: 16 x what the restatement deviates from the 50-digit
values by (``plane_stress_hosford_ref.MEASURED``, pinned by ``tests/test_plane_stress_hosford_cpu.py``), floored at 2e-14 --
tangent = 0: 2.6e-14 / 2e-14 / 1.04e-12, tangent = 1: 2.6e-14 / 3.84e-13 / 1.04e-12."""
import ctypes as C

import numpy as np
import pytest

from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.plane_stress import PlaneStressHosford

import plane_stress_hosford_ref as psh
from helpers import to_device
from test_gpu_plane_stress import Handle as _Handle
from test_gpu_plane_stress import err, same

pytestmark = pytest.mark.gpu

E, NU, SIG0 = 70e3, 0.2, 30.0
KAT = psh.load_kat()
CASES = {c[0]: c for c in psh.kat_cases(KAT)}
NLOOP = 206_147       # blocks_per_cu = 1: four passes of the tile loop on 256 CUs, a ragged last tile


class Handle(_Handle):
    def __init__(self, n, prm, law=psh.LAW):
        super().__init__(law, n, prm)
        self.tangent = self.prm[4] != 0

    def rows(self, eps, rows, top):
        """the rows form: point i of the launch goes to row rows[i] of the bases"""
        f, c, st = np.full((top, 3), np.nan), np.full((top, 9), np.nan), _lib.Stats()
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        rc = self.lib.dxm_integrate_rows(self.h, eps.ctypes.data, 0.0, f.ctypes.data, c.ctypes.data, rows.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()


def check(tag, prm, got, want, tangent):
    dev = (np.abs(got[0] - want["stress"]).max() / prm[2], np.abs(got[1] - want["tangent"]).max() / prm[0],
           np.abs(got[2] - want["state"]).max() / (prm[2] / prm[0]))
    bound = psh.gpu_bounds(tangent)
    print(f"plane-stress Hosford {tag}: stress {dev[0]:.3e} (bound {bound[0]:.2e})  tangent {dev[1]:.3e} ({bound[1]:.2e})  state {dev[2]:.3e} ({bound[2]:.2e})")
    assert all(d <= b for d, b in zip(dev, bound)), (tag, dev, bound)


def wanted(tag, k, tangent, idx):
    _, prm, eps, incs = CASES[tag]
    T = incs[k]["tangent"] if tangent else np.tile(psh.stiffness(prm[0], prm[1]).ravel(), (len(eps[k]), 1))
    return dict(stress=incs[k]["stress"][idx], tangent=T[idx], state=incs[k]["state"][idx])


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("tangent", [0, 1])
def test_fixture_parity_over_both_increments(tangent, N):
    for tag, (_, prm, eps, incs) in CASES.items():
        prm = prm.copy()
        prm[4] = tangent
        idx = (np.arange(N) * 5 + 3 * N) % len(eps[0])          # the sizes walk through different rows
        h = Handle(N, prm)
        for k in range(2):
            if k == 1:
                h.set_state(incs[0]["state"][idx])              # the second increment starts from the first one's stored state
            got = h.device(to_device(eps[k][idx]))
            check(f"fixture {tag} tangent={tangent} N={N} increment {k + 1}", prm, got, wanted(tag, k, tangent, idx), tangent)
            st = got[3]
            assert st["n_plastic"] == int(incs[k]["plastic"][idx].sum()) and st["n_not_converged"] == 0 and st["n_nan"] == 0 and st["n_points"] == N
            assert st["max_local_iters"] <= 16
        h.close()


@pytest.mark.parametrize("tangent", [0, 1])
def test_an_exponent_of_two_is_law_23_at_q_three_halves(tangent):
    _, prm, eps, incs = CASES["a2_nu20"]
    n = len(eps[0])
    mine, law23 = Handle(n, [E, NU, SIG0, 2.0, tangent]), Handle(n, [E, NU, SIG0, 1.5, tangent], law=_lib.LAW_PS_QUADRATIC)
    for k in range(2):
        if k == 1:
            mine.set_state(incs[0]["state"])
            law23.set_state(incs[0]["state"])
        e_dev = to_device(eps[k])
        a, b = mine.device(e_dev), law23.device(e_dev)
        check(f"a = 2 against law 23, tangent={tangent}, increment {k + 1}", mine.prm, a, dict(stress=b[0], tangent=b[1], state=b[2]), tangent)
        assert a[3]["n_plastic"] == b[3]["n_plastic"] == int(incs[k]["plastic"].sum())
    mine.close()
    law23.close()


# ---- the tile loop -----------------------------------------------------------------------------------------------------------------
def loop_rows(n_rows, plastic):
    """NLOOP points, tile by tile of 64 from fixture rows: wholly elastic | wholly yielded | alternating lanes | every row in turn"""
    el, pl = np.flatnonzero(~plastic), np.flatnonzero(plastic)
    i = np.arange(NLOOP)
    tile, lane = i // 64, i % 64
    kind = tile % 4
    alt = np.where(lane % 2 == 1, pl[(i // 2) % len(pl)], el[(i // 2) % len(el)])
    return np.where(kind == 0, el[i % len(el)], np.where(kind == 1, pl[(i + tile) % len(pl)], np.where(kind == 2, alt, (i + tile) % n_rows)))


@pytest.mark.parametrize("tangent", [0, 1])
def test_tile_loop_at_one_workgroup_per_cu_on_tiles_of_fixture_rows(tangent):
    _, prm, eps, incs = CASES["a10_nu20"]
    prm = prm.copy()
    prm[4] = tangent
    idx = loop_rows(len(eps[0]), incs[0]["plastic"])
    e = np.ascontiguousarray(eps[0][idx])
    e_dev = to_device(e)
    a, b = Handle(NLOOP, prm), Handle(NLOOP, prm)
    b.option("blocks_per_cu", 1)                       # a wave takes four tiles and a ragged last one
    ga, gb = a.device(e_dev), b.device(e_dev)
    assert same(ga, gb)
    check(f"tile loop tangent={tangent}", prm, gb, wanted("a10_nu20", 0, tangent, idx), tangent)
    ref = psh.stats(psh.update(e, np.zeros_like(e), prm), tangent)
    for key in ("n_plastic", "n_not_converged", "n_nan"):
        assert gb[3][key] == ref[key], (key, gb[3], ref)
    assert ref["n_plastic"] == int(incs[0]["plastic"][idx].sum()) and 0.3 * NLOOP < ref["n_plastic"] < 0.8 * NLOOP and ref["n_not_converged"] == 0
    assert abs(gb[3]["max_local_iters"] - ref["max_local_iters"]) <= 1
    # an elastic point's state: the zero bits it read; its tangent: C
    el = ~incs[0]["plastic"][idx]
    assert not gb[2][el].any() and np.array_equal(gb[1][el], np.tile(psh.stiffness(E, NU).ravel(), (int(el.sum()), 1)))
    a.close()
    b.close()


# ---- the cap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tangent", [0, 1])
def test_a_capped_iteration_is_counted_and_stays_admissible(tangent):
    _, prm, eps, incs = CASES["a10_nu20"]
    prm = prm.copy()
    prm[4] = tangent
    n = len(eps[0])
    h = Handle(n, prm)
    h.newton(maxit=1)
    got = h.device(to_device(eps[0]))
    want = psh.update(eps[0], np.zeros_like(eps[0]), prm, maxit=1)
    assert want["not_converged"].sum() >= n // 2
    assert abs(got[3]["n_not_converged"] - int(want["not_converged"].sum())) <= 2 and got[3]["max_local_iters"] == 1
    assert got[3]["n_plastic"] == int(incs[0]["plastic"].sum()) and got[3]["n_nan"] == 0
    assert all(np.isfinite(x).all() for x in got[:3])
    assert (psh.phi(got[0], prm[3]) <= SIG0 * (1 + 1e-12)).all()
    h.newton()
    got = h.device(to_device(eps[0]))
    assert got[3]["n_not_converged"] == 0 and 2 <= got[3]["max_local_iters"] <= 16
    check(f"after the cap is lifted, tangent={tangent}", prm, got, wanted("a10_nu20", 0, tangent, np.arange(n)), tangent)
    h.close()


# ---- the Python class --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tangent", ["elastic", "consistent"])
def test_two_increments_through_integrate_and_update(tangent):
    _, prm, eps, incs = CASES["a10_nu20"]
    T = int(tangent == "consistent")
    m = PlaneStressHosford(E=E, nu=NU, sig0=SIG0, a=10, tangent=tangent)         # the demo's constructor call
    n = len(eps[0])
    m.set_data_manager(n)
    assert set(m.get_initial_state_dict()) == {"Strain", "Stress"}
    state = np.zeros((n, 3))
    p = prm.copy()
    p[4] = T
    for k in range(2):
        sig, isv, Ct = m.integrate(eps[k])
        want = psh.update(eps[k], state, p)                # the class carries its own state on: the restatement follows it
        check(f"class {tangent} increment {k + 1}", p, (np.asarray(sig), np.asarray(Ct).reshape(n, 9), want["state"]), want, T)
        assert m.last_stats["n_plastic"] == int(incs[k]["plastic"].sum()) and m.last_stats["n_not_converged"] == 0
        if k == 0:
            check(f"class {tangent} against the fixture", p, (np.asarray(sig), np.asarray(Ct).reshape(n, 9), incs[0]["state"]), wanted("a10_nu20", 0, T, np.arange(n)), T)
        m.data_manager.update()
        state = want["state"]
    s0 = m.get_initial_state_dict()
    assert np.array_equal(np.asarray(s0["Strain"]), eps[1]) and np.array_equal(np.asarray(s0["Stress"]), np.asarray(sig))
    m.close()


def test_prestress_through_set_initial_state_dict():
    m = PlaneStressHosford(E=E, nu=NU, sig0=SIG0, a=10)
    prm = m.behavior.params()
    n = 500
    m.set_data_manager(n)
    pre = psh.sample_admissible(prm, n, np.random.default_rng(71)) * 0.8
    m.set_initial_state_dict({"Stress": pre})                        # a zero strain
    epsp = -(pre @ psh.compliance(E, NU).T)
    rng = np.random.default_rng(72)
    v = rng.normal(size=(n, 3))
    eps = (v * (SIG0 / psh.phi(v, 10.0) * rng.uniform(0.2, 3.0, n))[:, None]) @ psh.compliance(E, NU).T
    sig, _, Ct = m.integrate(eps)
    want = psh.update(eps, epsp, prm)
    assert 0.2 * n < want["plastic"].sum() < 0.95 * n
    check("prestress", prm, (np.asarray(sig), np.asarray(Ct).reshape(n, 9), want["state"]), want, 0)
    first = np.asarray(sig).copy()
    m.data_manager.revert()                                          # the increment is rejected: s1 <- s0
    back = m.get_final_state_dict()
    assert np.array_equal(np.asarray(back["Stress"]), pre) and not np.asarray(back["Strain"]).any()
    sig2, _, _ = m.integrate(eps)
    assert np.array_equal(np.asarray(sig2), first)
    m.close()


# ---- host forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tangent", [0, 1])
def test_host_buffer_and_rows_forms_equal_the_device_form_bit_for_bit(tangent):
    _, prm, eps, incs = CASES["a20_nu20"]
    prm = prm.copy()
    prm[4] = tangent
    n = 20_003
    idx = (np.arange(n) * 11) % len(eps[0])
    e = np.ascontiguousarray(eps[0][idx])
    h = Handle(n, prm)
    base = h.device(to_device(e))
    assert same(h.host(e), base)
    h.option("max_chunks", 3)
    assert same(h.host(e), base)
    rows = np.random.default_rng(5).permutation(n + 17)[:n]
    f, c, st, stats = h.rows(e, rows, n + 17)
    assert same((np.ascontiguousarray(f[rows]), np.ascontiguousarray(c[rows]), st, stats), base)
    untouched = np.setdiff1d(np.arange(n + 17), rows)
    assert np.isnan(f[untouched]).all() and np.isnan(c[untouched]).all()
    h.close()


def test_one_nan_strain_counts_once_and_is_not_projected():
    _, prm, eps, _ = CASES["a10_nu20"]
    h = Handle(len(eps[0]), prm)
    base = h.device(to_device(eps[0]))
    bad = eps[0].copy()
    bad[100, 1] = np.nan
    got = h.device(to_device(bad))
    ok = np.delete(np.arange(len(bad)), 100)
    assert got[3]["n_nan"] == 1 and base[3]["n_nan"] == 0 and np.isnan(got[0][100]).any() and not got[2][100].any()
    assert got[3]["n_plastic"] in (base[3]["n_plastic"], base[3]["n_plastic"] - 1)
    assert all(np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)) for a, b in zip(got[:3], base[:3]))
    h.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_what_the_library_refuses():
    lib = _lib.load()

    def refused(p, words):
        assert not lib.dxm_create(33, (C.c_double * len(p))(*p), len(p), 8, 0)
        assert words in err(lib), (words, err(lib))

    good = [E, NU, SIG0, 10.0, 0.0]
    for k, v, words in ((0, 0.0, "E must be > 0"), (1, 1.0, "nu must lie in (-1, 1)"), (2, 0.0, "sig0 must be > 0"),
                        (3, 1.5, "the exponent a must be >= 2"), (3, 101.0, "the exponent a must be <= 100"),
                        (4, 0.5, "tangent must be 0"), (3, float("nan"), "a must be finite")):
        p = list(good)
        p[k] = v
        refused(p, words)
    refused(good[:4], "expects 5 parameters")
    assert not lib.dxm_create(32, (C.c_double * 5)(*good), 5, 8, 0) and "unknown law id 32" in err(lib)
    assert not lib.dxm_create(34, (C.c_double * 5)(*good), 5, 8, 0) and "unknown law id 34" in err(lib)
    from dolfinx_materials_amd.gradient import gauss_points_hex

    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    h = Handle(8, good)
    u, fl, ct = np.zeros(24), np.zeros((8, 3)), np.zeros((8, 9))
    rows, st = np.arange(8, dtype=np.int64), _lib.Stats()
    for fused in (1, 0):
        h.option("fused_gradient", fused)
        rcs = (lib.dxm_integrate_displacement(h.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_rows(h.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_device(h.h, mesh, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
        for rc in rcs:
            assert rc < 0 and "plane-stress Hosford plasticity takes a 3-wide strain" in err(lib), err(lib)
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and "the plane-stress Hosford tangent is a 3x3 block of 9 entries" in err(lib)
    frame = np.eye(3)
    assert lib.dxm_set_frame(h.h, frame.ctypes.data) < 0 and "a material frame changes nothing" in err(lib)
    field = np.full(8, 1.0)
    assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "not served for plane-stress Hosford plasticity" in err(lib)
    assert lib.dxm_set_external_state_uniform(h.h, 0, 300.0) < 0 and "law 33 has no external state variable" in err(lib), err(lib)
    assert lib.dxm_kernel_name(h.h) == b"plane_stress_hosford_kernel<0"
    ep = h.state(_lib.S0)
    assert not ep.any()
    assert lib.dxm_get_state(h.h, _lib.S0, 1, ep.ctypes.data) < 0      # one field, the hidden one
    h.close()
    lib.dxm_mesh_destroy(mesh)
    with pytest.raises(ValueError, match="no packed tangent record"):
        PlaneStressHosford(E, NU, SIG0, 10, tangent_layout="sym")
