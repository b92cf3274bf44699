"""GPU: the plane-strain hypothesis (DXM_LAW_PE_ELASTIC_ISO = 26, DXM_LAW_PE_J2_LINEAR = 27, DXM_LAW_PE_J2_VOCE = 28;
``plane_strain_kernel<law>``) through the C ABI (ctypes): parity with the 6-wide oracle on the embedded input, restricted to the four
components; the 6-wide kernels of the same library on the same input; the grids and the routes of the library against each other
bit for bit; constructed tiles, histories, the status record, every refusal; and the reference's stand-alone sequence through
``HIPMaterial`` up to a known answer.

Bounds, of the field scale (``sig0`` for stresses, ``E`` for tangents, ``sig0 / E`` for strains): 1e-12 against the oracle (the
project's ``TIGHT`` of ``tests/test_gpu_parity.py`` for HIP against the oracle), 1e-13 against the 6-wide kernels (the same
arithmetic up to contraction and summation order).  Points with ``|f_trial| <= 1e-9 sig0`` are left out; the inputs are those of
``tests/test_plane_strain_cpu.py``, where the oracle alone is asserted to have none."""
import ctypes as C

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp

import plane_strain_ref as pe
import tile_loop_cases as tc
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

TIGHT, CROSS = 1e-12, 1e-13
GUARD, SENTINEL = 64, -7.25
SIZES = [1, 63, 64, 65, 4161]          # 4161: 65 tiles and a ragged one, crossing a workgroup of 4 waves many times
SIX_WIDE = {pe.ELASTIC: _lib.LAW_ELASTIC_ISO, pe.J2_LINEAR: _lib.LAW_J2_LINEAR, pe.J2_VOCE: _lib.LAW_J2_VOCE}
ALL_CASES = {"elastic": pe.ELASTIC_CASE, **pe.CASES}


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


class Handle:
    """one dxm_material of a plane-strain law (or, ``wide=6``, of its 6-wide law), driven through ctypes alone"""

    def __init__(self, law, n, prm, wide=4):
        p = [float(v) for v in prm]
        self.lib, self.n, self.law, self.prm, self.w = _lib.load(), n, law, p, wide
        self.has_state = law != pe.ELASTIC
        self.id = law if wide == 4 else SIX_WIDE[law]
        self.h = self.lib.dxm_create(self.id, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        if wide == 4:
            assert self.lib.dxm_tangent_size(self.h) == 16 and self.lib.dxm_algorithmic_bytes(self.h) == (272 if self.has_state else 192)

    def stats(self):
        st = _lib.Stats()
        rc = self.lib.dxm_get_stats(self.h, C.byref(st))
        assert rc >= 0, err(self.lib)
        return st.as_dict()

    def state(self, which=_lib.S1):
        """(n, 1 + w): p, then epsp"""
        if not self.has_state:
            return np.zeros((self.n, 0))
        p, ep = np.full((self.n, 1), np.nan), np.full((self.n, self.w), np.nan)
        assert self.lib.dxm_get_state(self.h, which, 0, p.ctypes.data) == 0, err(self.lib)
        assert self.lib.dxm_get_state(self.h, which, 1, ep.ctypes.data) == 0, err(self.lib)
        return np.concatenate([p, ep], axis=1)

    def device(self, eps_dev):
        """(stress, tangent, state of s1, stats); the output arrays end in guard cells that must keep their sentinel"""
        import torch

        w = self.w
        f = torch.full((self.n * w + GUARD,), SENTINEL, dtype=torch.float64, device=eps_dev.device)
        c = torch.full((self.n * w * w + GUARD,), SENTINEL, dtype=torch.float64, device=eps_dev.device)
        assert self.lib.dxm_integrate_device(self.h, eps_dev.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        f, c = to_host(f), to_host(c)
        assert (f[self.n * w:] == SENTINEL).all() and (c[self.n * w * w:] == SENTINEL).all()
        return f[: self.n * w].reshape(self.n, w), c[: self.n * w * w].reshape(self.n, w * w), self.state(), self.stats()

    def host(self, eps):
        w = self.w
        f, c, st = np.full((self.n, w), np.nan), np.full((self.n, w * w), np.nan), _lib.Stats()
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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def scales(prm):
    s = prm[2] if len(prm) > 2 else pe.SIG0
    return s, prm[0], s / prm[0]


def oracle(law, prm, eps4, ep6, p):
    """the embedded-and-restricted oracle: dict(stress, tangent (n, 16), state (n, 5) | (n, 0), plastic, skip, iters, raw)"""
    e6 = conventions.embed_plane_strain(eps4)
    n = len(e6)
    if law == pe.ELASTIC:
        sig, Ct = onp.elastic_iso(e6, prm[0], prm[1])
        return dict(stress=sig[:, :4], tangent=conventions.restrict_plane_strain_tangent(Ct).reshape(n, 16), state=np.zeros((n, 0)),
                    plastic=np.zeros(n, bool), skip=np.zeros(n, bool), iters=np.zeros(n, int), ep6=ep6, p=p)
    hard = onp.LinearHardening(prm[2], prm[3]) if law == pe.J2_LINEAR else onp.VoceHardening(prm[2], prm[3], prm[4])
    r = onp.j2_update(e6, ep6, p, prm[0], prm[1], hard)
    assert not r["sig"][:, 4:].any() and not r["epsp"][:, 4:].any()
    return dict(stress=r["sig"][:, :4], tangent=conventions.restrict_plane_strain_tangent(r["Ct"]).reshape(n, 16),
                state=np.concatenate([r["p"][:, None], r["epsp"][:, :4]], axis=1), plastic=r["plastic"],
                skip=np.abs(r["f_trial"]) <= pe.KINK * prm[2], iters=r["iters"], ep6=r["epsp"], p=r["p"])


def deviations(prm, got, want, keep=None):
    s, Em, e = scales(prm)
    keep = slice(None) if keep is None else keep
    d = [np.abs(got[0] - want["stress"])[keep].max() / s, np.abs(got[1] - want["tangent"])[keep].max() / Em]
    if got[2].shape[1]:
        d.append(np.abs(got[2] - want["state"])[keep].max() / e)
    return d


def check(tag, prm, got, want, bound=TIGHT):
    keep = ~want["skip"]
    assert want["skip"].mean() < 0.01
    dev = deviations(prm, got, want, keep)
    print(f"plane strain {tag}: stress / tangent / state " + " ".join(f"{d:.3e}" for d in dev) + f"  (bound {bound:.0e})")
    assert all(d <= bound for d in dev), (tag, dev)


# ---- parity with the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", list(ALL_CASES))
def test_parity_with_the_embedded_and_restricted_oracle_over_two_increments(case, N):
    law, prm = ALL_CASES[case]
    sig0, Em, _ = scales(prm)
    incs = [np.ascontiguousarray(e[:N]) for e in pe.increments(4161, sig0, Em)]      # the CPU test's inputs
    incs = [incs[0], incs[2]]                                          # load, then beyond it in another direction
    h = Handle(law, N, prm)
    ep6, p = np.zeros((N, 6)), np.zeros(N)
    for k, e in enumerate(incs):
        got = h.device(to_device(e))
        want = oracle(law, prm, e, ep6, p)
        check(f"{case} N={N} increment {k + 1}", prm, got, want)
        st = got[3]
        assert want["skip"].sum() == 0 and st["n_plastic"] == int(want["plastic"].sum()) and st["n_points"] == N
        assert st["n_not_converged"] == 0 and st["n_nan"] == 0
        assert st["max_local_iters"] == (int(want["iters"].max()) if law == pe.J2_VOCE else 0)
        ct = got[1].reshape(N, 4, 4)
        assert np.array_equal(bits(ct), bits(np.ascontiguousarray(ct.transpose(0, 2, 1))))       # exactly symmetric
        h.advance()
        ep6, p = want["ep6"], want["p"]
    if law != pe.ELASTIC and N >= 63:
        assert st["n_plastic"] > N // 4
    h.close()


# ---- the 6-wide kernels of the same library -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ALL_CASES))
def test_cross_check_with_the_6_wide_kernel_on_the_embedded_strains(case):
    law, prm = ALL_CASES[case]
    sig0, Em, _ = scales(prm)
    N = 4161
    h4, h6 = Handle(law, N, prm), Handle(law, N, prm, wide=6)
    for k, e in enumerate(pe.increments(N, sig0, Em, seed=60)):
        g4 = h4.device(to_device(e))
        g6 = h6.device(to_device(conventions.embed_plane_strain(e)))
        assert not g6[0][:, 4:].any()
        want = dict(stress=g6[0][:, :4], tangent=conventions.restrict_plane_strain_tangent(g6[1].reshape(N, 6, 6)).reshape(N, 16),
                    state=g6[2][:, :5], skip=np.zeros(N, bool))
        if g6[2].shape[1]:
            assert not g6[2][:, 5:].any()
        check(f"{case} against the 6-wide kernel, increment {k + 1}", prm, g4, want, CROSS)
        assert g4[3]["n_plastic"] == g6[3]["n_plastic"] and g4[3]["max_local_iters"] == g6[3]["max_local_iters"]
        assert g4[3]["n_not_converged"] == g6[3]["n_not_converged"] == 0 and g4[3]["n_nan"] == g6[3]["n_nan"] == 0
        h4.advance()
        h6.advance()
    h4.close()
    h6.close()


# ---- the tile loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["elastic", "linear_H5e3", "voce"])
def test_tile_loop_at_one_workgroup_per_cu_equals_the_shipped_grid(case):
    import torch

    law, prm = ALL_CASES[case]
    sig0, Em, _ = scales(prm)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    N = tc.size_for(cus)
    assert tc.passes(N, cus, 1) == 4
    a, b = Handle(law, N, prm), Handle(law, N, prm)
    b.option("blocks_per_cu", 1)
    incs = pe.increments(N, sig0, Em, seed=70)
    for k, e in enumerate((incs[0], incs[2])):
        e_dev = to_device(e)
        ga, gb = a.device(e_dev), b.device(e_dev)
        assert same(ga, gb), (case, k)
        assert ga[3]["n_nan"] == 0 and ga[3]["n_not_converged"] == 0
        if law != pe.ELASTIC:
            assert 0.2 * N < ga[3]["n_plastic"] < 0.95 * N
        if k == 0:   # a sample of the late passes against the oracle
            idx = tc.reference_sample(N, cus)
            want = oracle(law, prm, e[idx], np.zeros((len(idx), 6)), np.zeros(len(idx)))
            check(f"tile loop {case}", prm, tuple(x[idx] for x in ga[:3]), want)
        a.advance()
        b.advance()
    a.close()
    b.close()


# ---- constructed tiles --------------------------------------------------------------------------------------------------------------------------
def point_pair(law, prm):
    """one elastic and one yielded strain"""
    sig0, Em, _ = scales(prm)
    el = np.array([0.30, -0.10, 0.05, 0.20]) * (sig0 / Em)
    pl = np.array([2.10, -1.30, 0.00, 0.90]) * (sig0 / Em)
    return el, pl


@pytest.mark.parametrize("case", list(pe.CASES))
def test_constructed_tiles_are_bit_stable_across_positions(case):
    law, prm = pe.CASES[case]
    el, pl = point_pair(law, prm)
    tiles = [np.arange(64) == 0, np.arange(64) == 31, np.arange(64) == 63, np.zeros(64, bool), np.ones(64, bool), np.arange(17) % 3 == 0]
    pattern = np.concatenate(tiles)
    eps = np.where(pattern[:, None], pl, el)
    n = len(eps)
    h = Handle(law, n, prm)
    got = h.device(to_device(eps))
    want = oracle(law, prm, eps, np.zeros((n, 6)), np.zeros(n))
    assert np.array_equal(want["plastic"], pattern) and not want["skip"].any()
    check(f"constructed tiles {case}", prm, got, want)
    assert got[3]["n_plastic"] == int(pattern.sum()) and got[3]["n_nan"] == 0 and got[3]["n_not_converged"] == 0
    # the same input gives the same bits at every lane of every tile, whatever its neighbours do
    for mask in (pattern, ~pattern):
        first = np.flatnonzero(mask)[0]
        for a in got[:3]:
            assert (bits(a[mask]) == bits(a[first:first + 1])).all(), case
    # an elastic point: the zero state bits it read, the trial stress, the elastic block
    assert not got[2][~pattern].any()
    assert np.array_equal(got[1][~pattern][0].reshape(4, 4), got[1][~pattern][0].reshape(4, 4).T)
    h.close()


# ---- histories ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pe.CASES))
def test_load_unload_reload_revert_and_the_bits_of_points_that_stay_elastic(case):
    law, prm = pe.CASES[case]
    sig0, Em, _ = scales(prm)
    n = 1000
    steps = pe.increments(n, sig0, Em, seed=80)
    h = Handle(law, n, prm)
    ep6, p = np.zeros((n, 6)), np.zeros(n)
    shares = []
    for k, eps in enumerate(steps):
        got = h.device(to_device(eps))
        want = oracle(law, prm, eps, ep6, p)
        check(f"history {case} step {k}", prm, got, want)
        assert got[3]["n_plastic"] == int(want["plastic"].sum()) or want["skip"].any()
        before = h.state(_lib.S0)
        el = ~want["plastic"] & ~want["skip"]
        assert np.array_equal(bits(got[2][el]), bits(before[el]))        # elastic points keep the state bits they had
        if k == 1:   # the unloading step: every point is elastic, most from a plastic strain that is not zero
            assert el.sum() > 0.95 * n and (np.abs(before[el]).max(axis=1) > 0).sum() > 0.3 * n
            h.revert()                                                     # the increment is rejected: s1 <- s0
            assert np.array_equal(bits(h.state(_lib.S1)), bits(before))
            again = h.device(to_device(eps))
            assert same(again, got)
        shares.append(want["plastic"].mean())
        h.advance()
        ep6, p = want["ep6"], want["p"]
    assert 0.3 < shares[0] < 0.8 and shares[2] > shares[0]
    h.close()


# ---- host forms ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["elastic", "linear_H5e3", "voce"])
def test_host_buffer_form_equals_the_device_form_bit_for_bit(case):
    law, prm = ALL_CASES[case]
    sig0, Em, _ = scales(prm)
    n = 4161
    eps = pe.increments(n, sig0, Em, seed=90)[0]
    h = Handle(law, n, prm)
    base = h.device(to_device(eps))
    assert same(h.host(eps), base)                      # the default plan
    h.option("max_chunks", 3)
    assert same(h.host(eps), base)
    h.option("pipeline", 0)
    assert same(h.host(eps), base)
    if law != pe.ELASTIC:
        assert base[3]["n_plastic"] > n // 4
        isv = np.full((n, 5), np.nan)                   # the interleaved state rows of the host form
        f, c = np.empty((n, 4)), np.empty((n, 16))
        st = _lib.Stats()
        assert h.lib.dxm_integrate(h.h, eps.ctypes.data, 0.0, f.ctypes.data, isv.ctypes.data, c.ctypes.data, C.byref(st)) >= 0, err(h.lib)
        assert np.array_equal(bits(isv), bits(base[2]))
    h.close()


# ---- the status record --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["elastic", "linear_H5e3", "voce"])
def test_one_nan_strain_counts_once_and_leaves_its_neighbours_alone(case):
    law, prm = ALL_CASES[case]
    sig0, Em, _ = scales(prm)
    n = 777
    eps = pe.increments(n, sig0, Em, seed=100)[0]
    h = Handle(law, n, prm)
    base = h.device(to_device(eps))
    bad = eps.copy()
    bad[300, 1] = np.nan
    got = h.device(to_device(bad))
    ok = np.delete(np.arange(n), 300)
    assert got[3]["n_nan"] == 1 and base[3]["n_nan"] == 0 and np.isnan(got[0][300]).any()
    assert all(np.array_equal(bits(a[ok]), bits(b[ok])) for a, b in zip(got[:3], base[:3]))
    assert not got[2][300].any()             # the state of the point: the bits it read
    h.close()


def test_a_capped_newton_counts_its_points():
    law, prm = pe.CASES["voce"]
    sig0, Em, _ = scales(prm)
    n = 640
    eps = 2.0 * pe.increments(n, sig0, Em, seed=110)[0]
    h = Handle(law, n, prm)
    h.newton(maxit=1, rtol=1e-14)
    got = h.device(to_device(eps))
    want = pe.update(law, eps, np.zeros((n, 4)), np.zeros(n), prm, maxit=1)
    assert want["not_converged"].sum() >= n // 4
    # (a point whose residual after its one step sits at the tolerance may fall on either side)
    assert abs(got[3]["n_not_converged"] - int(want["not_converged"].sum())) <= 2 and got[3]["max_local_iters"] == 1
    assert got[3]["n_plastic"] == int(want["plastic"].sum())
    h.newton()
    got = h.device(to_device(eps))
    assert got[3]["n_not_converged"] == 0 and 2 <= got[3]["max_local_iters"] <= 25
    check("after the cap is lifted", prm, got, oracle(law, prm, eps, np.zeros((n, 6)), np.zeros(n)))
    h.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_library_refuses_on_a_live_handle():
    lib = _lib.load()
    from dolfinx_materials_amd.gradient import gauss_points_hex

    for law, p, words in ((26, [pe.E, 0.5], "invalid elastic constants"), (27, [pe.E, pe.NU, 250.0], "expects 4 parameters"),
                          (28, [-1.0, pe.NU, 350.0, 500.0, 1e3], "invalid elastic constants")):
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 8, 0) and words in err(lib), err(lib)
    for law in (25, 29):
        assert not lib.dxm_create(law, (C.c_double * 2)(pe.E, pe.NU), 2, 8, 0) and f"unknown law id {law}" in err(lib), err(lib)
    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    for case in ("elastic", "linear_H5e3", "voce"):
        law, prm = ALL_CASES[case]
        h = Handle(law, 8, prm)
        u, fl, ct = np.zeros(24), np.zeros((8, 4)), np.zeros((8, 16))
        rows, st = np.arange(8, dtype=np.int64), _lib.Stats()
        for fused in (1, 0):     # the fused gradient and the displacement forms: the mesh kernels produce 6-wide strains
            h.option("fused_gradient", fused)
            rcs = (lib.dxm_integrate_displacement(h.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
                   lib.dxm_integrate_displacement_rows(h.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
                   lib.dxm_integrate_displacement_device(h.h, mesh, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
            for rc in rcs:
                assert rc < 0 and "4-wide strain" in err(lib), err(lib)
        for layout in (1, 2, 3):
            assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and "4x4 block of 16 entries" in err(lib), err(lib)
        assert lib.dxm_set_tangent_layout(h.h, 0) == 0
        frame = np.eye(3)
        assert lib.dxm_set_frame(h.h, frame.ctypes.data) < 0 and "this law is isotropic: a material frame changes nothing" in err(lib), err(lib)
        field = np.full(8, 1.0)
        assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "not served under the plane-strain hypothesis" in err(lib), err(lib)
        assert lib.dxm_set_external_state_uniform(h.h, 0, 300.0) < 0 and "has no external state variable" in err(lib), err(lib)
        assert lib.dxm_set_external_state(h.h, 0, field.ctypes.data) < 0 and "has no external state variable" in err(lib), err(lib)
        assert lib.dxm_kernel_name(h.h) == f"plane_strain_kernel<{law - 26}".encode()
        if law != pe.ELASTIC:
            assert not h.state(_lib.S0).any()
            bad = np.zeros((8, 4))
            assert lib.dxm_get_state(h.h, _lib.S0, 2, bad.ctypes.data) < 0          # two fields
        h.close()
    lib.dxm_mesh_destroy(mesh)


def test_a_custom_hardening_build_refuses_the_three_laws_with_their_own_sentence():
    """(the expressions are those of tests/test_custom_hardening.py: one build in the cache serves every file that asks)"""
    hd = jm.CustomHardening("sig0 + K * (pow(p + p0, n) - pow(p0, n))", "K * n * pow(p + p0, n - 1.0)", sig0=250.0, K=600.0, n=0.3, p0=1e-3)
    lib = _lib.load_custom(hd.expr_R, hd.expr_dR)
    assert lib.dxm_has_custom_hardening() == 1
    for law, p in ((26, [pe.E, pe.NU]), (27, [pe.E, pe.NU, 250.0, 5e3]), (28, [pe.E, pe.NU, 350.0, 500.0, 1e3])):
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 64, 0)
        msg = err(lib)
        assert "the plane-strain laws take the stock hardening laws only" in msg and "not by a custom-hardening build" in msg, msg
        assert _lib.law_blocks(law, lib).tangent_width == 16


# ---- through HIPMaterial ------------------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_sequence_through_the_material_and_the_known_answer():
    """``set_data_manager(N)`` -> ``integrate`` -> ``data_manager.update()`` with ``hypothesis="plane_strain"``; then uniaxial
    plane-strain tension to ``2 / sqrt(3) [sig0, 0, sig0 / 2]`` (tests/mfront/test_elastoplasticity.py:31-36) as on the CPU"""
    from test_plane_strain_cpu import uniaxial_plane_strain_tension

    law, prm = pe.CASES["linear_H5e3"]
    el = jm.LinearElasticIsotropic(E=prm[0], nu=prm[1])
    m = JAXMaterial(jm.vonMisesIsotropicHardening(el, jm.LinearHardening(prm[2], prm[3]), hypothesis="plane_strain"), gradient_name="Strain", flux_name="Stress")
    n = 300
    m.set_data_manager(n)
    assert m.gradients == {"Strain": 4} and m.tangent_blocks == {("Stress", "Strain"): (4, 4)} and m.kernel_name.startswith("plane_strain_kernel<1")
    ep6, p = np.zeros((n, 6)), np.zeros(n)
    for k, e in enumerate(pe.increments(n, prm[2], prm[0], seed=120)):
        sig, isv, Ct = m.integrate(e)
        want = oracle(law, prm, e, ep6, p)
        check(f"material, increment {k + 1}", prm, (np.asarray(sig), np.asarray(Ct).reshape(n, 16), np.asarray(isv)), want)
        assert m.last_stats["n_plastic"] == int(want["plastic"].sum())
        m.data_manager.update()
        s0 = m.get_initial_state_dict()
        assert np.array_equal(np.asarray(s0["Strain"]), e) and np.array_equal(np.asarray(s0["Stress"]), np.asarray(sig))
        assert np.asarray(s0["epsp"]).shape == (n, 4)
        ep6, p = want["ep6"], want["p"]
    m.close()
    sig0 = 250.0
    m = JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=70e3, nu=0.3), jm.LinearHardening(sig0, 1e-6), hypothesis="plane_strain"))
    m.set_data_manager(1)
    sig, worst = uniaxial_plane_strain_tension(m, sig0=sig0)
    assert np.allclose(sig[:3], 2 / np.sqrt(3) * np.array([sig0, 0.0, sig0 / 2]), rtol=1e-2, atol=1e-8) and worst < 12
    m.close()
