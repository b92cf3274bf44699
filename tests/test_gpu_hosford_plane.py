"""GPU: plane-strain Hosford plasticity (DXM_LAW_PE_HOSFORD_LINEAR = 40, ``hosford_plane_kernel``) through ``JAXMaterial`` (ctypes -> C
ABI) against the law's definition ``hosford_plane_ref.update`` -- law 10's tensor-space restatement on the embedded strain,
restricted: a formulation neither kernel uses -- on every input class, two increments with ``advance`` in between and a non-trivial
initial state; against the 50-digit golden rows; against law 10 and law 27 of the same process; the tile loop past its first pass; the
routes of the library against each other bit for bit, the displacement forms on a ``PlaneMesh`` among them; every refusal on a live
handle; the Newton cap; the update protocol; a field map next to a law-28 map.

Bounds: read from ``tests/golden/hosford_plane.npz`` -- 8 x the largest deviation of the restatement from its 50-digit version, never
less than 1e-12 (``tests/golden/make_hosford_plane.py``; both sit on that floor).  Every test prints its figures before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions as cv
from dolfinx_materials_amd.field_map import QuadratureFieldMap
from dolfinx_materials_amd.jaxmat import JAXMaterial

import hosford_plane_ref as hp
import hosford_ref as hr
import tile_loop_cases as tlc
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hosford_plane.npz"))
B_STATE, B_TANGENT = float(GOLD["bound_state"]), float(GOLD["bound_tangent"])
P = hp.PROPS
NLOOP = 206_147       # blocks_per_cu = 1: three full passes of the tile loop on 256 CUs and a ragged fourth (tile_loop_cases.size_for)
KEYS = ("n_plastic", "n_not_converged", "n_nan", "max_local_iters")


def behaviour(a, hypothesis="plane_strain", **over):
    p = {**P, **over}
    return jm.HosfordIsotropicHardening(jm.LinearElasticIsotropic(E=p["E"], nu=p["nu"]), jm.LinearHardening(p["R0"], p["H"]), a=a,
                                        hypothesis=hypothesis)


def material(a, n, ep=None, p=None, props=None, hypothesis="plane_strain", **kw):
    m = JAXMaterial(behaviour(a, hypothesis, **(props or {})), lazy_isv=False, **kw)
    m.set_data_manager(n)
    if ep is not None:
        # a non-trivial initial state: eps_n = eps_p,n (no elastic strain), so that the hidden plastic strain is eps_p,n
        m.set_initial_state_dict({"Strain": ep, "ElasticStrain": np.zeros_like(ep), "EquivalentPlasticStrain": p})
    return m


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def compare(tag, sig, isv, Ct, ref, props=None, b_state=B_STATE, b_tangent=B_TANGENT):
    """Row-scaled deviations of (sig, isv, Ct) from ``ref`` (``hosford_plane_ref.errors``: what the bounds were made with)."""
    props = props or P
    n = ref["sig"].shape[0]
    if n == 0:
        return 0.0, 0.0
    isv = np.asarray(isv).reshape(n, 5)
    got = dict(sig=np.asarray(sig).reshape(n, 4), eel=isv[:, :4], p=isv[:, 4], Ct=np.asarray(Ct).reshape(n, 4, 4))
    es, ec = hp.errors(got, ref, props["E"], props["R0"])
    print(f"plane-strain hosford {tag}: stress / state {es.max():.3e} (bound {b_state:.2e})  tangent {ec.max():.3e} (bound {b_tangent:.2e})")
    assert es.max() <= b_state and ec.max() <= b_tangent, (tag, es.max(), ec.max())
    return es.max(), ec.max()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("a", hp.EXPONENTS)
def test_two_increments_match_the_restatement(N, a):
    """Every input class, from a non-trivial state; `advance`; a second increment from the state the first one left."""
    eps1, ep0, p0 = hp.mixed_inputs(N, a, seed=N + int(a))
    m = material(a, N, ep0, p0)
    assert m.kernel_name == "hosford_plane_kernel" and m.algorithmic_bytes_per_point == 304 and m.tangent_size == 16
    assert m.internal_state_variables == {"ElasticStrain": 4, "EquivalentPlasticStrain": 1} and m.gradients == {"Strain": 4}
    sig, isv, Ct = m.integrate(eps1)
    assert np.asarray(Ct).shape == (N, 4, 4) and np.asarray(sig).shape == (N, 4) and np.asarray(isv).shape == (N, 5)
    r1 = hp.update(eps1, ep0, p0, **P, a=a)
    assert r1["converged"].all()
    compare(f"N={N} a={a} increment 1", sig, isv, Ct, r1)
    T = np.asarray(Ct).reshape(N, 4, 4)
    assert np.array_equal(bits(T), bits(T.transpose(0, 2, 1)))                       # exactly symmetric
    st = m.last_stats
    safe = np.abs(r1["f_trial"]) > 1e-9 * P["R0"]
    assert st["n_not_converged"] == 0 and st["n_nan"] == 0, st
    assert abs(st["n_plastic"] - int(r1["plastic"].sum())) <= int((~safe).sum()), (st, int(r1["plastic"].sum()))
    assert st["max_local_iters"] <= int(r1["iters"].max(initial=0)) + 2
    m.data_manager.update()
    # second increment: a further step along the first one's deviatoric direction, inside the tested overshoot
    R = P["R0"] + P["H"] * r1["p"]
    lam, mu = hr.lame(P["E"], P["nu"])
    seq1 = hr.flow(cv.embed_plane_strain(r1["sig"]), a)[0]
    grow = np.random.default_rng(N).uniform(0.0, 0.4, N) * np.where(seq1 > 0, R / np.maximum(seq1, 1e-300), 0.0)
    e1 = eps1 - ep0
    dev = e1 - e1[:, :3].mean(axis=1, keepdims=True) * np.array([1.0, 1.0, 1.0, 0.0])
    eps2 = eps1 + (grow * (hr.max_overshoot(a) - 1.0) / 2.0)[:, None] * dev
    sig2, isv2, Ct2 = m.integrate(eps2)
    r2 = hp.update(eps2, r1["ep"], r1["p"], **P, a=a)
    assert r2["converged"].all()
    compare(f"N={N} a={a} increment 2", sig2, isv2, Ct2, r2)
    safe = np.abs(r2["f_trial"]) > 1e-9 * P["R0"]
    st = m.last_stats
    assert st["n_not_converged"] == 0 and st["n_nan"] == 0
    assert abs(st["n_plastic"] - int(r2["plastic"].sum())) <= int((~safe).sum())
    m.close()


def test_golden_set_matches_mpmath_directly():
    for a in hp.EXPONENTS:
        k = GOLD["a"] == a
        m = material(a, int(k.sum()), GOLD["ep_n"][k], GOLD["p_n"][k])
        sig, isv, Ct = m.integrate(GOLD["eps"][k])
        compare(f"golden a={a}", sig, isv, Ct, {q: GOLD[q][k] for q in ("sig", "eel", "p", "Ct")})
        assert m.last_stats["n_plastic"] == int(GOLD["plastic"][k].sum()) and m.last_stats["n_not_converged"] == 0
        m.close()


@pytest.mark.parametrize("a", hp.EXPONENTS)
def test_law_10_of_the_same_process_on_the_embedded_strain(a):
    """Agreement to rounding, not to the bit: five Jacobi sweeps there, one closed-form rotation here.  Each is within the bounds of
    the same reference, hence 2 x the bounds."""
    N = 1000
    eps, ep0, p0 = hp.mixed_inputs(N, a, seed=70 + int(a))
    m = material(a, N, ep0, p0)
    sig, isv, Ct = (np.array(x) for x in m.integrate(eps))
    w = material(a, N, cv.embed_plane_strain(ep0), p0, hypothesis="3d")
    assert w.kernel_name.startswith("hosford_kernel")
    s6, i7, C6 = (np.array(x) for x in w.integrate(cv.embed_plane_strain(eps)))
    C6 = C6.reshape(N, 6, 6)
    # what the restriction drops: zero for an embedded strain (exactly, by the arithmetic of hosford.hip; held here to rounding)
    dropped = max(np.abs(s6[:, 4:]).max() / P["R0"], P["E"] * np.abs(i7[:, 4:6]).max() / P["R0"], np.abs(C6[:, :4, 4:]).max() / P["E"],
                  np.abs(C6[:, 4:, :4]).max() / P["E"])
    print(f"law 10 on the embedded strain a={a}: dropped components {dropped:.3e}")
    assert dropped <= B_STATE
    want = dict(sig=cv.restrict_plane_strain(s6), eel=cv.restrict_plane_strain(i7[:, :6]), p=i7[:, 6], Ct=cv.restrict_plane_strain_tangent(C6))
    compare(f"vs law 10 restricted a={a}", sig, isv, Ct, want, b_state=2 * B_STATE, b_tangent=2 * B_TANGENT)
    assert m.last_stats["n_plastic"] == w.last_stats["n_plastic"] and m.last_stats["n_not_converged"] == w.last_stats["n_not_converged"] == 0
    m.close()
    w.close()


def test_a_2_equals_plane_strain_j2_with_linear_hardening():
    N = 1000
    eps, ep0, p0 = hp.mixed_inputs(N, 2.0, seed=7)
    m = material(2.0, N, ep0, p0)
    j2 = JAXMaterial(jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"]), jm.LinearHardening(P["R0"], P["H"]),
                                                   hypothesis="plane_strain"), lazy_isv=False)
    j2.set_data_manager(N)
    assert j2.kernel_name.startswith("plane_strain_kernel<1")
    j2.set_initial_state_dict({"p": p0, "epsp": ep0})
    sig, isv, Ct = m.integrate(eps)
    sj, ij, Cj = (np.array(x) for x in j2.integrate(eps))
    want = dict(sig=sj, eel=eps - ij[:, 1:5], p=ij[:, 0], Ct=Cj.reshape(N, 4, 4))
    # a point at the yield kink may take either branch: the two tangents differ there, the stresses do not
    ref = hp.update(eps, ep0, p0, **P, a=2.0)
    safe = np.abs(ref["f_trial"]) > 1e-9 * P["R0"]
    isv = np.asarray(isv)
    compare("a = 2 vs law 27", np.asarray(sig)[safe], isv[safe], np.asarray(Ct)[safe], {k: v[safe] for k, v in want.items()})
    assert abs(m.last_stats["n_plastic"] - j2.last_stats["n_plastic"]) <= int((~safe).sum())
    m.close()
    j2.close()


def test_tile_loop_at_one_workgroup_per_cu_equals_the_shipped_grid_bit_for_bit():
    torch = pytest.importorskip("torch")
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert NLOOP == tlc.size_for(256)
    N, a = tlc.size_for(num_cu), 10.0
    print(f"tile loop: {num_cu} CUs, {N} points, {tlc.passes(N, num_cu, 1)} passes at blocks_per_cu = 1, {tlc.passes(N, num_cu, 64)} at 64")
    assert tlc.passes(N, num_cu, 1) >= 4 and N % 64 != 0
    # yielded and elastic tiles interleaved: even tiles of 64 yield (every class that does), odd ones stay elastic
    ey, py_, pn = hp.make_inputs("generic", N, a, seed=8)
    ee = hp.make_inputs("elastic", N, a, seed=9, trivial_state=True)[0]
    odd = (np.arange(N) // 64) % 2 == 1
    eps = np.where(odd[:, None], ee, ey)
    ep0, p0 = np.where(odd[:, None], 0.0, py_), np.where(odd, 0.0, pn)
    g = to_device(eps)
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for bpc in (None, 1):
        m = material(a, N, ep0, p0)
        if bpc is not None:
            m.set_option("blocks_per_cu", bpc)
        f = torch.full((N + 3, 4), float("nan"), dtype=torch.float64, device="cuda:0")
        c = torch.full((N + 3, 16), float("nan"), dtype=torch.float64, device="cuda:0")
        m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), st)
        torch.cuda.synchronize()
        fin = m.get_final_state_dict()
        isv = np.concatenate([np.array(fin[k]).reshape(N, -1) for k in ("ElasticStrain", "EquivalentPlasticStrain")], axis=1)
        out.append((to_host(f), to_host(c), isv, m.stats()[1]))
        m.close()
    x, y = out
    for u, v in zip(x[:3], y[:3]):
        assert np.array_equal(bits(u), bits(v))
    assert {k: x[3][k] for k in KEYS} == {k: y[3][k] for k in KEYS}
    assert np.isnan(y[0][N:]).all() and np.isnan(y[1][N:]).all()               # nothing past 4 n / 16 n doubles
    assert y[3]["n_nan"] == 0 and y[3]["n_not_converged"] == 0 and y[3]["n_plastic"] == int((~odd).sum())
    idx = tlc.reference_sample(N, num_cu)
    ref = hp.update(eps[idx], ep0[idx], p0[idx], **P, a=a)
    assert ref["converged"].all() and (ref["plastic"] == ~odd[idx]).all()
    compare("tile loop sample", y[0][idx], y[2][idx], y[1][idx], ref)


def test_routes_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    N, a = 1003, 10.0
    eps, ep0, p0 = hp.mixed_inputs(N, a, seed=11)
    m = material(a, N, ep0, p0)
    dev = torch.device("cuda:0")
    g = to_device(eps)
    f = torch.empty((N, 4), dtype=torch.float64, device=dev)
    c = torch.empty((N, 16), dtype=torch.float64, device=dev)
    m.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    S, T = to_host(f).copy(), to_host(c).copy()
    rc, st_dev = m.stats()
    fin = m.get_final_state_dict()
    isv_dev = np.concatenate([np.array(fin[k]).reshape(N, -1) for k in ("ElasticStrain", "EquivalentPlasticStrain")], axis=1)
    compare("device arrays", S, isv_dev, T, hp.update(eps, ep0, p0, **P, a=a))
    # host buffers; option packed_transfer has nothing to pack for this law: the same bytes either way
    for pt in (2, 0):
        m.set_option("packed_transfer", pt)
        sig, isv, Ct = m.integrate(eps)
        assert np.array_equal(bits(sig), bits(S)) and np.array_equal(bits(np.array(Ct).reshape(N, 16)), bits(T)), pt
        assert np.array_equal(bits(isv), bits(isv_dev)), pt
        assert {k: m.last_stats[k] for k in KEYS} == {k: st_dev[k] for k in KEYS}
    m.set_option("packed_transfer", 2)
    # rows form over a permuted subset of a larger array, with ISV row deliveries
    M = N + 321
    rows = np.ascontiguousarray(np.random.default_rng(0).permutation(M)[:N], dtype=np.int64)
    flux, tang = np.full((M, 4), -7.0), np.full((M, 16), -9.0)
    big = {"ElasticStrain": np.full((M, 4), -3.0), "EquivalentPlasticStrain": np.full((M, 1), -5.0)}
    m.bind_state_outputs(big, deliver=True, rows=True)
    m.integrate_rows(eps, rows, flux, tang)
    assert np.array_equal(bits(flux[rows]), bits(S)) and np.array_equal(bits(tang[rows]), bits(T))
    assert np.array_equal(bits(big["ElasticStrain"][rows]), bits(isv_dev[:, :4])) and np.array_equal(bits(big["EquivalentPlasticStrain"][rows, 0]), bits(isv_dev[:, 4]))
    rest = np.setdiff1d(np.arange(M), rows)
    assert np.all(flux[rest] == -7.0) and np.all(tang[rest] == -9.0) and np.all(big["ElasticStrain"][rest] == -3.0)
    m.close()
    # explicit state in, explicit state out; the one-point form
    m = material(a, N)
    # (the explicit-state forms carry the internal state variables, not the previous strain, which is zero there: the hidden plastic
    # strain Strain_n - ElasticStrain_n is ep0 for ElasticStrain_n = -ep0, exactly)
    state = m.natural_state(N)
    state.update({"ElasticStrain": -ep0, "EquivalentPlasticStrain": p0.reshape(state["EquivalentPlasticStrain"].shape)})
    Ct, new = m.batched_constitutive_update(eps, state)
    assert np.array_equal(bits(new["Stress"]), bits(S)) and np.array_equal(bits(np.asarray(Ct).reshape(N, 16)), bits(T))
    assert np.array_equal(bits(new["ElasticStrain"]), bits(isv_dev[:, :4]))
    assert np.array_equal(bits(np.asarray(new["EquivalentPlasticStrain"]).reshape(N)), bits(isv_dev[:, 4]))
    k = 12
    one_state = {name: np.asarray(v)[k] for name, v in state.items()}
    sig1, one = m.constitutive_update(eps[k], one_state)
    assert np.array_equal(bits(sig1), bits(S[k])) and np.array_equal(bits(np.asarray(one["ElasticStrain"]).reshape(-1)), bits(isv_dev[k, :4]))
    m.close()


class _Handle:
    """one dxm_material of law 40, driven through ctypes alone"""

    def __init__(self, n, a=10.0):
        p = [P["E"], P["nu"], P["R0"], P["H"], a]
        self.lib, self.n = _lib.load(), n
        self.h = self.lib.dxm_create(_lib.LAW_PE_HOSFORD_LINEAR, (C.c_double * 5)(*p), 5, n, 0)
        assert self.h, err(self.lib)

    def state(self):
        out = []
        for f, dim in enumerate((4, 1, 4)):          # the hidden plastic strain included
            x = np.full((self.n, dim), np.nan)
            assert self.lib.dxm_get_state(self.h, _lib.S1, f, x.ctypes.data) == 0, err(self.lib)
            out.append(x)
        return np.concatenate(out, axis=1)

    def stats(self):
        st = _lib.Stats()
        assert self.lib.dxm_get_stats(self.h, C.byref(st)) >= 0, err(self.lib)
        return st.as_dict()

    def _outputs(self):
        import torch

        new = lambda cols: torch.full((self.n, cols), float("nan"), dtype=torch.float64, device="cuda:0")   # noqa: E731
        return new(4), new(16)

    def displacement_device(self, mesh, ud):
        import torch

        f, c = self._outputs()
        assert self.lib.dxm_integrate_displacement_device(self.h, mesh._handle, ud.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.state(), self.stats()

    def device(self, grad):
        import torch

        f, c = self._outputs()
        assert self.lib.dxm_integrate_device(self.h, grad.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.state(), self.stats()

    def displacement_host(self, mesh, u):
        f, c, st = np.full((self.n, 4), np.nan), np.full((self.n, 16), np.nan), _lib.Stats()
        rc = self.lib.dxm_integrate_displacement(self.h, mesh._handle, u.ctypes.data, 0.0, f.ctypes.data, None, c.ctypes.data, C.byref(st))
        assert rc >= 0, err(self.lib)
        return f, c, self.state(), st.as_dict()

    def advance(self):
        assert self.lib.dxm_advance(self.h) == 0, err(self.lib)

    def close(self):
        self.lib.dxm_destroy(self.h)


def _same(x, y):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(x[:3], y[:3])) and all(x[3][k] == y[3][k] for k in KEYS)


@pytest.mark.parametrize("cells", ["p1 triangles", "q1 quadrilaterals"])
def test_displacement_forms_on_a_plane_mesh_equal_gradient_kernel_then_array_form(cells):
    """The multi-material demo's route: from a displacement on a plane mesh.  ``dxm_integrate_displacement_device`` and
    ``dxm_integrate_displacement`` against ``dxm_mesh_gradient_device(kind 2)`` -> ``dxm_integrate_device``: the same kernels, arrays
    and grids, so stress, tangent and state (hidden field included) agree bit for bit, over two load steps with an advance between."""
    import torch

    import plane_gradient_ref as pg
    from dolfinx_materials_amd.gradient import PlaneMesh

    case = pg.tri_case("p1tri", "q1") if cells == "p1 triangles" else pg.quad_case("q1-x4")
    mesh = PlaneMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"], case["dphi"])
    n = mesh.npoints
    xd = case["xd"]
    # a uniaxial stretch past yield plus nodal noise: on the CPU, 61 % / 64 % of the points yield at t = 0.6, 97 % at t = 1, and the trial
    # stress stays below 2.3 R (the Newton domain ends at 3)
    field = xd * pg.STRETCH + 1e-3 / 9 * np.random.default_rng(5).standard_normal(xd.shape)
    a_, b_, c_ = _Handle(n), _Handle(n), _Handle(n)
    carry = (np.zeros((n, 4)), np.zeros(n))
    for step, t in enumerate((0.6, 1.0)):
        u = np.ascontiguousarray((t * field).ravel())
        ud = to_device(u)
        grad = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda:0")
        mesh.gradient_device(ud.data_ptr(), 2, grad.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got_a, got_b, got_c = a_.displacement_device(mesh, ud), b_.device(grad), c_.displacement_host(mesh, u)
        assert _same(got_a, got_b), f"{cells} step {step + 1}: device form"
        assert _same(got_c, got_b), f"{cells} step {step + 1}: host form"
        eps = to_host(grad)
        want = pg.rows(pg.reference(case, u), 2)
        assert np.abs(eps - want).max() < 1e-13 and not eps[:, 2].any()
        share = got_a[3]["n_plastic"] / n
        print(f"displacement forms {cells} step {step + 1}: {n} points, n_plastic {got_a[3]['n_plastic']}")
        assert 0.05 <= share <= (0.95 if step == 0 else 1.0) and got_a[3]["n_nan"] == 0 and got_a[3]["n_not_converged"] == 0
        ref = hp.update(eps, carry[0], carry[1], **P, a=10.0)
        compare(f"displacement {cells} step {step + 1}", got_a[0], got_a[2][:, :5], got_a[1], ref)
        assert np.abs(got_a[2][:, 5:] - ref["ep"]).max() <= B_STATE * P["R0"] / P["E"] * 10       # the hidden field is eps_p
        carry = (ref["ep"], ref["p"])
        for h in (a_, b_, c_):
            h.advance()
    for h in (a_, b_, c_):
        h.close()
    mesh.close()


def test_refusals_on_a_live_handle_each_with_its_own_sentence():
    from dolfinx_materials_amd.gradient import gauss_points_hex

    lib = _lib.load()
    n, a = 8, 10.0
    eps, ep0, p0 = hp.mixed_inputs(n, a, seed=3)
    m = material(a, n, ep0, p0)
    before = [np.array(x) for x in m.integrate(eps)]
    h = m._parts[0][0]
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h, layout) < 0 and "the plane-strain Hosford tangent is a general symmetric 4x4 block of 16 entries" in err(lib), err(lib)
    assert lib.dxm_tangent_size(h) == 16 and lib.dxm_set_tangent_layout(h, 0) == 0
    field = np.full(n, 1.0)
    assert lib.dxm_set_param_field(h, 2, field.ctypes.data) < 0
    assert "per-point parameter fields are not served for plane-strain Hosford plasticity" in err(lib), err(lib)
    frame = np.eye(3)
    assert lib.dxm_set_frame(h, frame.ctypes.data) < 0 and "this law is isotropic: a material frame changes nothing" in err(lib), err(lib)
    frames = np.tile(np.eye(3).reshape(9), (n, 1))
    assert lib.dxm_set_frame_field(h, frames.ctypes.data) < 0 and "this law is isotropic" in err(lib), err(lib)
    assert lib.dxm_set_external_state_uniform(h, 0, 300.0) < 0 and "law 40 has no external state variable" in err(lib), err(lib)
    assert lib.dxm_set_external_state(h, 0, field.ctypes.data) < 0 and "has no external state variable" in err(lib), err(lib)
    for bad, word in (((P["E"], P["nu"], 0.0, P["H"], 10.0), "R0"), ((P["E"], P["nu"], P["R0"], -1.0, 10.0), "H"),
                      ((P["E"], P["nu"], P["R0"], P["H"], 1.5), "exponent"), ((P["E"], 0.5, P["R0"], P["H"], 10.0), "invalid elastic constants")):
        assert lib.dxm_set_params(h, (C.c_double * 5)(*bad), 5) < 0 and word in err(lib), err(lib)
    assert lib.dxm_set_params(h, (C.c_double * 4)(P["E"], P["nu"], P["R0"], P["H"]), 4) < 0 and "expects 5 parameters" in err(lib)
    # a mesh that is not two-dimensional: the fused and the displacement forms, both settings of fused_gradient
    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    u, fl, ct = np.zeros(24), np.zeros((n, 4)), np.zeros((n, 16))
    rows, st = np.arange(n, dtype=np.int64), _lib.Stats()
    for fused in (1, 0):
        m.set_option("fused_gradient", fused)
        rcs = (lib.dxm_integrate_displacement(h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_rows(h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_device(h, mesh, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
        for rc in rcs:
            assert rc < 0 and "plane-strain Hosford plasticity takes a 4-wide strain" in err(lib), err(lib)
            assert "not served on a mesh that is not two-dimensional" in err(lib)
    m.set_option("fused_gradient", 1)
    lib.dxm_mesh_destroy(mesh)
    assert not fl.any() and not ct.any()
    for layout in ("sym", "coef", "pack4"):
        with pytest.raises(ValueError, match="general symmetric 4x4 block of 16 entries"):
            JAXMaterial(behaviour(a), tangent_layout=layout)
    prm = (C.c_double * 5)(P["E"], P["nu"], P["R0"], P["H"], 10.0)
    assert not lib.dxm_create(39, prm, 5, 8, 0) and "unknown law id 39" in err(lib)
    assert not lib.dxm_create(41, prm, 5, 8, 0) and "unknown law id 41" in err(lib)
    assert not lib.dxm_create(40, (C.c_double * 5)(P["E"], P["nu"], -1.0, P["H"], 10.0), 5, 8, 0) and "R0 must be" in err(lib)
    bad = np.zeros((n, 4))
    assert lib.dxm_get_state(h, _lib.S0, 3, bad.ctypes.data) < 0 and lib.dxm_get_state(h, _lib.S0, 2, bad.ctypes.data) == 0      # three fields
    assert np.array_equal(bad, ep0)
    with pytest.raises(NotImplementedError, match="varies from point to point"):
        m.update_material_property("yield_stress.sig0", np.linspace(100.0, 300.0, n))
    with pytest.raises(_lib.DxmError, match="exponent"):
        m.update_material_property("a", 1.0)
    assert m.material_properties["a"] == 10.0
    # the handle is what it was
    after = [np.array(x) for x in m.integrate(eps)]
    for x, y in zip(after, before):
        assert np.array_equal(bits(x), bits(y))
    assert lib.dxm_kernel_name(h) == b"hosford_plane_kernel" and lib.dxm_tangent_size(h) == 16
    m.close()


def test_a_custom_hardening_build_refuses_the_law_with_its_own_sentence():
    """(the expressions are those of tests/test_custom_hardening.py: one build in the cache serves every file that asks)"""
    hd = jm.CustomHardening("sig0 + K * (pow(p + p0, n) - pow(p0, n))", "K * n * pow(p + p0, n - 1.0)", sig0=250.0, K=600.0, n=0.3, p0=1e-3)
    lib = _lib.load_custom(hd.expr_R, hd.expr_dR)
    assert lib.dxm_has_custom_hardening() == 1
    assert not lib.dxm_create(40, (C.c_double * 5)(P["E"], P["nu"], P["R0"], P["H"], 10.0), 5, 64, 0)
    msg = (lib.dxm_last_error() or b"").decode()
    assert "plane-strain Hosford plasticity takes linear hardening only" in msg and "not by a custom-hardening build" in msg, msg


def test_one_newton_iteration_is_reported_as_not_converged():
    N = 512
    eps, ep0, p0 = hp.make_inputs("generic", N, 10.0, seed=2)
    m = material(10.0, N, ep0, p0)
    m.set_newton(maxit=1)
    m.integrate(eps)
    st = m.last_stats
    assert st["n_plastic"] == N and 0 < st["n_not_converged"] <= N and st["max_local_iters"] == 1, st
    m.set_newton()
    sig, isv, Ct = m.integrate(eps)
    assert m.last_stats["n_not_converged"] == 0
    compare("after the cap is lifted", sig, isv, Ct, hp.update(eps, ep0, p0, **P, a=10.0))
    m.close()


def test_protocol_revert_and_update_material_property():
    N = 1000
    eps, ep0, p0 = hp.mixed_inputs(N, 10.0, seed=5)
    m = material(10.0, N, ep0, p0)
    s0 = {k: np.array(v) for k, v in m.get_initial_state_dict().items()}
    sig, isv, Ct = m.integrate(eps)
    m.data_manager.revert()
    back = m.get_final_state_dict()
    for k in ("ElasticStrain", "EquivalentPlasticStrain"):
        assert np.array_equal(np.array(back[k]), s0[k]), k
    sig2, isv2, Ct2 = m.integrate(eps)
    assert np.array_equal(bits(sig2), bits(sig)) and np.array_equal(bits(Ct2), bits(Ct))
    for key, val in (("a", 6.0), ("yield_stress.sig0", 180.0), ("yield_stress.H", 25.0), ("elasticity.E", 69e3), ("elasticity.nu", 0.31)):
        m.update_material_property(key, val)
    over = dict(E=69e3, nu=0.31, R0=180.0, H=25.0)
    sig3, isv3, Ct3 = m.integrate(eps)
    ref = hp.update(eps, ep0, p0, **over, a=6.0)
    assert ref["converged"].all()
    compare("after update_material_property (a = 6)", sig3, isv3, Ct3, ref, props=over)
    assert m.last_stats["n_plastic"] == int(ref["plastic"].sum())
    m.close()


def test_field_map_over_a_cell_subset_next_to_a_plane_strain_voce_map():
    """The multi-material demo's arrangement at a handful of cells: Hosford on the matrix cells, von Mises + Voce (law 28) on the
    inclusion's, both under the plane-strain hypothesis, one field map each."""
    ncell, nqp, a = 23, 3, 10.0
    n = ncell * nqp
    rng = np.random.default_rng(1)
    perm = rng.permutation(ncell)
    matrix, incl = np.sort(perm[: 2 * ncell // 3]).astype(np.int32), np.sort(perm[2 * ncell // 3:]).astype(np.int32)
    eps_all = hp.mixed_inputs(n, a, seed=21, trivial_state=True)[0]
    now = {"g": np.zeros_like(eps_all)}     # the state is initialised at zero strain, as the demo's is
    ev = lambda c: now["g"].reshape(ncell, nqp, 4)[c].reshape(-1, 4)   # noqa: E731
    voce = jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(E=P["E"], nu=P["nu"]), jm.VoceHardening(250.0, 400.0, 100.0), hypothesis="plane_strain")
    mh, mv = JAXMaterial(behaviour(a)), JAXMaterial(voce, gradient_name="Strain", flux_name="Stress")
    qh = QuadratureFieldMap(ncell, nqp, mh, cells=matrix)
    qv = QuadratureFieldMap(ncell, nqp, mv, cells=incl)
    for q in (qh, qv):
        q.register_gradient("Strain", ev)
        q.initialize_state()
    now["g"] = eps_all
    for q in (qh, qv):
        q.update()
        q.advance()
    assert mh.kernel_name == "hosford_plane_kernel" and mv.kernel_name.startswith("plane_strain_kernel<2")
    rows = (matrix[:, None] * nqp + np.arange(nqp)[None]).ravel()
    rest = np.setdiff1d(np.arange(n), rows)
    ref = hp.update(eps_all[rows], np.zeros((rows.size, 4)), np.zeros(rows.size), **P, a=a)
    sig = qh.fluxes["Stress"].x.array.reshape(n, 4)
    jac = qh.jacobian_flatten.x.array.reshape(n, 16)
    pl = qh.internal_state_variables["EquivalentPlasticStrain"].x.array.reshape(n)
    eel = qh.internal_state_variables["ElasticStrain"].x.array.reshape(n, 4)
    compare("field map, matrix cells", sig[rows], np.concatenate([eel[rows], pl[rows, None]], axis=1), jac[rows], ref)
    assert not sig[rest].any() and not jac[rest].any() and not pl[rest].any()
    assert (pl[rows] > 0).sum() == int(ref["plastic"].sum()) > 0
    sv = qv.fluxes["Stress"].x.array.reshape(n, 4)
    assert sv[rest].any() and not sv[rows].any()
    for q in (qh, qv):
        q.close()
        q.material.close()
