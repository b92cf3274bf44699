"""GPU: the two heat-transfer laws (DXM_LAW_HEAT_STATIONARY, DXM_LAW_HEAT_PHASE_CHANGE; ``heat_transfer_kernel``) and the external state
variable of a handle, through the C ABI (ctypes): against the numpy restatement ``heat_transfer_ref`` and the committed 50-digit
values, the routes of the library against each other bit for bit, the setters, the launch generation, every refusal, and the
``QuadratureFieldMap`` on the engine.

Bound: max(1e-12, 8 x the restatement's recorded deviation from the 50-digit values), PER OUTPUT GROUP against that group's own scale
(the flux, each tangent block, the enthalpy): c is about 1e10 and k about 1e2, so a bound over the whole 13-wide row would hide k.
The recorded deviations (``tests/golden/heat_transfer_kat.npz``) are at most 2.6e-13 (flux and -k I of the phase-change law at the
default Tsmooth = 0.1: the double Ts against the exact one in (T - Ts) / Tsmooth).  Every test is held to the deviations recorded for
ITS parameter set: the tests on the file defaults / the demo's Tsmooth = 1.0 (cases st0, pc1) to 1e-12, the fixture test case by case
(1e-12, and 2.0e-12 to 2.1e-12 for flux and -k I of case pc0).  Measured on an MI355X: the kernel reproduces the restatement to 4.4e-16
(most groups bit for bit) and the 50-digit values to 2.6e-13 (flux), 2.5e-13 (-k I), 9.2e-14 (enthalpy), all on case pc0: the
restatement's own deviations."""
import ctypes as C
import json

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib

import heat_transfer_ref as ht
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

KAT = ht.load_kat()
NBIG = 100_003
NCHUNK = 400_003      # the unpacked host-buffer form is cut into three chunks from 393 216 points on (host_side.hpp::plan_chunks)
NLOOP = 206_147       # blocks_per_cu = 1: four passes of the tile loop on 256 CUs, a ragged last tile
LAWS = (ht.STATIONARY, ht.PHASE_CHANGE)
PARAMS = {ht.STATIONARY: ht.STATIONARY_DEFAULTS, ht.PHASE_CHANGE: ht.PHASE_CHANGE_DEFAULTS[:6] + (1.0,)}


#: the fixture case recorded with PARAMS[law]: its deviations bound every test that runs on these parameters
CASE = {ht.STATIONARY: "st0", ht.PHASE_CHANGE: "pc1"}


def bounds(law):
    """output group -> max(1e-12, 8 x the restatement's recorded deviation for that group on the parameters of PARAMS[law])"""
    (case,) = [c for c in json.loads(str(KAT["meta"]))["cases"] if c["tag"] == CASE[law]]
    assert case["law"] == law and np.array_equal(KAT[f"{case['tag']}_params"], PARAMS[law])
    return {name: max(1e-12, 8 * dev) for name, dev in case["restatement_deviation"].items()}


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def inputs(law, n, seed, prm=None):
    """gradients of mixed magnitude and temperatures over every branch, the ends of the transition included"""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(n, 3)) * rng.choice([1.0, 1e3, 1e-3], size=(n, 1))
    if law == ht.STATIONARY:
        return g, rng.uniform(250.0, 1600.0, n)
    Ts, Tl = ht.solidus_liquidus(prm or PARAMS[law])
    T = rng.choice([0, 1, 2], size=n)
    T = np.where(T == 0, rng.uniform(300.0, Ts, n), np.where(T == 1, rng.uniform(Ts, Tl, n), rng.uniform(Tl, 1500.0, n)))
    edge = [Ts, Tl, (Ts + Tl) / 2, np.nextafter(Ts, -np.inf), np.nextafter(Ts, np.inf), np.nextafter(Tl, -np.inf), np.nextafter(Tl, np.inf)]
    k = min(n, len(edge))
    T[n - k:] = edge[:k]
    return g, T


class Handle:
    """one dxm_material of a heat-transfer law, driven through ctypes alone"""

    def __init__(self, law, n, prm=None):
        p = list(prm if prm is not None else PARAMS[law])
        self.lib, self.n, self.law = _lib.load(), n, law
        self.h = self.lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        self.width = self.lib.dxm_tangent_size(self.h)
        assert self.width == ht.WIDTH[law]

    def temperature(self, T):
        """a number: uniform; an array: the host setter; None: back to uniform"""
        if T is None:
            rc = self.lib.dxm_set_external_state(self.h, 0, None)
        elif np.ndim(T) == 0:
            rc = self.lib.dxm_set_external_state_uniform(self.h, 0, float(T))
        else:
            a = np.ascontiguousarray(T, dtype=np.float64)
            assert a.shape == (self.n,)
            rc = self.lib.dxm_set_external_state(self.h, 0, a.ctypes.data)
        assert rc == 0, err(self.lib)
        return self

    def stats(self):
        st = _lib.Stats()
        assert self.lib.dxm_get_stats(self.h, C.byref(st)) == 0, err(self.lib)
        return st.as_dict()

    def enthalpy(self, which=_lib.S1):
        h = np.full((self.n, 1), np.nan)
        if self.law == ht.PHASE_CHANGE:
            assert self.lib.dxm_get_state(self.h, which, 0, h.ctypes.data) == 0, err(self.lib)
        return h

    def device(self, g_dev, stream=None):
        import torch

        f = torch.zeros((self.n, 3), dtype=torch.float64, device=g_dev.device)
        c = torch.zeros((self.n, self.width), dtype=torch.float64, device=g_dev.device)
        assert self.lib.dxm_integrate_device(self.h, g_dev.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), stream) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.enthalpy(), self.stats()

    def host(self, g):
        f, c, st = np.full((self.n, 3), np.nan), np.full((self.n, self.width), np.nan), _lib.Stats()
        isv = np.full((self.n, 1), np.nan) if self.law == ht.PHASE_CHANGE else None
        assert self.lib.dxm_integrate(self.h, g.ctypes.data, 0.0, f.ctypes.data, None if isv is None else isv.ctypes.data, c.ctypes.data,
                                      C.byref(st)) == 0, err(self.lib)
        return f, c, (isv if isv is not None else self.enthalpy()), st.as_dict()

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def generation(self):
        return self.lib.dxm_launch_generation(self.h)

    def close(self):
        self.lib.dxm_destroy(self.h)


def same(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def check(tag, law, got, want, limits=None):
    """got = (flux, tangent, enthalpy): each output group against its own scale; limits: group -> bound (default: bounds(law))"""
    groups = ht.group_values(law, dict(flux=got[0], tangent=got[1], enthalpy=got[2].reshape(-1)))
    for name, bound in (limits or bounds(law)).items():
        dev = ht.relative_deviation(groups[name], want[name])
        print(f"heat transfer parity {tag}: {name} {dev:.3e} (bound {bound:.2e})")
        assert dev <= bound, (tag, name, dev, bound)


@pytest.fixture(scope="module")
def big():
    """shared inputs at N = 100 003 per law, with the restatement"""
    out = {}
    for law in LAWS:
        g, T = inputs(law, NBIG, seed=40 + law)
        out[law] = dict(g=g, T=T, g_dev=to_device(g), ref=ht.update(law, g, T, PARAMS[law]))
    return out


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, NBIG])
def test_kernel_matches_the_restatement_group_by_group(big, N, law):
    if N == NBIG:
        g, T, g_dev, ref = (big[law][k] for k in ("g", "T", "g_dev", "ref"))
    else:
        g, T = inputs(law, N, seed=N)
        g_dev, ref = to_device(g), ht.update(law, g, T, PARAMS[law])
    h = Handle(law, N).temperature(T)
    got = h.device(g_dev)
    check(f"N={N} law {law} field", law, got, ht.group_values(law, ref))
    st = got[3]
    assert st == dict(n_points=N, n_plastic=0, n_not_converged=0, n_nan=0, max_local_iters=0)
    assert not got[1][:, [1, 2, 3, 5, 6, 7]].any()                       # the structural zeros are written
    assert h.lib.dxm_external_state_kind(h.h, 0) == 1 and h.lib.dxm_kernel_name(h.h) == f"heat_transfer_kernel<{law - 16}, 1".encode()
    # a uniform temperature: the default of dxm_create, then a set value
    h.temperature(None)
    assert h.lib.dxm_external_state_kind(h.h, 0) == 0 and h.lib.dxm_kernel_name(h.h) == f"heat_transfer_kernel<{law - 16}, 0".encode()
    got = h.device(g_dev)
    check(f"N={N} law {law} default T", law, got, ht.group_values(law, ht.update(law, g, ht.T_DEFAULT, PARAMS[law])))
    Tu = 933.4 if law == ht.PHASE_CHANGE else 1100.0                      # inside the transition of Tsmooth = 1
    got = h.temperature(Tu).device(g_dev)
    check(f"N={N} law {law} uniform T", law, got, ht.group_values(law, ht.update(law, g, Tu, PARAMS[law])))
    h.close()


def test_fixture_points_match_their_50_digit_values():
    """each case against its OWN recorded deviation: max(1e-12, 8 x what the restatement deviates by on that case and group)"""
    for law, tag, prm, g, T, exp, recorded in ht.kat_cases(KAT):
        h = Handle(law, len(g), prm).temperature(T)
        got = h.device(to_device(g))
        check(f"fixture {tag}", law, got, exp, {name: max(1e-12, 8 * dev) for name, dev in recorded.items()})
        assert got[3]["n_nan"] == 0
        h.close()


# ---- routes, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS)
def test_host_buffer_form_equals_the_device_form_and_one_chunk_equals_three(law):
    """Distinct temperatures per point: a field that is not offset with the chunk gives other numbers in chunks 2 and 3."""
    g, T = inputs(law, NCHUNK, seed=3)
    h = Handle(law, NCHUNK).temperature(T)
    base = h.device(to_device(g))
    for chunks in (1, 3):
        h.option("max_chunks", chunks)
        assert same(h.host(g), base), chunks
    h.option("pipeline", 0)
    assert same(h.host(g), base)
    h.close()


@pytest.mark.parametrize("law", LAWS)
def test_uniform_equals_a_constant_field_and_host_setter_equals_device_setter(big, law):
    torch = pytest.importorskip("torch")
    g_dev, T = big[law]["g_dev"], big[law]["T"]
    Tu = 933.4 if law == ht.PHASE_CHANGE else 700.0
    u, f = Handle(law, NBIG).temperature(Tu), Handle(law, NBIG).temperature(np.full(NBIG, Tu))
    assert u.lib.dxm_algorithmic_bytes(u.h) + 8 == f.lib.dxm_algorithmic_bytes(f.h)
    assert same(u.device(g_dev), f.device(g_dev))
    # the same field through the device setter, on the stream of the launch
    base = f.temperature(T).device(g_dev)
    stream = torch.cuda.current_stream().cuda_stream
    t_dev = to_device(T)
    gen = u.generation()
    assert u.lib.dxm_set_external_state_device(u.h, 0, t_dev.data_ptr(), stream) == 0, err(u.lib)
    assert u.lib.dxm_external_state_kind(u.h, 0) == 1 and u.generation() > gen
    assert same(u.device(g_dev, stream), base)
    assert u.lib.dxm_set_external_state_device(u.h, 0, None, None) == 0 and u.lib.dxm_external_state_kind(u.h, 0) == 0
    assert same(u.device(g_dev), Handle(law, NBIG).temperature(Tu).device(g_dev))      # the uniform value was kept
    u.close()
    f.close()


def test_rows_form_with_a_bound_enthalpy_row_equals_the_contiguous_form_through_a_permutation(big):
    law = ht.PHASE_CHANGE
    g, T = big[law]["g"], big[law]["T"]
    h = Handle(law, NBIG).temperature(T)
    base = h.device(big[law]["g_dev"])
    M = NBIG + 1000
    rows = np.ascontiguousarray(np.random.default_rng(8).permutation(M)[:NBIG], dtype=np.int64)
    rest = np.setdiff1d(np.arange(M), rows)
    bound = _lib.PinnedArray((M, 1))
    bound.array[...] = -5.0
    assert h.lib.dxm_bind_isv_output(h.h, 0, bound.ptr) == 0, err(h.lib)
    flux, ct, st = np.full((M, 3), -7.0), np.full((M, 13), -9.0), _lib.Stats()
    assert h.lib.dxm_integrate_rows(h.h, g.ctypes.data, 0.0, flux.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)) == 0, err(h.lib)
    assert np.array_equal(flux[rows], base[0]) and np.array_equal(ct[rows], base[1]) and np.array_equal(bound.array[rows], base[2])
    assert np.all(flux[rest] == -7.0) and np.all(ct[rest] == -9.0) and np.all(bound.array[rest] == -5.0) and st.n_nan == 0
    # the contiguous host-buffer form delivers the bound field too
    assert h.lib.dxm_bind_isv_output(h.h, 0, None) == 0
    own = _lib.PinnedArray((NBIG, 1))
    assert h.lib.dxm_bind_isv_output(h.h, 0, own.ptr) == 0, err(h.lib)
    assert same(h.host(g), base) and np.array_equal(own.array, base[2])
    assert h.lib.dxm_bind_isv_output(h.h, 0, None) == 0
    # dxm_isv_host and dxm_isv_device
    isv = np.full((NBIG, 1), np.nan)
    assert h.lib.dxm_isv_host(h.h, _lib.S1, isv.ctypes.data) == 0 and np.array_equal(isv, base[2])
    isv_dev = to_device(np.zeros((NBIG, 1)))
    assert h.lib.dxm_isv_device(h.h, _lib.S1, isv_dev.data_ptr(), None) == 0, err(h.lib)
    import torch

    torch.cuda.synchronize()
    assert np.array_equal(to_host(isv_dev), base[2])
    h.close()


# ---- the field, the generation, the tile loop, the status record ------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS)
def test_a_field_rewritten_in_place_is_seen_without_a_new_generation(big, law):
    g, g_dev, T = big[law]["g"], big[law]["g_dev"], big[law]["T"]
    h = Handle(law, NBIG)
    gens = [h.generation()]
    h.temperature(T)
    gens.append(h.generation())
    first = h.device(g_dev)
    T2 = T[::-1].copy()
    h.temperature(T2)                                    # rewritten in place: the same allocation, the same generation
    assert h.generation() == gens[-1]
    second = h.device(g_dev)
    check(f"law {law} rewritten field", law, second, ht.group_values(law, ht.update(law, g, T2, PARAMS[law])))
    assert not np.array_equal(first[0], second[0])
    h.temperature(500.0)
    gens.append(h.generation())
    h.temperature(500.0)                                 # nothing changed
    assert h.generation() == gens[-1]
    h.temperature(501.0)
    gens.append(h.generation())
    h.temperature(T)
    gens.append(h.generation())
    h.temperature(None)
    gens.append(h.generation())
    assert len(set(gens)) == len(gens) and gens == sorted(gens), gens
    check(f"law {law} back to 501", law, h.device(g_dev), ht.group_values(law, ht.update(law, g, 501.0, PARAMS[law])))
    h.close()


@pytest.mark.parametrize("law", LAWS)
def test_tile_loop_at_one_workgroup_per_cu_equals_the_shipped_grid_and_counts_non_finite_points(law):
    g, T = inputs(law, NLOOP, seed=12)
    g_dev = to_device(g)
    h = Handle(law, NLOOP).temperature(T)
    base = h.device(g_dev)
    h.option("blocks_per_cu", 1)
    assert same(h.device(g_dev), base)
    assert base[3]["n_nan"] == 0
    # one NaN gradient in a late-pass tile
    late = NLOOP - 70
    g2 = g.copy()
    g2[late, 1] = np.nan
    got = h.device(to_device(g2))
    assert got[3]["n_nan"] == 1 and np.isnan(got[0][late, 1]) and np.isfinite(np.delete(got[0], late, axis=0)).all()
    ok = np.delete(np.arange(NLOOP), late)
    assert np.array_equal(got[0][ok], base[0][ok]) and np.array_equal(got[1][ok], base[1][ok])
    h.close()


def test_a_point_with_a_vanishing_a_plus_b_t_is_counted_not_refused():
    n = 1000
    g, _ = inputs(ht.STATIONARY, n, seed=2)
    T = np.full(n, 300.0)
    T[777] = -2.0                                         # A + B T = 1 - 1 = 0 exactly
    h = Handle(ht.STATIONARY, n, (1.0, 0.5)).temperature(T)
    got = h.device(to_device(g))
    assert got[3]["n_nan"] == 1 and not np.isfinite(got[1][777, 0]) and np.isfinite(np.delete(got[1], 777, axis=0)).all()
    T[777] = -3.0                                         # A + B T < 0: a negative conductivity, not refused
    got = h.temperature(T).device(to_device(g))
    assert got[3]["n_nan"] == 0 and got[1][777, 0] == 2.0
    h.close()


def test_advance_and_revert_on_the_enthalpy():
    law, n = ht.PHASE_CHANGE, 1000
    g, T1 = inputs(law, n, seed=5)
    T2 = T1[::-1].copy()
    h1, h2 = (ht.phase_change(g, T, PARAMS[law])["enthalpy"].reshape(n, 1) for T in (T1, T2))
    h = Handle(law, n).temperature(T1)
    g_dev = to_device(g)
    got = h.device(g_dev)
    assert np.abs(got[2] - h1).max() <= bounds(law)["enthalpy"] * np.abs(h1).max()
    e1 = got[2]
    assert not h.enthalpy(_lib.S0).any()                  # written by every update, read by none: s0 is the natural state
    assert h.lib.dxm_advance(h.h) == 0
    assert np.array_equal(h.enthalpy(_lib.S0), e1) and np.array_equal(h.enthalpy(_lib.S1), e1)
    e2 = h.temperature(T2).device(g_dev)[2]
    assert np.abs(e2 - h2).max() <= bounds(law)["enthalpy"] * np.abs(h2).max() and np.array_equal(h.enthalpy(_lib.S0), e1)
    assert h.lib.dxm_revert(h.h) == 0
    assert np.array_equal(h.enthalpy(_lib.S1), e1)
    assert h.lib.dxm_set_state(h.h, _lib.S0, 0, h2.ctypes.data) == 0, err(h.lib)
    assert np.array_equal(h.enthalpy(_lib.S0), h2) and np.array_equal(h.enthalpy(_lib.S1), e1)
    h.close()


def test_algorithmic_bytes_with_and_without_a_field():
    sizes = []
    for law in LAWS:
        h = Handle(law, 64)
        sizes.append(h.lib.dxm_algorithmic_bytes(h.h))
        h.temperature(np.full(64, 300.0))
        sizes.append(h.lib.dxm_algorithmic_bytes(h.h))
        h.close()
    assert sizes == [120, 128, 136, 144]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS)
def test_every_refusal_has_its_sentence_and_leaves_the_handle_as_it_was(law):
    n = 300
    g, T = inputs(law, n, seed=6)
    h = Handle(law, n).temperature(T)
    lib = h.lib
    before, gen = h.device(to_device(g)), h.generation()
    what = "stationary heat" if law == ht.STATIONARY else "phase-change"
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and what in err(lib) and "only DXM_TANGENT_FULL" in err(lib)
    assert lib.dxm_tangent_size(h.h) == ht.WIDTH[law]
    eye, eyes = np.eye(3), np.tile(np.eye(3).reshape(9), (n, 1))
    for rc in (lib.dxm_set_frame(h.h, eye.ctypes.data), lib.dxm_set_frame_field(h.h, eyes.ctypes.data),
               lib.dxm_set_frame_field_device(h.h, to_device(eyes).data_ptr(), None)):
        assert rc < 0 and "a scalar conductivity" in err(lib)
    field = np.full(n, 1.0)
    assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "per-point parameter fields are not served for" in err(lib)
    assert lib.dxm_set_param_field_device(h.h, 0, to_device(field).data_ptr(), None) < 0 and "dxm_set_external_state" in err(lib)
    # the external state variable: a non-finite value is named with its point; an index the law does not have
    bad = T.copy()
    bad[123] = np.inf
    assert lib.dxm_set_external_state(h.h, 0, bad.ctypes.data) < 0 and "Temperature is not finite at point 123 (inf)" in err(lib)
    assert lib.dxm_set_external_state_uniform(h.h, 0, float("nan")) < 0 and "Temperature must be finite, got nan" in err(lib)
    for rc in (lib.dxm_set_external_state(h.h, 1, T.ctypes.data), lib.dxm_set_external_state_uniform(h.h, -1, 1.0),
               lib.dxm_set_external_state_device(h.h, 2, to_device(T).data_ptr(), None)):
        assert rc < 0 and "has no external state variable" in err(lib)
    assert lib.dxm_external_state_kind(h.h, 1) == -1 and lib.dxm_external_state_kind(h.h, 0) == 1
    # parameters: the offending value is in the message
    p = list(PARAMS[law])
    cases = [(1, np.inf, "B must be finite, got inf")] if law == ht.STATIONARY else \
        [(6, 0.0, "Tsmooth must be > 0, got 0"), (6, -1.0, "Tsmooth must be > 0, got -1"), (3, np.nan, "LiquidConductivity must be finite, got nan")]
    for idx, value, text in cases:
        q = list(p)
        q[idx] = value
        assert lib.dxm_set_params(h.h, (C.c_double * len(q))(*q), len(q)) < 0 and text in err(lib), err(lib)
        assert not lib.dxm_create(law, (C.c_double * len(q))(*q), len(q), 8, 0) and text in err(lib)
    assert not lib.dxm_create(law, (C.c_double * 3)(1.0, 2.0, 3.0), 3, 8, 0) and f"expects {len(p)} parameters" in err(lib)
    assert h.generation() == gen and same(h.device(to_device(g)), before)
    h.close()
    # the displacement forms: a 3-wide gradient is not a strain
    from dolfinx_materials_amd.gradient import gauss_points_hex

    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    h8 = Handle(law, 8)
    u, fl, ct = np.zeros(24), np.zeros((8, 3)), np.zeros((8, 13))
    rows, st = np.arange(8, dtype=np.int64), _lib.Stats()
    for fused in (1, 0):
        h8.option("fused_gradient", fused)
        rcs = (lib.dxm_integrate_displacement(h8.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, None, ct.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_rows(h8.h, mesh, u.ctypes.data, 0.0, fl.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)),
               lib.dxm_integrate_displacement_device(h8.h, mesh, to_device(u).data_ptr(), 0.0, to_device(fl).data_ptr(), to_device(ct).data_ptr(), None))
        for rc in rcs:
            assert rc < 0 and "takes a temperature gradient, not a strain" in err(lib), err(lib)
    h8.close()
    lib.dxm_mesh_destroy(mesh)


def test_a_custom_hardening_build_refuses_both_laws_with_their_own_sentence():
    """The library compiled for a user-supplied hardening law is dxmat.hip alone: it has no heat-transfer kernel and says so at
    dxm_create (the expressions are those of tests/test_custom_hardening.py: one build in the cache serves both files)."""
    import dolfinx_materials_amd.materials as mats

    h = mats.CustomHardening("sig0 + K * (pow(p + p0, n) - pow(p0, n))", "K * n * pow(p + p0, n - 1.0)", sig0=250.0, K=600.0, n=0.3, p0=1e-3)
    lib = _lib.load_custom(h.expr_R, h.expr_dR)
    assert lib.dxm_has_custom_hardening() == 1
    for law, text in ((ht.STATIONARY, "stationary heat transfer has no hardening law"), (ht.PHASE_CHANGE, "heat transfer with phase change has no hardening law")):
        p = list(PARAMS[law])
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 64, 0)
        msg = err(lib)
        assert text in msg and "served by the stock libdxmat, not by a custom-hardening build" in msg, msg
        # the tables are host code and answer in that build too
        b = _lib.law_blocks(law, lib)
        assert (b.n_external, b.tangent_width) == (1, ht.WIDTH[law])
    # ... while the stock library creates them
    Handle(ht.STATIONARY, 64).close()


def test_laws_without_an_external_state_variable_refuse_the_setters():
    lib = _lib.load()
    p = [70e3, 0.3, 250.0, 1e3]
    j2 = lib.dxm_create(_lib.LAW_J2_LINEAR, (C.c_double * 4)(*p), 4, 64, 0)
    assert j2, err(lib)
    T = np.full(64, 300.0)
    gen = lib.dxm_launch_generation(j2)
    for rc in (lib.dxm_set_external_state(j2, 0, T.ctypes.data), lib.dxm_set_external_state(j2, 0, None), lib.dxm_set_external_state_uniform(j2, 0, 300.0),
               lib.dxm_set_external_state_device(j2, 0, to_device(T).data_ptr(), None)):
        assert rc < 0 and "law 1 has no external state variable" in err(lib)
    assert lib.dxm_external_state_kind(j2, 0) == -1 and lib.dxm_launch_generation(j2) == gen and lib.dxm_algorithmic_bytes(j2) == 496
    lib.dxm_destroy(j2)


# ---- the map on the engine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", [False, True])
def test_quadrature_field_map_on_the_engine(subset):
    from dolfinx_materials_amd.field_map import QuadratureFieldMap, evaluate_block
    from dolfinx_materials_amd.jaxmat import JAXMaterial

    ncell, nqp = 1201, 4
    n = ncell * nqp
    law, prm = ht.PHASE_CHANGE, PARAMS[ht.PHASE_CHANGE]
    cells = np.sort(np.random.default_rng(5).permutation(ncell)[: 2 * ncell // 3]).astype(np.int32) if subset else None
    rows = np.arange(n) if cells is None else (cells[:, None] * nqp + np.arange(nqp)[None]).ravel()
    rest = np.setdiff1d(np.arange(n), rows)
    m = JAXMaterial(jm.HeatTransferPhaseChange.from_mfront_properties({"Tsmooth": 1.0}))
    q = QuadratureFieldMap(ncell, nqp, m, cells=cells)
    g, T = inputs(law, n, seed=21)
    temps = [T]
    q.register_gradient("TemperatureGradient", lambda c: g.reshape(ncell, nqp, 3)[c].reshape(-1, 3))
    q.register_external_state_variable("Temperature", lambda c: temps[0].reshape(ncell, nqp)[c].reshape(-1, 1))
    b = bounds(law)
    for step in range(2):
        q.update()
        ref = ht.phase_change(g[rows], temps[0][rows], prm)
        flux = q.fluxes["HeatFlux"].x.array.reshape(n, 3)
        jac = q.jacobian_flatten.x.array.reshape(n, 13)
        enth = np.asarray(q.internal_state_variables["Enthalpy"].x.array).reshape(n, 1)
        check(f"map subset={subset} step {step}", law, (flux[rows], jac[rows], enth[rows]), ht.group_values(law, ref))
        assert not flux[rest].any() and not jac[rest].any() and not enth[rest].any()
        K = evaluate_block(q.jacobians[("HeatFlux", "TemperatureGradient")], rows)
        assert K.shape == (len(rows), 3, 3) and np.array_equal(K.reshape(-1, 9), jac[rows, :9])
        dj = evaluate_block(q.jacobians[("HeatFlux", "Temperature")], rows)
        c = evaluate_block(q.jacobians[("Enthalpy", "Temperature")], rows)
        assert dj.shape == (len(rows), 3, 1) and np.array_equal(dj[:, :, 0], jac[rows, 9:12])
        assert c.shape == (len(rows), 1, 1) and np.abs(c[:, 0, 0] - ref["tangent"][:, 12]).max() <= b["dh_dT"] * np.abs(ref["tangent"][:, 12]).max()
        assert m.last_stats["n_nan"] == 0 and m.algorithmic_bytes_per_point == 144
        q.advance()
        temps[0] = T[::-1].copy()
    m.update_external_state_variable("Temperature", 400.0)
    assert m.algorithmic_bytes_per_point == 136 and m.kernel_name == "heat_transfer_kernel<1, 0"
    q.close()
    m.close()
