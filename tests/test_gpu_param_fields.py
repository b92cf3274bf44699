"""GPU: per-point material property fields of the small-strain J2 laws (``dxm_set_param_field`` and the kernels of
``csrc/param_fields.hip``), through ctypes and the C ABI, against the oracle.

The oracle (``oracle/constitutive_np.py``) takes scalar parameters: piecewise-constant fields are checked against one oracle call
per group, continuous fields against ``tests/param_fields_ref.py``, which ``tests/test_param_fields_cpu.py`` pins to the oracle.
Bound: 1e-12 relative per point row, the project's J2 bound (``tests/test_gpu_parity.py::TIGHT``).  Measured on an MI355X: at
most 5.5e-14 over all cases (stress, tangent, state), no point with an undecidable branch."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib, conventions
from dolfinx_materials_amd._lib import DxmError
from dolfinx_materials_amd.hip_material import HIPMaterial
from oracle import constitutive_np as onp
from param_fields_ref import (BASE, NAMES, graded_fields, group_slices, j2_update_fields, load_history, param_arrays, undecidable)

pytestmark = pytest.mark.gpu
TIGHT = 1e-12
SIZES = [1, 63, 64, 65, 100003]
LINEAR_SUBSETS = [c for r in range(1, 5) for c in itertools.combinations(NAMES["linear"], r)]
VOCE_SUBSETS = [("sig0",), ("E",), ("sig0", "sigu", "b"), tuple(NAMES["voce"])]


def _behavior(kind):
    b = BASE[kind]
    hard = jm.LinearHardening(b["sig0"], b["H"]) if kind == "linear" else jm.VoceHardening(b["sig0"], b["sigu"], b["b"])
    return jm.vonMisesIsotropicHardening(jm.LinearElasticIsotropic(b["E"], b["nu"]), hard)


def _key(name):
    return ("elasticity." if name in ("E", "nu") else "yield_stress.") + name


def _material(kind, n, fields, **kw):
    mat = HIPMaterial(_behavior(kind), property_fields=True, lazy_isv=False, **kw)
    mat.set_data_manager(n)
    for name, a in fields.items():
        mat.update_material_property(_key(name), a)
        if np.all(a == a[0]):    # (one point, a constant group: a number to the Python layer -- bound as a field at the C ABI)
            for h, lo, hi, _ in mat._parts:
                mat._chk(mat._lib.dxm_set_param_field(h, NAMES[kind].index(name), np.ascontiguousarray(a[lo:hi]).ctypes.data))
    return mat


def _row_rel(a, b):
    a, b = np.asarray(a).reshape(len(b), -1), np.asarray(b).reshape(len(b), -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)


def _check_history(kind, n, fields, reference):
    """Three increments with advance; ``reference(eps, epsp, p)`` -> dictionary of the oracle."""
    mat = _material(kind, n, fields)
    streams = (2 if ("E" in fields or "nu" in fields) else 0) + sum(1 for k in fields if k not in ("E", "nu"))
    assert mat._lib.dxm_algorithmic_bytes(mat._require()) == 496 + 8 * streams and mat.kernel_name.startswith("small_strain_field_kernel<")
    assert n == 1 or mat.algorithmic_bytes_per_point == 496 + 8 * streams
    epsp, p = np.zeros((n, 6)), np.zeros(n)
    sig0 = fields.get("sig0", BASE[kind]["sig0"])
    any_plastic = False
    for eps in load_history(n):
        flux, isv, ct = mat.integrate(eps)
        flux, isv, ct = np.asarray(flux), np.asarray(isv), np.asarray(ct)
        ref = reference(eps, epsp, p)
        skip = undecidable(ref, sig0)
        share = skip.mean()
        print(f"{kind} n={n} fields={sorted(fields)} undecidable share {share:.2e} plastic {ref['plastic'].mean():.3f}")
        assert share <= 1e-4
        ok = ~skip
        errs = dict(stress=_row_rel(flux, ref["sig"])[ok].max(initial=0.0), tangent=_row_rel(ct, ref["Ct"])[ok].max(initial=0.0),
                    epsp=(np.abs(isv[:, 1:] - ref["epsp"]).max(axis=1) / max(np.abs(ref["epsp"]).max(), 1e-300))[ok].max(initial=0.0),
                    p=(np.abs(isv[:, 0] - ref["p"]) / max(ref["p"].max(), 1e-300))[ok].max(initial=0.0))
        print("   errors", {k: f"{v:.2e}" for k, v in errs.items()})
        assert all(v <= TIGHT for v in errs.values()), errs
        st = mat.last_stats
        assert st["n_nan"] == 0 and st["n_not_converged"] == 0 and abs(st["n_plastic"] - int(ref["plastic"].sum())) <= int(skip.sum())
        any_plastic |= bool(ref["plastic"].any())
        mat.data_manager.update()
        epsp, p = ref["epsp"], ref["p"]
    mat.close()
    return any_plastic


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,subset", [("linear", s) for s in LINEAR_SUBSETS] + [("voce", s) for s in VOCE_SUBSETS])
def test_continuous_fields_match_the_pinned_restatement_of_the_oracle(kind, subset, n):
    fields = graded_fields(kind, n, subset)
    plastic = _check_history(kind, n, fields, lambda eps, epsp, p: j2_update_fields(eps, epsp, p, kind, *param_arrays(kind, fields, n)))
    assert plastic or n < 63


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_seven_group_fields_match_the_oracle_called_group_by_group(kind, n):
    groups = 7
    fields = graded_fields(kind, n, NAMES[kind], groups=groups)

    def reference(eps, epsp, p):
        out = None
        for sl in group_slices(n, groups):
            v = {k: float(fields[k][sl.start]) for k in NAMES[kind]}
            hard = onp.LinearHardening(v["sig0"], v["H"]) if kind == "linear" else onp.VoceHardening(v["sig0"], v["sigu"], v["b"])
            r = onp.j2_update(eps[sl], epsp[sl], p[sl], v["E"], v["nu"], hard)
            if out is None:
                out = {k: np.zeros((n,) + r[k].shape[1:], dtype=r[k].dtype) for k in ("sig", "epsp", "p", "Ct", "plastic", "f_trial")}
            for k in out:
                out[k][sl] = r[k]
        return out

    _check_history(kind, n, fields, reference)


@pytest.mark.parametrize("layout", ["full", "sym", "coef", "pack4"])
@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_a_constant_field_equals_the_uniform_handle_bit_for_bit(kind, layout):
    n = 20011
    uni = HIPMaterial(_behavior(kind), lazy_isv=False, tangent_layout=layout)
    uni.set_data_manager(n)
    fld = HIPMaterial(_behavior(kind), property_fields=True, lazy_isv=False, tangent_layout=layout)
    fld.set_data_manager(n)
    for name in NAMES[kind]:
        fld.update_material_property(_key(name), np.full(n, BASE[kind][name]) + 0.0)   # (uniform array: stays uniform)
    assert fld.kernel_name == uni.kernel_name
    for h in fld._handles():     # bind constant fields at the C ABI: the Python layer would turn them into numbers
        for i, name in enumerate(NAMES[kind]):
            a = np.full(n, BASE[kind][name])
            fld._chk(fld._lib.dxm_set_param_field(h, i, a.ctypes.data))
        assert fld._lib.dxm_param_field_mask(h) == (1 << len(NAMES[kind])) - 1
    assert fld.kernel_name.startswith("small_strain_field_kernel<")
    for eps in load_history(n):
        a, b = uni.integrate(eps), fld.integrate(eps)
        for x, y, what in zip(a, b, ("stress", "state", "tangent")):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, kind, layout)
        assert uni.last_stats == fld.last_stats and uni.last_stats["n_plastic"] > 0
        uni.data_manager.update()
        fld.data_manager.update()
    uni.close()
    fld.close()


@pytest.mark.parametrize("layout", ["sym", "coef", "pack4"])
@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_packed_tangent_layouts_hold_the_block_of_the_full_layout(kind, layout):
    n = 4099
    fields = graded_fields(kind, n, NAMES[kind])
    full, packed = _material(kind, n, fields), _material(kind, n, fields, tangent_layout=layout)
    eps = load_history(n)[-1]
    f0, i0, c0 = (np.asarray(x) for x in full.integrate(eps))
    f1, i1, c1 = (np.asarray(x) for x in packed.integrate(eps))
    assert np.array_equal(f0, f1) and np.array_equal(i0, i1)
    block = {"sym": conventions.unpack_sym_tangent, "coef": conventions.tangent_from_coefficients,
             "pack4": lambda c: conventions.tangent_from_pack4(f1, c)}[layout](c1)
    assert _row_rel(block, c0.reshape(n, 36)).max() <= 1e-14
    full.close()
    packed.close()


@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_chunked_host_path_offsets_the_streams(kind):
    """100 003 points: three chunks of the packed host path.  One chunk (option pipeline = 0) gives the same bits."""
    n = 100003
    fields = graded_fields(kind, n, NAMES[kind])
    a, b = _material(kind, n, fields), _material(kind, n, fields)
    b.set_option("pipeline", 0)
    eps = load_history(n)[-1]
    ra, rb = a.integrate(eps), b.integrate(eps)
    for x, y in zip(ra, rb):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    ref = j2_update_fields(eps, np.zeros((n, 6)), np.zeros(n), kind, *param_arrays(kind, fields, n))
    assert _row_rel(np.asarray(ra[0]), ref["sig"]).max() <= TIGHT          # (and every chunk read ITS points' parameters)
    # rows form with the internal state variables delivered into bound rows
    rows = np.ascontiguousarray(np.random.default_rng(3).permutation(n + 50)[:n].astype(np.int64))
    flux, tang = np.zeros((n + 50, 6)), np.zeros((n + 50, 36))
    isv_p, isv_e = np.zeros((n + 50, 1)), np.zeros((n + 50, 6))
    a.bind_state_outputs({"p": isv_p, "epsp": isv_e}, deliver=True, rows=True)
    a.integrate_rows(eps, rows, flux, tang)
    assert np.array_equal(flux[rows], np.asarray(rb[0])) and np.array_equal(tang[rows], np.asarray(rb[2]).reshape(n, 36))
    assert np.array_equal(isv_p[rows, 0], np.asarray(rb[1])[:, 0]) and np.array_equal(isv_e[rows], np.asarray(rb[1])[:, 1:])
    a.close()
    b.close()


def test_device_pointer_forms():
    torch = pytest.importorskip("torch")
    kind, n = "voce", 5003
    fields = graded_fields(kind, n, ["sig0", "E", "b"])
    host = _material(kind, n, fields)
    eps = load_history(n)[-1]
    f0, i0, c0 = (np.asarray(x) for x in host.integrate(eps))
    # fields from device arrays (law-level values), update from device arrays
    dev = HIPMaterial(_behavior(kind), property_fields=True, lazy_isv=False)
    dev.set_data_manager(n)
    h = dev._require()
    st = torch.cuda.current_stream().cuda_stream
    g0 = dev.launch_generation
    keep = []
    for name, a in fields.items():
        t = torch.from_numpy(a).to("cuda:0")
        keep.append(t)
        dev._chk(dev._lib.dxm_set_param_field_device(h, NAMES[kind].index(name), t.data_ptr(), st or None))
    assert dev._lib.dxm_param_field_mask(h) == 0b10101 and dev._lib.dxm_algorithmic_bytes(h) == 496 + 8 * 4
    assert dev.launch_generation != g0
    d_eps = torch.from_numpy(eps).to("cuda:0")
    d_flux = torch.empty((n, 6), dtype=torch.float64, device="cuda:0")
    d_ct = torch.empty((n, 36), dtype=torch.float64, device="cuda:0")
    dev.integrate_device(d_eps.data_ptr(), d_flux.data_ptr(), d_ct.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(d_flux.cpu().numpy(), f0) and np.array_equal(d_ct.cpu().numpy(), c0.reshape(n, 36))
    assert dev.stats()[1]["n_nan"] == 0
    host.close()
    dev.close()


@pytest.mark.parametrize("mesh_kind", ["hex8", "tet4", "tet10"])
def test_fused_gradients_read_the_fields(mesh_kind):
    """The three in-kernel gradient sources against the same material fed by the gradient kernel (option fused_gradient = 0)."""
    from dolfinx_materials_amd.gradient import Hex8Mesh, SimplexMesh, Tet4Mesh
    from helpers import KUHN
    from test_gpu_gradient import make_mesh

    m, coords = make_mesh(6, distort=0.2, seed=4)
    rng = np.random.default_rng(8)
    if mesh_kind == "hex8":
        mesh = Hex8Mesh(coords, m.conn)
    else:
        tets = np.concatenate([m.conn[:, list(k)] for k in KUHN], axis=0).astype(np.int32)
        if mesh_kind == "tet4":
            mesh = Tet4Mesh(coords, tets, nqp=4)
        else:
            mesh, coords = SimplexMesh.lagrange(coords, tets, degree=2)
    u = (coords * np.array([6e-3, -2e-3, -2e-3]) + 2e-4 * rng.standard_normal(coords.shape)).ravel()
    n = mesh.npoints
    kind = "voce"
    fields = graded_fields(kind, n, NAMES[kind])
    a, b = _material(kind, n, fields), _material(kind, n, fields)
    b.set_option("fused_gradient", 0)
    ra, rb = a.integrate_displacement(mesh, u), b.integrate_displacement(mesh, u)
    assert a.last_stats["n_plastic"] > 0 and a.last_stats["n_plastic"] < n
    assert abs(a.last_stats["n_plastic"] - b.last_stats["n_plastic"]) <= max(1, n // 10000)
    same = _row_rel(np.asarray(ra[0]), np.asarray(rb[0])) <= 1e-9       # (a point may change branch with the gradient's last bits)
    assert same.mean() >= 1 - 1e-4
    assert _row_rel(np.asarray(ra[0])[same], np.asarray(rb[0])[same]).max() <= 1e-11
    a.close()
    b.close()


@pytest.mark.parametrize("kind,n", [("linear", 1001), ("voce", 70001)])
def test_two_parts_on_one_gpu_equal_one_handle(kind, n):
    fields = graded_fields(kind, n, NAMES[kind])
    one, two = _material(kind, n, fields), _material(kind, n, fields, devices=[0, 0])
    for eps in load_history(n):
        for x, y in zip(one.integrate(eps), two.integrate(eps)):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        one.data_manager.update()
        two.data_manager.update()
    one.close()
    two.close()


def test_masks_and_bytes_for_every_subset():
    lib = _lib.load()
    for kind, law in (("linear", _lib.LAW_J2_LINEAR), ("voce", _lib.LAW_J2_VOCE)):
        names = NAMES[kind]
        n = 130
        prm = np.array([BASE[kind][k] for k in names])
        h = lib.dxm_create(law, prm.ctypes.data_as(C.POINTER(C.c_double)), prm.size, n, 0)
        assert h
        vals = graded_fields(kind, n, names)
        for mask in range(1 << len(names)):
            for i, name in enumerate(names):
                a = vals[name] if mask >> i & 1 else None
                assert lib.dxm_set_param_field(h, i, None if a is None else a.ctypes.data) == 0
            streams = (2 if mask & 3 else 0) + bin(mask >> 2).count("1")
            assert lib.dxm_param_field_mask(h) == mask and lib.dxm_algorithmic_bytes(h) == 496 + 8 * streams
        assert lib.dxm_set_param_field(h, len(names), vals["E"].ctypes.data) < 0
        lib.dxm_destroy(h)


def test_bad_values_are_refused_with_the_point_and_nothing_changes():
    kind, n = "linear", 777
    fields = graded_fields(kind, n, ["E", "sig0"])
    mat = _material(kind, n, fields)
    eps = load_history(n)[-1]
    before = [np.array(x) for x in mat.integrate(eps)]
    gen = mat.launch_generation
    for name, at, value in (("E", 5, np.nan), ("E", 700, 0.0), ("E", 13, -3.0), ("nu", 64, 0.5), ("nu", 0, -1.0), ("sig0", 776, np.inf), ("H", 1, np.nan)):
        bad = graded_fields(kind, n, [name])[name]
        bad[at] = value
        with pytest.raises(DxmError, match=rf"point {at}\b"):
            mat.update_material_property(_key(name), bad)
        assert mat.launch_generation == gen
    assert mat._lib.dxm_param_field_mask(mat._require()) == 0b101
    after = [np.array(x) for x in mat.integrate(eps)]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # bind / unbind change the launch generation
    mat.update_material_property(_key("H"), graded_fields(kind, n, ["H"])["H"])
    g1 = mat.launch_generation
    assert g1 != gen
    mat.update_material_property(_key("H"), 5e3)
    assert mat.launch_generation != g1 and mat._lib.dxm_param_field_mask(mat._require()) == 0b101
    # a new uniform nu while E is a field: the (lambda, mu) streams follow
    mat.update_material_property(_key("nu"), 0.25)
    got = np.asarray(mat.integrate(eps)[0])
    f2 = dict(fields, nu=np.full(n, 0.25))
    ref = j2_update_fields(eps, np.zeros((n, 6)), np.zeros(n), kind, *param_arrays(kind, f2, n))
    assert _row_rel(got, ref["sig"]).max() <= TIGHT
    mat.close()


@pytest.mark.parametrize("make", [lambda: jm.ElasticBehavior(jm.LinearElasticIsotropic(70e3, 0.3)),
                                  lambda: jm.RambergOsgoodNonLinearElasticity(jm.LinearElasticIsotropic(70e3, 0.3), 100.0, 0.5, 4.0),
                                  lambda: jm.FeFpJ2Plasticity(jm.LinearElasticIsotropic(70e3, 0.3), jm.VoceHardening(500.0, 750.0, 1e3))])
def test_laws_out_of_scope_refuse_at_the_c_abi(make):
    mat = HIPMaterial(make(), property_fields=True)
    mat.set_data_manager(16)
    h = mat._require()
    a = np.full(16, 70e3)
    assert mat._lib.dxm_set_param_field(h, 0, a.ctypes.data) < 0 and b"only" in mat._lib.dxm_last_error()
    assert mat._lib.dxm_set_param_field_device(h, 0, None, None) < 0
    assert mat._lib.dxm_param_field_mask(h) == 0
    assert mat._lib.dxm_algorithmic_bytes(h) == mat._info.algorithmic_bytes_per_point
    with pytest.raises(NotImplementedError):
        mat.update_material_property("elasticity.E", np.linspace(1.0, 2.0, 16))
    mat.close()
