"""What the C ABI shows of every law's descriptor (``kLaws`` of ``csrc/dxmat.hip``), asked of a loaded library through ctypes alone:
sizes and names, accepted tangent layouts, refusals with their texts, parameter validation, the initial state, and two increments
of ``dxm_integrate_device`` in every accepted layout at N = 65 (one full 64-point tile plus a one-point partial tile).

``survey(lib)`` returns ``(meta, arrays)``.  ``tests/golden/make_law_surface.py`` records it from the PARENT's library;
``tests/test_gpu_law_surface.py`` asks the library under test the same questions and compares: the host side decides nothing the
kernels compute, so with unchanged device code every array is equal bit for bit."""
import ctypes as C

import numpy as np

from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.gradient import gauss_points_hex

import hosford_ref as hr
import ogden_ref as og
from helpers import B_F, B_V, E, H_LIN, NU, SIG0_F, SIG0_LIN, SIG0_V, SIGU_F, SIGU_V, fefp_path, j2_history, to_device, to_host
from test_gpu_ogden import inputs as ogden_inputs
from test_gpu_ramberg_osgood import strains as ro_strains
from test_ramberg_osgood_cpu import PRM as RO_PRM

N = 65
HOSFORD_A = 6.0
LAYOUTS = (0, 1, 2, 3)   # DXM_TANGENT_FULL, _SYM, _COEF, _PACK4
UNASSIGNED = (6, 8, 9, -1, 11)   # 11 = DXM_LAW_COUNT
INF = float("inf")

#: law id -> a valid parameter set
PARAMS = {
    _lib.LAW_ELASTIC_ISO: [E, NU],
    _lib.LAW_J2_LINEAR: [E, NU, SIG0_LIN, H_LIN],
    _lib.LAW_J2_VOCE: [E, NU, SIG0_V, SIGU_V, B_V],
    _lib.LAW_FEFP_J2_VOCE: [E, NU, SIG0_F, SIGU_F, B_F],
    _lib.LAW_FEFP_J2_LINEAR: [E, NU, SIG0_F, H_LIN],
    _lib.LAW_RAMBERG_OSGOOD: list(RO_PRM),
    _lib.LAW_OGDEN: [og.DEFAULTS["alpha"], og.DEFAULTS["mu"], og.DEFAULTS["K"]],
    _lib.LAW_HOSFORD_LINEAR: [hr.PROPS["E"], hr.PROPS["nu"], hr.PROPS["R0"], hr.PROPS["H"], HOSFORD_A],
}
ELASTIC_BRANCHES = [(0, 0.0), (0, -1.0), (1, 0.5), (1, -1.0)]
#: law id -> (parameter index, value) of every refusing branch of the law's parameter builder
INVALID = {law: list(ELASTIC_BRANCHES) for law in PARAMS if law != _lib.LAW_OGDEN}
INVALID[_lib.LAW_RAMBERG_OSGOOD] += [(2, 0.0), (3, 0.0), (4, 0.5), (4, INF)]
INVALID[_lib.LAW_OGDEN] = [(0, 0.0), (0, INF), (1, 0.0), (1, INF), (2, 0.0), (2, INF)]
INVALID[_lib.LAW_HOSFORD_LINEAR] += [(2, 0.0), (2, INF), (3, -1.0), (3, INF), (4, 1.0), (4, INF)]


def make_inputs():
    """law id -> the gradients of the two increments, (N, n_grad) each: the generators of the per-law GPU tests, seeded, with a fair
    share of yielded points (the recorded stats say how many)."""
    lin, voce = j2_history(N, seed=11, sig0=SIG0_LIN), j2_history(N, seed=12, sig0=SIG0_V)
    fefp = fefp_path(N, seed=13)
    heps = hr.mixed_inputs(N, HOSFORD_A, seed=14, trivial_state=True)[0]
    return {
        _lib.LAW_ELASTIC_ISO: [lin[1], lin[2]],
        _lib.LAW_J2_LINEAR: [lin[1], lin[2]],
        _lib.LAW_J2_VOCE: [voce[1], voce[2]],
        _lib.LAW_FEFP_J2_VOCE: [fefp[6], fefp[12]],
        _lib.LAW_FEFP_J2_LINEAR: [fefp[6], fefp[12]],
        _lib.LAW_RAMBERG_OSGOOD: [ro_strains(N, 15), ro_strains(N, 16)],
        _lib.LAW_OGDEN: [ogden_inputs(N, 17), ogden_inputs(N, 18)],
        _lib.LAW_HOSFORD_LINEAR: [heps, 1.5 * heps],
    }


def _err(lib):
    return (lib.dxm_last_error() or b"").decode()


def _create(lib, law, params, n=N):
    arr = (C.c_double * max(len(params), 1))(*params)
    return lib.dxm_create(law, arr, len(params), n, 0)


def _law_info(lib, law):
    info = _lib.LawInfo()
    rc = lib.dxm_law_info_get(law, C.byref(info))
    if rc != 0:
        return {"rc": rc, "error": _err(lib)}
    out = {k: getattr(info, k) for k in ("n_grad", "n_flux", "n_params", "n_isv_fields", "n_isv_total", "algorithmic_bytes_per_point")}
    out["isv_dim"] = list(info.isv_dim)
    out["isv_name"] = [(s or b"").decode() for s in info.isv_name]
    return out


def _states(lib, h, dims, which):
    """every addressable field of one state buffer: field index -> (n, dim) array"""
    out = {}
    for f, dim in enumerate(dims):
        a = np.full((N, dim), np.nan)
        assert lib.dxm_get_state(h, which, f, a.ctypes.data) == 0, _err(lib)
        out[f] = a
    return out


def _field_dims(lib, h, info):
    """dimensions of the addressable fields, hidden ones included, and what the first index past them is answered with"""
    dims = [d for d in info["isv_dim"][: info["n_isv_fields"]]]
    probe = np.zeros((N, 6))
    f = len(dims)
    while f < _lib.DXM_MAX_STATE_FIELDS and lib.dxm_get_state(h, _lib.S0, f, probe.ctypes.data) == 0:
        dims.append(6)   # the hidden fields of FeFp and Hosford are symmetric tensors
        f += 1
    rc = lib.dxm_get_state(h, _lib.S0, len(dims), probe.ctypes.data)
    return dims, {"rc": rc, "error": _err(lib)}


def _unit_cell():
    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    return coords, np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)


def _fused_refusal(lib, law, info):
    coords, conn, qp = _unit_cell()
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, _err(lib)
    h = _create(lib, law, PARAMS[law], n=8)
    assert h, _err(lib)
    u = to_device(np.zeros(24))
    flux = to_device(np.zeros((8, info["n_flux"])))
    ct = to_device(np.zeros((8, info["n_flux"] * info["n_grad"])))
    rc = lib.dxm_integrate_displacement_device(h, mesh, u.data_ptr(), 0.0, flux.data_ptr(), ct.data_ptr(), None)
    out = {"rc": rc, "error": _err(lib) if rc else ""}
    lib.dxm_destroy(h)
    lib.dxm_mesh_destroy(mesh)
    return out


def _two_increments(lib, law, layout, grads, dims, arrays, key):
    h = _create(lib, law, PARAMS[law])
    assert h and lib.dxm_set_tangent_layout(h, layout) == 0, _err(lib)
    tsize = lib.dxm_tangent_size(h)
    stats = []
    for k, g in enumerate(grads):
        gd = to_device(g)
        flux = to_device(np.zeros_like(g))
        ct = to_device(np.zeros((N, tsize)))
        assert lib.dxm_integrate_device(h, gd.data_ptr(), 0.0, flux.data_ptr(), ct.data_ptr(), None) == 0, _err(lib)
        st = _lib.Stats()
        rc = lib.dxm_get_stats(h, C.byref(st))
        stats.append({"rc": rc, **st.as_dict()})
        arrays[f"{key}/inc{k}/flux"] = to_host(flux)
        arrays[f"{key}/inc{k}/tangent"] = to_host(ct)
        for f, a in _states(lib, h, dims, _lib.S1).items():
            arrays[f"{key}/inc{k}/state{f}"] = a
        if k == 0:
            assert lib.dxm_advance(h) == 0
    lib.dxm_destroy(h)
    return stats


def survey(lib, inputs=None):
    inputs = make_inputs() if inputs is None else inputs
    meta, arrays = {"laws": {}, "unassigned": {}}, {}
    for law in UNASSIGNED:
        info = _law_info(lib, law)
        h = _create(lib, law, [E, NU])
        meta["unassigned"][str(law)] = {"law_info": info, "create_null": not h, "create_error": _err(lib)}
        if h:
            lib.dxm_destroy(h)
    for law, prm in PARAMS.items():
        m = meta["laws"][str(law)] = {}
        info = m["law_info"] = _law_info(lib, law)
        h = _create(lib, law, prm)
        assert h, _err(lib)
        m["dxm_law"] = lib.dxm_law(h)
        m["kernel_name"] = lib.dxm_kernel_name(h).decode()
        m["algorithmic_bytes"] = lib.dxm_algorithmic_bytes(h)
        m["layouts"] = {}
        for layout in LAYOUTS:
            rc = lib.dxm_set_tangent_layout(h, layout)
            m["layouts"][str(layout)] = {"rc": rc, "error": _err(lib) if rc else "", "tangent_size": lib.dxm_tangent_size(h)}
        rc = lib.dxm_set_tangent_layout(h, 7)
        m["layouts"]["7"] = {"rc": rc, "error": _err(lib)}
        # per-point parameter fields
        field = np.full(N, prm[0])
        rc = lib.dxm_set_param_field(h, 0, field.ctypes.data)
        m["param_field"] = {"rc": rc, "error": _err(lib) if rc else ""}
        if rc == 0:
            m["param_field"].update(kernel_name=lib.dxm_kernel_name(h).decode(), algorithmic_bytes=lib.dxm_algorithmic_bytes(h),
                                    mask=lib.dxm_param_field_mask(h))
            assert lib.dxm_set_param_field(h, 0, None) == 0, _err(lib)
            m["param_field"]["kernel_name_after_unbind"] = lib.dxm_kernel_name(h).decode()
        # the state straight after dxm_create, both buffers
        dims, past = _field_dims(lib, h, info)
        m["field_dims"], m["field_past_the_last"] = dims, past
        for which in (_lib.S0, _lib.S1):
            for f, a in _states(lib, h, dims, which).items():
                arrays[f"law{law}/initial/s{which}/state{f}"] = a
        lib.dxm_destroy(h)
        # parameter validation
        bad = _create(lib, law, prm + [1.0])
        m["wrong_count"] = {"null": not bad, "error": _err(lib)}
        m["invalid"] = []
        for idx, value in INVALID[law]:
            q = list(prm)
            q[idx] = value
            bad = _create(lib, law, q)
            m["invalid"].append({"index": idx, "value": repr(value), "null": not bad, "error": _err(lib)})
            if bad:
                lib.dxm_destroy(bad)
        if law in (_lib.LAW_OGDEN, _lib.LAW_HOSFORD_LINEAR):
            m["fused_displacement"] = _fused_refusal(lib, law, info)
        m["stats"] = {}
        for layout in LAYOUTS:
            if m["layouts"][str(layout)]["rc"] == 0:
                m["stats"][str(layout)] = _two_increments(lib, law, layout, inputs[law], dims, arrays, f"law{law}/layout{layout}")
    return meta, arrays
