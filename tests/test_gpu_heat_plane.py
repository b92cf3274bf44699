"""GPU: the two-dimensional heat-transfer laws (DXM_LAW_HEAT_STATIONARY_2D = 35, DXM_LAW_HEAT_PHASE_CHANGE_2D = 36;
``heat_plane_kernel<law, 0>``) in their array form, through the C ABI (ctypes).

* Against laws 16 / 17 on the padded gradient ``[g0, g1, 0]`` BIT FOR BIT: flux, the corresponding tangent entries, the enthalpy and
  ``n_nan``; uniform temperature and a temperature field; N = 1, 63, 64, 65, 257 and ``tile_loop_cases.size_for(num_cu, 1)``, the last
  with option ``blocks_per_cu = 1`` (the tile loop past its first pass) and with the shipped grid.  The outputs are allocated 8 rows
  longer and pre-filled with NaN: those rows stay NaN.
* Against ``heat_transfer_ref`` at the bounds ``tests/test_gpu_heat_transfer.py`` uses for laws 16 / 17 (``max(1e-12, 8 x the
  restatement's recorded deviation)`` per output group).
* Law 36: the temperatures of every batch of 63 points or more span solid, transition and liquid with at least a tenth of the points
  in each -- a condition on the inputs, checked here in numpy before anything is launched (a batch of ONE point cannot hold it and is
  exempt).
* A point with ``A + B T = 0`` is counted in ``n_nan``, not refused, its neighbours untouched.
"""
import ctypes as C

import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import heat_plane_ref as hp
import heat_transfer_ref as ht
import tile_loop_cases as tl
from helpers import to_device, to_host
from test_gpu_heat_transfer import bounds as wide_bounds

pytestmark = pytest.mark.gpu
PAD = 8


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


class Handle:
    """one dxm_material of a heat-transfer law of either width, driven through ctypes alone"""

    def __init__(self, law, n, prm=None):
        two = law in hp.LAWS_2D
        p = list(prm if prm is not None else hp.PARAMS[law if two else {v: k for k, v in hp.WIDE.items()}[law]])
        self.lib, self.n, self.law = _lib.load(), n, law
        self.ng = 2 if two else 3
        self.h = self.lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        self.width = self.lib.dxm_tangent_size(self.h)
        assert self.width == (hp.WIDTH[law] if two else ht.WIDTH[law])
        self.has_state = law in (hp.PHASE_CHANGE_2D, ht.PHASE_CHANGE)

    def temperature(self, T):
        if np.ndim(T) == 0:
            rc = self.lib.dxm_set_external_state_uniform(self.h, 0, float(T))
        else:
            a = np.ascontiguousarray(T, dtype=np.float64)
            assert a.shape == (self.n,)
            rc = self.lib.dxm_set_external_state(self.h, 0, a.ctypes.data)
        assert rc == 0, err(self.lib)
        return self

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def stats(self):
        st = _lib.Stats()
        assert self.lib.dxm_get_stats(self.h, C.byref(st)) == 0, err(self.lib)
        return st.as_dict()

    def enthalpy(self, which=_lib.S1):
        h = np.full((self.n, 1), np.nan)
        if self.has_state:
            assert self.lib.dxm_get_state(self.h, which, 0, h.ctypes.data) == 0, err(self.lib)
        return h

    def device(self, g_dev):
        """(flux, tangent, enthalpy, stats); the PAD rows past the batch must come back NaN"""
        import torch

        f = torch.full((self.n + PAD, self.ng), float("nan"), dtype=torch.float64, device=g_dev.device)
        c = torch.full((self.n + PAD, self.width), float("nan"), dtype=torch.float64, device=g_dev.device)
        assert self.lib.dxm_integrate_device(self.h, g_dev.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        f, c = to_host(f), to_host(c)
        assert np.isnan(f[self.n:]).all() and np.isnan(c[self.n:]).all(), "rows past the launch's points were written"
        return f[:self.n], c[:self.n], self.enthalpy(), self.stats()

    def close(self):
        self.lib.dxm_destroy(self.h)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def num_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def mix_condition(law, T, n):
    if law == hp.PHASE_CHANGE_2D and n >= 63:
        shares = hp.branch_shares(T, hp.PARAMS[law])
        assert min(shares) >= 0.1, shares


def compare_with_the_wide_law(law, n, g, T, tag, blocks_per_cu=None):
    """the 2-wide law on g against the 3-wide law on [g0, g1, 0], bit for bit; returns the 2-wide result"""
    g_dev, g3_dev = to_device(g), to_device(hp.pad(g))
    a, b = Handle(law, n).temperature(T), Handle(hp.WIDE[law], n).temperature(T)
    if blocks_per_cu:
        a.option("blocks_per_cu", blocks_per_cu)
    got, wide = a.device(g_dev), b.device(g3_dev)
    flux, tangent = hp.narrow(law, wide[0], wide[1])
    assert bits(got[0], flux), tag
    assert bits(got[1], tangent), tag
    assert bits(got[2], wide[2]) or not a.has_state, tag
    assert got[3] == wide[3], (tag, got[3], wide[3])
    assert not got[1][:, [1, 2]].any()                                  # the two structural zeros are written
    a.close()
    b.close()
    return got


def check_against_restatement(tag, law, got, ref):
    limits = wide_bounds(hp.WIDE[law])
    groups = hp.wide_groups(law, got[0], got[1], got[2])
    want = hp.wide_groups(law, ref["flux"], ref["tangent"], ref["enthalpy"])
    for name, bound in limits.items():
        dev = ht.relative_deviation(groups[name], want[name])
        print(f"heat plane parity {tag}: {name} {dev:.3e} (bound {bound:.2e})")
        assert dev <= bound, (tag, name, dev, bound)


@pytest.mark.parametrize("law", hp.LAWS_2D)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_array_form_equals_the_three_wide_law_on_the_padded_gradient_bit_for_bit(N, law):
    g, T = hp.inputs(law, N, seed=100 + N)
    mix_condition(law, T, N)
    got = compare_with_the_wide_law(law, N, g, T, f"N={N} law {law} field")
    check_against_restatement(f"N={N} law {law} field", law, got, hp.update(law, g, T, hp.PARAMS[law]))
    assert got[3] == dict(n_points=N, n_plastic=0, n_not_converged=0, n_nan=0, max_local_iters=0)
    Tu = 933.4 if law == hp.PHASE_CHANGE_2D else 1100.0                  # inside the transition of Tsmooth = 1
    got = compare_with_the_wide_law(law, N, g, Tu, f"N={N} law {law} uniform")
    check_against_restatement(f"N={N} law {law} uniform", law, got, hp.update(law, g, Tu, hp.PARAMS[law]))


@pytest.mark.parametrize("law", hp.LAWS_2D)
def test_tile_loop_at_one_workgroup_per_cu_equals_the_three_wide_law_and_the_shipped_grid(law):
    cu = num_cu()
    N = tl.size_for(cu, 1)
    assert tl.passes(N, cu, 1) == 4
    g, T = hp.inputs(law, N, seed=12)
    mix_condition(law, T, N)
    one = compare_with_the_wide_law(law, N, g, T, f"tile loop law {law}", blocks_per_cu=1)
    shipped = compare_with_the_wide_law(law, N, g, T, f"shipped grid law {law}")
    assert all(bits(x, y) for x, y in zip(one[:3], shipped[:3])) and one[3] == shipped[3]
    check_against_restatement(f"tile loop law {law}", law, one, hp.update(law, g, T, hp.PARAMS[law]))
    # a uniform temperature through the loop, and one NaN gradient in a late-pass tile
    compare_with_the_wide_law(law, N, g, 900.0, f"tile loop law {law} uniform", blocks_per_cu=1)
    late = N - 70
    g2 = g.copy()
    g2[late, 1] = np.nan
    got = compare_with_the_wide_law(law, N, g2, T, f"tile loop law {law} NaN", blocks_per_cu=1)
    ok = np.delete(np.arange(N), late)
    assert got[3]["n_nan"] == 1 and np.isnan(got[0][late, 1]) and bits(got[0][ok], one[0][ok]) and bits(got[1][ok], one[1][ok])


def test_a_point_with_a_vanishing_a_plus_b_t_is_counted_not_refused():
    n = 1000
    law = hp.STATIONARY_2D
    g, _ = hp.inputs(law, n, seed=2)
    T = np.full(n, 300.0)
    T[777] = -2.0                                         # A + B T = 1 - 1 = 0 exactly
    a, b = Handle(law, n, (1.0, 0.5)).temperature(T), Handle(hp.WIDE[law], n, (1.0, 0.5)).temperature(T)
    got, wide = a.device(to_device(g)), b.device(to_device(hp.pad(g)))
    assert got[3]["n_nan"] == 1 == wide[3]["n_nan"] and not np.isfinite(got[1][777, 0])
    assert np.isfinite(np.delete(got[1], 777, axis=0)).all() and np.isfinite(np.delete(got[0], 777, axis=0)).all()
    ref = hp.update(law, g, np.full(n, 300.0), (1.0, 0.5))
    ok = np.delete(np.arange(n), 777)
    assert bits(got[0][ok], a.temperature(np.full(n, 300.0)).device(to_device(g))[0][ok])       # the neighbours are untouched
    assert np.abs(got[0][ok] - ref["flux"][ok]).max() <= 1e-12 * np.abs(ref["flux"]).max()
    T[777] = -3.0                                         # A + B T < 0: a negative conductivity, not refused
    got = a.temperature(T).device(to_device(g))
    assert got[3]["n_nan"] == 0 and got[1][777, 0] == 2.0 and got[1][777, 3] == 2.0
    a.close()
    b.close()


def test_algorithmic_bytes_kernel_names_and_the_custom_build():
    sizes = []
    for law in hp.LAWS_2D:
        h = Handle(law, 64)
        sizes.append(h.lib.dxm_algorithmic_bytes(h.h))
        assert h.lib.dxm_kernel_name(h.h) == f"heat_plane_kernel<{law - 35}, 0".encode()
        h.temperature(np.full(64, 300.0))
        sizes.append(h.lib.dxm_algorithmic_bytes(h.h))
        assert h.lib.dxm_external_state_kind(h.h, 0) == 1
        h.close()
    assert sizes == [64, 72, 80, 88]


@pytest.mark.parametrize("law", hp.LAWS_2D)
def test_refusals_mirror_the_three_wide_laws_each_with_its_own_sentence(law):
    n = 300
    g, T = hp.inputs(law, n, seed=6)
    h = Handle(law, n).temperature(T)
    lib = h.lib
    before, gen = h.device(to_device(g)), lib.dxm_launch_generation(h.h)
    what = "two-dimensional stationary heat" if law == hp.STATIONARY_2D else "two-dimensional phase-change"
    for layout in (1, 2, 3):
        assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and what in err(lib) and "only DXM_TANGENT_FULL" in err(lib)
    assert lib.dxm_tangent_size(h.h) == hp.WIDTH[law]
    eye, eyes = np.eye(3), np.tile(np.eye(3).reshape(9), (n, 1))
    for rc in (lib.dxm_set_frame(h.h, eye.ctypes.data), lib.dxm_set_frame_field(h.h, eyes.ctypes.data)):
        assert rc < 0 and "two-dimensional" in err(lib) and "a scalar conductivity" in err(lib)
    field = np.full(n, 1.0)
    assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "per-point parameter fields are not served for two-dimensional" in err(lib)
    bad = T.copy()
    bad[123] = np.inf
    assert lib.dxm_set_external_state(h.h, 0, bad.ctypes.data) < 0 and "Temperature is not finite at point 123 (inf)" in err(lib)
    assert lib.dxm_set_external_state_uniform(h.h, 0, float("nan")) < 0 and "Temperature must be finite, got nan" in err(lib)
    assert lib.dxm_set_external_state(h.h, 1, T.ctypes.data) < 0 and "has no external state variable" in err(lib)
    p = list(hp.PARAMS[law])
    idx, value, text = (1, np.inf, "B must be finite, got inf") if law == hp.STATIONARY_2D else (6, 0.0, "Tsmooth must be > 0, got 0")
    q = list(p)
    q[idx] = value
    assert lib.dxm_set_params(h.h, (C.c_double * len(q))(*q), len(q)) < 0 and text in err(lib), err(lib)
    assert not lib.dxm_create(law, (C.c_double * len(q))(*q), len(q), 8, 0) and text in err(lib)
    assert not lib.dxm_create(law, (C.c_double * 3)(1.0, 2.0, 3.0), 3, 8, 0) and f"expects {len(p)} parameters" in err(lib)
    assert not lib.dxm_create(34, (C.c_double * 2)(1.0, 2.0), 2, 8, 0) and "unknown law id" in err(lib)
    after = h.device(to_device(g))
    assert lib.dxm_launch_generation(h.h) == gen and all(bits(x, y) for x, y in zip(after[:3], before[:3]))
    h.close()


def test_a_custom_hardening_build_refuses_both_laws_and_the_scalar_calls():
    import dolfinx_materials_amd.materials as mats

    hd = mats.CustomHardening("sig0 + K * (pow(p + p0, n) - pow(p0, n))", "K * n * pow(p + p0, n - 1.0)", sig0=250.0, K=600.0, n=0.3, p0=1e-3)
    lib = _lib.load_custom(hd.expr_R, hd.expr_dR)
    assert lib.dxm_has_custom_hardening() == 1
    for law, text in ((hp.STATIONARY_2D, "two-dimensional stationary heat transfer has no hardening law"),
                      (hp.PHASE_CHANGE_2D, "two-dimensional heat transfer with phase change has no hardening law")):
        p = list(hp.PARAMS[law])
        assert not lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), 64, 0)
        msg = err(lib)
        assert text in msg and "served by the stock libdxmat, not by a custom-hardening build" in msg, msg
        b = _lib.law_blocks(law, lib)
        assert (b.n_external, b.tangent_width) == (1, hp.WIDTH[law])
    case = hp.quad_case("q1-x1")
    arrs = [np.ascontiguousarray(case[k]) for k in ("coords", "cells", "dofmap", "geom_dphi", "phi", "dphi")]
    mesh = lib.dxm_mesh_create_plane_scalar(arrs[0].ctypes.data, len(arrs[0]), arrs[1].ctypes.data, 4, len(arrs[1]), arrs[2].ctypes.data, 4,
                                            case["n_dofs"], arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data, 1, 0)
    assert mesh, err(lib)
    t, out = to_device(np.full(case["n_dofs"], 300.0)), to_device(np.full((case["npoints"], 2), np.nan))
    assert lib.dxm_mesh_scalar_gradient_device(mesh, t.data_ptr(), out.data_ptr(), None, None) < 0
    assert "served by the stock libdxmat, not by a custom-hardening build" in err(lib)
    assert np.isnan(to_host(out)).all()
    lib.dxm_mesh_destroy(mesh)
