"""GPU: orthotropic elasticity with material frames (DXM_LAW_ORTHOTROPIC_ELASTIC, ``orthotropic_kernel``) through the C ABI (ctypes)
against the numpy restatement ``orthotropic_ref.update`` and the committed 50-digit values; the three frame states of a handle against
each other; the routes of the library against each other bit for bit; the frame setters and every refusal.

Bound: max(1e-12, 8 x the largest deviation of the restatement from its 50-digit version) relative to the field scale, read from
``tests/golden/orthotropic_frames.npz`` (measured 5.7e-16: the bound is 1e-12)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from dolfinx_materials_amd import _lib

import orthotropic_ref as orf
from helpers import to_device, to_host

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orthotropic_frames.npz"))
BOUND = max(1e-12, 8 * max(json.loads(str(GOLD["meta"]))["restatement_deviation"].values()))
SETS = orf.PARAMETER_SETS
NBIG = 100_003
LAW = _lib.LAW_ORTHOTROPIC_ELASTIC


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


class Handle:
    """one dxm_material of the law, driven through ctypes alone"""

    def __init__(self, p, n, layout=0, law=LAW):
        self.lib, self.n = _lib.load(), n
        self.h = self.lib.dxm_create(law, (C.c_double * len(p))(*p), len(p), n, 0)
        assert self.h, err(self.lib)
        assert self.lib.dxm_set_tangent_layout(self.h, layout) == 0, err(self.lib)
        self.width = self.lib.dxm_tangent_size(self.h)

    def frame(self, R):
        """None, (3, 3) or (n, 3, 3)"""
        if R is None:
            rc = self.lib.dxm_set_frame(self.h, None)
        else:
            a = np.array(R, dtype=np.float64, order="C")   # a copy that lives until the call has returned
            rc = self.lib.dxm_set_frame(self.h, a.ctypes.data) if a.shape == (3, 3) else self.lib.dxm_set_frame_field(self.h, a.reshape(self.n, 9).ctypes.data)
        assert rc == 0, err(self.lib)
        return self

    def stats(self):
        st = _lib.Stats()
        assert self.lib.dxm_get_stats(self.h, C.byref(st)) == 0, err(self.lib)
        return st.as_dict()

    def device(self, eps_dev):
        import torch

        f = torch.zeros((self.n, 6), dtype=torch.float64, device=eps_dev.device)
        c = torch.zeros((self.n, self.width), dtype=torch.float64, device=eps_dev.device)
        assert self.lib.dxm_integrate_device(self.h, eps_dev.data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), None) == 0, err(self.lib)
        torch.cuda.synchronize()
        return to_host(f), to_host(c), self.stats()

    def host(self, eps):
        f, c, st = np.full((self.n, 6), np.nan), np.full((self.n, self.width), np.nan), _lib.Stats()
        assert self.lib.dxm_integrate(self.h, eps.ctypes.data, 0.0, f.ctypes.data, None, c.ctypes.data, C.byref(st)) == 0, err(self.lib)
        return f, c, st.as_dict()

    def option(self, name, value):
        assert self.lib.dxm_set_option(self.h, name.encode(), float(value)) == 0, err(self.lib)

    def close(self):
        self.lib.dxm_destroy(self.h)


def tri(ct):
    """(n, 36) -> the 21 upper-triangle entries, row by row"""
    iu = np.triu_indices(6)
    return ct.reshape(-1, 6, 6)[:, iu[0], iu[1]]


def check(tag, sig, ct, ref_sig, ref_ct):
    n = len(ref_sig)
    es = np.abs(sig - ref_sig).max() / np.abs(ref_sig).max()
    ec = np.abs(ct.reshape(n, -1) - ref_ct.reshape(n, -1)).max() / np.abs(ref_ct).max()
    print(f"orthotropic parity {tag}: stress {es:.3e} tangent {ec:.3e} (bound {BOUND:.2e})")
    assert es <= BOUND and ec <= BOUND, (tag, es, ec)


@pytest.fixture(scope="module")
def big():
    """shared inputs at N = 100 003: strains, per-point frames of every class, and the restatement per parameter set"""
    eps = orf.strains(NBIG, seed=31)
    labels, R = orf.frames(NBIG, seed=32)
    ref = {name: orf.update(eps, p, R) for name, p in SETS.items()}
    return {"eps": eps, "R": R, "labels": labels, "ref": ref, "eps_dev": to_device(eps)}


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("N", [1, 63, 64, 65, NBIG])
def test_kernel_matches_the_restatement_with_field_and_uniform_frames_full_and_sym(big, N, name):
    p = SETS[name]
    if N == NBIG:
        eps, R, (rs, rc), eps_dev = big["eps"], big["R"], big["ref"][name], big["eps_dev"]
    else:
        eps = orf.strains(N, seed=N)
        R = orf.frames(max(N, 10), seed=N + 1)[1][-N:]      # N = 1: the near-identity frame
        rs, rc = orf.update(eps, p, R)
        eps_dev = to_device(eps)
    full, sym = Handle(p, N, 0), Handle(p, N, 1)
    # one frame per point
    S, T, st = full.frame(R).device(eps_dev)
    check(f"N={N} {name} field full", S, T, rs, rc)
    S1, T1, st1 = sym.frame(R).device(eps_dev)
    assert T1.shape == (N, 21) and np.array_equal(S1, S) and np.array_equal(T1, tri(T)) and st1 == st
    assert st["n_nan"] == 0 and st["n_plastic"] == 0 and st["n_not_converged"] == 0 and st["max_local_iters"] == 0 and st["n_points"] == N
    assert np.array_equal(T.reshape(N, 6, 6), T.reshape(N, 6, 6).transpose(0, 2, 1))      # (i, j) and (j, i): the same bits
    assert full.lib.dxm_frame_kind(full.h) == 2 and full.lib.dxm_kernel_name(full.h) == b"orthotropic_kernel<2"
    # one frame per handle, every class
    for cls, Ru in zip(orf.FRAME_CLASSES, orf.frames(10, seed=7)[1]):
        C6 = orf.update(np.zeros((1, 6)), p, Ru)[1][0]
        S, T, st = full.frame(Ru).device(eps_dev)
        check(f"N={N} {name} uniform {cls} full", S, T, eps @ C6.T, np.broadcast_to(C6, (N, 6, 6)))
        S1, T1, _ = sym.frame(Ru).device(eps_dev)
        assert np.array_equal(S1, S) and np.array_equal(T1, tri(T))
        assert np.array_equal(T.reshape(N, 6, 6), T.reshape(N, 6, 6).transpose(0, 2, 1)) and st["n_nan"] == 0
    assert full.lib.dxm_frame_kind(full.h) == 1 and full.lib.dxm_kernel_name(full.h) == b"orthotropic_kernel<1"
    full.close()
    sym.close()


@pytest.mark.parametrize("name", list(SETS))
def test_fixture_points_match_their_50_digit_values(name):
    eps, R = GOLD[f"{name}/eps"], GOLD[f"{name}/R"]
    n = len(eps)
    h = Handle(SETS[name], n).frame(R)
    S, T, st = h.device(to_device(eps))
    check(f"golden {name}", S, T, GOLD[f"{name}/sig"], GOLD[f"{name}/ct"])
    assert st["n_nan"] == 0
    h.close()


@pytest.mark.parametrize("layout", [0, 1])
def test_a_constant_field_equals_the_uniform_handle_bit_for_bit(big, layout):
    p = SETS["strong"]
    for Ru in (orf.frames(10, seed=7)[1][8], orf.axis_rotation(2, np.pi / 3)):
        u, f = Handle(p, NBIG, layout).frame(Ru), Handle(p, NBIG, layout).frame(np.broadcast_to(Ru, (NBIG, 3, 3)))
        Su, Tu, stu = u.device(big["eps_dev"])
        Sf, Tf, stf = f.device(big["eps_dev"])
        assert np.array_equal(Su.view(np.uint64), Sf.view(np.uint64)) and np.array_equal(Tu.view(np.uint64), Tf.view(np.uint64)) and stu == stf
        u.close()
        f.close()


@pytest.mark.parametrize("name", list(SETS))
def test_identity_frames_give_what_the_no_frame_handle_gives_and_its_tangent_is_the_hosts_stiffness(big, name):
    p = SETS[name]
    h = Handle(p, NBIG)
    lib = h.lib
    assert lib.dxm_frame_kind(h.h) == 0 and lib.dxm_kernel_name(h.h) == b"orthotropic_kernel<0" and lib.dxm_algorithmic_bytes(h.h) == 384
    S0, T0, st0 = h.device(big["eps_dev"])
    Ch = orf.host_stiffness(p)
    assert np.array_equal(T0.view(np.uint64), np.broadcast_to(Ch.reshape(36), (NBIG, 36)).copy().view(np.uint64))   # bit for bit
    check(f"{name} no frame", S0, T0, big["eps"] @ orf.stiffness(p).T, np.broadcast_to(orf.stiffness(p), (NBIG, 6, 6)))
    for R in (np.eye(3), np.broadcast_to(np.eye(3), (NBIG, 3, 3))):
        S, T, st = h.frame(R).device(big["eps_dev"])
        check(f"{name} identity {'field' if np.ndim(R) == 3 else 'uniform'}", S, T, S0, T0.reshape(NBIG, 6, 6))
        assert st == st0
    assert lib.dxm_algorithmic_bytes(h.h) == 456
    h.frame(np.eye(3))
    assert lib.dxm_algorithmic_bytes(h.h) == 384
    h.frame(None)
    assert lib.dxm_frame_kind(h.h) == 0 and lib.dxm_algorithmic_bytes(h.h) == 384
    S, T, _ = h.device(big["eps_dev"])
    assert np.array_equal(S, S0) and np.array_equal(T, T0)
    h.close()


def test_host_buffer_form_equals_the_device_form_in_one_and_in_three_chunks(big):
    """Distinct frames per point: a frame stream that is not offset with the chunk gives other numbers in chunks 2 and 3.  Chunks at
    N = 100 003 (host_side.hpp::plan_chunks): the packed transfer of a full-layout handle and every transfer of a "sym" handle are cut
    into 3, option max_chunks 1 makes them one; a full-layout handle with packed_transfer 0 moves its 36 entries in one chunk."""
    p, eps, R = SETS["strong"], big["eps"], big["R"]
    base = {}
    for layout in (0, 1):
        h = Handle(p, NBIG, layout).frame(R)
        base[layout] = h.device(big["eps_dev"])
        for packed in (1, 0):
            for chunks in (64, 1):
                h.option("packed_transfer", packed)
                h.option("max_chunks", chunks)
                S, T, st = h.host(eps)
                assert np.array_equal(S, base[layout][0]) and np.array_equal(T, base[layout][1]), (layout, packed, chunks)
                assert {k: v for k, v in st.items()} == base[layout][2], (layout, packed, chunks)
        h.close()
    assert np.array_equal(base[1][1], tri(base[0][1]))


def test_rows_form_indexes_the_frames_by_the_maps_own_point(big):
    p, eps, R = SETS["cubic"], big["eps"], big["R"]
    rows = np.ascontiguousarray(2 * np.arange(NBIG), dtype=np.int64)
    for layout, width in ((0, 36), (1, 21)):
        h = Handle(p, NBIG, layout).frame(R)
        S, T, _ = h.device(big["eps_dev"])
        flux, ct, st = np.full((2 * NBIG, 6), -7.0), np.full((2 * NBIG, width), -9.0), _lib.Stats()
        assert h.lib.dxm_integrate_rows(h.h, eps.ctypes.data, 0.0, flux.ctypes.data, ct.ctypes.data, rows.ctypes.data, C.byref(st)) == 0, err(h.lib)
        assert np.array_equal(flux[rows], S) and np.array_equal(ct[rows], T)
        assert np.all(flux[1::2] == -7.0) and np.all(ct[1::2] == -9.0) and st.n_nan == 0
        h.close()


def test_frame_field_from_device_memory_and_the_launch_generation(big):
    torch = pytest.importorskip("torch")
    p, R = SETS["strong"], big["R"]
    ref = Handle(p, NBIG).frame(R)
    S, T, _ = ref.device(big["eps_dev"])
    ref.close()
    h = Handle(p, NBIG)
    lib = h.lib
    gens = [lib.dxm_launch_generation(h.h)]
    rdev = to_device(R.reshape(NBIG, 9))
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.dxm_set_frame_field_device(h.h, rdev.data_ptr(), stream) == 0, err(lib)
    gens.append(lib.dxm_launch_generation(h.h))
    assert lib.dxm_frame_kind(h.h) == 2 and lib.dxm_algorithmic_bytes(h.h) == 456
    f = torch.zeros((NBIG, 6), dtype=torch.float64, device=rdev.device)
    c = torch.zeros((NBIG, 36), dtype=torch.float64, device=rdev.device)
    assert lib.dxm_integrate_device(h.h, big["eps_dev"].data_ptr(), 0.0, f.data_ptr(), c.data_ptr(), stream) == 0, err(lib)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(f), S) and np.array_equal(to_host(c), T)
    eye, R9 = np.eye(3), np.ascontiguousarray(R.reshape(NBIG, 9))
    for call in (lambda: lib.dxm_set_frame(h.h, eye.ctypes.data), lambda: lib.dxm_set_frame_field(h.h, R9.ctypes.data),
                 lambda: lib.dxm_set_frame_field_device(h.h, None, None), lambda: lib.dxm_set_frame(h.h, eye.ctypes.data),
                 lambda: lib.dxm_set_frame(h.h, None)):
        assert call() == 0, err(lib)
        gens.append(lib.dxm_launch_generation(h.h))
    assert len(set(gens)) == len(gens) and gens == sorted(gens), gens
    assert lib.dxm_frame_kind(h.h) == 0
    h.close()


def test_refusals_leave_the_handle_as_it_was(big):
    p = SETS["strong"]
    n = 300
    eps = orf.strains(n, seed=3)
    R = orf.frames(n, seed=4)[1]
    h = Handle(p, n).frame(R)
    lib = h.lib
    before = h.device(to_device(eps))
    gen = lib.dxm_launch_generation(h.h)
    for layout in (2, 3):
        assert lib.dxm_set_tangent_layout(h.h, layout) < 0 and "general symmetric 6x6" in err(lib)
    assert lib.dxm_tangent_size(h.h) == 36
    field = np.full(n, p[0])
    assert lib.dxm_set_param_field(h.h, 0, field.ctypes.data) < 0 and "per-point stiffness fields are not served" in err(lib)
    # a non-orthonormal and a NaN frame, named by their point; the handle keeps its field
    bad = R.reshape(n, 9).copy()
    bad[17] *= 1.0 + 1e-6
    assert lib.dxm_set_frame_field(h.h, bad.ctypes.data) < 0 and "point 17" in err(lib) and "not orthonormal" in err(lib)
    bad = R.reshape(n, 9).copy()
    bad[211, 4] = np.nan
    assert lib.dxm_set_frame_field(h.h, bad.ctypes.data) < 0 and "point 211" in err(lib) and "not finite" in err(lib)
    scaled, inf = 1.001 * np.eye(3), np.full((3, 3), np.inf)
    assert lib.dxm_set_frame(h.h, scaled.ctypes.data) < 0 and "not orthonormal" in err(lib)
    assert lib.dxm_set_frame(h.h, inf.ctypes.data) < 0 and "not finite" in err(lib)
    assert lib.dxm_frame_kind(h.h) == 2 and lib.dxm_launch_generation(h.h) == gen
    # parameters: the offending value is in the message
    for idx, value, text in ((0, 0.0, "E1 must be > 0, got 0"), (8, -2.0, "G13 must be > 0, got -2"), (4, np.nan, "nu23 must be finite"),
                             (3, 2.3, "not positive definite"), (4, 2.1, "not positive definite")):
        q = list(p)
        q[idx] = value
        assert lib.dxm_set_params(h.h, (C.c_double * 9)(*q), 9) < 0 and text in err(lib), (idx, err(lib))
        assert not lib.dxm_create(LAW, (C.c_double * 9)(*q), 9, 8, 0) and text in err(lib)
    assert not lib.dxm_create(LAW, (C.c_double * 2)(1.0, 0.3), 2, 8, 0) and "expects 9 parameters" in err(lib)
    after = h.device(to_device(eps))
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    # the fused displacement gradient
    from dolfinx_materials_amd.gradient import gauss_points_hex

    coords = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    conn, qp = np.arange(8, dtype=np.int32)[None, :].copy(), np.ascontiguousarray(gauss_points_hex(2), dtype=np.float64)
    mesh = lib.dxm_mesh_create_hex8(coords.ctypes.data, 8, conn.ctypes.data, 1, qp.ctypes.data, 8, 0)
    assert mesh, err(lib)
    h8 = Handle(p, 8)
    u, fl, ct = to_device(np.zeros(24)), to_device(np.zeros((8, 6))), to_device(np.zeros((8, 36)))
    assert lib.dxm_integrate_displacement_device(h8.h, mesh, u.data_ptr(), 0.0, fl.data_ptr(), ct.data_ptr(), None) < 0
    assert "no fused displacement-gradient form" in err(lib)
    h8.option("fused_gradient", 0)
    assert lib.dxm_integrate_displacement_device(h8.h, mesh, u.data_ptr(), 0.0, fl.data_ptr(), ct.data_ptr(), None) == 0, err(lib)
    h8.stats()
    h8.close()
    lib.dxm_mesh_destroy(mesh)
    h.close()
    # a frame on an isotropic handle
    j2 = Handle([70e3, 0.3, 250.0, 1e3], 64, law=_lib.LAW_J2_LINEAR)
    eye, eyes = np.eye(3), np.tile(np.eye(3).reshape(9), (64, 1))
    rdev = to_device(eyes)
    for rc in (lib.dxm_set_frame(j2.h, eye.ctypes.data), lib.dxm_set_frame(j2.h, None), lib.dxm_set_frame_field(j2.h, eyes.ctypes.data),
               lib.dxm_set_frame_field_device(j2.h, rdev.data_ptr(), None)):
        assert rc < 0
    assert lib.dxm_set_frame(j2.h, eye.ctypes.data) < 0 and "isotropic" in err(lib) and "law 1" in err(lib)
    assert lib.dxm_frame_kind(j2.h) == 0
    j2.close()


def test_a_nan_strain_is_counted():
    n = 130
    eps = orf.strains(n, seed=9)
    eps[[5, 64, 129], [0, 3, 5]] = np.nan
    for R in (None, orf.axis_rotation(0, 0.3), orf.frames(n, seed=1)[1]):
        h = Handle(SETS["cubic"], n).frame(R)
        S, T, st = h.device(to_device(eps))
        assert st["n_nan"] == 3, st
        ok = np.setdiff1d(np.arange(n), [5, 64, 129])
        assert np.isfinite(S[ok]).all() and np.isfinite(T).all() and np.isnan(S[[5, 64, 129]]).any(axis=1).all()
        h.close()
