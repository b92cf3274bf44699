"""GPU: the stand-alone gradient kernels of ``csrc/gradient.hpp`` against ``gradient_ref`` (an independent numpy restatement, held
to its own longdouble evaluation within 1e-14 by ``test_gradient_ref_cpu.py``), and the fused ``GRAD = 1 / 2 / 3`` forms of the
update kernels against "gradient kernel, then update kernel" in the instantiations and launch ranges the rest of the suite never
reaches.

Stand-alone kernels (bound 1e-13 absolute, both output kinds, a random field and the affine patch field, outputs filled with NaN
beforehand):

=================================  ==========================================================================================
``hex8_gradient_kernel``           nqp 1 (centroid), 3 (arbitrary points) on 7^3 cells: 343 and 1029 points
``hex8_gradient_staged_kernel``    nqp 4, 5, 7 (arbitrary points), 27 (Gauss) on 6^3 cells: a 256-point block starts inside a cell for
                                   5, 7 and 27; 64 cells per block for 4
``tet4_gradient_kernel``           nqp 1, 4, 5 on 162 tetrahedra
``simplex_gradient_kernel``        P1 / P2 on triangles / tetrahedra with tables of 1, 5, 7 arbitrary points and the degree-2 rule
=================================  ==========================================================================================

Instantiation sweep (``dxm_integrate_displacement_device``; the handle's layout is the kernel's TL; G: 1 on ``hex8x8``, 2 on
``tet4x4``, 3 on ``tet10x4`` and ``tri6x3``).  Each law x layout below runs on each of the four meshes, except the four the sweep of
``test_gpu_gradient.py`` has (elastic full, J2 Voce full, J2 linear sym, FeFp Voce):

==========================================  ============================================================================
elastic x {full, sym}                       ``small_strain_kernel<LAW_ELASTIC, TL_FULL | TL_SYM, G>``
J2 linear x {full, sym, coef, pack4}        ``small_strain_kernel<LAW_J2_LINEAR, TL, G>``
J2 Voce x {full, sym, coef, pack4}          ``small_strain_kernel<LAW_J2_VOCE, TL, G>``
Ramberg-Osgood x {full, sym, coef, pack4}   ``small_strain_kernel<LAW_RAMBERG_OSGOOD, TL, G>`` (``ramberg_osgood_launch``)
J2 linear, every field bound x {full, pack4}  ``small_strain_field_kernel<LAW_J2_LINEAR, TL_FULL | TL_PACK4, G>`` (``param_fields_launch``)
FeFp x {Voce, linear}                       ``fefp_kernel<HARD = 1 | 0, G, T = 0>`` (``launch_fefp``)
==========================================  ============================================================================

Chunks that start inside a cell (``dxm_integrate_displacement``, host buffers; ``MeshSource.point0`` = the chunk's offset):

==========================================  ============================================================================
J2 linear, pack4 handle                     ``small_strain_kernel<LAW_J2_LINEAR, TL_PACK4, G>`` (the handle's own layout)
J2 linear, sym handle                       the same kernel (packed transfer: the 21 entries are rebuilt on the host), or
                                            ``TL_SYM`` where the stress does not land in page-locked memory
FeFp linear, full handle                    ``fefp_kernel<HARD = 0, G = 2, T = 1>`` (packed transfer: the coefficient record)
==========================================  ============================================================================
on tri6 x 3 (G = 3, 66 150 points, second chunk at 33 280 = 1 mod 3) and tet4 x 5 (G = 2, 65 910 points, second chunk at
33 024 = 4 mod 5).

Observed on an MI355X (largest error per kernel family; each test prints its own; the small-strain laws of the sweep stay
below 5e-16 and their chunked cases agree bit for bit):

=================================  ================  =========
family                             largest error     bound
=================================  ================  =========
``hex8_gradient_kernel``           2.2e-16           1e-13
``hex8_gradient_staged_kernel``    2.2e-16           1e-13
``tet4_gradient_kernel``           2.2e-16           1e-13
``simplex_gradient_kernel``        4.4e-16           1e-13
instantiation sweep (relative)     2.0e-14 (FeFp)    1e-12
chunked host form (relative)       1.5e-14 (FeFp)    1e-12
=================================  ================  ========="""
import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
import gradient_ref as gr
import tile_loop_cases as tc
from dolfinx_materials_amd.gradient import Hex8Mesh, SimplexMesh, Tet4Mesh
from dolfinx_materials_amd.jaxmat import JAXMaterial
from helpers import (B_F, B_V, E, H_LIN, NU, SIG0_F, SIG0_LIN, SIG0_V, SIGU_F, SIGU_V, deformation_gradient9, mandel_strain, to_device, to_host)

pytestmark = pytest.mark.gpu
BOUND = 1e-13      # absolute, |H| <~ 0.1: the bound of test_gpu_gradient.py
FUSED = 1e-12      # relative: fused against gradient kernel -> update kernel (same arithmetic up to contraction)


def _device_mesh(kind, case):
    if kind == "hex8":
        return Hex8Mesh(case["coords"], case["conn"], qpoints=case["points"])
    if kind == "tet4":
        return Tet4Mesh(case["coords"], case["conn"], nqp=case["nqp"])
    return SimplexMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["dphi"])


def _against_reference(family, tag):
    """Both output kinds of the mesh's gradient kernel, for the random and the patch field; returns the largest error."""
    import torch

    kind, case = gr.get_case(tag)
    mesh = _device_mesh(kind, case)
    assert mesh.displacement_size == case["xd"].size
    st = torch.cuda.current_stream().cuda_stream
    worst = 0.0
    for name in ("random", "patch"):
        u = case["u_" + name]
        H = gr.reference(kind, case, u)
        assert mesh.npoints == len(H) and np.abs(H).max() < 0.15
        ud = to_device(np.array(u))
        for out_kind, ref in ((0, mandel_strain(H)), (1, deformation_gradient9(H))):
            out = torch.full((mesh.npoints, ref.shape[1]), float("nan"), dtype=torch.float64, device="cuda:0")
            mesh.gradient_device(ud.data_ptr(), out_kind, out.data_ptr(), st)
            torch.cuda.synchronize()
            got = to_host(out)
            assert np.isfinite(got).all(), f"{family} {tag} {name} kind {out_kind}: rows left unwritten"
            err = float(np.abs(got - ref).max())
            worst = max(worst, err)
            print(f"gradient kernels {family} {tag} {name} kind {out_kind}: {mesh.npoints} points, error {err:.3e} (bound {BOUND:.0e})")
            assert err < BOUND
            if case["xd"].shape[1] == 2:      # plane strain: eps_zz = 0, F_zz = 1, no out-of-plane shear
                zero = got[:, [2, 4, 5]] if out_kind == 0 else got[:, 5:]
                assert np.all(zero == 0.0) and (out_kind == 0 or np.all(got[:, 2] == 1.0))
    mesh.close()
    return worst


@pytest.mark.parametrize("nqp", gr.HEX_DIRECT_NQP)
def test_hex8_direct_kernel(nqp):
    """``hex8_gradient_kernel`` (nqp < 4): every thread gathers its cell's 8 nodes itself.  7^3 cells: 2 and 5 blocks, the last ragged."""
    case = gr.hex_case(nqp)
    n = len(case["conn"]) * nqp
    assert nqp < 4 and n == 343 * nqp and n > 256 and n % 256 != 0
    _against_reference("hex8_gradient_kernel", f"hex8-direct-x{nqp}")


@pytest.mark.parametrize("nqp", gr.HEX_STAGED_NQP)
def test_hex8_staged_kernel(nqp):
    """``hex8_gradient_staged_kernel`` (nqp >= 4): the block stages its cells' nodes in LDS from cell ``c0 = p0 / nqp`` on and a point
    reads record ``cell - c0``.  With 5, 7 or 27 points per cell a 256-point block starts inside a cell; with 4 it holds 64 cells, the
    most there can be."""
    case = gr.hex_case(nqp)
    n = len(case["conn"]) * nqp
    assert nqp >= 4 and n == 216 * nqp
    if nqp in (5, 7, 27):
        assert 256 % nqp != 0
        assert any((b * 256) % nqp != 0 for b in range(1, -(-n // 256)))       # a block does start inside a cell
    else:
        assert 256 // nqp == 64
    assert n % 256 != 0                                                        # ... and the last block is ragged, for every nqp here
    _against_reference("hex8_gradient_staged_kernel", f"hex8-staged-x{nqp}")


@pytest.mark.parametrize("nqp", gr.TET4_NQP)
def test_tet4_kernel(nqp):
    """``tet4_gradient_kernel<0>`` and ``<1>``: the cell's constant gradient at each of its nqp points."""
    _against_reference("tet4_gradient_kernel", f"tet4-x{nqp}")


@pytest.mark.parametrize("rule", gr.SIMPLEX_RULES)
@pytest.mark.parametrize("element", gr.SIMPLEX_ELEMENTS)
def test_simplex_kernel(element, rule):
    """``simplex_gradient_kernel`` with tables handed to ``SimplexMesh`` directly: 1, 5 and 7 arbitrary interior points and the
    degree-2 rule; triangles embedded as plane strain."""
    _against_reference("simplex_gradient_kernel", f"{element}-{rule}")


# ---- fused forms: instantiation sweep ------------------------------------------------------------------------------------------
def _elastic():
    return jm.LinearElasticIsotropic(E=E, nu=NU)


def _ramberg_osgood():
    from test_gpu_ramberg_osgood import behavior

    return behavior()


#: law -> (behaviour, gradient kind, displacement scale, plastic, tangent layouts)
LAWS = {
    "elastic": (lambda: jm.ElasticBehavior(_elastic()), 0, 5e-3, False, ("full", "sym")),
    "j2_linear": (lambda: jm.vonMisesIsotropicHardening(_elastic(), jm.LinearHardening(SIG0_LIN, H_LIN)), 0, 8e-3, True, ("full", "sym", "coef", "pack4")),
    "j2_voce": (lambda: jm.vonMisesIsotropicHardening(_elastic(), jm.VoceHardening(SIG0_V, SIGU_V, B_V)), 0, 8e-3, True, ("full", "sym", "coef", "pack4")),
    "ramberg_osgood": (_ramberg_osgood, 0, 8e-3, True, ("full", "sym", "coef", "pack4")),
    "j2_linear_fields": (lambda: jm.vonMisesIsotropicHardening(_elastic(), jm.LinearHardening(SIG0_LIN, H_LIN)), 0, 8e-3, True, ("full", "pack4")),
    "fefp_voce": (lambda: jm.FeFpJ2Plasticity(_elastic(), jm.VoceHardening(SIG0_F, SIGU_F, B_F)), 1, 2e-2, True, ("full",)),
    "fefp_linear": (lambda: jm.FeFpJ2Plasticity(_elastic(), jm.LinearHardening(400.0, 2e3)), 1, 2e-2, True, ("full",)),
}
SWEEP_MESHES = ("hex8x8", "tet4x4", "tet10x4", "tri6x3")
ALREADY_SWEPT = {("elastic", "full"), ("j2_voce", "full"), ("j2_linear", "sym"), ("fefp_voce", "full")}   # test_gpu_gradient.py, on these mesh kinds
SWEEP = [(law, layout, mesh) for law, spec in LAWS.items() for layout in spec[4] if (law, layout) not in ALREADY_SWEPT for mesh in SWEEP_MESHES]


def _sweep_mesh(name):
    """(device mesh, dof positions)"""
    if name == "hex8x8":
        coords, conn = gr.hex_grid(3, 0.15, seed=0)          # 27 cells x 8 Gauss points = 216 points: a ragged tile
        return Hex8Mesh(coords, conn), coords
    if name == "tet4x4":
        coords, conn = gr.tet_mesh()
        return Tet4Mesh(coords, conn, nqp=4), coords
    case = gr.simplex_case("p2tet" if name == "tet10x4" else "p2tri", "deg2")
    return _device_mesh("simplex", case), case["xd"]


def _material(law, layout, n):
    make = LAWS[law][0]
    if law != "j2_linear_fields":
        mat = JAXMaterial(make(), tangent_layout=layout)
        mat.set_data_manager(n)
        return mat
    from param_fields_ref import NAMES, graded_fields

    mat = JAXMaterial(make(), tangent_layout=layout, property_fields=True, lazy_isv=False)
    mat.set_data_manager(n)
    for name, a in graded_fields("linear", n, NAMES["linear"]).items():
        mat.update_material_property(("elasticity." if name in ("E", "nu") else "yield_stress.") + name, a)
    assert mat._lib.dxm_param_field_mask(mat._require()) == (1 << len(NAMES["linear"])) - 1 and mat.kernel_name.startswith("small_strain_field_kernel<")
    return mat


@pytest.mark.parametrize("law,layout,mesh_name", SWEEP, ids=["-".join(s) for s in SWEEP])
def test_fused_instantiation_equals_gradient_then_update(law, layout, mesh_name):
    """``dxm_integrate_displacement_device`` (gradient inside the update kernel) against ``dxm_mesh_gradient_device`` ->
    ``dxm_integrate_device`` on a second handle of the same layout, over two increments with an advance between."""
    import torch

    mesh, xd = _sweep_mesh(mesh_name)
    n = mesh.npoints
    assert n == {"hex8x8": 216, "tet4x4": 648, "tet10x4": 648, "tri6x3": 294}[mesh_name]
    _, kind, scale, plastic, _ = LAWS[law]
    a, b = _material(law, layout, n), _material(law, layout, n)
    ng, nf, nt = a._info.n_grad, a._info.n_flux, a.tangent_size
    assert nt == {"full": nf * ng, "sym": 21, "coef": 9, "pack4": 4}[layout]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    new = lambda cols: torch.full((n, cols), float("nan"), dtype=torch.float64, device=dev)   # noqa: E731
    grad, fa, fb, ca, cb = new(ng), new(nf), new(nf), new(nt), new(nt)
    rng = np.random.default_rng(3)
    worst = 0.0
    for t in (0.6, 1.0):
        u = t * (xd * np.array([scale, -0.4 * scale, -0.4 * scale][:xd.shape[1]]) + rng.standard_normal(xd.shape) * 0.05 * scale)
        ud = to_device(u.ravel().copy())
        mesh.gradient_device(ud.data_ptr(), kind, grad.data_ptr(), st)
        a.integrate_device(grad.data_ptr(), fa.data_ptr(), ca.data_ptr(), st)
        b.integrate_displacement_device(mesh, ud.data_ptr(), fb.data_ptr(), cb.data_ptr(), st)
        torch.cuda.synchronize()
        sa, sb = a.stats()[1], b.stats()[1]
        assert sa == sb and sa["n_nan"] == 0, (sa, sb)
        if plastic:
            assert sa["n_plastic"] > 0
        assert bool(torch.isfinite(fb).all()) and bool(torch.isfinite(cb).all())
        ef = float((fa - fb).abs().max()) / float(fa.abs().max())
        ec = float((ca - cb).abs().max()) / float(ca.abs().max())
        es = 0.0
        fin_a, fin_b = a.get_final_state_dict(), b.get_final_state_dict()
        for k, v in fin_a.items():
            if k in a.gradients or k in a.fluxes:   # device-pointer forms: the host never saw them ("unknown" placeholders)
                assert np.isnan(v).all() and np.isnan(fin_b[k]).all(), k
                continue
            es = max(es, float(np.abs(v - fin_b[k]).max() / max(np.abs(v).max(), 1e-300)))
        print(f"fused sweep {law} {layout} {mesh_name} t={t}: n_plastic {sa['n_plastic']} of {n}, flux {ef:.3e} tangent {ec:.3e} state {es:.3e} (bound {FUSED:.0e})")
        worst = max(worst, ef, ec, es)
        assert ef <= FUSED and ec <= FUSED and es <= FUSED
        a.data_manager.update()
        b.data_manager.update()
    a.close()
    b.close()
    mesh.close()


# ---- fused forms: chunks of the host-buffer form that start inside a cell -----------------------------------------------------------
CHUNKED = [("tri6x3", "j2_linear", "pack4"), ("tri6x3", "j2_linear", "sym"), ("tet4x5", "j2_linear", "pack4"), ("tet4x5", "j2_linear", "sym"),
           ("tet4x5", "fefp_linear", "full")]


@pytest.mark.parametrize("mesh_name,law,layout", CHUNKED, ids=["-".join(s) for s in CHUNKED])
def test_chunks_of_the_host_form_that_start_inside_a_cell(mesh_name, law, layout):
    """The chunked host path hands every launch its first point (``MeshSource.point0``, a multiple of 256); the fused kernels take
    cell ``(point0 + i) / nqp`` and point ``point0 + i - cell nqp``.  With 3 or 5 points per cell the second chunk starts inside a
    cell.  Against the device-pointer sequence gradient kernel -> update kernel, which is one launch from point 0."""
    import torch

    case = gr.chunk_case(mesh_name)
    n, nqp = case["npoints"], case["nqp"]
    chunks = tc.host_chunks(n, 64, fused=True)
    assert len(chunks) >= 2 and any(off % nqp != 0 for off, _ in chunks), chunks
    if case["kind"] == "tet4":
        mesh = Tet4Mesh(case["coords"], case["cells"], nqp=nqp)
    else:
        mesh = _device_mesh("simplex", case)
    assert mesh.npoints == n
    a, b = _material(law, layout, n), _material(law, layout, n)
    fa, _, ca = a.integrate_displacement(mesh, np.array(case["u"]))              # host buffers: chunked, fused
    fa, ca = np.asarray(fa), np.asarray(ca).reshape(n, -1)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    ng, nf, nt = b._info.n_grad, b._info.n_flux, b.tangent_size
    assert ca.shape[1] == nt
    ud = to_device(np.array(case["u"]))
    grad = torch.empty((n, ng), dtype=torch.float64, device=dev)
    fb = torch.empty((n, nf), dtype=torch.float64, device=dev)
    cb = torch.empty((n, nt), dtype=torch.float64, device=dev)
    mesh.gradient_device(ud.data_ptr(), LAWS[law][1], grad.data_ptr(), st)
    b.integrate_device(grad.data_ptr(), fb.data_ptr(), cb.data_ptr(), st)
    torch.cuda.synchronize()
    sb = b.stats()[1]
    assert a.last_stats["n_nan"] == 0 and sb["n_nan"] == 0
    assert 0 < a.last_stats["n_plastic"] < n and a.last_stats["n_plastic"] == sb["n_plastic"]
    fbh, cbh = to_host(fb), to_host(cb)
    ef = float(np.abs(fa - fbh).max() / np.abs(fbh).max())
    ec = float(np.abs(ca - cbh).max() / np.abs(cbh).max())
    # per chunk as well: an error confined to the (smaller) last chunk must not hide behind the largest entry of the first
    for off, cnt in chunks:
        sl = slice(off, off + cnt)
        ef = max(ef, float(np.abs(fa[sl] - fbh[sl]).max() / np.abs(fbh[sl]).max()))
        ec = max(ec, float(np.abs(ca[sl] - cbh[sl]).max() / np.abs(cbh[sl]).max()))
    print(f"chunked host form {mesh_name} {law} {layout}: {n} points, chunks {chunks}, n_plastic {sb['n_plastic']}, flux {ef:.3e} tangent {ec:.3e} (bound {FUSED:.0e})")
    assert ef <= FUSED and ec <= FUSED
    a.close()
    b.close()
    mesh.close()
