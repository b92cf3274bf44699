"""CPU: the C boundary of the plane mesh (``dxm_mesh_create_plane``: declared, bound, exported; every host-side check reached on a
machine without a GPU, in the order the header states), the law rows that name the gradient kind of a two-dimensional mesh, the
Python constructors, and the yield mix of the displacement the GPU tests of the displacement forms use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plane_gradient_ref as pg
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd import gradient as gm
from helpers import triangle_grid
from plane_laws_2d import LAWS, increments, reference_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dolfinx_materials_amd", "csrc")


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def _create(lib, case, **over):
    a = dict(coords=case["coords"], n_vertices=len(case["coords"]), conn=np.ascontiguousarray(case["cells"], dtype=np.int32),
             nv=case["cells"].shape[1], n_cells=len(case["cells"]), dofmap=case["dofmap"], nd=case["dofmap"].shape[1], n_dofs=case["n_dofs"],
             gd=case["geom_dphi"], dphi=case["dphi"], nqp=case["dphi"].shape[0], device=0)
    a.update(over)
    keep = [np.ascontiguousarray(a[k]) for k in ("coords", "conn", "dofmap", "gd", "dphi")]
    ptr = [k.ctypes.data for k in keep]
    return lib.dxm_mesh_create_plane(ptr[0], a["n_vertices"], ptr[1], a["nv"], a["n_cells"], ptr[2], a["nd"], a["n_dofs"], ptr[3], ptr[4],
                                     a["nqp"], a["device"])


def test_the_constructor_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dxmat.h")).read()
    assert re.search(r"dxm_mesh\* dxm_mesh_create_plane\(const double\* coords, int64_t n_vertices, const int32_t\* geom_conn, int nv,", hdr)
    assert "#define DXM_ABI_VERSION 6" in hdr
    assert "dxm_mesh_create_plane" in _lib.SYMBOLS and len(_lib.SYMBOLS["dxm_mesh_create_plane"][1]) == 12
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dolfinx_materials_amd", "libdxmat.so")], capture_output=True, text=True).stdout
    assert re.search(r"\sT\s+dxm_mesh_create_plane$", out, flags=re.M)
    assert not re.search(r"plane_gradient_launch", "\n".join(ln for ln in out.splitlines() if " T " in ln))     # hidden: not exported
    assert _lib.load().dxm_abi_version() == 6


def test_host_side_checks_in_their_order():
    """arguments, then indices, then det J, then the device: each with its own sentence, none of them needing a GPU"""
    lib = _lib.load()
    case = pg.quad_case("q1-x4")
    for nv in (2, 5, 8):
        assert not _create(lib, case, nv=nv) and "nv = 3 (triangles) or nv = 4 (bilinear quadrilaterals)" in err(lib), err(lib)
    for over in (dict(nd=3), dict(nd=65), dict(nqp=0), dict(nqp=65), dict(n_cells=0), dict(n_dofs=0), dict(n_vertices=0)):
        assert not _create(lib, case, **over) and "invalid plane mesh arguments" in err(lib), (over, err(lib))
    assert not lib.dxm_mesh_create_plane(None, 4, None, 4, 1, None, 4, 4, None, None, 1, 0) and "invalid plane mesh arguments" in err(lib)
    # indices: the geometry's, then the field's; an argument error comes first, a bad cell after
    bad = case["cells"].copy()
    bad[40, 2] = 100
    assert not _create(lib, case, conn=bad) and "geometry connectivity entry 162 out of range" in err(lib), err(lib)
    bad[40, 2] = -1
    assert not _create(lib, case, conn=bad) and "geometry connectivity entry 162 out of range" in err(lib), err(lib)
    dm = case["dofmap"].copy()
    dm[80, 3] = case["n_dofs"]
    assert not _create(lib, case, dofmap=dm) and "dofmap entry 323 out of range" in err(lib), err(lib)
    bow = case["cells"].copy()
    bow[17, [2, 3]] = bow[17, [3, 2]]                       # a bow-tie quadrilateral
    assert not _create(lib, case, dofmap=dm, conn=bow) and "dofmap entry 323 out of range" in err(lib)   # indices before det J
    assert not _create(lib, case, conn=bow) and "cell 17 is " in err(lib) and "det J" in err(lib), err(lib)
    flat = case["coords"].copy()
    flat[case["cells"][5]] = flat[case["cells"][5, 0]]       # a cell of zero area
    assert not _create(lib, case, coords=flat) and "cell 5 is degenerate" in err(lib), err(lib)
    nan = case["coords"].copy()
    nan[case["cells"][80, 3], 0] = np.nan
    assert not _create(lib, case, coords=nan) and "cell 80 is degenerate" in err(lib), err(lib)
    # cells numbered the other way round are no error: one sign per cell (a dolfinx mesh numbers its cells either way)
    tri = pg.tri_case("p1tri", "deg2")
    flip = tri["cells"].copy()
    flip[::2] = flip[::2][:, [0, 2, 1]]
    have_gpu = _lib.device_count() > 0                        # (asked first: the question itself leaves a last error)
    for c, over in ((case, {}), (tri, {}), (tri, dict(conn=flip, dofmap=flip))):
        h = _create(lib, c, **over)
        if have_gpu:
            assert h, err(lib)
            assert lib.dxm_mesh_npoints(h) == len(c["cells"]) * c["dphi"].shape[0] and lib.dxm_mesh_displacement_size(h) == 2 * c["n_dofs"]
            lib.dxm_mesh_destroy(h)
        else:
            assert not h and "no usable HIP device" in err(lib), err(lib)       # last: every check above came first


def test_python_constructors_reach_the_library():
    case = pg.quad_case("q2-x9")
    with pytest.raises(ValueError, match="geom_dphi must be"):
        gm.PlaneMesh(case["coords"], case["cells"], case["dofmap"], case["n_dofs"], case["geom_dphi"][:4], case["dphi"])
    with pytest.raises(ValueError, match="dphi must be"):
        gm.PlaneMesh(case["coords"], case["cells"], case["dofmap"][:, :4], case["n_dofs"], case["geom_dphi"], case["dphi"])
    xv, cells = pg.quad_grid()
    with pytest.raises(ValueError, match="degree 1 or 2"):
        gm.PlaneMesh.lagrange(xv, cells, degree=3)
    assert gm.PlaneMesh.tdim == 2 and gm.Hex8Mesh.tdim == 3 and gm.Tet4Mesh.tdim == 3
    for k in ("0:", "1:", "2:", "3:"):
        assert k in gm._DeviceMesh.gradient_device.__doc__
    if _lib.device_count() > 0:
        return          # a GPU is present: test_gpu_plane_gradient.py builds these meshes
    bow = cells.copy()
    bow[3, [2, 3]] = bow[3, [3, 2]]
    with pytest.raises(_lib.DxmError, match="dxm_mesh_create_plane failed: cell 3 is "):
        gm.PlaneMesh.lagrange(xv, bow, degree=2)
    for degree in (1, 2):
        with pytest.raises(_lib.DxmError, match="no usable HIP device"):
            gm.PlaneMesh.lagrange(xv, cells, degree=degree)
        with pytest.raises(_lib.DxmError, match="no usable HIP device"):
            gm.PlaneMesh.lagrange(*triangle_grid(7, seed=3), degree=degree)


def test_the_rows_name_the_kind_of_a_two_dimensional_mesh():
    src = open(os.path.join(CSRC, "dxmat.hip")).read()
    assert "int plane_kind;" in src[src.index("struct LawDesc {"):src.index("constexpr int ct_full_of")]
    for fn, kind in (("plane_stress_law(", "GRAD_IN_PLANE3"), ("plane_strain_law(", "GRAD_PLANE_STRAIN4"), ("plane_stress_j2_law(", "GRAD_IN_PLANE3"),
                     ("law_ps_hosford(", "GRAD_IN_PLANE3")):
        row = src[src.index("constexpr LawDesc " + fn):]
        assert f"d.plane_kind = {kind};" in row[:row.index("\n}\n")], fn
    assert src.count("d.plane_kind = ") == 4
    # the choice is the row's, not an `if` on law ids; the old refusals stay and govern the other meshes
    body = src[src.index("static int integrate_displacement_host("):src.index("const double* dxm_state_ptr(")]
    assert "DXM_LAW_P" not in body and body.count(".plane_kind && mesh_2d(mesh)") == 2 and body.count("no_displacement && !plane_law") == 2
    assert src.count("d.no_fused = d.no_displacement = ") >= 7 and src.count("not served on a mesh that is not two-dimensional") == 5
    # dxmat.hip names no kernel of the unit
    assert "plane_gradient_kernel" not in src and '#include "plane_gradient.hpp"' in src


# ---- the yield mix of the displacement-form tests: a condition, established here on the CPU ------------------------------------------------
@pytest.mark.parametrize("mesh_name", pg.LAW_MESHES)
@pytest.mark.parametrize("law", sorted(LAWS))
def test_at_least_a_tenth_of_the_points_yields_and_a_tenth_stays_elastic(law, mesh_name):
    case = pg.law_mesh(mesh_name)
    n = case["npoints"]
    state = None
    for k, u in enumerate(increments(law, mesh_name)):
        eps = pg.rows(pg.reference(case, u), LAWS[law]["kind"])
        r = reference_update(law, eps, state)
        state = r["carry"]
        share = float(np.mean(r["plastic"]))
        print(f"law {law} {mesh_name} increment {k + 1}: {int(r['plastic'].sum())} of {n} points yield")
        if LAWS[law]["yields"]:
            assert 0.1 <= share <= 0.9, (law, mesh_name, k, share)
        else:
            assert share == 0.0
