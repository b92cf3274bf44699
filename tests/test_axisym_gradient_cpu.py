"""CPU: the C boundary of the axisymmetric mesh (``dxm_mesh_create_axisymmetric``, ``dxm_mesh_axisymmetric_gradient_device``: declared,
bound, exported; every host-side check of the constructor reached on a machine without a GPU, in the order the header states), the
Python constructor's shape errors, ``radii`` against the restatement, the hypothesis string still refused, and the yield mix of the
displacement the GPU tests of the displacement forms use."""
import os
import re
import subprocess

import numpy as np
import pytest

import axisym_gradient_ref as ag
import plane_gradient_ref as pg
from dolfinx_materials_amd import _lib, materials
from dolfinx_materials_amd import gradient as gm
from plane_laws_2d import increments, reference_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dolfinx_materials_amd", "csrc")


def err(lib):
    return (lib.dxm_last_error() or b"").decode()


def _create(lib, case, **over):
    a = dict(coords=case["coords"], n_vertices=len(case["coords"]), conn=np.ascontiguousarray(case["cells"], dtype=np.int32),
             nv=case["cells"].shape[1], n_cells=len(case["cells"]), dofmap=case["dofmap"], nd=case["dofmap"].shape[1], n_dofs=case["n_dofs"],
             gp=case["geom_phi"], gd=case["geom_dphi"], phi=case["phi"], dphi=case["dphi"], nqp=case["dphi"].shape[0], device=0)
    a.update(over)
    keep = [np.ascontiguousarray(a[k]) for k in ("coords", "conn", "dofmap", "gp", "gd", "phi", "dphi")]
    ptr = [k.ctypes.data for k in keep]
    return lib.dxm_mesh_create_axisymmetric(ptr[0], a["n_vertices"], ptr[1], a["nv"], a["n_cells"], ptr[2], a["nd"], a["n_dofs"], ptr[3], ptr[4],
                                            ptr[5], ptr[6], a["nqp"], a["device"])


def test_both_functions_are_declared_bound_and_exported_and_the_launcher_hidden():
    hdr = open(os.path.join(ROOT, "include", "dxmat.h")).read()
    assert re.search(r"dxm_mesh\* dxm_mesh_create_axisymmetric\(const double\* coords, int64_t n_vertices, const int32_t\* geom_conn, int nv,", hdr)
    assert re.search(r"int dxm_mesh_axisymmetric_gradient_device\(dxm_mesh\* mesh, const double\* u_dev, int kind, double\* grad_dev, double\* radius_dev,", hdr)
    assert "#define DXM_ABI_VERSION 6" in hdr
    assert len(_lib.SYMBOLS["dxm_mesh_create_axisymmetric"][1]) == 14 and len(_lib.SYMBOLS["dxm_mesh_axisymmetric_gradient_device"][1]) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dolfinx_materials_amd", "libdxmat.so")], capture_output=True, text=True).stdout
    for name in ("dxm_mesh_create_axisymmetric", "dxm_mesh_axisymmetric_gradient_device"):
        assert re.search(rf"\sT\s+{name}$", out, flags=re.M), name
    assert "axisym_gradient_launch" not in "\n".join(ln for ln in out.splitlines() if " T " in ln)      # hidden: not exported
    assert _lib.load().dxm_abi_version() == 6
    # the hand-off of the displacement forms comes before the functions whose text the plane-gradient tests pin
    src = open(os.path.join(CSRC, "dxmat.hip")).read()
    assert src.index("static int integrate_axisym_host(") < src.index("static int integrate_displacement_host(")
    body = src[src.index("static int integrate_displacement_host("):src.index("const double* dxm_state_ptr(")]
    assert body.count("if (mesh->axisym) return integrate_axisym_") == 2


def test_host_side_checks_in_their_order():
    """arguments, then indices, then det J, then the tables, then r at every Gauss point, then the device: each with its own sentence,
    none of them needing a GPU"""
    lib = _lib.load()
    case = ag.quad_case("q1-x4")
    for nv in (2, 5, 8):
        assert not _create(lib, case, nv=nv) and "nv = 3 (triangles) or nv = 4 (bilinear quadrilaterals)" in err(lib), err(lib)
    for over in (dict(nd=3), dict(nd=65), dict(nqp=0), dict(nqp=65), dict(n_cells=0), dict(n_dofs=0), dict(n_vertices=0)):
        assert not _create(lib, case, **over) and "invalid plane mesh arguments" in err(lib), (over, err(lib))
    assert not lib.dxm_mesh_create_axisymmetric(None, 4, None, 4, 1, None, 4, 4, None, None, None, None, 1, 0) and "invalid plane mesh arguments" in err(lib)
    keep = [np.ascontiguousarray(case[k]) for k in ("coords", "cells", "dofmap", "geom_dphi", "dphi")]
    p = [k.ctypes.data for k in keep]
    n = (len(case["coords"]), 4, len(case["cells"]), 4, case["n_dofs"])
    for gp, phi in ((None, case["phi"].ctypes.data), (case["geom_phi"].ctypes.data, None)):       # either value table missing
        assert not lib.dxm_mesh_create_axisymmetric(p[0], n[0], p[1], n[1], n[2], p[2], n[3], n[4], gp, p[3], phi, p[4], 4, 0)
        assert "invalid plane mesh arguments" in err(lib), err(lib)
    # indices: the geometry's, then the field's
    bad = case["cells"].copy()
    bad[40, 2] = 100
    assert not _create(lib, case, conn=bad) and "geometry connectivity entry 162 out of range" in err(lib), err(lib)
    dm = case["dofmap"].copy()
    dm[80, 3] = case["n_dofs"]
    assert not _create(lib, case, dofmap=dm) and "dofmap entry 323 out of range" in err(lib), err(lib)
    # det J after the indices, before the tables
    bow = case["cells"].copy()
    bow[17, [2, 3]] = bow[17, [3, 2]]
    assert not _create(lib, case, dofmap=dm, conn=bow) and "dofmap entry 323 out of range" in err(lib)
    assert not _create(lib, case, conn=bow) and "cell 17 is " in err(lib) and "det J" in err(lib), err(lib)
    nanphi = case["phi"].copy()
    nanphi[2, 1] = np.nan
    assert not _create(lib, case, conn=bow, phi=nanphi) and "cell 17 is " in err(lib), err(lib)
    # every table entry finite: phi, dphi, geom_phi, geom_dphi (a NaN in geom_dphi is a det J that is not finite: caught above)
    assert not _create(lib, case, phi=nanphi) and "table phi: entry 9 is not finite" in err(lib), err(lib)
    for name, key, at, entry in (("dphi", "dphi", (1, 3, 0), 14), ("geom_phi", "gp", (3, 0), 12)):
        tab = np.array(case["geom_phi" if key == "gp" else key])
        tab[at] = np.inf
        assert not _create(lib, case, **{key: tab}) and f"table {name}: entry {entry} is not finite" in err(lib), err(lib)
    nangd = case["geom_dphi"].copy()
    nangd[0, 0, 0] = np.nan
    assert not _create(lib, case, gd=nangd) and "cell 0 is degenerate" in err(lib), err(lib)
    # r at every Gauss point: one vertex moved across the axis puts a Gauss point of its cells at r <= 0; the tables come first
    # (the mesh at r = x + 0.01; the corner vertex, which cell 0 alone holds, moved to r = -0.06: the cell stays convex)
    across = pg.quad_case("q1-x4")["coords"].copy()
    across[:, 0] += 0.01
    vert = case["cells"][0, 0]
    assert (case["cells"] == vert).sum() == 1
    across[vert, 0] = -0.06
    rad = ag.radius(dict(case, coords=across)).reshape(len(case["cells"]), -1)
    assert rad[0].min() < 0.0 and rad[1:].min() > 0.0
    assert not _create(lib, case, coords=across, phi=nanphi) and "table phi" in err(lib), err(lib)
    assert not _create(lib, case, coords=across)
    assert "cell 0: r = -" in err(lib) and "one side of the axis" in err(lib) and "no Gauss point on it" in err(lib), err(lib)
    # a mesh that touches the axis with a Gauss point on it: a quadrilateral mesh at r = x (no shift), one point per cell at a vertex
    onaxis = dict(case, coords=pg.quad_case("q1-x4")["coords"])
    vertex_rule = np.zeros((4, 4))
    vertex_rule[:, 0] = 1.0                          # every "Gauss point" is vertex 0 of its cell: r = 0 for the first column of cells
    assert not _create(lib, onaxis, gp=vertex_rule) and "cell 0: r = 0 at Gauss point 0" in err(lib) and "one side of the axis" in err(lib), err(lib)
    left = pg.quad_case("q1-x4")["coords"].copy()
    left[:, 0] -= 2.0                                # the whole mesh at r < 0: det J is fine, r is not
    assert not _create(lib, case, coords=left) and "cell 0: r = -" in err(lib), err(lib)
    # the device last
    tri = ag.tri_case("p2tri", "deg2")
    have_gpu = _lib.device_count() > 0                        # (asked first: the question itself leaves a last error)
    for c in (case, tri):
        h = _create(lib, c)
        if have_gpu:
            assert h, err(lib)
            assert lib.dxm_mesh_npoints(h) == c["npoints"] and lib.dxm_mesh_displacement_size(h) == 2 * c["n_dofs"]
            lib.dxm_mesh_destroy(h)
        else:
            assert not h and "no usable HIP device" in err(lib), err(lib)       # last: every check above came first


def test_python_shape_errors_and_the_constructors_reach_the_library():
    case = ag.quad_case("q2-x9")
    args = lambda **o: [dict(case, **o)[k] for k in ("coords", "cells", "dofmap", "n_dofs", "geom_phi", "geom_dphi", "phi", "dphi")]   # noqa: E731
    with pytest.raises(ValueError, match="geom_dphi must be"):
        gm.AxisymmetricMesh(*args(geom_dphi=case["geom_dphi"][:4]))
    with pytest.raises(ValueError, match="dphi must be"):
        gm.AxisymmetricMesh(*args(dofmap=case["dofmap"][:, :4]))
    with pytest.raises(ValueError, match="phi must be"):
        gm.AxisymmetricMesh(*args(phi=case["phi"][:, :4]))
    with pytest.raises(ValueError, match="geom_phi must be"):
        gm.AxisymmetricMesh(*args(geom_phi=case["geom_phi"][:, :3]))
    xv, cells = pg.quad_grid()
    xv = xv + np.array([1.0, 0.0])
    with pytest.raises(ValueError, match="degree 1 or 2"):
        gm.AxisymmetricMesh.lagrange(xv, cells, degree=3)
    with pytest.raises(ValueError, match="3 .triangles. or 4 .quadrilaterals."):
        gm.AxisymmetricMesh.lagrange(xv, cells[:, :2])
    assert gm.AxisymmetricMesh.tdim == 2 and gm.AxisymmetricMesh.axisymmetric is True and not hasattr(gm.PlaneMesh, "axisymmetric")
    for k in ("0:", "1:", "2:", "3:"):
        assert k in gm.AxisymmetricMesh.axisymmetric_gradient_device.__doc__
    if _lib.device_count() > 0:
        return          # a GPU is present: test_gpu_axisym_gradient.py builds these meshes
    with pytest.raises(_lib.DxmError, match="dxm_mesh_create_axisymmetric failed: cell 0: r = "):
        gm.AxisymmetricMesh.lagrange(xv - np.array([3.0, 0.0]), cells, degree=2)
    for degree in (1, 2):
        with pytest.raises(_lib.DxmError, match="no usable HIP device"):
            gm.AxisymmetricMesh.lagrange(xv, cells, degree=degree)
        with pytest.raises(_lib.DxmError, match="no usable HIP device"):
            gm.AxisymmetricMesh(*args())


def test_radii_against_the_restatement():
    """``AxisymmetricMesh.radii`` returns ``gradient.axisymmetric_radii`` of its tables (a mesh object itself needs a device)"""
    for case in (ag.quad_case("q2-x5"), ag.tri_case("p2tri", "deg2"), ag.tri_case("p1tri", "q7")):
        got = gm.axisymmetric_radii(case["coords"], case["cells"], case["geom_phi"])
        assert got.shape == (case["npoints"],) and np.array_equal(got, ag.radius(case))
        assert np.abs(got - ag.radius(case, np.longdouble)).max() / 2.0 < 1e-15 and got.min() >= 1.0 and got.max() <= 2.0


def test_the_hypothesis_string_is_still_refused():
    with pytest.raises(NotImplementedError, match="needs a gradient of its own"):
        materials._check_hypothesis("axisymmetric")
    with pytest.raises(NotImplementedError, match='hypothesis="axisymmetric" is not served yet'):
        materials.ElasticBehavior(materials.LinearElasticIsotropic(E=70e3, nu=0.3), hypothesis="axisymmetric")


# ---- the yield mix of the displacement-form tests: a condition, established here on the CPU ------------------------------------------------
@pytest.mark.parametrize("mesh_name", pg.LAW_MESHES)
@pytest.mark.parametrize("law", [26, 27, 28])
def test_at_least_a_tenth_of_the_points_yields_and_a_tenth_stays_elastic(law, mesh_name):
    """laws 27 and 28 on the axisymmetric strain of ``plane_laws_2d.increments`` at r = x + 1: the hoop strain u_r / r shifts the mix
    of the plane meshes, not out of [0.1, 0.9]; law 26 never yields"""
    case = ag.law_mesh(mesh_name)
    state = None
    for k, u in enumerate(increments(law, mesh_name)):
        r = reference_update(law, ag.strain(case, u, 0), state)
        state = r["carry"]
        share = float(np.mean(r["plastic"]))
        print(f"law {law} {mesh_name} increment {k + 1}: {int(r['plastic'].sum())} of {case['npoints']} points yield ({share:.2f})")
        if law == 26:
            assert share == 0.0
        else:
            assert 0.1 <= share <= 0.9, (law, mesh_name, k, share)
