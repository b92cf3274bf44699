"""GPU: every update kernel's tile loop beyond its first pass.

The parity tests of the laws stop at 100 003 points, where no wave of the shipped grids (32 ... 256 workgroups per compute unit) takes
a second trip through ``for (tile = ...; tile < ntiles; tile += gridDim.x * WAVES_PER_BLOCK)``.  Here every kernel runs
``tile_loop_cases.size_for(num_cu)`` points (206 147 on 256 compute units) twice: on handle A with the shipped grid -- one pass --
and on handle B with option ``blocks_per_cu = 1`` -- ``num_cu`` workgroups, three full passes and a ragged fourth that 38 workgroups
enter.  Per case:

a. flux, tangent, every state field and the whole status record of B equal A's bit for bit (a point's arithmetic does not depend
   on the trip that handles it: nothing is excluded);
b. on ``tile_loop_cases.reference_sample`` (all of pass 4, the edges of passes 2 and 3, every 97th point between) B agrees with the
   law's float64 restatement / the oracle within the bound and with the comparison of the law's own GPU test, imported from there;
c. a second launch with three poisoned inputs (pass 1, pass 3, the last valid point of the ragged tile) counts ``n_nan == 3`` on
   both handles and leaves every other point's bits alone.

``test_tile_loop_cpu.py`` shows without a GPU that the inputs put both branches of every law into every pass."""
import os

import numpy as np
import pytest

import dolfinx_materials_amd.materials as jm
from dolfinx_materials_amd import _lib
from dolfinx_materials_amd.conventions import tangent_from_coefficients, tangent_from_pack4, unpack_sym_tangent
from dolfinx_materials_amd.jaxmat import JAXMaterial
from oracle import constitutive_np as onp

import law_fuzz as lf
import ogden_ref as og
import orthotropic_ref as orf
import test_gpu_fefp as gfe
import test_gpu_hosford as gh
import test_gpu_orthotropic as gor
import test_gpu_param_fields as gpf
import test_gpu_parity as gj2
import test_gpu_ramberg_osgood as gro
import tile_loop_cases as tc
from helpers import E, NU, to_host
from helpers import to_device as _to_device

pytestmark = pytest.mark.gpu
BOUNDS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "law_fuzz_bounds.npz"))
STAT_KEYS = ("n_points", "n_plastic", "n_not_converged", "n_nan", "max_local_iters")


@pytest.fixture(scope="module")
def cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_device(a):
    """(the shared inputs are read-only arrays: the staging tensor is filled from a copy)"""
    return _to_device(np.array(a))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def announce(tag, law, n, cu):
    """The pass counts of the two handles, asserted and printed."""
    pa, pb = tc.passes(n, cu, tc.SHIPPED_BLOCKS_PER_CU[law]), tc.passes(n, cu, 1)
    print(f"tile loop {tag}: {n} points on {cu} compute units, passes A {pa} (blocks_per_cu {tc.SHIPPED_BLOCKS_PER_CU[law]}) B {pb} (blocks_per_cu 1)")
    assert pa == 1 and pb >= 4, (tag, pa, pb)


def state_of(mat, dims):
    """Every state field of s1 (hidden ones included), through dxm_get_state."""
    out = []
    for f, dim in enumerate(dims):
        a = np.empty((mat._n, dim))
        mat._chk(mat._lib.dxm_get_state(mat._require(), _lib.S1, f, a.ctypes.data))
        out.append(a)
    return out


class Launch:
    """flux, tangent, state fields and status record of one launch"""

    def __init__(self, flux, ct, state, stats):
        self.flux, self.ct, self.state, self.stats = flux, ct, state, {k: stats[k] for k in STAT_KEYS}


def drive(mat, launch, grads, state_dims, poisoned=None):
    """One ``launch(mat, gradient)`` per increment with ``advance`` in between; then, from the same initial state as the last increment,
    the poisoned one.  Returns ([Launch per increment], Launch of the poisoned one or None)."""
    import torch

    n = mat._n
    f = torch.zeros((n, mat._info.n_flux), dtype=torch.float64, device="cuda:0")
    c = torch.zeros((n, mat.tangent_size), dtype=torch.float64, device="cuda:0")

    def one(g):
        launch(mat, g, f, c)
        torch.cuda.synchronize()
        rc, st = mat.stats()
        assert rc >= 0
        return Launch(to_host(f), to_host(c), state_of(mat, state_dims), st)

    out = []
    for k, g in enumerate(grads):
        if k:
            mat.data_manager.update()
        out.append(one(g))
    return out, (one(poisoned) if poisoned is not None else None)


def launch_array(mat, g, f, c):
    mat.integrate_device(g.data_ptr(), f.data_ptr(), c.data_ptr())


def assert_same_launch(tag, a, b, but=None):
    """(a): every bit of b is a's; ``but``: points left out (the poisoned ones)."""
    keep = slice(None) if but is None else np.setdiff1d(np.arange(len(a.flux)), but)
    assert same(a.flux[keep], b.flux[keep]), (tag, "flux")
    assert same(a.ct[keep], b.ct[keep]), (tag, "tangent")
    assert len(a.state) == len(b.state)
    for f, (x, y) in enumerate(zip(a.state, b.state)):
        assert same(x[keep], y[keep]), (tag, "state field", f)


def run_pair(tag, law, make, grads, state_dims, cu, poisoned, bad, launch=launch_array):
    """Handles A (shipped grid) and B (one workgroup per compute unit) over the same device arrays; assertions (a) and (c).
    Returns B's launches for (b)."""
    A, B = make(), make()
    n = A._n
    announce(tag, law, n, cu)
    B.set_option("blocks_per_cu", 1)
    try:
        ra, pa = drive(A, launch, grads, state_dims, poisoned)
        rb, pb = drive(B, launch, grads, state_dims, poisoned)
    finally:
        A.close()
        B.close()
    for k, (a, b) in enumerate(zip(ra, rb)):
        assert_same_launch(f"{tag} increment {k + 1}", a, b)
        assert a.stats == b.stats and a.stats["n_points"] == n and a.stats["n_nan"] == 0, (tag, k, a.stats, b.stats)
    if poisoned is not None:
        print(f"tile loop {tag}: poisoned launch n_nan A {pa.stats['n_nan']} B {pb.stats['n_nan']} (expected {len(bad)})")
        assert pa.stats["n_nan"] == len(bad) and pb.stats["n_nan"] == len(bad), (tag, pa.stats, pb.stats)
        assert_same_launch(f"{tag} poisoned A against B", pa, pb, but=bad)
        assert_same_launch(f"{tag} poisoned against clean", rb[-1], pb, but=bad)
        assert not np.isfinite(pb.flux[bad]).all(axis=1).any(), tag
    return rb


def nan_strain(eps, points):
    bad = np.array(eps)
    bad[points, [0, 3, 5]] = np.nan
    return bad


def inverted(F9, points):
    """det F <= 0: row 1 of F reflected at the first two points (entries 11, 12, 13 of [11,22,33,12,21,13,31,23,32]), a flat F at the last"""
    bad = np.array(F9)
    for k in (0, 3, 5):
        bad[points[:2], k] *= -1.0
    bad[points[2]] = 0.0
    bad[points[2], :2] = 1.0
    return bad


def block_of(layout, flux, ct):
    """The (n, 36) block a packed small-strain tangent stands for."""
    if layout == "full":
        return ct.reshape(len(ct), 36)
    return {"sym": unpack_sym_tangent, "coef": tangent_from_coefficients, "pack4": lambda c: tangent_from_pack4(flux, c)}[layout](ct).reshape(len(ct), 36)


# ---- small strain, uniform parameters ------------------------------------------------------------------------------------------
def _j2_behaviour(kind):
    el = jm.LinearElasticIsotropic(E=E, nu=NU)
    hard = jm.LinearHardening(gj2.SIG0_LIN, gj2.H_LIN) if kind == "linear" else jm.VoceHardening(gj2.SIG0_V, gj2.SIGU_V, gj2.B_V)
    return jm.vonMisesIsotropicHardening(el, hard)


def check_j2(tag, layout, runs, refs, sample):
    for k, (r, ref) in enumerate(zip(runs, refs)):
        ok = ~ref["skip"]
        sig, blk = r.flux[sample], block_of(layout, r.flux[sample], r.ct[sample])
        p, epsp = r.state[0][sample, 0], r.state[1][sample]
        es, ec = gj2.relerr(sig[ok], ref["sig"][ok]), gj2.relerr(blk[ok], ref["Ct"][ok].reshape(-1, 36))
        ep = np.abs(p[ok] - ref["p"][ok]).max() / max(ref["p"].max(), 1e-300)
        ee = np.abs(epsp[ok] - ref["epsp"][ok]).max() / max(np.abs(ref["epsp"]).max(), 1e-300)
        print(f"tile loop parity {tag} increment {k + 1}: stress {es:.3e} tangent {ec:.3e} p {ep:.3e} epsp {ee:.3e} (bound {gj2.TIGHT:.0e}), "
              f"{int((~ok).sum())} of {len(sample)} at the kink")
        assert es < gj2.TIGHT and ec < gj2.TIGHT and ep < gj2.TIGHT and ee < gj2.TIGHT, (tag, k, es, ec, ep, ee)
        assert (~ok).mean() <= tc.J2_KINK_CAP


@pytest.mark.parametrize("kind,layout", [(k, l) for k in ("linear", "voce") for l in ("full", "sym", "coef", "pack4")])
def test_j2_uniform_parameters(kind, layout, cu):
    N = tc.size_for(cu)
    strains = tc.j2_strains(kind, N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)

    def make():
        m = JAXMaterial(_j2_behaviour(kind), tangent_layout=layout)
        m.set_data_manager(N)
        return m

    tag = f"J2 {kind} {layout}"
    runs = run_pair(tag, "j2_" + kind, make, [to_device(e) for e in strains], (1, 6), cu, to_device(nan_strain(strains[-1], bad)), bad)
    assert 0 < runs[-1].stats["n_plastic"] < N and runs[-1].stats["n_not_converged"] == 0
    check_j2(tag, layout, runs, tc.j2_reference(kind, strains, sample), sample)


def test_elastic(cu):
    N = tc.size_for(cu)
    eps = tc.elastic_strain(N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)

    def make():
        m = JAXMaterial(jm.ElasticBehavior(jm.LinearElasticIsotropic(E=E, nu=NU)))
        m.set_data_manager(N)
        return m

    (r,) = run_pair("elastic", "elastic", make, [to_device(eps)], (), cu, to_device(nan_strain(eps, bad)), bad)
    so, Co = onp.elastic_iso(eps[sample], E, NU)
    es, ec = gj2.relerr(r.flux[sample], so), gj2.relerr(r.ct[sample].reshape(-1, 6, 6), Co)
    print(f"tile loop parity elastic: stress {es:.3e} tangent {ec:.3e} (bound {gj2.TIGHT:.0e})")
    assert es < gj2.TIGHT and ec < gj2.TIGHT


@pytest.mark.parametrize("layout", ["full", "pack4"])
def test_ramberg_osgood(layout, cu):
    N = tc.size_for(cu)
    prm, eps = tc.ramberg_osgood_case(N)
    E_, nu_, sig0, alpha, n_exp = prm
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    assert float(BOUNDS["bound_ro_stress"]) == 1e-12 and float(BOUNDS["bound_ro_tangent"]) == 1e-11      # what check_against_ref applies

    def make():
        m = JAXMaterial(jm.RambergOsgoodNonLinearElasticity(jm.LinearElasticIsotropic(E=E_, nu=nu_), sig0=sig0, alpha=alpha, n=n_exp), tangent_layout=layout)
        m.set_data_manager(N)
        return m

    tag = f"Ramberg-Osgood {layout}"
    (r,) = run_pair(tag, "ramberg_osgood", make, [to_device(eps)], (), cu, to_device(nan_strain(eps, bad)), bad)
    blk = block_of(layout, r.flux[sample], r.ct[sample])
    ref = gro.ro.update(eps[sample], *prm)
    es, ec = (float(e.max()) for e in lf.ramberg_osgood_errors(r.flux[sample], blk, ref["sig"], ref["Ct_mfront"]))
    print(f"tile loop parity {tag}: stress {es:.3e} (bound 1e-12) tangent {ec:.3e} (bound 1e-11)")
    # the sample's own Newton count stands in for the status record, which counts the whole batch: compared below
    gro.check_against_ref(r.flux[sample], blk, eps[sample], prm, dict(n_plastic=int(ref["newton"].sum()), n_nan=r.stats["n_nan"]), tag=tag)
    assert r.stats["n_plastic"] == tc.ramberg_osgood_newton_count(N) and r.stats["n_not_converged"] == 0, (tag, r.stats)


# ---- per-point parameter fields ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_field_kernels_with_every_parameter_stream_bound(kind, cu):
    N = tc.size_for(cu)
    fields, strains = tc.field_case(kind, N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    streams = len(fields)       # E and nu become the two streams lambda and mu

    def make():
        m = gpf._material(kind, N, fields)
        assert m.kernel_name.startswith("small_strain_field_kernel<") and m._lib.dxm_param_field_mask(m._require()) == (1 << len(fields)) - 1
        assert m._lib.dxm_algorithmic_bytes(m._require()) == 496 + 8 * streams
        return m

    tag = f"field J2 {kind}"
    runs = run_pair(tag, "j2_" + kind, make, [to_device(e) for e in strains], (1, 6), cu, to_device(nan_strain(strains[-1], bad)), bad)
    for k, (r, ref) in enumerate(zip(runs, tc.field_reference(kind, fields, strains, sample))):
        ok = ~ref["skip"]
        errs = dict(stress=gpf._row_rel(r.flux[sample], ref["sig"])[ok].max(), tangent=gpf._row_rel(r.ct[sample], ref["Ct"])[ok].max(),
                    epsp=(np.abs(r.state[1][sample] - ref["epsp"]).max(axis=1) / max(np.abs(ref["epsp"]).max(), 1e-300))[ok].max(),
                    p=(np.abs(r.state[0][sample, 0] - ref["p"]) / max(ref["p"].max(), 1e-300))[ok].max())
        print(f"tile loop parity {tag} increment {k + 1}:", {q: f"{v:.2e}" for q, v in errs.items()}, f"(bound {gpf.TIGHT:.0e})")
        assert all(v <= gpf.TIGHT for v in errs.values()), (tag, k, errs)
        assert (~ok).mean() <= tc.J2_KINK_CAP
    assert 0 < runs[-1].stats["n_plastic"] < N


# ---- fused displacement gradient -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hex8", "tet4"])
def test_fused_displacement_gradient(kind, cu):
    """J2 linear on a hex8 mesh, Ramberg-Osgood on a tet4 mesh: the kernels that evaluate the gradient themselves index the mesh's
    connectivity by the cell of the CURRENT tile.  A NaN displacement at a node reaches every Gauss point of the cells around it: the
    poisoned launch counts those."""
    import torch

    from dolfinx_materials_amd.gradient import Hex8Mesh, Tet4Mesh

    case = tc.fused_case(kind, tc.size_for(cu))
    n = case["npoints"]
    mesh = Hex8Mesh(case["coords"], case["conn"]) if kind == "hex8" else Tet4Mesh(case["coords"], case["conn"], nqp=4)
    assert mesh.npoints == n and tc.size_for(cu) <= n < tc.size_for(cu) + case["nqp"]
    law = "j2_linear" if kind == "hex8" else "ramberg_osgood"
    dims = (1, 6) if kind == "hex8" else ()

    def make():
        m = JAXMaterial(_j2_behaviour("linear") if kind == "hex8" else gro.behavior())
        m.set_data_manager(n)
        return m

    def launch(mat, u, f, c):
        mat.integrate_displacement_device(mesh, u.data_ptr(), f.data_ptr(), c.data_ptr())

    nodes, bad = tc.poisoned_nodes(case, cu)
    u_bad = np.array(case["u"]).reshape(-1, 3)
    u_bad[nodes, 1] = np.nan
    assert {1, 3, 4} <= set(tc.pass_of_point(bad, cu, 1)) and n - 1 in bad
    tag = f"fused {kind}"
    (rb,) = run_pair(tag, law, make, [to_device(case["u"])], dims, cu, to_device(u_bad.ravel()), bad, launch=launch)
    assert 0 < rb.stats["n_plastic"] < n and rb.stats["n_not_converged"] == 0
    # against the gradient kernel followed by the update (option fused_gradient = 0): the comparison of
    # test_fused_displacement_forms_match_gradient_then_integrate
    ref = make()
    ref.set_option("fused_gradient", 0)
    (rc,), _ = drive(ref, launch, [to_device(case["u"])], dims)
    ref.close()
    ef, ec = np.abs(rb.flux - rc.flux).max() / np.abs(rc.flux).max(), np.abs(rb.ct - rc.ct).max() / np.abs(rc.ct).max()
    print(f"tile loop {tag}: against fused_gradient = 0 flux {ef:.3e} tangent {ec:.3e} (bound 1e-9)")
    assert ef < 1e-9 and ec < 1e-9
    torch.cuda.synchronize()
    del mesh


# ---- FeFp ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["voce", "linear"])
def test_fefp(kind, cu):
    N = tc.size_for(cu)
    grads = tc.fefp_gradients(kind, N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    hard = jm.VoceHardening(*tc.FEFP[kind]["params"]) if kind == "voce" else jm.LinearHardening(*tc.FEFP[kind]["params"])

    def make():
        m = JAXMaterial(jm.FeFpJ2Plasticity(jm.LinearElasticIsotropic(E=E, nu=NU), hard))
        m.set_data_manager(N)
        return m

    tag = f"FeFp {kind}"
    runs = run_pair(tag, "fefp_" + kind, make, [to_device(F) for F in grads], (1, 6, 6), cu, to_device(inverted(grads[-1], bad)), bad)
    for k, (r, ref) in enumerate(zip(runs, tc.fefp_reference(kind, grads, sample))):
        ok = ~ref["skip"]
        eP, eC = gfe.relerr(r.flux[sample][ok], ref["P"][ok]), gfe.relerr(r.ct[sample][ok], ref["Ct"][ok].reshape(-1, 81))
        ep = np.abs(r.state[0][sample, 0][ok] - ref["p"][ok]).max() / max(ref["p"].max(), 1e-300)
        eb, ecp = gfe.relerr(r.state[1][sample][ok], ref["be_bar"][ok]), gfe.relerr(r.state[2][sample][ok], ref["cpinv"][ok])
        print(f"tile loop parity {tag} increment {k + 1}: P {eP:.3e} tangent {eC:.3e} p {ep:.3e} be_bar {eb:.3e} cp_bar_inv {ecp:.3e} (bound {gfe.TIGHT:.0e})")
        assert eP < gfe.TIGHT and eC < gfe.TIGHT and ep < gfe.TIGHT and eb < gfe.TIGHT and ecp < gfe.TIGHT, (tag, k)
        assert (~ok).mean() <= tc.J2_KINK_CAP
        assert r.stats["n_not_converged"] == 0
    assert 0 < runs[-1].stats["n_plastic"] < N


# ---- Ogden -----------------------------------------------------------------------------------------------------------------------
def test_ogden(cu):
    N = tc.size_for(cu)
    prm, F = tc.ogden_case(N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    bound = float(BOUNDS["bound_ogden"])

    def make():
        m = JAXMaterial(jm.OgdenHyperelasticity(**prm), lazy_isv=False)
        m.set_data_manager(N)
        return m

    (r,) = run_pair("Ogden", "ogden", make, [to_device(F)], (6,), cu, to_device(inverted(F, bad)), bad)
    eP, eA, eI = (float(e.max()) for e in lf.ogden_errors((r.flux[sample], r.ct[sample], r.state[0][sample]), og.closed_form(F[sample], **prm)))
    print(f"tile loop parity Ogden {prm}: P {eP:.3e} A {eA:.3e} PK2Stress {eI:.3e} (bound {bound:.1e})")
    assert eP <= bound and eA <= bound and eI <= bound


# ---- Hosford ---------------------------------------------------------------------------------------------------------------------
def _hosford_material(case, N, layout):
    return gh.material(tc.HOSFORD_A, N, np.array(case["ep0"]), np.array(case["p0"]), tangent_layout=layout)


def check_hosford(tag, layout, runs, case, sample):
    E_, R0 = gh.P["E"], gh.P["R0"]
    for k, r in enumerate(runs):
        ref, skip = tc.hosford_reference(case, k, sample)
        keep = ~skip
        assert ref["converged"].all() and skip.mean() <= lf.KINK_CAP
        isv = np.concatenate([r.state[0][sample], r.state[1][sample]], axis=1)
        blk = block_of(layout, r.flux[sample], r.ct[sample])
        gh.compare(f"tile loop {tag} increment {k + 1}", r.flux[sample][keep], isv[keep], blk[keep], {q: ref[q][keep] for q in ("sig", "eel", "p", "Ct")})
        sc = np.maximum(np.abs(ref["sig"]).max(axis=1), R0)
        ehid = (E_ * np.abs(r.state[2][sample] - ref["ep"]).max(axis=1) / sc)[keep].max()
        print(f"tile loop parity {tag} increment {k + 1}: hidden plastic strain {ehid:.3e} (bound {gh.B_STATE:.2e})")
        assert ehid <= gh.B_STATE
        assert r.stats["n_not_converged"] == 0


@pytest.mark.parametrize("layout", ["full", "sym"])
def test_hosford(layout, cu):
    N = tc.size_for(cu)
    case = tc.hosford_case(N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    tag = f"Hosford a = {tc.HOSFORD_A:g} {layout}"
    runs = run_pair(tag, "hosford", lambda: _hosford_material(case, N, layout), [to_device(e) for e in case["eps"]], (6, 1, 6), cu,
                    to_device(nan_strain(case["eps"][-1], bad)), bad)
    check_hosford(tag, layout, runs, case, sample)


# ---- orthotropic elasticity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("frame", ["none", "uniform", "field"])
def test_orthotropic(frame, layout, cu):
    N = tc.size_for(cu)
    p, eps, R, Ru = tc.orthotropic_case(N)
    sample, bad = tc.reference_sample(N, cu), tc.poisoned_points(N, cu)
    frames = {"none": None, "uniform": Ru, "field": R}[frame]
    tag = f"orthotropic frame {frame} {'sym' if layout else 'full'}"
    announce(tag, "orthotropic", N, cu)
    A, B = gor.Handle(p, N, layout).frame(frames), gor.Handle(p, N, layout).frame(frames)
    B.option("blocks_per_cu", 1)
    assert A.lib.dxm_kernel_name(A.h) == b"orthotropic_kernel<%d" % {"none": 0, "uniform": 1, "field": 2}[frame]
    g, gbad = to_device(eps), to_device(nan_strain(eps, bad))
    try:
        (Sa, Ta, sta), (Sb, Tb, stb) = A.device(g), B.device(g)
        (Pa, Qa, psta), (Pb, Qb, pstb) = A.device(gbad), B.device(gbad)
    finally:
        A.close()
        B.close()
    assert same(Sa, Sb) and same(Ta, Tb) and sta == stb and sta["n_points"] == N and sta["n_nan"] == 0, (tag, sta, stb)
    rs, rc = orf.update(eps[sample], p, None if frames is None else (Ru if frame == "uniform" else R[sample]))
    gor.check(f"tile loop {tag}", Sb[sample], Tb[sample], rs, gor.tri(rc.reshape(-1, 36)) if layout else rc)
    print(f"tile loop {tag}: poisoned launch n_nan A {psta['n_nan']} B {pstb['n_nan']} (expected 3)")
    assert psta["n_nan"] == 3 and pstb["n_nan"] == 3 and psta == pstb
    keep = np.setdiff1d(np.arange(N), bad)
    assert same(Pa[keep], Pb[keep]) and same(Qa[keep], Qb[keep]) and same(Pb[keep], Sb[keep]) and same(Qb[keep], Tb[keep]), tag
    assert np.isnan(Pb[bad]).any(axis=1).all()


# ---- host-buffer form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hosford", "voce_sig0_field"])
def test_host_buffer_form_appends_the_records_of_chunks_that_take_two_passes_each(which, cu):
    """``dxm_integrate`` with a page-locked gradient array, ``max_chunks = 64`` and ``blocks_per_cu = 1``: the packed transfer runs the
    three-stream scheme, whose chunk cap at this size leaves three chunks of more than ``num_cu`` * 256 points.  Each chunk's launch
    takes two passes, indexes state and parameter streams from the chunk's offset and appends its block records behind those of the
    chunks before.  Output, status and state equal the device form on the shipped grid."""
    N = tc.size_for(cu)
    chunks = tc.host_chunks(N, 64)
    print(f"tile loop host-buffer {which}: chunks {chunks}, passes per chunk {[tc.passes(c, cu, 1) for _, c in chunks]}")
    assert len(chunks) >= 2 and all(c > cu * 256 and tc.passes(c, cu, 1) >= 2 for _, c in chunks)
    if which == "hosford":
        case = tc.hosford_case(N)
        strains, dims, law = case["eps"], (6, 1, 6), "hosford"
        make = lambda: _hosford_material(case, N, "full")   # noqa: E731
    else:
        fields, strains = tc.field_case("voce", N)
        dims, law = (1, 6), "j2_voce"
        make = lambda: gpf._material("voce", N, {"sig0": fields["sig0"]})   # noqa: E731
    announce(f"host-buffer {which}", law, N, cu)
    A = make()
    ra, _ = drive(A, launch_array, [to_device(e) for e in strains], dims)
    A.close()
    H = make()
    H.set_option("max_chunks", 64)
    H.set_option("blocks_per_cu", 1)
    assert N >= 32768 and H.tangent_layout == "full"      # the call's transfer is a packed one (options packed_transfer, packed_min_points)
    try:
        for k, (eps, a) in enumerate(zip(strains, ra)):
            if k:
                H.data_manager.update()
            g = H.pinned_array((N, 6))
            g[...] = eps
            flux, isv, ct = H.integrate(g)
            assert H.last_upload == _lib.Stats.UPLOAD[1], H.last_upload       # page-locked: no staging, so the three-stream plan applies
            tag = f"host-buffer {which} increment {k + 1}"
            assert same(np.asarray(flux), a.flux) and same(np.asarray(ct).reshape(N, -1), a.ct), tag
            assert {q: H.last_stats[q] for q in STAT_KEYS} == a.stats, (tag, H.last_stats, a.stats)
            for f, (x, y) in enumerate(zip(state_of(H, dims), a.state)):
                assert same(x, y), (tag, "state field", f)
            visible = np.concatenate([a.state[f] for f in range(2)], axis=1)
            assert same(np.asarray(isv), visible), tag
    finally:
        H.close()
    assert 0 < ra[-1].stats["n_plastic"] < N
