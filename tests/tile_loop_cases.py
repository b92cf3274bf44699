"""Inputs and pass arithmetic for the tests of the update kernels' tile loop beyond its first pass (``test_tile_loop_cpu.py`` pins
them with the references alone, ``test_gpu_tile_loop.py`` holds every kernel to them).  TEST INFRASTRUCTURE ONLY; no GPU.

Every law kernel walks its tiles with ``for (tile = blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += gridDim.x *
WAVES_PER_BLOCK)``: workgroup b owns the 256 points [256 b, 256 b + 256) in its first trip, then those of workgroup b + grid, and
so on.  The grid is ``host_side.hpp::launch_grid``.  With option ``blocks_per_cu = 1`` it has ``num_cu`` workgroups and
:func:`size_for` points take four trips, the last one ragged.

The inputs come from the generators of the laws' own tests, at that size.  Three of them needed help to serve here:

* Hosford: ``law_fuzz.hosford_history`` runs the restatement on every point of every increment (13 s per increment at 2e5 points);
  the history is drawn at ``HOSFORD_PERIOD`` points and point i of the batch is its point ``i % HOSFORD_PERIOD``.  The period is
  odd, so the pattern lines up with no tile (64), workgroup (256) or pass (``num_cu`` * 256).
* per-point parameter fields: ``param_fields_ref.graded_fields`` are smooth profiles along the batch (yield strain 6 x from end to
  end: no single amplitude puts the plastic share of the first and of the last pass inside [0.2, 0.8]); the values are dealt out
  to the points by one seeded permutation, the same for every field, so that each pass sees the whole range and neighbouring lanes
  hold unrelated values (a stream read one lane off gives other numbers).
* FeFp: ``helpers.fefp_path`` with the amplitude that puts increments 9 and 10 of 19 at plastic shares of about 0.4 and 0.7."""
import functools

import numpy as np

import hosford_ref as hr
import law_fuzz as lf
import ogden_ref as og
import orthotropic_ref as orf
import param_fields_ref as pfr
import ramberg_osgood_ref as ro
from helpers import B_F, B_V, E, H_LIN, NU, SIG0_F, SIG0_LIN, SIG0_V, SIGU_F, SIGU_V, fefp_path, j2_history
from oracle import constitutive_np as onp
from test_ramberg_osgood_cpu import PRM as FUSED_RO_PRM   # (E, nu, sig0, alpha, n) of test_gpu_ramberg_osgood.behavior()

WORKGROUP = 256            # points per workgroup and trip: WAVE * WAVES_PER_BLOCK
#: blocks_per_cu a handle of each law is created with (dxmat.hip::kLaws and the headers it names; test_tile_loop_cpu.py reads them
#: from the sources).  The per-point-field and fused-gradient kernels run on their law's handle and take its figure.
SHIPPED_BLOCKS_PER_CU = {"elastic": 32, "j2_linear": 32, "j2_voce": 256, "ramberg_osgood": 64, "fefp_voce": 256, "fefp_linear": 256,
                         "ogden": 256, "hosford": 64, "orthotropic": 64}
KINK = 1e-9                # |f_trial| <= KINK sig0: either branch is right (the rule of every J2 / FeFp parity test)
J2_KINK_CAP = 1e-3         # share of the sample such points may have (J2, FeFp); Hosford: law_fuzz.KINK_CAP
SHARE = (0.2, 0.8)         # plastic / Newton-branch share of every pass
OGDEN_SHARE = 0.05         # of every pass, for each form of the divided difference


# ---- pass arithmetic ------------------------------------------------------------------------------------------------------------
def workgroups(N):
    return -(-int(N) // WORKGROUP)


def grid(N, num_cu, bpc):
    """``host_side.hpp::launch_grid``"""
    return max(1, min(workgroups(N), int(num_cu) * int(bpc)))


def passes(N, num_cu, bpc):
    """Trips the busiest workgroup makes through its tile loop."""
    return -(-workgroups(N) // grid(N, num_cu, bpc))


def pass_of_point(i, num_cu, bpc):
    """1-based pass in which point ``i`` (scalar or array) is processed by a grid that is at its cap of num_cu * bpc workgroups."""
    return np.asarray(i) // (WORKGROUP * int(num_cu) * int(bpc)) + 1


def size_for(num_cu, bpc=1):
    """Three full passes and a fourth that 38 workgroups enter, the last of them with one full wave, one wave of 3 points and two
    waves without a tile."""
    return (3 * int(num_cu) * int(bpc) + 37) * WORKGROUP + 67


def pass_bounds(N, num_cu, bpc=1):
    """[(first, one past the last)] of every pass."""
    span = WORKGROUP * int(num_cu) * int(bpc)
    return [(lo, min(lo + span, N)) for lo in range(0, N, span)]


def reference_sample(N, num_cu):
    """Sorted unique indices: all of pass 4, the first and last 256 points of passes 2 and 3, every 97th point of the rest of
    passes 2 - 4 (``blocks_per_cu = 1``)."""
    b = pass_bounds(N, num_cu)
    assert len(b) >= 4
    parts = [np.arange(b[3][0], N)]
    for lo, hi in b[1:3]:
        parts += [np.arange(lo, lo + WORKGROUP), np.arange(hi - WORKGROUP, hi)]
    parts.append(np.arange(b[1][0], N, 97))
    return np.unique(np.concatenate(parts))


def poisoned_points(N, num_cu):
    """One point in pass 1, one in pass 3 (neither at a tile's edge), the last valid point of the ragged tile."""
    b = pass_bounds(N, num_cu)
    return np.array([b[0][0] + 5 * WORKGROUP + 77, b[2][0] + 11 * WORKGROUP + 130, N - 1])


def plan_chunks(n, packed, staged_upload, max_chunks, pipeline=True):
    """(nchunks, csize) of ``host_side.hpp::plan_chunks``."""
    MAX_CHUNKS = 64
    nchunks = min(n // ((65536 if n >= 2097152 else 32768) if packed else 131072), MAX_CHUNKS * 1024)
    nchunks = max(nchunks, 1)
    if not packed:
        nchunks = min(nchunks, 32 if staged_upload else 8)
    nchunks = min(nchunks, max_chunks, MAX_CHUNKS)
    if not pipeline:
        nchunks = 1
    return nchunks, (-(-n // nchunks) + 255) // 256 * 256


def host_chunks(n, max_chunks=64, fused=False):
    """[(first, count)] of the chunks a host-buffer call makes of n points when its transfer is a packed one and the gradient array
    is page-locked: ``plan_transfer`` then runs the three-stream scheme and caps the chunks at ``int(7 sqrt(n / 1e6))`` in [1, 24].
    ``fused``: the displacement form with the gradient evaluated inside the update kernel (short chunks: a packed transfer or a handle
    whose own layout is packed).  Nothing is uploaded per chunk, the two alternating streams stay and that cap does not apply."""
    split_cap = min(max(int(7.0 * np.sqrt(n / 1e6)), 1), 24)
    nchunks, csize = plan_chunks(n, True, False, split_cap if max_chunks > split_cap and not fused else max_chunks)
    return [(c * csize, min(csize, n - c * csize)) for c in range(nchunks) if c * csize < n]


def share_per_pass(mask, num_cu, N=None, index=None):
    """Share of True per pass; ``index``: the points ``mask`` was evaluated at (else all N)."""
    N = len(mask) if N is None else N
    idx = np.arange(N) if index is None else np.asarray(index)
    return [float(np.mean(mask[(idx >= lo) & (idx < hi)])) for lo, hi in pass_bounds(N, num_cu)]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)          # shared between tests: computed once, left unchanged
    return arrays[0] if len(arrays) == 1 else arrays


# ---- small strain: elastic, J2 -----------------------------------------------------------------------------------------------------
J2 = {"linear": dict(sig0=SIG0_LIN, hard=onp.LinearHardening(SIG0_LIN, H_LIN)), "voce": dict(sig0=SIG0_V, hard=onp.VoceHardening(SIG0_V, SIGU_V, B_V))}


@functools.lru_cache(maxsize=None)
def j2_strains(kind, N):
    """Two increments of ``helpers.j2_history`` (2/3 and 3/3 of the proportional path: 57 % and 72 % of the points yield)."""
    h = j2_history(N, seed=2024, sig0=J2[kind]["sig0"])
    return _frozen(h[1], h[2])


def j2_reference(kind, strains, idx):
    """The oracle on the points ``idx``, increment after increment from the virgin state."""
    ep, p, out = np.zeros((len(idx), 6)), np.zeros(len(idx)), []
    for eps in strains:
        r = onp.j2_update(eps[idx], ep, p, E, NU, J2[kind]["hard"])
        r["skip"] = np.abs(r["f_trial"]) <= KINK * J2[kind]["sig0"]
        out.append(r)
        ep, p = r["epsp"], r["p"]
    return out


@functools.lru_cache(maxsize=None)
def elastic_strain(N):
    return _frozen(j2_history(N, seed=2025)[2])


# ---- per-point parameter fields ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field_case(kind, N):
    perm = np.random.default_rng(77).permutation(N)
    fields = {k: _frozen(np.ascontiguousarray(v[perm])) for k, v in pfr.graded_fields(kind, N, pfr.NAMES[kind]).items()}
    h = pfr.load_history(N, seed=4321)
    return fields, _frozen(h[1], h[2])


def field_case(kind, N):
    """(fields: name -> (N,) array, every parameter of the law; two strain increments)"""
    return _field_case(kind, N)


def field_reference(kind, fields, strains, idx):
    ep, p, out = np.zeros((len(idx), 6)), np.zeros(len(idx)), []
    at = {k: v[idx] for k, v in fields.items()}
    for eps in strains:
        r = pfr.j2_update_fields(eps[idx], ep, p, kind, *pfr.param_arrays(kind, at, len(idx)))
        r["skip"] = pfr.undecidable(r, at["sig0"])
        out.append(r)
        ep, p = r["epsp"], r["p"]
    return out


# ---- Ramberg-Osgood ----------------------------------------------------------------------------------------------------------------
RO_SEED = 3     # n = 20, alpha = 0.07: up to 8 local iterations


@functools.lru_cache(maxsize=None)
def ramberg_osgood_case(N):
    prm, eps = lf.ramberg_osgood_inputs(RO_SEED, N)
    return prm, _frozen(eps)


@functools.lru_cache(maxsize=None)
def ramberg_osgood_newton_count(N):
    """Points of the whole batch on the Newton branch: what the status record's ``n_plastic`` counts for this law."""
    prm, eps = ramberg_osgood_case(N)
    return int(ro.update(eps, *prm)["newton"].sum())


# ---- FeFp --------------------------------------------------------------------------------------------------------------------------
FEFP = {"voce": dict(sig0=SIG0_F, hard=onp.VoceHardening(SIG0_F, SIGU_F, B_F), params=(SIG0_F, SIGU_F, B_F)),
        "linear": dict(sig0=400.0, hard=onp.LinearHardening(400.0, 2e3), params=(400.0, 2e3))}   # the two laws of test_gpu_fefp.py


@functools.lru_cache(maxsize=None)
def fefp_gradients(kind, N):
    """Increments 9 and 10 of the 19 of ``helpers.fefp_path``, at 0.6 of its amplitude per 500 of yield stress."""
    path = fefp_path(N, eps=1.2e-2 * FEFP[kind]["sig0"] / 500.0, seed=4322)
    return _frozen(path[8], path[9])


def fefp_reference(kind, gradients, idx):
    st = onp.fefp_initial_state(len(idx))
    cp, p, out = st["cpinv"], st["p"], []
    for F in gradients:
        r = onp.fefp_update(F[idx], cp, p, E, NU, FEFP[kind]["hard"])
        r["skip"] = np.abs(r["f_trial"]) <= KINK * FEFP[kind]["sig0"]
        out.append(r)
        cp, p = r["cpinv"], r["p"]
    return out


# ---- Ogden -------------------------------------------------------------------------------------------------------------------------
OGDEN_SEED = 2  # alpha = 7.5, stretches up to 1.6


@functools.lru_cache(maxsize=None)
def ogden_case(N):
    prm = lf.draw_ogden(OGDEN_SEED)
    return prm, _frozen(lf.ogden_F(OGDEN_SEED, N, lf.OGDEN_AMPS[OGDEN_SEED % len(lf.OGDEN_AMPS)]))


# ---- Hosford -----------------------------------------------------------------------------------------------------------------------
HOSFORD_PERIOD = 8209
HOSFORD_A = 10.0
HOSFORD_INCREMENTS = 3
HOSFORD_PRM = (hr.PROPS["E"], hr.PROPS["nu"], hr.PROPS["R0"], hr.PROPS["H"], HOSFORD_A)


def hosford_case(N):
    """dict(ep0, p0, eps: three (N, 6), of, hist): point i is point ``of[i]`` of the history ``hist`` (``law_fuzz.hosford_history``:
    every input class, then unloading with re-yielding on the other side, then a non-proportional step)."""
    return _hosford_case(N)


@functools.lru_cache(maxsize=None)
def _hosford_case(N):
    hist = lf.hosford_history(11, HOSFORD_PERIOD, HOSFORD_PRM)
    of = np.arange(N) % HOSFORD_PERIOD
    eps = [np.ascontiguousarray(hist["eps"][k][of]) for k in range(HOSFORD_INCREMENTS)]
    ep0, p0 = np.ascontiguousarray(hist["ep0"][of]), np.ascontiguousarray(hist["p0"][of])
    _frozen(of, ep0, p0, *eps)
    return dict(ep0=ep0, p0=p0, eps=eps, of=of, hist=hist)


def hosford_reference(case, inc, idx):
    """(restatement's results, kink mask) of increment ``inc`` at the points ``idx``."""
    k = case["of"][idx]
    return {q: v[k] for q, v in case["hist"]["ref"][inc].items()}, case["hist"]["skip"][inc][k]


# ---- orthotropic elasticity --------------------------------------------------------------------------------------------------------
ORTHOTROPIC_SET = "strong"


@functools.lru_cache(maxsize=None)
def orthotropic_case(N):
    """(parameters, strains (N, 6), per-point frames (N, 3, 3): every class of ``orthotropic_ref.FRAME_CLASSES`` in turn, one uniform frame)"""
    R = orf.frames(N, seed=42)[1]
    Ru = orf.frames(10, seed=7)[1][8]     # the random class
    return orf.PARAMETER_SETS[ORTHOTROPIC_SET], _frozen(orf.strains(N, seed=41)), _frozen(np.ascontiguousarray(R)), _frozen(Ru)


# ---- fused displacement gradient ---------------------------------------------------------------------------------------------------
FUSED_AMPLITUDE = {"hex8": 2.4e-3, "tet4": 1.0e-2}   # nodal displacement / cell size


@functools.lru_cache(maxsize=None)
def fused_case(kind, N):
    """A distorted hexahedral grid cut down to the cells that reach N Gauss points (whole cells: up to 7 points more), and a random
    nodal displacement.  ``hex8``: 8 Gauss points per cell; ``tet4``: every hexahedron split into 6 tetrahedra of 4 points each.
    Returns dict(coords, conn, u, nqp, npoints, H): H the (npoints, 3, 3) displacement gradients evaluated in numpy."""
    from helpers import KUHN
    from test_gpu_gradient import host_gradient, make_mesh

    from dolfinx_materials_amd.gradient import gauss_points_hex

    nqp = 8 if kind == "hex8" else 4
    ncells = -(-N // nqp)
    side = 1
    while side ** 3 * (1 if kind == "hex8" else 6) < ncells:
        side += 1
    m, coords = make_mesh(side, distort=0.2, seed=5)
    u = FUSED_AMPLITUDE[kind] * m.h * np.random.default_rng(6).standard_normal(m.ndof)
    # layers of nodes at rest (node = (i (side + 1) + j) (side + 1) + k; three layers in six): a third of the cells has no strain at
    # all and stays elastic / below the Ramberg-Osgood threshold, in every pass (k runs fastest in the cell order)
    u.reshape(-1, 3)[(np.arange(m.num_nodes) % (side + 1)) % 6 < 3] = 0.0
    if kind == "hex8":
        conn = np.ascontiguousarray(m.conn[:ncells]).astype(np.int32)
        H = host_gradient(coords, conn, u, gauss_points_hex(2)).reshape(-1, 3, 3)
    else:
        conn = np.ascontiguousarray(np.concatenate([m.conn[:, list(k)] for k in KUHN], axis=0)[:ncells]).astype(np.int32)
        X, U = coords[conn], u.reshape(-1, 3)[conn]
        Hc = (U[:, 1:] - U[:, :1]).transpose(0, 2, 1) @ np.linalg.inv((X[:, 1:] - X[:, :1]).transpose(0, 2, 1))
        H = np.repeat(Hc, nqp, axis=0)
    _frozen(coords, conn, u, H)
    return dict(coords=coords, conn=conn, u=u, nqp=nqp, npoints=ncells * nqp, H=H)


def fused_branch(kind, case):
    """Which points take the plastic (J2 linear on hex8) / Newton (Ramberg-Osgood on tet4) branch, from the numpy gradient."""
    from helpers import mandel_strain

    eps = mandel_strain(case["H"])
    if kind == "hex8":
        return onp.j2_update(eps, np.zeros_like(eps), np.zeros(len(eps)), E, NU, J2["linear"]["hard"])["plastic"]
    return ro.update(eps, *FUSED_RO_PRM)["newton"]




def poisoned_nodes(case, num_cu):
    """(nodes, points): a node of a cell in pass 1, one of a cell in pass 3 and one of the last cell -- a NaN displacement there
    reaches every Gauss point of every cell that holds the node -- and those points."""
    nqp, conn = case["nqp"], case["conn"]
    cells = poisoned_points(case["npoints"], num_cu) // nqp
    nodes = np.array([conn[c, 0] for c in cells])
    hit = np.flatnonzero(np.isin(conn, nodes).any(axis=1))
    return nodes, np.unique((hit[:, None] * nqp + np.arange(nqp)[None]).ravel())
