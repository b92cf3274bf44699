"""No GPU: the inputs of ``test_gpu_tile_loop.py`` are fit for their purpose, shown with the references alone at 256 compute units.

* the pass arithmetic of ``tile_loop_cases`` is that of ``host_side.hpp::launch_grid`` and of the kernels' loop; the shipped grids
  (read from the sources) take one pass over ``size_for(256)`` points, ``blocks_per_cu = 1`` takes four;
* both branches of every law occur in every pass (plastic / Newton share in [0.2, 0.8]; both forms of Ogden's divided difference on
  at least 5 %);
* every reference converges on the sample the GPU tests compare on, and the points left out of the comparison (within 1e-9 of the
  yield kink) stay under their caps: ``law_fuzz.KINK_CAP`` for Hosford, 1e-3 for J2 and FeFp, none anywhere else."""
import os
import re

import numpy as np
import pytest

import law_fuzz as lf
import ogden_ref as og
import orthotropic_ref as orf
import ramberg_osgood_ref as ro
import tile_loop_cases as tc

CU = 256
N = tc.size_for(CU)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dolfinx_materials_amd", "csrc")


@pytest.fixture(scope="module")
def sample():
    return tc.reference_sample(N, CU)


def _in_share(shares, what):
    print(f"{what}: share per pass {[round(s, 3) for s in shares]}")
    assert len(shares) == 4 and all(tc.SHARE[0] <= s <= tc.SHARE[1] for s in shares), (what, shares)


def test_pass_arithmetic():
    assert N == 206_147 and tc.workgroups(N) == 3 * CU + 38
    assert tc.passes(N, CU, 1) == 4 and tc.grid(N, CU, 1) == CU
    b = tc.pass_bounds(N, CU)
    assert [hi - lo for lo, hi in b] == [65536, 65536, 65536, 37 * 256 + 67]
    # the last workgroup: one full wave, one wave of 3 points, two waves without a tile
    last = N - (tc.workgroups(N) - 1) * 256
    assert last == 67 and -(-last // 64) == 2 and last - 64 == 3
    for k, (lo, hi) in enumerate(b):
        assert tc.pass_of_point(lo, CU, 1) == k + 1 and tc.pass_of_point(hi - 1, CU, 1) == k + 1
    # the loop itself, for a small device: workgroup w of a grid of g takes the 256-point blocks w, w + g, w + 2 g, ...
    for n, cu, bpc in ((tc.size_for(3), 3, 1), (tc.size_for(2, 2), 2, 2), (1000, 8, 1), (1, 4, 1)):
        g = tc.grid(n, cu, bpc)
        trips = [len(range(w, tc.workgroups(n), g)) for w in range(g)]
        assert max(trips) == tc.passes(n, cu, bpc)
        if tc.workgroups(n) >= cu * bpc:
            for w in range(g):
                for t, blk in enumerate(range(w, tc.workgroups(n), g)):
                    assert tc.pass_of_point(blk * 256, cu, bpc) == t + 1 == tc.pass_of_point(min(blk * 256 + 255, n - 1), cu, bpc)
    for cu in (64, 104, 256, 304):
        assert tc.passes(tc.size_for(cu), cu, 1) == 4 and (tc.size_for(cu) - 67) % 256 == 0


def _shipped_blocks_per_cu():
    """law -> the figure of its row in dxmat.hip::kLaws, named constants looked up in the headers"""
    text = open(os.path.join(CSRC, "dxmat.hip")).read()
    consts = {}
    for name in os.listdir(CSRC):
        if name.endswith(".hpp"):
            consts.update({k: int(v) for k, v in re.findall(r"constexpr int (\w+_BLOCKS_PER_CU) = (\d+);", open(os.path.join(CSRC, name)).read())})
    out = {}
    for fn, laws in (("law_elastic", ["elastic"]), ("law_j2_linear", ["j2_linear"]), ("law_j2_voce", ["j2_voce"]), ("law_ramberg_osgood", ["ramberg_osgood"]),
                     ("law_fefp", ["fefp_voce", "fefp_linear"]), ("law_ogden", ["ogden"]), ("law_hosford", ["hosford"]), ("law_orthotropic", ["orthotropic"])):
        body = re.search(r"constexpr LawDesc %s\([^)]*\) \{(.*?)\n\}" % fn, text, re.S).group(1)
        (value,) = re.findall(r"d\.blocks_per_cu = (\w+);", body)
        for law in laws:
            out[law] = int(value) if value.isdigit() else consts[value]
    return out


def test_the_shipped_grids_take_one_pass_and_one_workgroup_per_cu_takes_four():
    shipped = _shipped_blocks_per_cu()
    assert shipped == tc.SHIPPED_BLOCKS_PER_CU
    text = open(os.path.join(CSRC, "host_side.hpp")).read()
    assert "const int64_t tiles = (cnt + 255) / 256;" in text and "std::max<int64_t>(1, std::min<int64_t>(tiles, cap))" in text   # what grid() restates
    for law, bpc in shipped.items():
        assert tc.passes(N, CU, bpc) == 1, law
        assert tc.passes(N + 7, CU, bpc) == 1 and tc.passes(N + 7, CU, 1) == 4   # the mesh cases: whole cells


def test_the_sample_covers_the_late_passes(sample):
    b = tc.pass_bounds(N, CU)
    assert np.array_equal(sample, np.unique(sample)) and sample[0] == b[1][0] and sample[-1] == N - 1
    assert np.isin(np.arange(b[3][0], N), sample).all()
    for lo, hi in b[1:3]:
        assert np.isin(np.r_[lo:lo + 256, hi - 256:hi], sample).all()
    assert np.isin(np.arange(b[1][0], N, 97), sample).all()
    print(f"reference sample: {len(sample)} of {N} points")
    assert 10_000 <= len(sample) <= 20_000
    p = tc.poisoned_points(N, CU)
    assert list(tc.pass_of_point(p, CU, 1)) == [1, 3, 4] and p[2] == N - 1


def test_host_chunks_take_two_passes_each():
    text = open(os.path.join(CSRC, "host_side.hpp")).read()
    for piece in ("n / (packed ? (n >= 2097152 ? 65536 : 32768) : 131072)", "((n + nchunks - 1) / nchunks + 255) / 256 * 256", "(int)(7.0 * std::sqrt((double)r.n / 1e6))",
                  "split_ok && r.max_chunks > p.split_cap ? p.split_cap : r.max_chunks"):
        assert piece in text, piece                     # what plan_chunks() / host_chunks() restate
    chunks = tc.host_chunks(N, 64)
    print("host-buffer chunks:", chunks)
    assert len(chunks) == 3 and sum(c for _, c in chunks) == N and all(c > CU * 256 for _, c in chunks)
    assert all(tc.passes(c, CU, 1) >= 2 for _, c in chunks)
    assert tc.plan_chunks(100_003, True, False, 64) == (3, 33536) and tc.plan_chunks(20_000_000, False, True, 64) == (32, 625152)
    # the fused displacement form keeps the two alternating streams: no three-stream cap, the planner's own count
    assert "const bool split_ok = r.split_streams && r.pipeline && !r.staged_grad && !r.fused;" in text
    for n in (65_535, 65_536, 66_150, 100_003, N, 3_000_000):
        nchunks, csize = tc.plan_chunks(n, True, False, 64)
        fused = tc.host_chunks(n, 64, fused=True)
        assert fused == [(c * csize, min(csize, n - c * csize)) for c in range(nchunks) if c * csize < n]
        assert sum(c for _, c in fused) == n and all(off % 256 == 0 for off, _ in fused)
    assert len(tc.host_chunks(65_535, 64, fused=True)) == 1 and len(tc.host_chunks(65_536, 64, fused=True)) == 2   # chunks from 65 536 points
    assert len(tc.host_chunks(66_150, 64)) == 1 and tc.host_chunks(66_150, 64, fused=True) == [(0, 33280), (33280, 32870)]
    assert tc.host_chunks(N, 64, fused=True) != chunks and tc.host_chunks(N, 2, fused=True) == tc.host_chunks(N, 2)


@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_j2_inputs(kind, sample):
    strains = tc.j2_strains(kind, N)
    full = tc.j2_reference(kind, strains, np.arange(N))
    for inc, r in enumerate(full):
        _in_share(tc.share_per_pass(r["plastic"], CU), f"J2 {kind} increment {inc + 1}")
        assert not r["notconv"].any() if "notconv" in r else True
        excluded = r["skip"][sample].mean()
        print(f"J2 {kind} increment {inc + 1}: {excluded:.2e} of the sample excluded")
        assert excluded <= tc.J2_KINK_CAP
    ref = tc.j2_reference(kind, strains, sample)
    assert all(np.array_equal(a["sig"], b["sig"][sample]) for a, b in zip(ref, full))     # the oracle is point-wise: the sample alone gives the same


@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_field_inputs(kind, sample):
    fields, strains = tc.field_case(kind, N)
    assert set(fields) == set(tc.pfr.NAMES[kind])
    for k, v in fields.items():
        assert len(np.unique(v)) > N // 2, k              # varies from point to point
        assert np.abs(np.diff(v)).mean() > 0.05 * (v.max() - v.min()), k   # ... sharply: neighbouring lanes hold unrelated values
    if kind == "voce":
        assert (fields["sigu"] > fields["sig0"]).all()
    for inc, r in enumerate(tc.field_reference(kind, fields, strains, np.arange(N))):
        _in_share(tc.share_per_pass(r["plastic"], CU), f"field J2 {kind} increment {inc + 1}")
        assert r["skip"][sample].mean() <= tc.J2_KINK_CAP


def test_ramberg_osgood_inputs(sample):
    prm, eps = tc.ramberg_osgood_case(N)
    r = ro.update(eps, *prm)
    _in_share(tc.share_per_pass(r["newton"], CU), f"Ramberg-Osgood {prm}")
    assert r["converged"].all() and r["iters"].max() <= 10          # nothing excluded


@pytest.mark.parametrize("kind", ["voce", "linear"])
def test_fefp_inputs(kind, sample):
    grads = tc.fefp_gradients(kind, N)
    every8 = np.arange(0, N, 8)         # the oracle takes 3 s per increment on all points: the shares from every 8th (8192 per pass)
    for inc, r in enumerate(tc.fefp_reference(kind, grads, every8)):
        _in_share(tc.share_per_pass(r["plastic"], CU, N, every8), f"FeFp {kind} increment {inc + 1}")
    for inc, r in enumerate(tc.fefp_reference(kind, grads, sample)):
        assert not r["notconv"].any() and np.isfinite(r["P"]).all() and np.isfinite(r["Ct"]).all()
        assert r["skip"].mean() <= tc.J2_KINK_CAP
        assert (np.linalg.det(og.to_matrix(grads[inc][sample])) > 0.5).all() if grads[inc].shape[1] == 9 else True


def test_ogden_inputs(sample):
    prm, F = tc.ogden_case(N)
    series, quotient = lf.ogden_paths(F, prm["alpha"])
    s, q = tc.share_per_pass(series, CU), tc.share_per_pass(quotient, CU)
    print(f"Ogden {prm}: series {[round(x, 3) for x in s]} quotient {[round(x, 3) for x in q]}")
    assert min(s) >= tc.OGDEN_SHARE and min(q) >= tc.OGDEN_SHARE
    P, A, S = og.closed_form(F[sample], **prm)
    assert np.isfinite(P).all() and np.isfinite(A).all() and np.isfinite(S).all()     # nothing excluded


def test_hosford_inputs(sample):
    case = tc.hosford_case(N)
    assert tc.HOSFORD_PERIOD % 2 == 1 and (CU * 256) % tc.HOSFORD_PERIOD != 0
    assert len(case["hist"]["ref"]) >= tc.HOSFORD_INCREMENTS
    for inc in range(tc.HOSFORD_INCREMENTS):
        r, skip = tc.hosford_reference(case, inc, np.arange(N))
        _in_share(tc.share_per_pass(r["plastic"], CU), f"Hosford increment {inc + 1}")
        r, skip = tc.hosford_reference(case, inc, sample)
        assert r["converged"].all() and skip.mean() <= lf.KINK_CAP
    # increment 2 unloads most points and yields some again on the other side
    r1, r2 = case["hist"]["ref"][0], case["hist"]["ref"][1]
    assert (r1["plastic"] & ~r2["plastic"]).mean() > 0.1 and (r1["plastic"] & r2["plastic"]).mean() > 0.1


def test_orthotropic_inputs(sample):
    p, eps, R, Ru = tc.orthotropic_case(N)
    labels = orf.frames(N, seed=42)[0]
    for lo, hi in tc.pass_bounds(N, CU):
        assert set(labels[lo:hi]) == set(orf.FRAME_CLASSES)          # every frame class in every pass
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-8 and np.abs(Ru @ Ru.T - np.eye(3)).max() <= 1e-8
    for frame in (None, Ru, R[sample]):
        s, c = orf.update(eps[sample], p, frame)
        assert np.isfinite(s).all() and np.isfinite(c).all()         # nothing excluded


@pytest.mark.parametrize("kind", ["hex8", "tet4"])
def test_fused_gradient_inputs(kind):
    case = tc.fused_case(kind, N)
    n = case["npoints"]
    assert N <= n < N + case["nqp"] and tc.passes(n, CU, 1) == 4 and n % 64 != 0
    assert case["conn"].max() < len(case["coords"]) and case["conn"].min() >= 0 and case["u"].size == 3 * len(case["coords"])
    _in_share(tc.share_per_pass(tc.fused_branch(kind, case), CU), f"fused {kind}")
    nodes, points = tc.poisoned_nodes(case, CU)
    hit = set(tc.pass_of_point(points, CU, 1))
    assert {1, 3, 4} <= hit and n - 1 in points and len(points) % case["nqp"] == 0
