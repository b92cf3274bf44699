"""CPU: the plane-strain J2 laws (DXM_LAW_PE_J2_LINEAR = 27, DXM_LAW_PE_J2_VOCE = 28) over the parameter draws of
``plane_stress_j2_cases`` -- the softening ones included -- without a GPU: the restatement ``plane_strain_ref`` against the 6-wide
oracle ``oracle.constitutive_np.j2_update`` on the embedded strains, as ``test_plane_strain_cpu.py`` does at its one parameter set.
What the sweep of the plane-stress law has and a 4-wide closed form makes meaningless is left out: no safeguarded iteration, no
bracket, no rows at its edges.

Bound: the rule of ``test_gpu_plane_strain.py``, 1e-12 of the field scale, points within 1e-9 sig0 of the surface left out (none
here); the scales are ``plane_stress_j2_cases.plane_strain_scales``.  Measured here, largest over the 24 draws and both increments:
see the test's output (``-s``)."""
import numpy as np
import pytest

import plane_strain_ref as pe
import plane_stress_j2_cases as cs
from test_gpu_plane_strain import TIGHT, oracle

LAW4 = {cs.LAWS[0]: pe.J2_LINEAR, cs.LAWS[1]: pe.J2_VOCE}
DRAWS = [(law, k) for law in cs.LAWS for k in range(cs.N_DRAWS)]


def deviations(prm, got, want, keep):
    s, t, e = cs.plane_strain_scales(prm)
    return [np.abs(got[0] - want["stress"])[keep].max() / s, np.abs(got[1] - want["tangent"])[keep].max() / t,
            np.abs(got[2] - want["state"])[keep].max() / e]


@pytest.mark.parametrize("lk", DRAWS, ids=lambda lk: cs.tag(*lk))
def test_the_restatement_against_the_embedded_oracle_over_the_draws(lk):
    law, k = lk
    prm = cs.draw(law, k)
    n = cs.N_PLANE_STRAIN
    R, _ = pe.hardening(LAW4[law], prm)
    ep6, p, ep4, p4 = np.zeros((n, 6)), np.zeros(n), np.zeros((n, 4)), np.zeros(n)
    for q, e in enumerate(cs.plane_strain_increments(prm)):
        want = oracle(LAW4[law], prm, e, ep6, p)
        r = pe.update(LAW4[law], e, ep4, p4, prm)
        got = (r["stress"], r["tangent"], np.concatenate([r["p"][:, None], r["epsp"]], axis=1))
        dev = deviations(prm, got, want, ~want["skip"])
        print(f"plane strain {cs.tag(law, k)} increment {q + 1}: stress / tangent / state " + " ".join(f"{d:.3e}" for d in dev)
              + f"; yielded {int(want['plastic'].sum())} of {n}, Newton steps at most {int(r['iters'].max())}")
        assert all(d <= TIGHT for d in dev), (cs.tag(law, k), q, dev)
        assert want["skip"].sum() == 0 and np.array_equal(r["plastic"], want["plastic"]) and 0.3 * n <= want["plastic"].sum() <= 0.9 * n      # (trials at U(0, 3) sig0: two thirds, then more)
        assert not r["not_converged"].any() and pe.stats(LAW4[law], r)["n_nan"] == 0
        assert int(r["iters"].max()) == (int(want["iters"].max()) if law == cs.LAWS[1] else 0)
        # the yielded points end on their surface, which for a softening draw has shrunk, and stays positive
        seq = np.sqrt(1.5 * ((r["stress"][:, :3] - r["stress"][:, :3].mean(axis=1, keepdims=True)) ** 2).sum(axis=1) + 1.5 * r["stress"][:, 3] ** 2)
        pl = want["plastic"]
        assert np.abs(seq[pl] - R(r["p"][pl])).max() <= 1e-12 * prm[2] and (R(r["p"]) >= cs.R_FLOOR * prm[2]).all()
        if cs.softening(law, k):
            assert R(r["p"][pl]).max() < prm[2]
        ep6, p, ep4, p4 = want["ep6"], want["p"], r["epsp"], r["p"]
