"""Inputs shared by the CPU and GPU tests of the finite-strain single-crystal law (law id 21): the committed 50-digit fixture, the
error measure its generator uses, the bounds that follow from it, and batches drawn from the fixture's own points (a yielded point
carries the history the fixture recorded for it).  The restatement ``fs_single_crystal_ref.update`` answers for every batch once."""
import json
import os

import numpy as np

import fs_single_crystal_ref as fx

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fs_single_crystal_kat.npz"))
META = json.loads(str(GOLD["meta"]))
MAXIT = META["maxit"]          # 60: every fixture point converges in the restatement at this cap
#: max(1e-12, 8 x the deviation of the restatement from the 50-digit values), relative to the scale of the field AT THE POINT
BOUND = {k: max(1e-12, 8 * v) for k, v in META["restatement_deviation"].items()}
STATE = ("g", "p", "a", "Fp")   # state fields 0..3 of the law
DT = 0.1
PRM = GOLD["params"][0]


def errors(got, ref):
    """(stress, tangent, state) deviations as the generator measures them: per point, relative to the largest entry of the field
    at that point (the four state fields share one scale); the largest over the points"""
    n = len(ref["stress"])
    es = np.abs(got["stress"] - ref["stress"]).max(axis=1) / np.abs(ref["stress"]).max(axis=1)
    T, Tr = np.asarray(got["tangent"]).reshape(n, 81), np.asarray(ref["tangent"]).reshape(n, 81)
    et = np.abs(T - Tr).max(axis=1) / np.abs(Tr).max(axis=1)
    scale = np.max([np.abs(ref[k]).max(axis=1) for k in STATE], axis=0)
    ev = np.max([np.abs(got[k] - ref[k]).max(axis=1) for k in STATE], axis=0) / scale
    return float(es.max()), float(et.max()), float(ev.max())


def check(tag, got, ref):
    es, et, ev = errors(got, ref)
    print(f"fs single crystal {tag}: stress {es:.3e} (bound {BOUND['stress']:.1e}) tangent {et:.3e} ({BOUND['tangent']:.1e}) "
          f"state {ev:.3e} ({BOUND['state']:.1e})")
    assert es <= BOUND["stress"] and et <= BOUND["tangent"] and ev <= BOUND["state"], (tag, es, et, ev)


def fixture_group(pset, dt):
    """the 30 fixture points of one parameter set and time step (three frame classes x ten stages): inputs and 50-digit answers"""
    m = (GOLD["pset"] == pset) & (GOLD["dt"] == dt)
    inp = {"F": GOLD["F"][m], "R": GOLD["R"][m], "state": {k: GOLD[k + "0"][m] for k in STATE}}
    ref = {k: GOLD[k][m] for k in ("stress", "tangent") + STATE}
    ref["plastic"] = GOLD["yielded"][m]
    return inp, ref


def _pool(yielded):
    m = (GOLD["pset"] == 0) & (GOLD["dt"] == DT) & (GOLD["yielded"] == yielded)
    return {"F": GOLD["F"][m], "R": GOLD["R"][m], **{k: GOLD[k + "0"][m] for k in STATE}}


YIELDED, ELASTIC = _pool(True), _pool(False)   # 18 and 12 points
PERIOD = 36


def case(n, yielded):
    """n points: point i is fixture point i % 18 of the yielded ones or i % 12 of the elastic ones (first parameter set, dt = 0.1),
    with its recorded state and frame.  Returns F, R, state and the restatement's answer; a pattern of period 36 is answered once."""
    y = np.asarray(yielded, dtype=bool)
    i = np.arange(n)

    def pick(k):
        return np.where(y[:, None] if YIELDED[k].ndim == 2 else y[:, None, None], YIELDED[k][i % 18], ELASTIC[k][i % 12])

    F, R = pick("F"), pick("R")
    state = {k: pick(k) for k in STATE}
    if n > PERIOD and (y == y[i % PERIOD]).all():
        one = fx.update(F[:PERIOD], {k: v[:PERIOD] for k, v in state.items()}, PRM, DT, R=R[:PERIOD], maxit=MAXIT)
        ref = {k: v[i % PERIOD] for k, v in one.items()}
    else:
        ref = fx.update(F, state, PRM, DT, R=R, maxit=MAXIT)
    assert (ref["status"] == 0).all() and (ref["plastic"] == y).all()
    return F, R, state, ref
