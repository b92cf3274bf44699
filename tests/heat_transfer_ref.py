"""numpy restatement of the two heat-transfer laws (``DXM_LAW_HEAT_STATIONARY``, ``DXM_LAW_HEAT_PHASE_CHANGE``) from the equations of
``StationaryHeatTransfer.mfront`` and ``HeatTransferPhaseChange.mfront`` (its lines 41-56).  Every operation is one numpy operation
(individually rounded, nothing fused), in the order the file writes it, and the branch test is the double comparison against
``Ts = Tm - Tsmooth / 2`` and ``Tl = Tm + Tsmooth / 2``, each one rounded operation -- what the kernel does too.

Tangent layout (``dxm_law_blocks_get``): ``-k I`` row-major with its six zeros (9), then ``dj/dT`` (3), then for the phase-change law
``dh/dT = c`` (1): 12 / 13 numbers per point.  ``GROUPS[law]`` names the column ranges of the output groups a bound is taken over.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

STATIONARY, PHASE_CHANGE = 16, 17
STATIONARY_DEFAULTS = (0.0375, 2.165e-4)
PHASE_CHANGE_DEFAULTS = (933.15, 210.0, 3.0e6, 95.0, 2.58e6, 1.08048e9, 0.1)   # Tm, ks, cs, kl, cl, dhsl, Tsmooth
WIDTH = {STATIONARY: 12, PHASE_CHANGE: 13}
#: output group -> columns of the tangent row
GROUPS = {STATIONARY: {"dj_dg": slice(0, 9), "dj_dT": slice(9, 12)},
          PHASE_CHANGE: {"dj_dg": slice(0, 9), "dj_dT": slice(9, 12), "dh_dT": slice(12, 13)}}
T_DEFAULT = 293.15


def solidus_liquidus(params):
    Tm, Tsm = np.float64(params[0]), np.float64(params[6])
    half = Tsm / 2
    return Tm - half, Tm + half


def _tangent(nk, slope, g, c=None):
    n = len(g)
    ct = np.zeros((n, 12 if c is None else 13))
    ct[:, 0] = ct[:, 4] = ct[:, 8] = nk
    ct[:, 9:12] = slope[:, None] * g
    if c is not None:
        ct[:, 12] = c
    return ct


def stationary(g, T, params=STATIONARY_DEFAULTS):
    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (len(g),))
    A, B = np.float64(params[0]), np.float64(params[1])
    with np.errstate(all="ignore"):
        k = 1.0 / (A + B * T)
        nk = -k
        slope = (B * k) * k
        flux = nk[:, None] * g
        ct = _tangent(nk, slope, g)
    return dict(flux=flux, tangent=ct, k=k)


def phase_change(g, T, params=PHASE_CHANGE_DEFAULTS):
    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (len(g),))
    Tm, ks, cs, kl, cl, dhsl, Tsm = (np.float64(v) for v in params)
    Ts, Tl = solidus_liquidus(params)
    solid, liquid = T < Ts, T > Tl
    with np.errstate(all="ignore"):
        dT = T - Ts
        k_tr = ks + ((kl - ks) * dT) / Tsm
        c_tr = (cs + cl) / 2 + dhsl / Tsm
        csTs = cs * Ts
        h_tr = csTs + c_tr * dT
        h_liq = ((cl * (T - Tl) + dhsl) + csTs) + ((cs + cl) * Tsm) / 2
        h_sol = cs * T
        k = np.where(solid, ks, np.where(liquid, kl, k_tr))
        c = np.where(solid, cs, np.where(liquid, cl, c_tr))
        h = np.where(solid, h_sol, np.where(liquid, h_liq, h_tr))
        slope = np.where(solid | liquid, 0.0, -(kl - ks) / Tsm)
        nk = -k
        flux = nk[:, None] * g
        ct = _tangent(nk, slope, g, c)
    return dict(flux=flux, tangent=ct, enthalpy=h, k=k, branch=np.where(solid, 0, np.where(liquid, 2, 1)))


def update(law, g, T, params):
    return stationary(g, T, params) if law == STATIONARY else phase_change(g, T, params)


def n_nan(out):
    bad = ~np.isfinite(out["flux"]).all(axis=1) | ~np.isfinite(out["tangent"]).all(axis=1)
    if "enthalpy" in out:
        bad |= ~np.isfinite(out["enthalpy"])
    return int(bad.sum())


def group_values(law, out):
    """output group -> array: the flux, each tangent block, the enthalpy"""
    groups = {"flux": out["flux"]}
    for name, cols in GROUPS[law].items():
        groups[name] = out["tangent"][:, cols]
    if law == PHASE_CHANGE:
        groups["enthalpy"] = out["enthalpy"][:, None]
    return groups


def load_kat():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heat_transfer_kat.npz"), allow_pickle=False)


def kat_cases(kat):
    """(law, set index, params, g, T, expected groups, recorded restatement deviation per group) of the fixture"""
    import json
    meta = json.loads(str(kat["meta"]))
    for case in meta["cases"]:
        tag = case["tag"]
        exp = {name: kat[f"{tag}_{name}"] for name in case["groups"]}
        yield case["law"], tag, kat[f"{tag}_params"], kat[f"{tag}_g"], kat[f"{tag}_T"], exp, case["restatement_deviation"]


def relative_deviation(got, want):
    """max |got - want| over the group against the group's own scale max |want|"""
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got - want).max())
