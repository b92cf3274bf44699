"""The J2 radial return of ``oracle/constitutive_np.py::j2_update`` with ARRAY parameters: every line of that function and of its
``_solve_dp``, the scalars ``E, nu, sig0, H | sigu, b`` replaced by arrays of one value per point (scalars broadcast).  The
oracle keeps scalar parameters; ``tests/test_param_fields_cpu.py`` pins this restatement to it on piecewise-constant fields, and the
GPU tests (``tests/test_gpu_param_fields.py``) then compare the kernels with it on continuous fields.

Also the synthetic graded fields and load histories those tests share."""
import numpy as np

from oracle import constitutive_np as onp

ONE = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])


def _R(kind, sig0, h1, h2, p):
    if kind == "linear":
        return sig0 + h1 * p
    return sig0 + (h1 - sig0) * (1.0 - np.exp(-h2 * p))


def _dR(kind, sig0, h1, h2, p):
    if kind == "linear":
        return h1 + 0.0 * p
    return (h1 - sig0) * h2 * np.exp(-h2 * p)


def j2_update_fields(eps, epsp_n, p_n, kind, E, nu, sig0, h1, h2=0.0, maxit=onp.NEWTON_MAXIT, rtol=onp.NEWTON_RTOL):
    """``kind``: "linear" (h1 = H) or "voce" (h1 = sigu, h2 = b).  Returns the dictionary of ``onp.j2_update``."""
    eps = np.asarray(eps, dtype=np.float64)
    N = eps.shape[0]
    E, nu, sig0, h1, h2 = (np.broadcast_to(np.asarray(a, dtype=np.float64), (N,)) for a in (E, nu, sig0, h1, h2))
    epsp_n = np.asarray(epsp_n, dtype=np.float64)
    p_n = np.asarray(p_n, dtype=np.float64).reshape(-1)
    lmbda, mu = onp.lame(E, nu)

    eel = eps - epsp_n
    tr = eel[:, 0] + eel[:, 1] + eel[:, 2]
    se = 2 * mu[:, None] * (eel - tr[:, None] / 3.0 * ONE)
    seq = np.sqrt(1.5 * np.einsum("ni,ni->n", se, se))
    f_trial = seq - _R(kind, sig0, h1, h2, p_n)
    plastic = f_trial > 0.0

    dp = np.zeros(N)
    iters = np.zeros(N, dtype=np.int32)
    n = np.zeros((N, 6))
    c1 = np.array(lmbda)
    c2 = 2 * mu
    c3 = np.zeros(N)
    w = np.zeros(N)
    idx = np.nonzero(plastic)[0]
    if idx.size:
        s_, m_, a_, b_, c_, pn_ = seq[idx], mu[idx], sig0[idx], h1[idx], h2[idx], p_n[idx]
        if kind == "linear":
            dp_i = (s_ - a_ - b_ * pn_) / (b_ + 3 * m_)
            it_i = np.zeros(idx.size, dtype=np.int32)
        else:
            dp_i = np.zeros_like(s_)
            it_i = np.zeros(idx.size, dtype=np.int32)
            scale = np.maximum(np.abs(a_), 2e-8 * m_)          # onp.stress_scale, per point
            for _ in range(maxit):
                r = s_ - 3 * m_ * dp_i - _R(kind, a_, b_, c_, pn_ + dp_i)
                active = np.abs(r) > np.maximum(rtol * scale, rtol * s_)
                if not active.any():
                    break
                dr = -3 * m_ - _dR(kind, a_, b_, c_, pn_ + dp_i)
                dp_i = np.where(active, dp_i - r / dr, dp_i)
                it_i += active
        dp[idx] = dp_i
        iters[idx] = it_i
        n[idx] = 1.5 * se[idx] / s_[:, None]
        beta = dp_i / s_
        gamma = 1.0 / (_dR(kind, a_, b_, c_, pn_ + dp_i) + 3 * m_)
        c1[idx] = lmbda[idx] + 2 * m_ * m_ * beta
        c2 = np.array(c2)
        c2[idx] = 2 * m_ - 6 * m_ * m_ * beta
        c3[idx] = 4 * m_ * m_ * (beta - gamma)
        w[idx] = 1.5 / (s_ - 3 * m_ * dp_i)

    epsp = epsp_n + dp[:, None] * n
    p = p_n + dp
    eel = eel - dp[:, None] * n
    tr = eel[:, 0] + eel[:, 1] + eel[:, 2]
    sig = lmbda[:, None] * tr[:, None] * ONE + 2 * mu[:, None] * eel
    Ct = (c1[:, None, None] * np.outer(ONE, ONE)[None] + np.asarray(c2)[:, None, None] * np.eye(6)[None]
          + c3[:, None, None] * n[:, :, None] * n[:, None, :])
    return dict(sig=sig, epsp=epsp, p=p, Ct=Ct, plastic=plastic, iters=iters, f_trial=f_trial,
                coef=np.stack([c1, np.asarray(c2), c3], axis=1), n=n, w=w)


# ---- inputs shared by the CPU and GPU tests -----------------------------------------------------------------------------------
#: uniform values (tests/helpers.py) and the order of the law's parameter vector
BASE = {"linear": dict(E=70e3, nu=0.3, sig0=250.0, H=5e3), "voce": dict(E=70e3, nu=0.3, sig0=350.0, sigu=500.0, b=1e3)}
NAMES = {"linear": ["E", "nu", "sig0", "H"], "voce": ["E", "nu", "sig0", "sigu", "b"]}


def graded_fields(kind, n, which, groups=None, seed=99):
    """name -> (n,) array for the names in ``which``.  Continuous (``groups=None``): E varies 3x and sig0 2x across the batch,
    nu, H, sigu, b by tens of percent, each along its own smooth profile.  ``groups=g``: piecewise constant over g contiguous
    groups of points (the group's value: the profile at its first point)."""
    t = (np.arange(n) + 0.5) / max(n, 1)
    if groups is not None:
        first = (np.arange(groups) * n) // groups
        gid = np.searchsorted(first, np.arange(n), side="right") - 1
        t = t[first[gid]] if n else t
    b = BASE[kind]
    prof = {
        "E": b["E"] * (0.5 + 1.0 * t),                                   # 35e3 .. 105e3: 3x
        "nu": 0.2 + 0.15 * np.sin(3.0 * t) ** 2,                        # 0.2 .. 0.35
        "sig0": b["sig0"] * (2.0 / 3.0) * (1.0 + 1.0 * (1.0 - t)),       # 2x, decreasing
        "H": 5e3 * (0.6 + 0.8 * t),
        "sigu": 500.0 * (1.0 + 0.2 * np.cos(5.0 * t)) + 100.0,           # stays above every sig0 (<= 467)
        "b": 1e3 * (0.7 + 0.6 * t * t),
    }
    return {k: np.ascontiguousarray(prof[k]) for k in which}


def group_slices(n, groups):
    first = (np.arange(groups) * n) // groups
    ends = list(first[1:]) + [n]
    return [slice(int(a), int(e)) for a, e in zip(first, ends) if e > a]


def load_history(n, seed=1234):
    """Three increments of proportional loading, about half of the points plastic at the end (amplitudes 0 .. 3 times a yield
    strain of the UNIFORM parameters: with graded sig0 / E the yield surface crosses the batch)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 6))
    d /= np.linalg.norm(d, axis=1)[:, None]
    mu = 70e3 / 2 / 1.3
    s = rng.uniform(0.0, 3.0, n) * (300.0 / (2 * mu) * np.sqrt(2.0 / 3.0))
    e = d * s[:, None]
    return [e * 0.4, e * 0.8, e]


def param_arrays(kind, fields, n):
    """(E, nu, sig0, h1, h2) for :func:`j2_update_fields`: the field where one is given, else the uniform value."""
    b = BASE[kind]
    get = lambda k: fields[k] if k in fields else b[k]   # noqa: E731
    if kind == "linear":
        return get("E"), get("nu"), get("sig0"), get("H"), 0.0
    return get("E"), get("nu"), get("sig0"), get("sigu"), get("b")


def undecidable(ref, sig0):
    """Points whose elastic / plastic branch is a matter of rounding: |f_trial| <= 1e-9 sig0 of that point."""
    return np.abs(ref["f_trial"]) <= 1e-9 * np.broadcast_to(np.asarray(sig0, dtype=np.float64), ref["f_trial"].shape)
