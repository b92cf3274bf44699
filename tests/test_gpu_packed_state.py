"""The J2 update with option ``pack_old_state`` (from the third update of a load step on, the clean kernel reads the old state from
a packed copy of s0 that leaves out the points whose seven slots are all bit-zero; ``csrc/small_strain_packed.hip``, DESIGN.md
section 2), through the C ABI.

After EVERY call a handle with the option on is held against
  * the numpy oracle at 1e-12 of the field scale, and
  * a twin handle with ``pack_old_state = 0`` with ``np.array_equal`` on flux, tangent, both state buffers as ``dxm_get_state``
    returns them, and the stats;
and ``dxm_packed_state`` against a model of the s0 epoch kept on the host: no valid copy before the second full-range launch since
s0 last may have changed, then all tiles and the points of s0 that have a slot which is not bit-zero.

Every load step has at least four integrates (plain, build, use, use) with a different strain each, over a load / reload / unload
history.  Tiles by class (``tile_class``): V never yields (k = 0), P all lanes yield (k = 64 from the second load step on), M one
yielding lane among virgin ones -- lane 0, lane 63, or the last valid lane of the ragged last tile (always M).  Sizes: 1, 63, 64, 65,
401, and 131153 with ``blocks_per_cu = 1`` (2050 tiles on at most 256 workgroups: the tile loop takes further passes)."""
import ctypes as C

import numpy as np
import pytest

from dolfinx_materials_amd import _lib
from oracle import constitutive_np as onp
from oracle import host_rebuild_np as hr

from helpers import E, NU, SIG0_LIN, H_LIN, SIG0_V, SIGU_V, B_V, to_device, to_host

pytestmark = pytest.mark.gpu

TIGHT = 1e-12
S0, S1 = 0, 1
LAYOUTS = {"full": (0, 36), "sym": (1, 21), "coef": (2, 9), "pack4": (3, 4)}
IU = np.triu_indices(6)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _law(kind):
    if kind == "linear":
        return _lib.LAW_J2_LINEAR, [E, NU, SIG0_LIN, H_LIN], onp.LinearHardening(SIG0_LIN, H_LIN)
    return _lib.LAW_J2_VOCE, [E, NU, SIG0_V, SIGU_V, B_V], onp.VoceHardening(SIG0_V, SIGU_V, B_V)


def tile_class(t, ntiles, n):
    if t == ntiles - 1 and n % 64:
        return "M"
    return "VPM"[t % 3]


def factors(n):
    """Per point: the multiple of the yield strain of its tile class (V 0.3, P 2, M 0.3 but for one lane at 2)."""
    f = np.empty(n)
    ntiles = (n + 63) // 64
    for t in range(ntiles):
        lo, hi = t * 64, min(n, t * 64 + 64)
        cls = tile_class(t, ntiles, n)
        f[lo:hi] = 2.0 if cls == "P" else 0.3
        if cls == "M":
            lane = hi - lo - 1 if hi - lo < 64 else (0 if (t // 3) % 2 == 0 else 63)
            f[lo + lane] = 2.0
    return f


def nonzero_bits(ep, p):
    """points with a slot that is not bit-zero (-0.0 and NaN count)"""
    return (np.ascontiguousarray(ep).view(np.uint64).reshape(ep.shape) != 0).any(axis=1) | (np.ascontiguousarray(p).view(np.uint64) != 0)


class Pair:
    """The handle under test, its twin with the option off, the oracle's copy of the state and the model of the s0 epoch."""

    def __init__(self, kind, layout, n, blocks_per_cu=None):
        import torch

        self.torch = torch
        self.lib = _lib.load()
        self.n, self.ntiles = n, (n + 63) // 64
        self.law, prm, self.hard = _law(kind)
        self.tl, self.nt = LAYOUTS[layout]
        self.layout = layout
        self.prm = np.asarray(prm, dtype=np.float64)
        self.h = []
        for pack in (1, 0):
            h = self.lib.dxm_create(self.law, self.prm.ctypes.data_as(C.POINTER(C.c_double)), self.prm.size, n, 0)
            assert h, _lib.last_error(self.lib)
            self.h.append(h)
            self.chk(self.lib.dxm_set_tangent_layout(h, self.tl))
            if blocks_per_cu:
                self.chk(self.lib.dxm_set_option(h, b"blocks_per_cu", float(blocks_per_cu)))
            self.chk(self.lib.dxm_set_option(h, b"pack_old_state", float(pack)))
        dev = torch.device("cuda:0")
        self.g = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        self.f = [torch.zeros((n, 6), dtype=torch.float64, device=dev) for _ in range(2)]
        self.c = [torch.zeros((n, self.nt), dtype=torch.float64, device=dev) for _ in range(2)]
        self.s0 = (np.zeros((n, 6)), np.zeros(n))
        self.s1 = (np.zeros((n, 6)), np.zeros(n))
        # the model (host_side.hpp: PackEpoch)
        self.launches, self.built, self.exposed = 0, False, False
        rng = np.random.default_rng(200 + n)
        d = rng.standard_normal((n, 6))
        d[:, :3] -= d[:, :3].mean(axis=1)[:, None]
        d /= np.linalg.norm(d, axis=1)[:, None]
        _, mu = onp.lame(E, NU)
        self.unit = d * (self.hard.sig0 / (2 * mu) * np.sqrt(2.0 / 3.0)) * factors(n)[:, None]

    def chk(self, rc):
        assert rc >= 0, _lib.last_error(self.lib)
        return rc

    def close(self):
        for h in self.h:
            self.lib.dxm_destroy(h)
        self.h = []

    # ---- what the handles hold --------------------------------------------------------------------------------------
    def state(self, k, which):
        p, ep = np.empty((self.n, 1)), np.empty((self.n, 6))
        self.chk(self.lib.dxm_get_state(self.h[k], which, 0, p.ctypes.data))
        self.chk(self.lib.dxm_get_state(self.h[k], which, 1, ep.ctypes.data))
        return ep, p[:, 0]

    def stats(self, k):
        st = _lib.Stats()
        self.chk(self.lib.dxm_get_stats(self.h[k], C.byref(st)))
        return st.as_dict()

    def packed_state(self, k=0):
        a, b = C.c_int64(-1), C.c_int64(-1)
        self.chk(self.lib.dxm_packed_state(self.h[k], C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- the model ----------------------------------------------------------------------------------------------------
    def model_move(self):
        self.launches, self.built = 0, False

    def model_launch(self, candidate=True):
        if not candidate or self.exposed:
            self.model_move()      # a plain launch behind a moved-on stamp
            return
        if self.launches >= 1:
            self.built = True
        self.launches += 1

    def expected_packed(self):
        if not self.built or self.exposed:
            return (0, 0)
        ep, p = self.state(1, S0)      # (the twin's s0: equal to the handle's, checked)
        return (self.ntiles, int(nonzero_bits(ep, p).sum()))

    def check_packed(self, what=""):
        assert self.packed_state(0) == self.expected_packed(), (what, self.packed_state(0), self.expected_packed())
        assert self.packed_state(1) == (0, 0), what

    # ---- one call on both handles, checked ------------------------------------------------------------------------------
    def tangent_blocks(self, flux, ct):
        if self.layout == "coef":
            return hr.coef_np(ct)
        if self.layout == "pack4":
            return hr.pack4_np(flux, ct)
        return ct

    def check_state(self, what=""):
        for which, (ep_ref, p_ref) in ((S0, self.s0), (S1, self.s1)):
            a, b = self.state(0, which), self.state(1, which)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, which)
            assert np.array_equal(np.signbit(a[0]), np.signbit(b[0])) and np.array_equal(np.signbit(a[1]), np.signbit(b[1])), (what, which)
            assert np.abs(a[1] - p_ref).max() <= TIGHT * max(np.abs(p_ref).max(), 1e-300), (what, which)
            assert np.abs(a[0] - ep_ref).max() <= TIGHT * max(np.abs(ep_ref).max(), 1e-300), (what, which)

    def integrate(self, scale, what="", candidate=True):
        torch = self.torch
        eps = self.unit * scale
        ref = onp.j2_update(eps, self.s0[0], self.s0[1], E, NU, self.hard)
        assert np.abs(ref["f_trial"]).min() > 1e-6 * self.hard.sig0, what   # oracle and kernel take the same branch
        self.g.copy_(to_device(eps))
        st = torch.cuda.current_stream().cuda_stream
        for k in range(2):
            self.f[k].fill_(-7.0)
            self.c[k].fill_(-7.0)
            self.chk(self.lib.dxm_integrate_device(self.h[k], self.g.data_ptr(), 0.0, self.f[k].data_ptr(), self.c[k].data_ptr(), st or None))
        torch.cuda.synchronize()
        flux, ct = [to_host(t) for t in self.f], [to_host(t) for t in self.c]
        assert np.array_equal(flux[0], flux[1]) and np.array_equal(ct[0], ct[1]), what
        assert relerr(flux[0], ref["sig"]) < TIGHT, what
        want = ref["Ct"][:, IU[0], IU[1]] if self.layout == "sym" else ref["Ct"].reshape(self.n, 36)
        assert relerr(self.tangent_blocks(flux[0], ct[0]), want) < TIGHT, what
        self.s1 = (ref["epsp"], ref["p"])
        self.check_state(what)
        s = [self.stats(k) for k in range(2)]
        assert s[0] == s[1] and s[0]["n_plastic"] == int(ref["plastic"].sum()) and s[0]["n_nan"] == 0 and s[0]["n_not_converged"] == 0, what
        self.model_launch(candidate)
        self.check_packed(what)
        return ref

    def load_step(self, scales, what, revert_after=None):
        """plain, build, use, use, ...: the copy exists from the second call on"""
        for i, s in enumerate(scales):
            self.integrate(s, f"{what}, call {i}")
            assert self.packed_state()[0] == (self.ntiles if i >= 1 else 0), (what, i)
            if revert_after == i:
                self.revert()
                self.check_state(f"{what}: after revert")
                self.check_packed(f"{what}: after revert")      # revert keeps the copy
                assert self.packed_state()[0] == (self.ntiles if i >= 1 else 0)

    def advance(self):
        for h in self.h:
            self.chk(self.lib.dxm_advance(h))
        self.s0 = self.s1
        self.model_move()

    def revert(self):
        for h in self.h:
            self.chk(self.lib.dxm_revert(h))
        self.s1 = self.s0

    def set_state(self, ep, p):
        for h in self.h:
            a = np.ascontiguousarray(p.reshape(-1, 1))
            self.chk(self.lib.dxm_set_state(h, S0, 0, a.ctypes.data))
            b = np.ascontiguousarray(ep)
            self.chk(self.lib.dxm_set_state(h, S0, 1, b.ctypes.data))
        self.s0 = (ep, p)
        self.model_move()


def run_sequences(kind, layout, n, blocks_per_cu=None):
    torch = pytest.importorskip("torch")
    P = Pair(kind, layout, n, blocks_per_cu)
    try:
        nt, f = P.ntiles, factors(n)
        classes = [tile_class(t, nt, n) for t in range(nt)]
        P.check_packed("fresh handles")

        # 1. loading from the virgin state: every tile has k = 0, the use launches load no state at all
        P.load_step([1.0, 1.2, 0.9, 1.1], "1: load")
        assert P.packed_state() == (nt, 0)
        P.advance()
        P.check_packed("1: after advance")
        assert P.packed_state() == (0, 0)
        # 2. reloading: V tiles k = 0, P tiles k = 64, M tiles k = 1 (lane 0 / lane 63 / the last valid lane); a revert in between
        P.load_step([1.5, 1.3, 1.6, 1.4], "2: reload", revert_after=1)
        assert P.packed_state() == (nt, int((f == 2.0).sum()))
        P.advance()
        # 3. unloading
        P.load_step([0.5, 0.4, 0.6, 0.45], "3: unload", revert_after=2)
        assert P.packed_state() == (nt, int((f == 2.0).sum()))

        # 4. invalidation, each between a build and the next launch: the event opens a fresh epoch, two calls (plain, build), the
        # event again, then plain, build, use ------------------------------------------------------------------------------------
        def after_build(event, what):
            event()
            assert P.packed_state() == (0, 0), what
            P.load_step([0.55, 0.35], what + ", before")
            event()
            P.check_packed(what)
            assert P.packed_state() == (0, 0), what
            P.load_step([0.5, 0.4, 0.6], what + ", after")

        # 4a. advance
        after_build(P.advance, "4a: advance")
        # 4b. dxm_set_state: a point with only p != 0, one with a single epsp component != 0, one with -0.0 in a slot -- all in lanes
        # that never yielded, where there are any
        virgin = np.flatnonzero(f != 2.0)
        # (the first and the last such point, and one in lane 31 -- the top bit of the mask's low word -- where there is one)
        lane31 = [int(i) for i in virgin if i % 64 == 31]
        picks = sorted({int(virgin[0]), lane31[0] if lane31 else int(virgin[len(virgin) // 2]), int(virgin[-1])}) if len(virgin) else []
        base = (P.s0[0].copy(), P.s0[1].copy())
        amounts = iter([1e-4, 2e-4])

        def set_values():
            ep_new, p_new = base[0].copy(), base[1].copy()
            x = next(amounts)
            if len(picks) >= 1:
                p_new[picks[0]] = x
            if len(picks) >= 2:
                ep_new[picks[1], 3] = 0.1 * x
            if len(picks) >= 3:
                ep_new[picks[2], 0] = -0.0
            P.set_state(ep_new, p_new)

        after_build(set_values, "4b: dxm_set_state")
        kept = int((f == 2.0).sum()) + len(picks)
        assert P.packed_state() == (nt, kept)
        if len(picks) >= 3:      # -0.0 came back as -0.0 in s1, through a use launch
            for k in range(2):
                ep1, _ = P.state(k, S1)
                assert ep1[picks[2], 0] == 0.0 and np.signbit(ep1[picks[2], 0]), k

        # 4c. option off and on: the copy is freed, and built again by the second launch after
        def off_and_on():
            P.chk(P.lib.dxm_set_option(P.h[0], b"pack_old_state", 0.0))
            assert P.packed_state() == (0, 0)
            P.chk(P.lib.dxm_set_option(P.h[0], b"pack_old_state", 1.0))
            P.model_move()

        after_build(off_and_on, "4c: option off and on")
        assert P.packed_state() == (nt, kept)

        # 4d. a launch with a parameter field bound (the constant sig0: the uniform kernel's bits) runs the plain kernel
        def field_launch():
            field = np.full(n, P.prm[2])
            for h in P.h:
                P.chk(P.lib.dxm_set_param_field(h, 2, field.ctypes.data))
            P.integrate(0.45, "4d: field bound", candidate=False)
            for h in P.h:
                P.chk(P.lib.dxm_set_param_field(h, 2, None))

        after_build(field_launch, "4d: launch with a parameter field")
        assert P.packed_state() == (nt, kept)
        # 4e. a state address handed out: no copy from then on, the results stay
        P.advance()
        P.load_step([0.55, 0.35], "4e: before dxm_state_ptr")
        for h in P.h:
            assert P.lib.dxm_state_ptr(h, S1, 0, 0)
        P.exposed = True
        assert P.packed_state() == (0, 0)
        for i, s in enumerate([0.5, 0.4, 1.7]):
            P.integrate(s, f"4e: after dxm_state_ptr, call {i}")
            assert P.packed_state() == (0, 0)
    finally:
        torch.cuda.synchronize()
        P.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["linear", "voce"])
def test_every_sequence_both_laws_all_layouts(kind, layout):
    run_sequences(kind, layout, 401)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_every_sequence_small_sizes(n):
    run_sequences("linear", "full", n)


def test_every_sequence_beyond_the_first_pass_of_the_tile_loop():
    run_sequences("linear", "full", 131153, blocks_per_cu=1)
