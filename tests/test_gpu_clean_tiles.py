"""The J2 update with option ``elide_clean_state`` (default 1: a 64-point tile without a yielding point whose state is known to be
the same in both state buffers skips its state store; ``csrc/small_strain_clean.hip``), through the C ABI.

After EVERY call a handle with the default option is held against
  * the numpy oracle at the tolerance of ``tests/test_gpu_parity.py`` (1e-12 of the field scale), and
  * a twin handle with ``elide_clean_state = 0`` -- the kernels the option does not touch -- with ``np.array_equal`` on flux,
    tangent, both state buffers as ``dxm_get_state`` returns them, and the stats;
and ``dxm_clean_tiles`` against a model of the protocol kept on the host: a tile is clean after an eliding launch in which none of
its points yields, and no tile is after anything else has written a state buffer or told of such a write.

Strains by tile class, |f| >= 0.4 sig0 away from the yield surface by construction and checked (> 1e-6 sig0) on the oracle for
every call: E all lanes at 0.3 of the yield strain, P all at 2 x, M one plastic lane among elastic ones (lane 0, lane 63, the last
valid lane of the ragged tile).  Sizes: 1, 63, 64, 65, 401, and 131153 with ``blocks_per_cu = 1`` (2050 tiles on at most 256
workgroups: the grid-stride loop takes further passes)."""
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
CLASSES_A = "EPEMPEM"   # tile t of pattern A is CLASSES_A[t % 7]; pattern B is A moved on by one tile (E -> P, P -> E, M -> E, ...)
IU = np.triu_indices(6)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _law(kind):
    if kind == "linear":
        return _lib.LAW_J2_LINEAR, [E, NU, SIG0_LIN, H_LIN], onp.LinearHardening(SIG0_LIN, H_LIN)
    return _lib.LAW_J2_VOCE, [E, NU, SIG0_V, SIGU_V, B_V], onp.VoceHardening(SIG0_V, SIGU_V, B_V)


def _factors(n, shift):
    """Per point: the multiple of the yield strain of its tile class in pattern A (shift 0) or B (shift 1)."""
    f = np.empty(n)
    ntiles = (n + 63) // 64
    for t in range(ntiles):
        lo, hi = t * 64, min(n, t * 64 + 64)
        cls = CLASSES_A[(t + shift) % 7]
        f[lo:hi] = 2.0 if cls == "P" else 0.3
        if cls == "M":
            lane = hi - lo - 1 if hi - lo < 64 else (0 if t % 2 == 0 else 63)
            f[lo + lane] = 2.0
    return f


class Pair:
    """The handle under test, its twin with the option off, the oracle's copy of the state and the model of the stamps."""

    def __init__(self, kind, layout, n, blocks_per_cu=None):
        import torch

        self.torch = torch
        self.lib = _lib.load()
        self.n, self.ntiles = n, (n + 63) // 64
        self.law, prm, self.hard = _law(kind)
        self.tl, self.nt = LAYOUTS[layout]
        self.layout = layout
        p = np.asarray(prm, dtype=np.float64)
        self.h = []
        for elide in (1, 0):
            h = self.lib.dxm_create(self.law, p.ctypes.data_as(C.POINTER(C.c_double)), p.size, n, 0)
            assert h, _lib.last_error(self.lib)
            self.h.append(h)
            self.chk(self.lib.dxm_set_tangent_layout(h, self.tl))
            if blocks_per_cu:
                self.chk(self.lib.dxm_set_option(h, b"blocks_per_cu", float(blocks_per_cu)))
            if not elide:
                self.chk(self.lib.dxm_set_option(h, b"elide_clean_state", 0.0))
        dev = torch.device("cuda:0")
        self.g = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        self.f = [torch.zeros((n, 6), dtype=torch.float64, device=dev) for _ in range(2)]
        self.c = [torch.zeros((n, self.nt), dtype=torch.float64, device=dev) for _ in range(2)]
        # the oracle's state: s0 and the s1 of the last call
        self.s0 = (np.zeros((n, 6)), np.zeros(n))
        self.s1 = (np.zeros((n, 6)), np.zeros(n))
        self.clean = np.zeros(self.ntiles, dtype=bool)   # the model
        self.exposed = False
        # one fixed deviatoric unit direction per point: |dev| = 1 in the Mandel norm, so that a multiple x of the yield strain
        # gives a trial von Mises stress of x sig0 from the virgin state
        rng = np.random.default_rng(100 + n)
        d = rng.standard_normal((n, 6))
        d[:, :3] -= d[:, :3].mean(axis=1)[:, None]
        d /= np.linalg.norm(d, axis=1)[:, None]
        _, mu = onp.lame(E, NU)
        self.unit = d * (self.hard.sig0 / (2 * mu) * np.sqrt(2.0 / 3.0))

    def chk(self, rc):
        assert rc >= 0, _lib.last_error(self.lib)
        return rc

    def close(self):
        for h in self.h:
            self.lib.dxm_destroy(h)
        self.h = []

    def strain(self, pattern, scale=1.0):
        return self.unit * (_factors(self.n, "AB".index(pattern)) * scale)[:, None]

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

    def clean_tiles(self, k=0):
        a, b = C.c_int64(-1), C.c_int64(-1)
        self.chk(self.lib.dxm_clean_tiles(self.h[k], C.byref(a), C.byref(b)))
        assert b.value == self.ntiles
        return a.value

    # ---- the model of the protocol ------------------------------------------------------------------------------------
    def model_bump(self):
        self.clean[:] = False

    def model_launch(self, plastic, eliding=True):
        if not eliding or self.exposed:
            self.model_bump()
            return
        pad = np.zeros(self.ntiles * 64, dtype=bool)
        pad[: self.n] = plastic
        self.clean = ~pad.reshape(self.ntiles, 64).any(axis=1)

    def expected_clean(self):
        return 0 if self.exposed else int(self.clean.sum())

    # ---- one call on both handles, checked ------------------------------------------------------------------------------
    def reference(self, eps):
        ref = onp.j2_update(eps, self.s0[0], self.s0[1], E, NU, self.hard)
        assert np.abs(ref["f_trial"]).min() > 1e-6 * self.hard.sig0   # oracle and kernel take the same branch
        return ref

    def tangent_blocks(self, flux, ct):
        """the handle's layout -> what it says about the (n, 36) block"""
        if self.layout == "full":
            return ct
        if self.layout == "coef":
            return hr.coef_np(ct)
        if self.layout == "pack4":
            return hr.pack4_np(flux, ct)
        return ct   # sym: compared with the upper triangle

    def check(self, eps, ref, flux, ct, eliding=True, what=""):
        """flux / ct: per handle, as numpy arrays; then the state, the stats and the count"""
        assert np.array_equal(flux[0], flux[1]) and np.array_equal(ct[0], ct[1]), what
        assert relerr(flux[0], ref["sig"]) < TIGHT, what
        want = ref["Ct"][:, IU[0], IU[1]] if self.layout == "sym" else ref["Ct"].reshape(self.n, 36)
        assert relerr(self.tangent_blocks(flux[0], ct[0]), want) < TIGHT, what
        self.s1 = (ref["epsp"], ref["p"])
        self.check_state(what)
        st = [self.stats(k) for k in range(2)]
        assert st[0] == st[1] and st[0]["n_plastic"] == int(ref["plastic"].sum()) and st[0]["n_nan"] == 0 and st[0]["n_not_converged"] == 0, what
        self.model_launch(ref["plastic"], eliding)
        assert self.clean_tiles() == self.expected_clean(), what
        assert self.clean_tiles(1) == 0, what

    def check_state(self, what=""):
        for which, (ep_ref, p_ref) in ((S0, self.s0), (S1, self.s1)):
            a, b = self.state(0, which), self.state(1, which)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, which)
            assert np.abs(a[1] - p_ref).max() <= TIGHT * max(np.abs(p_ref).max(), 1e-300), (what, which)
            assert np.abs(a[0] - ep_ref).max() <= TIGHT * max(np.abs(ep_ref).max(), 1e-300), (what, which)

    def integrate_device(self, eps, what=""):
        torch = self.torch
        ref = self.reference(eps)
        self.g.copy_(to_device(eps))
        st = torch.cuda.current_stream().cuda_stream
        for k in range(2):
            self.f[k].fill_(-7.0)
            self.c[k].fill_(-7.0)
            self.chk(self.lib.dxm_integrate_device(self.h[k], self.g.data_ptr(), 0.0, self.f[k].data_ptr(), self.c[k].data_ptr(), st or None))
        torch.cuda.synchronize()
        self.check(eps, ref, [to_host(t) for t in self.f], [to_host(t) for t in self.c], what=what)
        return ref

    def integrate_host(self, eps, what=""):
        """the host-buffer form (chunked from 32768 points on): its launches cover whole tiles of the handle and elide too"""
        ref = self.reference(eps)
        flux, ct = [], []
        for k in range(2):
            f, c = np.full((self.n, 6), -7.0), np.full((self.n, self.nt), -7.0)
            self.chk(self.lib.dxm_integrate(self.h[k], eps.ctypes.data, 0.0, f.ctypes.data, None, c.ctypes.data, None))
            flux.append(f)
            ct.append(c)
        self.check(eps, ref, flux, ct, what=what)

    def advance(self):
        for h in self.h:
            self.chk(self.lib.dxm_advance(h))
        self.s0 = self.s1

    def revert(self):
        for h in self.h:
            self.chk(self.lib.dxm_revert(h))
        self.s1 = self.s0


def run_sequences(kind, layout, n, blocks_per_cu=None):
    torch = pytest.importorskip("torch")
    P = Pair(kind, layout, n, blocks_per_cu)
    try:
        A, B = P.strain("A"), P.strain("B")
        n_E = sum(1 for t in range(P.ntiles) if CLASSES_A[t % 7] == "E")
        assert P.clean_tiles() == 0

        # 1. pattern A twice: the second call elides the E tiles
        P.integrate_device(A, "1: A, first")
        assert P.clean_tiles() == n_E
        P.integrate_device(A, "1: A, second")
        assert P.clean_tiles() == n_E
        # 2. pattern B: former P tiles that are E now store and come back clean, former E tiles that yield now are marked dirty
        P.integrate_device(B, "2: B")
        # 3. pattern A again: the former-P tiles hold s0's bits in s1 now, and must get A's plastic state back
        P.integrate_device(A, "3: A again")
        assert P.clean_tiles() == n_E
        # 4. advance, then an all-elastic unloading step twice: the clean tiles survive the pointer swap
        before = P.clean_tiles()
        P.advance()
        assert P.clean_tiles() == before
        P.check_state("4: after advance")
        ref = P.integrate_device(0.5 * A, "4: unloading, first")
        assert not ref["plastic"].any() and P.clean_tiles() == P.ntiles
        P.integrate_device(0.5 * A, "4: unloading, second")
        assert P.clean_tiles() == P.ntiles
        # 5. revert, then integrate from the hardened state
        P.revert()
        P.check_state("5: after revert")
        assert P.clean_tiles() == P.ntiles
        P.integrate_device(1.5 * B, "5: after revert")
        # 6. new values into an E tile of S0: every stamp is stale, the count restarts, the results follow the new state
        t_E = [t for t in range(P.ntiles) if CLASSES_A[(t + 1) % 7] == "E" or P.ntiles == 1][0]
        p_new = P.s0[1].copy()
        p_new[t_E * 64: t_E * 64 + 64] += 1e-4
        for h in P.h:
            a = np.ascontiguousarray(p_new.reshape(-1, 1))
            P.chk(P.lib.dxm_set_state(h, S0, 0, a.ctypes.data))
        P.s0 = (P.s0[0], p_new)
        P.model_bump()
        assert P.clean_tiles() == 0
        P.integrate_device(1.5 * B, "6: after set_state, first")     # (the count is the model's: the tiles without a yielding point)
        P.integrate_device(1.5 * B, "6: after set_state, second")
        # 7. a host-buffer call between two eliding launches
        P.integrate_host(0.5 * A, "7: host-buffer form")
        P.integrate_device(1.5 * B, "7: eliding launch after it")
        P.integrate_device(0.5 * A, "7: and an elastic one")
        # 9. one captured graph of a single launch per handle, replayed twice, then an eager launch
        eps9 = 1.5 * B
        ref = P.reference(eps9)
        P.g.copy_(to_device(eps9))
        torch.cuda.synchronize()
        graphs = []
        for k in range(2):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                P.chk(P.lib.dxm_integrate_device(P.h[k], P.g.data_ptr(), 0.0, P.f[k].data_ptr(), P.c[k].data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream))
            graphs.append(gr)
        P.model_bump()                       # the captured launch is the plain kernel behind a moved-on stamp
        assert P.clean_tiles() == 0
        for rep in range(2):
            for k in range(2):
                P.f[k].fill_(-7.0)
                graphs[k].replay()
                P.chk(P.lib.dxm_notify_replay(P.h[k]))
            torch.cuda.synchronize()
            P.check(eps9, ref, [to_host(t) for t in P.f], [to_host(t) for t in P.c], eliding=False, what=f"9: replay {rep}")
        P.integrate_device(0.5 * A, "9: eager launch after the replays")
        assert P.clean_tiles() == P.ntiles
        P.integrate_device(0.5 * A, "9: eager launch after the replays, eliding")
        del graphs
        # 8. a state address handed out: no store is elided from then on, the results stay
        for h in P.h:
            assert P.lib.dxm_state_ptr(h, S1, 0, 0)
        P.exposed = True
        assert P.clean_tiles() == 0
        P.integrate_device(0.5 * A, "8: after dxm_state_ptr")
        P.integrate_device(1.5 * B, "8: after dxm_state_ptr, plastic")
        assert P.clean_tiles() == 0
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
