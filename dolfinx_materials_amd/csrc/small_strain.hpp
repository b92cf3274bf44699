// Small-strain constitutive updates for gfx950: isotropic elasticity, J2 plasticity with linear or
// Voce isotropic hardening, Ramberg-Osgood nonlinear elasticity.  One fused kernel per law: trial state,
// yield test, local Newton, stress, consistent tangent and state write-back.
//
// Replaces, per Gauss point, what the reference obtains from
//   vmap(jacfwd(behavior.constitutive_update))      dolfinx_materials/jaxmat.py:147-164
// Arithmetic spec (the only in-tree statement of the return mapping):
//   tests/mfront/IsotropicLinearHardeningPlasticity.mfront:49-77
//   python_materials/elasticity.py:12-24 (elastic), tests/test_FeFp_jax.py:14-15 (Voce law)
//   tests/mfront/RambergOsgoodNonLinearElasticity.mfront (Ramberg-Osgood; DESIGN.md section "Ramberg-Osgood")
//
// Mapping (HBM-bound streaming kernel, ~1 flop/B fp64, no MFMA):
//   * one thread per Gauss point, one wave per tile of 64 points, grid-stride over tiles;
//   * the AoS boundary arrays (strain (N,6) in, stress (N,6) and tangent (N,36) out: the memory
//     of the dolfinx quadrature Functions) are moved with 16 B-per-lane, fully coalesced
//     accesses and re-distributed between lanes through a wave-private LDS region (no s_barrier);
//   * persistent state (p, eps_p) is SoA in HBM: 8 B-per-lane coalesced loads/stores;
//   * the 6x6 tangent is never materialised per thread: each point stages 9 doubles
//     (c1, c2, c3, n[6]) in LDS and the whole wave then evaluates
//         Ct = c1 1x1 + c2 I + c3 n x n
//     entry by entry in output order, so the dominant 288 B/point stream leaves as contiguous
//     1 KiB wave stores (SYM = true: only the 21 entries of the upper triangle, 168 B/point).
//
// One text, two kernels.  small_strain_kernel (uniform parameters) and small_strain_field_kernel (the J2 laws with per-point
// parameter streams, param_fields.hpp) are the same tile body, small_strain_body.hpp, included inside the braces of each
// __global__ function with a compile-time FIELDS.  By text and not by a call: with the body in a __device__ __forceinline__ template,
// or only its row load / take / store steps in helpers, the compiler schedules and allocates these kernels differently (thousands
// of differing assembly lines, SGPR spills move, one instantiation 101 -> 102 VGPRs), whereas the included text compiles to the
// instruction streams of two hand-kept copies (tools/check_device_asm.py --parent REV compares).  Every register-pressure measure
// in the body therefore serves both.  What FIELDS = true changes, all of it `if constexpr (FIELDS)` in the body:
//   * lambda, mu, sig0, h1 (and h2 for Voce) of a point are loaded from the bound streams before step 3, 8 B per lane at the
//     point's index; the point's LawParams is a copy written per point (uniform: a reference to the kernel argument -- a copy
//     there changes the uniform kernels' code);
//   * Voce: the Newton tolerance rtol max(|sig0|, 2e-8 mu) of dxmat.hip::build_params is formed per point when sig0 or mu is a stream;
//   * linear hardening: the H < 0 gate of the "rho <= 0" report is a per-lane test when H is a stream;
//   * the opaque re-read of the lane index once per tile is done for both J2 laws, not for Voce only.
// A third kernel of the same text, small_strain_clean_kernel (small_strain_clean.hip, CLEAN = true: the J2 laws, strain-array form),
// adds the per-tile stamp load, the wave-wide vote after the yield test and the skipped state store; here CLEAN is false.
// The elastic and Ramberg-Osgood branches are never instantiated with FIELDS.  The two smaller fragments, small_strain_stage_coef.hpp
// (the nine staged numbers of a point) and small_strain_expand_store.hpp (the rebuild kernels' store loop), are shared the same way
// for the same reason: as helper functions they change dxmat.hip's code (about 1 200 differing assembly lines for the loop alone).
// The row load / take / store steps themselves (steps 1, 2 and 6 of the strain-array path) are tile_rows6_{load,take,store}.hpp, the
// text the Hosford and orthotropic kernels include as well.
#pragma once
#include "dxm_common.hpp"
#include "gradient.hpp"
#include "param_fields.hpp"   // ParamStreams, PF_*: declarations only (a custom-hardening build, dxmat.hip alone, never instantiates a field kernel)

namespace dxm {

enum { LAW_ELASTIC = 0, LAW_J2_LINEAR = 1, LAW_J2_VOCE = 2, LAW_RAMBERG_OSGOOD = 3 };

// What a law streams besides strain, stress and tangent: the J2 laws read and write the SoA state (p, eps_p); every law but
// the elastic one writes per-point tangent coefficients (c1, c2, c3, w).  Ramberg-Osgood has coefficients and no state.
template <int LAW> constexpr bool ss_has_state = LAW == LAW_J2_LINEAR || LAW == LAW_J2_VOCE;
template <int LAW> constexpr bool ss_has_coef = LAW != LAW_ELASTIC;

// Ramberg-Osgood parameters in LawParams (the c[] slots serve user hardening laws in JIT builds only, which never
// instantiate this law), per-handle constants of the local Newton computed on the host: products formed in the kernel
// would be held in vector registers (c[] below, and h1 = 3 mu, h2 = n beta, tol = e_eps / (3 mu), the floor of f')
constexpr int RO_I3MU = 0, RO_BETA = 1, RO_ISIG0 = 2, RO_N = 3, RO_INVN = 4, RO_ESIG = 5;
constexpr double RO_EPS = 1e-12;   // MFront's NumericalThreshold e_eps

// state slots (SoA, leading dimension ld): 0 = p, 1..6 = eps_p (Mandel)
constexpr int SS_NSLOTS = 7;

constexpr int SS_STAGE = 64 * 6;   // doubles per wave: strain in / stress out staging
constexpr int SS_COEF = 64 * 9;    // doubles per wave: (c1,c2,c3,n0..n5) per point
constexpr int SS_LDS_PER_WAVE = SS_STAGE + SS_COEF;
static_assert(8 * HEX_FUSED_REC <= SS_COEF, "the 8 cell records of a fused tile live in the coefficient region");

template <int LAW>
__device__ __forceinline__ double hardening_R(const LawParams& prm, double p) {
  if constexpr (LAW == LAW_J2_LINEAR) {
    return prm.sig0 + prm.h1 * p;
  } else {
#ifdef DXM_CUSTOM_HARDENING
    return custom_R(prm, p);
#else
    return prm.sig0 + DXM_MUL(prm.h1 - prm.sig0, 1.0 - exp(DXM_MUL(-prm.h2, p)));
#endif
  }
}
template <int LAW>
__device__ __forceinline__ double hardening_dR(const LawParams& prm, double p) {
  if constexpr (LAW == LAW_J2_LINEAR) {
    return prm.h1;
  } else {
#ifdef DXM_CUSTOM_HARDENING
    return custom_dR(prm, p);
#else
    return DXM_MUL((prm.h1 - prm.sig0) * prm.h2, exp(DXM_MUL(-prm.h2, p)));
#endif
  }
}

// Ramberg-Osgood nonlinear elasticity (tests/mfront/RambergOsgoodNonLinearElasticity.mfront): stress s of the total strain e
// and the coefficients of Ct = c1 1x1 + c2 I + c3 n x n, n = dev(s) wn (c1..wn hold the linear-branch values on entry).
//   eps_e = sqrt(2/3 dev(e):dev(e)), ne = 2 dev(e) / (3 max(eps_e, e_eps)), sigma = K tr(e) 1 + sig_e ne,
//   sig_e the root of f(x) = x / (3 mu) + beta (x / sig0)^n - eps_e (linear branch: 3 mu eps_e below e_eps).
// Two deviations from the .mfront integrator: Newton starts from min(3 mu eps_e, sig0 (eps_e / beta)^(1/n)), an
// upper bound of the root from which it converges monotonically (f increasing and convex for n >= 1), and stops on the
// step relative to the iterate, |dx| <= rtol x.  The tangent slope d sig_e / d eps_e = 1 / f' is taken from the last
// evaluation (one power per iteration, none after the loop); its change over a step of <= rtol x is n rtol relative.
// (x / sig0)^n is exp(n log(x / sig0)), not pow: with pow inlined the fused-gradient instantiations spill 2-5 VGPRs at the
// 128 of __launch_bounds__ (with exp / log none does).  The rounding of n log(.) costs about n |log(.)| ulp in the power
// term, i.e. <= 1e-15 of it on the reference curve; the root moves by that divided by n.
// `park`: this lane's three LDS pairs of the stress staging (step 5 stores the stress there).  The strain waits in them
// while the local Newton runs: 12 registers fewer live through the inlined exp / log.
__device__ __forceinline__ void ramberg_osgood_update(const LawParams& prm, const double mu, const double* e, double2_t* park,
                                                      double* s, double& c1, double& c2, double& c3, double& wn, const bool valid,
                                                      unsigned long long& c_plastic, unsigned long long& c_notconv,
                                                      unsigned long long& c_maxit) {
  park[0] = double2_t{e[0], e[1]};
  park[1] = double2_t{e[2], e[3]};
  park[2] = double2_t{e[4], e[5]};
  double eq;
  {
    const double third = (e[0] + e[1] + e[2]) * (1.0 / 3.0);
    const double d[6] = {e[0] - third, e[1] - third, e[2] - third, e[3], e[4], e[5]};
    double dd = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) dd += d[c] * d[c];
    eq = sqrt((2.0 / 3.0) * dd);
  }
  double se;
  if (eq < RO_EPS) {
    se = 3.0 * mu * eq;                                   // linear branch: c1 = lambda, c2 = 2 mu, c3 = 0, wn = 0
  } else {
    const double i3mu = prm.c[RO_I3MU], beta = prm.c[RO_BETA], isig0 = prm.c[RO_ISIG0], n = prm.c[RO_N];
    const double nbeta = prm.h2;
    double x = fmin(prm.h1 * eq, prm.sig0 * exp(log(eq / beta) * prm.c[RO_INVN]));
    double df;
    unsigned iters = 0;
    for (;;) {
      const double r = exp(n * log(x * isig0));
      const double f = x * i3mu + beta * r - eq;
      df = i3mu + nbeta * r / fmax(prm.c[RO_ESIG], x);
      const double dx = f / df;
      x -= dx;
      ++iters;
      if (fabs(dx) <= prm.rtol * x) break;
      if (iters >= (unsigned)prm.maxit) { if (valid) ++c_notconv; break; }
    }
    se = x;
    const double dse = 1.0 / fmax(df, prm.tol);
    const double sr = se / eq;
    // K 1x1 + dse ne x ne + sr (2/3 P - ne x ne),  P = I - 1/3 1x1
    c1 = prm.kappa - (2.0 / 9.0) * sr;
    c2 = (2.0 / 3.0) * sr;
    c3 = dse - sr;
    wn = 1.0 / se;
    if (valid) {
      ++c_plastic;
      c_maxit = iters > c_maxit ? iters : c_maxit;
    }
  }
  asm volatile("" ::: "memory");   // the strain is read back from LDS, not kept in registers
  double et[6];
  {
    const double2_t a = park[0], b = park[1], c = park[2];
    et[0] = a.x; et[1] = a.y; et[2] = b.x; et[3] = b.y; et[4] = c.x; et[5] = c.y;
  }
  const double tr = et[0] + et[1] + et[2];
  const double third = tr * (1.0 / 3.0);
  const double d[6] = {et[0] - third, et[1] - third, et[2] - third, et[3], et[4], et[5]};
  const double g = se * (2.0 / 3.0) / fmax(eq, RO_EPS);   // sig_e ne = g dev(e)
  const double ktr = prm.kappa * tr;
  s[0] = ktr + g * d[0];
  s[1] = ktr + g * d[1];
  s[2] = ktr + g * d[2];
  s[3] = g * d[3];
  s[4] = g * d[4];
  s[5] = g * d[5];
}

// GRAD = 0: the strain comes from the (N,6) array `eps`.  GRAD = 1: it is evaluated in the kernel from
// the displacement vector of a hex8 mesh with 8 Gauss points per cell (`src`; `eps` unused): lane
// (cell c of the tile, corner k) gathers one node into a wave-private LDS record, every lane then
// evaluates the isoparametric gradient at its own point -- the strain array (48 B/point written by the
// gradient kernel and read back here) never exists.  GRAD = 2: tet4 mesh, every lane gathers the 4
// nodes of its own cell (the gradient is constant per cell).  GRAD = 3: straight-sided simplices with a Lagrange
// displacement of any order (tet10, tri6 in plane strain, ...: gradient.hpp::simplex_disp_grad), also gathered per lane.
// Entries (i, j) and (i, j+1) of Ct = c1 1x1 + c2 I + c3 n x n from the nine staged numbers cf = (c1, c2, c3, n[6]).
// k3 (ni nj), not (k3 ni) nj: the product ni nj commutes bit for bit, so the block is EXACTLY symmetric and can be
// rebuilt from its coefficients with this very expression elsewhere (host path: dxmat.hip::expand_coef_tangent;
// after an all-gather of coefficients: expand_tangent_kernel below).
__device__ __forceinline__ double2_t tangent_pair(const double* cf, int i, int j) {
  const double k1 = cf[0], k2 = cf[1], k3 = cf[2];
  const double ni = cf[3 + i], nj0 = cf[3 + j], nj1 = cf[4 + j];
  const double t0 = ((i < 3 && j < 3) ? k1 : 0.0) + ((i == j) ? k2 : 0.0);
  const double t1 = ((i < 3 && j + 1 < 3) ? k1 : 0.0) + ((i == j + 1) ? k2 : 0.0);
  double2_t v;
  v.x = t0 + k3 * (ni * nj0);
  v.y = t1 + k3 * (ni * nj1);
  return v;
}

// TL: layout of the tangent output.  TL_FULL the 6x6 block, row-major (what jacobian_flatten holds,
// quadrature_map.py:83-105); TL_SYM its 21 upper-triangle entries; TL_COEF the 9 coefficients
// (c1, c2, c3, n[6]) of Ct = c1 1x1 + c2 I + c3 n x n themselves (72 B/point); TL_PACK4 only (c1, c2, c3, w): the flow
// direction is n = dev(sigma) w by definition (below), so a consumer that receives the stress anyway -- the host-buffer
// form, dxmat.hip::expand_pack4_tangent -- rebuilds n and the block from 32 B/point, bit for bit.
enum { TL_FULL = 0, TL_SYM = 1, TL_COEF = 2, TL_PACK4 = 3 };
constexpr double SS_THIRD = 1.0 / 3.0;

template <int LAW, int TL, int GRAD = 0>
__global__ void __launch_bounds__(BLOCK, 4)  // 4 waves per SIMD (the launcher pads the LDS of the J2 kernels so that a fifth never fits)
small_strain_kernel(const LawParams prm, const int64_t n, const double* __restrict__ eps,
                    const double* __restrict__ s0, double* __restrict__ s1, const int64_t ld,
                    double* __restrict__ sig, double* __restrict__ ct,
                    BlockStats* __restrict__ stats, const MeshSource src) {
  constexpr bool FIELDS = false;
  constexpr ParamStreams pf = {};   // no stream: named by the discarded FIELDS blocks of the body only
  constexpr bool CLEAN = false;
  constexpr uint32_t* stamps = nullptr;   // (small_strain_clean.hip: named by the discarded CLEAN blocks of the body only)
  constexpr uint32_t stamp = 0;
  constexpr int PACKED = 0;               // (small_strain_packed.hip: named by the discarded PACKED blocks of the body only)
  constexpr unsigned long long* pack_mask = nullptr;
  constexpr double* pack_buf = nullptr;
#include "small_strain_body.hpp"
}

// The same kernel for the two J2 laws with the bound streams of `pf` read per point (instantiated in param_fields.hip only).  A field
// that is constant gives the bits of the uniform kernel (tests/test_gpu_param_fields.py).
template <int LAW, int TL, int GRAD = 0>
__global__ void __launch_bounds__(BLOCK, 4)
small_strain_field_kernel(const LawParams prm, const ParamStreams pf, const int64_t n, const double* __restrict__ eps,
                          const double* __restrict__ s0, double* __restrict__ s1, const int64_t ld,
                          double* __restrict__ sig, double* __restrict__ ct,
                          BlockStats* __restrict__ stats, const MeshSource src) {
  static_assert(LAW == LAW_J2_LINEAR || LAW == LAW_J2_VOCE, "parameter fields: the J2 laws");
  constexpr bool FIELDS = true;
  constexpr bool CLEAN = false;
  constexpr uint32_t* stamps = nullptr;
  constexpr uint32_t stamp = 0;
  constexpr int PACKED = 0;               // (small_strain_packed.hip: named by the discarded PACKED blocks of the body only)
  constexpr unsigned long long* pack_mask = nullptr;
  constexpr double* pack_buf = nullptr;
#include "small_strain_body.hpp"
}

#ifndef DXM_UPDATE_KERNELS_ONLY   // (ramberg_osgood.hip: the rebuild kernels below are dxmat.hip's)
// coefficients (N, 9) -> full tangent (N, 36), both in HBM: what a rank runs after all-gathering the 72 B/point
// coefficient form of the J2 tangent instead of its 288 B/point block (sharding.allgather_tangent): 360 B/point of
// HBM traffic buy 216 B/point less on the xGMI links.  Same staging and store loops as step 7 of the update kernel.
__global__ void __launch_bounds__(BLOCK, 4)
expand_tangent_kernel(const int64_t n, const double* __restrict__ cin, double* __restrict__ ct) {
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * SS_COEF];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* coef = lds_all + wid * SS_COEF;
  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    if (npts == WAVE) {
      const double2_t* g = reinterpret_cast<const double2_t*>(cin + base * 9);
      double2_t v[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] = (k * WAVE + lane < 288) ? g[k * WAVE + lane] : double2_t{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 5; ++k)
        if (k * WAVE + lane < 288) reinterpret_cast<double2_t*>(coef)[k * WAVE + lane] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int idx = k * WAVE + lane;
        coef[idx] = idx < npts * 9 ? cin[base * 9 + idx] : 0.0;
      }
    }
    wave_lds_sync();
#include "small_strain_expand_store.hpp"
    wave_lds_sync();
  }
}

// (stress (N, 6), (c1, c2, c3, w) (N, 4)) -> full tangent (N, 36): every lane forms the nine staged numbers of its point with the
// update kernel's own three lines (step 5), then the same store loops.  408 B/point of HBM traffic.
__global__ void __launch_bounds__(BLOCK, 4)
expand_pack4_kernel(const int64_t n, const double* __restrict__ sig, const double* __restrict__ cw, double* __restrict__ ct) {
  constexpr int PER_WAVE = 64 * 6 + 64 * 4;   // staging of a tile's stress rows and packs; the 64 x 9 coefficients reuse it
  static_assert(PER_WAVE >= SS_COEF, "the coefficient records live in the staging region");
  __shared__ __attribute__((aligned(16))) double lds_all[WAVES_PER_BLOCK * PER_WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* coef = lds_all + wid * PER_WAVE;
  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  for (int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wid; tile < ntiles; tile += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // stage the tile's stress rows (3 KiB) and packs (2 KiB) with 16 B-per-lane loads, then one point per lane
    double2_t* st2 = reinterpret_cast<double2_t*>(coef);            // [0, 192) pairs: stress, [192, 320): packs
    {
      const double2_t* g = reinterpret_cast<const double2_t*>(sig + base * 6);
      const double2_t* h = reinterpret_cast<const double2_t*>(cw + base * 4);
      double2_t v[5];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = (k * WAVE + lane < npts * 3) ? g[k * WAVE + lane] : double2_t{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) v[3 + k] = (k * WAVE + lane < npts * 2) ? h[k * WAVE + lane] : double2_t{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 5; ++k) st2[k * WAVE + lane] = v[k];
    }
    wave_lds_sync();
    double s[6], c1, c2, c3, wn;
    {
      const double2_t a = st2[lane * 3], b = st2[lane * 3 + 1], c = st2[lane * 3 + 2];
      s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = b.y; s[4] = c.x; s[5] = c.y;
      const double2_t u = st2[192 + lane * 2], w = st2[192 + lane * 2 + 1];
      c1 = u.x; c2 = u.y; c3 = w.x; wn = w.y;
    }
    wave_lds_sync();
#include "small_strain_stage_coef.hpp"
    wave_lds_sync();
#include "small_strain_expand_store.hpp"
    wave_lds_sync();
  }
}
#endif  // DXM_UPDATE_KERNELS_ONLY

}  // namespace dxm

