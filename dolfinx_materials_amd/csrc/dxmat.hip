// libdxmat.so -- C ABI (include/dxmat.h) over the gfx950 constitutive-update kernels.
//
// Host side of the batch dispatch that the reference performs in
//   JAXMaterial.integrate / DataManager           dolfinx_materials/jaxmat.py:30-43, :208-234
//   Material.integrate / MaterialStateManager     dolfinx_materials/generic.py:176-295
// with the state kept device-resident in SoA form instead of dicts of (N, dim) arrays.
// There is deliberately no CPU implementation behind this ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dxmat.h"
#include "dxm_common.hpp"
#include "fefp.hpp"
#include "gradient.hpp"
#include "small_strain.hpp"
#include "ramberg_osgood.hpp"
#include "small_strain_clean.hpp"
#include "param_fields.hpp"
#include "hyperelastic.hpp"
#include "hosford.hpp"
#include "orthotropic.hpp"
#include "single_crystal.hpp"
#include "heat_transfer.hpp"
#include "log_strain.hpp"
#include "fs_single_crystal.hpp"
#include "plane_stress.hpp"
#include "plane_strain.hpp"
#include "plane_stress_j2.hpp"
#include "plane_stress_hosford.hpp"
#include "plane_gradient.hpp"
#include "axisym_gradient.hpp"
#include "heat_plane.hpp"
#include "ogden_plane.hpp"
#include "hosford_plane.hpp"
#include "log_strain_plane.hpp"
#include "host_side.hpp"

using namespace dxm;
static_assert(TL_FULL == DXM_TANGENT_FULL && TL_SYM == DXM_TANGENT_SYM && TL_COEF == DXM_TANGENT_COEF && TL_PACK4 == DXM_TANGENT_PACK4, "kernel and ABI layout ids");

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

// A failing runtime call is reported through the library's own channel (return code + dxm_last_error) and CONSUMED here: the
// runtime's per-thread "last error" is shared with the host application (torch checks it after its own launches), which must not
// find an error of this library in it (tests/conftest.py checks the state after every GPU test).
#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      (void)hipGetLastError();                                                             \
      return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    }                                                                                      \
  } while (0)

// Selects the handle's device for the duration of a call and restores the caller's current
// device afterwards (the host application, e.g. torch, owns the thread's current device).
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) ok = (hipSetDevice(device) == hipSuccess);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
#define DEVICE_GUARD(m)                                                        \
  DeviceGuard _guard((m)->device);                                             \
  if (!_guard.ok) return fail(-2, "hipSetDevice(%d) failed", (m)->device)

// A handle, a mesh or a page-locked block may be released while ANOTHER part of the application is capturing a stream on this thread:
// a garbage collector runs finalizers wherever it likes, inside `with torch.cuda.graph(...)` for one, whose capture mode is global, and
// there a free or a wait counts as an unsafe call that invalidates the capture (hipErrorStreamCaptureInvalidated at its next launch).
// What is released here is no part of that capture, so the releasing calls run in the thread's relaxed mode.
struct RelaxedCaptureMode {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  bool swapped = false;
  RelaxedCaptureMode() {
    swapped = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
    if (!swapped) (void)hipGetLastError();
  }
  ~RelaxedCaptureMode() {
    if (swapped && hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError();
  }
};

// ------------------------------------------------------------------------------------------
// law descriptors: one row of kLaws per law carries everything that law decides; the host code below reads the row of the
// handle's law and tests no law id ("Adding a law")
// ------------------------------------------------------------------------------------------
#ifdef DXM_CUSTOM_HARDENING
// A JIT build with a user-supplied hardening law is dxmat.hip alone: the other translation units' entry points do not exist
constexpr bool kCustomBuild = true;
#define DXM_STOCK_ONLY(entry) nullptr
#else
constexpr bool kCustomBuild = false;
#define DXM_STOCK_ONLY(entry) entry
#endif

struct dxm_material;

// One launch over the point range [off, off + cnt) (off a multiple of 256): the chunk-pipelined host
// path issues several of these on alternating streams; everything else launches the whole batch.
// The block records of the launch go to m->d_stats[stats_off ...).
struct LaunchArgs {
  dxm_material* m;
  int grid;
  hipStream_t st;
  int64_t off, cnt;
  const double* grad;
  double* flux;
  double* ct;
  int stats_off;
  const MeshSource* fused;   // gradient evaluated inside the kernel from this mesh; null: read from `grad`
  int tl;                    // tangent layout of THIS launch (the host path may ask for the coefficient form although the
                             // handle's layout is the full block: it rebuilds the block on the host)
  double dt;                 // the time increment of the call: read by the rate-dependent laws only (LawDesc::rate_dependent)
  bool host_chunk;           // issued by the host-buffer form: kept off the packed copy of s0 (small_strain_clean.hpp)
};

constexpr unsigned L_FULL = 1u << TL_FULL, L_SYM = 1u << TL_SYM, L_COEF = 1u << TL_COEF, L_PACK4 = 1u << TL_PACK4;
constexpr unsigned L_ALL = L_FULL | L_SYM | L_COEF | L_PACK4;

struct LawDesc {
  int id;                                 // DXM_LAW_*: the row's own index in kLaws
  int n_grad, n_flux;
  int n_params, n_params_custom;          // parameters in the stock build / in a custom-hardening build
  int n_isv_fields;                       // user-visible
  int n_fields;                           // incl. hidden state fields (addressable by set/get_state)
  int isv_dim[DXM_MAX_STATE_FIELDS];
  const char* isv_name[DXM_MAX_STATE_FIELDS];
  int isv_slot[DXM_MAX_STATE_FIELDS];     // first SoA slot of the field
  int n_slots;                            // SoA slots incl. hidden ones
  unsigned unit_fields;                   // bit f: field f is a symmetric tensor that starts as the identity (else: zeros)
  int alg_bytes;
  const char* kernel;                     // null: the id is not assigned (law_known)
  const char* field_kernel;               // the kernel while per-point parameter fields are bound; null: the law serves none ...
  const char* no_fields;                  // ... for this reason
  int (*build)(const double* p, LawParams& q);   // validates the n_params parameters and forms the kernel's record from them
  const char* stock_only;                 // what a custom-hardening build answers dxm_create with; null: it serves the law too
  const void* (*residency_kernel)();      // the kernel whose registers and LDS give the residency estimate of dxm_create
  int blocks_per_cu;                      // grid size in workgroups per CU; 0: the residency estimate
  unsigned set_layouts;                   // tangent layouts a handle may be set to (L_* bits) ...
  const char* set_refusal;                // ... and what dxm_set_tangent_layout says to the others
  unsigned launch_layouts;                // layouts a launch may be asked for: the host path also asks for records it expands itself
  const char* launch_refusal;
  const char* no_fused;                   // null: the kernel can evaluate the displacement gradient itself; else the refusal
  const char* no_frame;                   // null: the kernel reads a material frame (dxm_set_frame*); else the refusal
  const char* frame_kernel[2];            // the kernel while a uniform frame / a frame field is bound
  const char* ext_kernel;                 // the kernel while an external state variable is held as a field
  void (*launch)(const LaunchArgs& a);    // null: not launchable in this build
  bool rate_dependent;                    // the update reads the dt of the dxm_integrate* call; the other laws ignore it
  // external state variables (scalars, one value per point: dxm_set_external_state*) and the blocks of the tangent
  int n_ext;
  const char* ext_name[DXM_MAX_EXTERNAL_STATE];
  double ext_default[DXM_MAX_EXTERNAL_STATE];
  int n_blocks;                           // 0: the single block n_flux x n_grad
  dxm_tangent_block blocks[DXM_MAX_TANGENT_BLOCKS];
  int ct_full;                            // doubles per point of the full tangent; 0: n_flux * n_grad (ct_full_of)
  const char* no_displacement;            // null: the gradient may be evaluated from a displacement (dxm_integrate_displacement*); else the refusal
  int plane_kind;                         // the gradient kind a two-dimensional mesh is asked for (plane_gradient.hpp: 2 the plane-strain
                                          // 4-vector, 3 the in-plane 3-vector); there the two refusals above do not apply and the gradient
                                          // kernel always runs on its own.  0: the law is 6 or 9 wide on every mesh
  bool nodal_scalar;                      // the displacement forms take the nodal values of a SCALAR field on a scalar mesh
                                          // (dxm_mesh_create_plane_scalar) in place of a displacement: the law's gradient is that
                                          // field's and its external state variable 0 the field's value at the point
};

// doubles per point of the full tangent layout: the sum of the law's blocks
constexpr int ct_full_of(const LawDesc& d) { return d.ct_full ? d.ct_full : d.n_flux * d.n_grad; }

// ---- parameters: [E, nu, ...] for all laws but Ogden ----
static int elastic_constants(const double* p, LawParams& q) {
  const double E = p[0], nu = p[1];
  if (!(E > 0.0) || !(nu > -1.0 && nu < 0.5)) return fail(-1, "invalid elastic constants E=%g nu=%g", E, nu);
  q.lambda = E * nu / (1 + nu) / (1 - 2 * nu);  // python_materials/elasticity.py:12-13
  q.mu = E / 2 / (1 + nu);
  q.kappa = q.lambda + 2.0 * q.mu / 3.0;
  q.sig0 = 1.0;
  return 0;
}

// residual tolerance of the local Newton: relative to the initial yield stress, floored so that a law with R(0) = 0 keeps a
// reachable tolerance
static void yield_tolerance(LawParams& q) { q.tol = q.rtol * fmax(fabs(q.sig0), 2e-8 * q.mu); }

static int build_elastic(const double* p, LawParams& q) {
  if (int rc = elastic_constants(p, q)) return rc;
  yield_tolerance(q);
  return 0;
}

// [E, nu, sig0, H]
static int build_linear_hardening(const double* p, LawParams& q) {
  if (int rc = elastic_constants(p, q)) return rc;
  q.sig0 = p[2]; q.h1 = p[3];
  yield_tolerance(q);
  return 0;
}

// [E, nu, sig0, sigu, b]; a custom-hardening build: [E, nu, sig0, c0..c5]
static int build_voce_hardening(const double* p, LawParams& q) {
  if (int rc = elastic_constants(p, q)) return rc;
  q.sig0 = p[2];
  if (kCustomBuild) { for (int k = 0; k < 6; ++k) q.c[k] = p[3 + k]; }
  else { q.h1 = p[3]; q.h2 = p[4]; }
  yield_tolerance(q);
  return 0;
}

// [E, nu, sig0, alpha, n]; the local Newton's monotone convergence needs a convex f, i.e. n >= 1
static int build_ramberg_osgood(const double* p, LawParams& q) {
  if (int rc = elastic_constants(p, q)) return rc;
  const double E = p[0], nu = p[1], sig0 = p[2], alpha = p[3], n = p[4];
  if (!(sig0 > 0.0)) return fail(-1, "Ramberg-Osgood: sig0 must be > 0, got %g", sig0);
  if (!(alpha > 0.0)) return fail(-1, "Ramberg-Osgood: alpha must be > 0, got %g", alpha);
  if (!(n >= 1.0) || !std::isfinite(n)) return fail(-1, "Ramberg-Osgood: n must be a finite number >= 1, got %g", n);
  q.sig0 = sig0;
  q.kappa = E / (3.0 * (1.0 - 2.0 * nu));   // the .mfront file's K
  q.c[RO_I3MU] = 1.0 / (3.0 * q.mu);
  q.c[RO_BETA] = alpha * sig0 / E;
  q.c[RO_ISIG0] = 1.0 / sig0;
  q.c[RO_N] = n;
  q.c[RO_INVN] = 1.0 / n;
  q.c[RO_ESIG] = E * RO_EPS;
  q.h1 = 3.0 * q.mu;
  q.h2 = n * q.c[RO_BETA];
  q.tol = q.c[RO_I3MU] * RO_EPS;   // no residual tolerance: the floor of f' (small_strain.hpp)
  return 0;
}

// [alpha, mu, K] (Ogden.mfront); the exponents the kernel needs are formed here once
static int build_ogden(const double* p, LawParams& q) {
  const double alpha = p[0], mu = p[1], K = p[2];
  if (!(alpha != 0.0) || !std::isfinite(alpha)) return fail(-1, "Ogden: alpha must be finite and non-zero, got %g", alpha);
  if (!(mu > 0.0) || !std::isfinite(mu)) return fail(-1, "Ogden: mu must be finite and > 0, got %g", mu);
  if (!(K > 0.0) || !std::isfinite(K)) return fail(-1, "Ogden: K must be finite and > 0, got %g", K);
  const double a = 0.5 * alpha;
  q.mu = mu;
  q.kappa = K;
  q.c[OG_A] = a;
  q.c[OG_AM2] = a - 2.0;
  q.c[OG_MA3] = -a / 3.0;
  q.c[OG_M] = a - 1.0;
  return 0;
}

// [E, nu, R0, H, a]: the exponent's derived constants are formed here once
static int build_hosford(const double* p, LawParams& q) {
  if (int rc = elastic_constants(p, q)) return rc;
  const double R0 = p[2], H = p[3], a = p[4];
  if (!(R0 > 0.0) || !std::isfinite(R0)) return fail(-1, "Hosford: R0 must be finite and > 0, got %g", R0);
  if (!(H >= 0.0) || !std::isfinite(H)) return fail(-1, "Hosford: the hardening slope H must be finite and >= 0, got %g", H);
  if (!(a >= 2.0) || !std::isfinite(a)) return fail(-1, "Hosford: the exponent a must be a finite number >= 2, got %g", a);
  q.sig0 = R0;
  q.h1 = H;
  q.c[HF_A] = a;
  q.c[HF_AM2] = a - 2.0;
  q.c[HF_INVA] = 1.0 / a;
  q.c[HF_AM1] = a - 1.0;
  yield_tolerance(q);
  return 0;
}

// [E1, E2, E3, nu12, nu23, nu13, G12, G23, G13]: the 3x3 normal block of the stiffness is the inverse of the compliance block
// (closed-form adjugate, every operation individually rounded: tests restate it), the shear diagonal is 2 G in Mandel order
static int build_orthotropic(const double* p, LawParams& q) {
#pragma clang fp contract(off)
  static const char* const names[9] = {"E1", "E2", "E3", "nu12", "nu23", "nu13", "G12", "G23", "G13"};
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "orthotropic elasticity: %s must be finite, got %g", names[k], p[k]);
  for (int k : {0, 1, 2, 6, 7, 8})
    if (!(p[k] > 0.0)) return fail(-1, "orthotropic elasticity: %s must be > 0, got %g", names[k], p[k]);
  const double E1 = p[0], E2 = p[1], E3 = p[2], nu12 = p[3], nu23 = p[4], nu13 = p[5], G12 = p[6], G23 = p[7], G13 = p[8];
  const double s11 = 1.0 / E1, s22 = 1.0 / E2, s33 = 1.0 / E3, s12 = -nu12 / E1, s13 = -nu13 / E1, s23 = -nu23 / E2;
  // positive definite: the leading minors, scaled to 1 - nu12^2 E2 / E1 > 0 and det(S) E1 E2 E3 > 0
  const double m2 = 1.0 - nu12 * nu12 * E2 / E1;
  if (!(m2 > 0.0)) return fail(-1, "orthotropic elasticity: the compliance is not positive definite: 1 - nu12^2 E2/E1 = %g (nu12 = %g)", m2, nu12);
  const double c11 = s22 * s33 - s23 * s23, c12 = s13 * s23 - s12 * s33, c13 = s12 * s23 - s13 * s22;
  const double c22 = s11 * s33 - s13 * s13, c23 = s12 * s13 - s11 * s23, c33 = s11 * s22 - s12 * s12;
  const double det = s11 * c11 + s12 * c12 + s13 * c13;
  const double m3 = det * E1 * E2 * E3;
  if (!(m3 > 0.0) || !std::isfinite(m3))
    return fail(-1, "orthotropic elasticity: the compliance is not positive definite: det(S) E1 E2 E3 = %g (nu12 = %g, nu23 = %g, nu13 = %g)", m3, nu12, nu23, nu13);
  OrthoStiffness s{};
  s.c[0] = c11 / det; s.c[1] = s.c[3] = c12 / det; s.c[2] = s.c[6] = c13 / det;
  s.c[4] = c22 / det; s.c[5] = s.c[7] = c23 / det; s.c[8] = c33 / det;
  s.g2[0] = 2.0 * G12; s.g2[1] = 2.0 * G13; s.g2[2] = 2.0 * G23;
  for (double v : s.c)
    if (!std::isfinite(v)) return fail(-1, "orthotropic elasticity: the stiffness is not finite (%g): the compliance is singular to working precision", v);
  ortho_store(q, s);
  return 0;
}

// [E1, E2, E3, nu12, nu23, nu13, G12, G23, G13, n, K, tau0, Q, b, d, C, h_self, h_coplanar, h_Hirth, h_collinear, h_glissile, h_Lomer]:
// the stiffness is the orthotropic law's, in the same twelve doubles; the rest is read from the handle's parameters by the launcher
static int build_single_crystal(const double* p, LawParams& q) {
  static const char* const names[13] = {"n", "K", "tau0", "Q", "b", "d", "C", "h_self", "h_coplanar", "h_Hirth", "h_collinear", "h_glissile", "h_Lomer"};
  for (int k = 9; k < 22; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "single-crystal viscoplasticity: %s must be finite, got %g", names[k - 9], p[k]);
  if (int rc = build_orthotropic(p, q)) return rc;
  if (!(p[9] >= 1.0)) return fail(-1, "single-crystal viscoplasticity: the Norton exponent n must be >= 1, got %g", p[9]);
  if (!(p[10] > 0.0)) return fail(-1, "single-crystal viscoplasticity: K must be > 0, got %g", p[10]);
  if (!(p[11] >= 0.0)) return fail(-1, "single-crystal viscoplasticity: tau0 must be >= 0, got %g", p[11]);
  if (!(p[13] >= 0.0)) return fail(-1, "single-crystal viscoplasticity: b must be >= 0, got %g", p[13]);
  if (!(p[14] >= 0.0)) return fail(-1, "single-crystal viscoplasticity: d must be >= 0, got %g", p[14]);
  if (!(p[15] >= 0.0)) return fail(-1, "single-crystal viscoplasticity: C must be >= 0, got %g", p[15]);
  return 0;
}

// [A, B]: A + B T <= 0 is the caller's business, as it is MFront's
static int build_heat_stationary(const double* p, LawParams&) {
  static const char* const names[2] = {"A", "B"};
  for (int k = 0; k < 2; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "stationary heat transfer: %s must be finite, got %g", names[k], p[k]);
  return 0;
}

// [Tm, ks, cs, kl, cl, dhsl, Tsmooth]; what the kernel reads is formed by the launcher (heat_transfer.hpp: HeatParams)
static int build_heat_phase_change(const double* p, LawParams&) {
  static const char* const names[7] = {"MeltingTemperature", "SolidConductivity", "SolidHeatCapacity", "LiquidConductivity", "LiquidHeatCapacity",
                                       "FusionEnthalpy", "Tsmooth"};
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "heat transfer with phase change: %s must be finite, got %g", names[k], p[k]);
  if (!(p[6] > 0.0)) return fail(-1, "heat transfer with phase change: Tsmooth must be > 0, got %g", p[6]);
  return 0;
}

// [E, nu, s0, H0] (LogarithmicStrainPlasticity.mfront; the file writes E and nu in, the material properties are s0 and H0)
static int build_log_strain(const double* p, LawParams& q) {
  static const char* const names[4] = {"E", "nu", "s0", "H0"};
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "logarithmic-strain plasticity: %s must be finite, got %g", names[k], p[k]);
  if (int rc = elastic_constants(p, q)) return rc;
  if (!(p[2] > 0.0)) return fail(-1, "logarithmic-strain plasticity: s0 must be > 0, got %g", p[2]);
  if (!(p[3] >= 0.0)) return fail(-1, "logarithmic-strain plasticity: the hardening slope H0 must be >= 0, got %g", p[3]);
  q.sig0 = p[2];
  q.h1 = p[3];
  yield_tolerance(q);
  return 0;
}

// [E, nu, G, n, K, tau0, Q, b, d, C, h_self, h_coplanar, h_Hirth, h_collinear, h_glissile, h_Lomer]: the cubic stiffness is the
// orthotropic law's with E1 = E2 = E3 = E, nu12 = nu23 = nu13 = nu, G12 = G23 = G13 = G, in the same twelve doubles; the rest is
// read from the handle's parameters by the launcher
static int build_fs_single_crystal(const double* p, LawParams& q) {
  static const char* const names[16] = {"E", "nu", "G", "n", "K", "tau0", "Q", "b", "d", "C", "h_self", "h_coplanar", "h_Hirth", "h_collinear",
                                        "h_glissile", "h_Lomer"};
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "finite-strain single-crystal viscoplasticity: %s must be finite, got %g", names[k], p[k]);
  if (!(p[0] > 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: E must be > 0, got %g", p[0]);
  if (!(p[1] > -1.0 && p[1] < 0.5)) return fail(-1, "finite-strain single-crystal viscoplasticity: nu must lie in (-1, 0.5), got %g", p[1]);
  if (!(p[2] > 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: G must be > 0, got %g", p[2]);
  if (!(p[3] >= 1.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: the Norton exponent n must be >= 1, got %g", p[3]);
  if (!(p[4] > 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: K must be > 0, got %g", p[4]);
  if (!(p[5] >= 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: tau0 must be >= 0, got %g", p[5]);
  if (!(p[7] >= 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: b must be >= 0, got %g", p[7]);
  if (!(p[8] >= 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: d must be >= 0, got %g", p[8]);
  if (!(p[9] >= 0.0)) return fail(-1, "finite-strain single-crystal viscoplasticity: C must be >= 0, got %g", p[9]);
  const double cubic[9] = {p[0], p[0], p[0], p[1], p[1], p[1], p[2], p[2], p[2]};
  return build_orthotropic(cubic, q);
}

// [E, nu, sig0, q, tangent] (the reference's demos/cvxpy/cvxpy_materials.py:89-93 with q = 1); what the kernel reads is formed by
// the launcher (plane_stress.hpp: PsParams).  nu < 1 suffices in plane stress: C is positive definite for -1 < nu < 1
static int build_ps_quadratic(const double* p, LawParams& q) {
  static const char* const names[5] = {"E", "nu", "sig0", "q", "tangent"};
  for (int k = 0; k < 5; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "plane-stress quadratic yield set: %s must be finite, got %g", names[k], p[k]);
  if (!(p[0] > 0.0)) return fail(-1, "plane-stress quadratic yield set: E must be > 0, got %g", p[0]);
  if (!(p[1] > -1.0 && p[1] < 1.0)) return fail(-1, "plane-stress quadratic yield set: nu must lie in (-1, 1), got %g", p[1]);
  if (!(p[2] > 0.0)) return fail(-1, "plane-stress quadratic yield set: sig0 must be > 0, got %g", p[2]);
  if (!(p[3] > 0.0)) return fail(-1, "plane-stress quadratic yield set: the shear weight q must be > 0, got %g", p[3]);
  if (!(p[4] == 0.0 || p[4] == 1.0))
    return fail(-1, "plane-stress quadratic yield set: tangent must be 0 (the elastic C) or 1 (the algorithmic tangent), got %g", p[4]);
  q.sig0 = p[2];
  q.tol = q.rtol * p[2];   // on sqrt(s^T Q s) - sig0
  return 0;
}

// [E, nu, M, n1_0, n2_0, d_0, ... ] padded to PS_MAX_PLANES rows (the rows past M are not read): half-planes n . (sI, sII) <= d in
// the unordered plane of the principal stresses (cvxpy_materials.py:54-86 for the reference's two)
static int build_ps_polygon(const double* p, LawParams&) {
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "plane-stress polygonal yield set: %s must be finite, got %g", k == 0 ? "E" : (k == 1 ? "nu" : "M"), p[k]);
  if (!(p[0] > 0.0)) return fail(-1, "plane-stress polygonal yield set: E must be > 0, got %g", p[0]);
  if (!(p[1] > -1.0 && p[1] < 1.0)) return fail(-1, "plane-stress polygonal yield set: nu must lie in (-1, 1), got %g", p[1]);
  const int M = (int)p[2];
  if (!(p[2] == (double)M) || M < 1 || M > PS_MAX_PLANES)
    return fail(-1, "plane-stress polygonal yield set: the number of half-planes M must be an integer in [1, %d], got %g", PS_MAX_PLANES, p[2]);
  for (int k = 0; k < M; ++k) {
    const double* r = p + 3 + 3 * k;
    if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]))
      return fail(-1, "plane-stress polygonal yield set: half-plane %d (%g, %g, %g) must be finite", k, r[0], r[1], r[2]);
    if (!(r[2] > 0.0))
      return fail(-1, "plane-stress polygonal yield set: half-plane %d has d = %g: d must be > 0, the origin lies strictly inside the set", k, r[2]);
    if (r[0] == 0.0 && r[1] == 0.0) return fail(-1, "plane-stress polygonal yield set: half-plane %d has a zero normal", k);
  }
  // closed under the exchange of the two principal stresses: the mirror (n2, n1, d) of every row is a row, exactly.  Without it the
  // projection of an ordered trial can leave the set
  for (int k = 0; k < M; ++k) {
    const double* r = p + 3 + 3 * k;
    bool found = false;
    for (int j = 0; j < M; ++j) {
      const double* o = p + 3 + 3 * j;
      found = found || (o[0] == r[1] && o[1] == r[0] && o[2] == r[2]);
    }
    if (!found)
      return fail(-1, "plane-stress polygonal yield set: the half-planes are not symmetric under the exchange of the principal stresses: "
                      "the mirror (%g, %g, %g) of half-plane %d is not in the list", r[1], r[0], r[2], k);
  }
  return 0;
}

// [E, nu, sig0, a, tangent] (the reference's demos/cvxpy/cvxpy_materials.py:96-110); what the kernel reads is formed by the launcher
// (plane_stress_hosford.hpp: PshParams).  The exponent's range is PSH_A_MIN .. PSH_A_MAX there
static int build_ps_hosford(const double* p, LawParams& q) {
  static const char* const names[5] = {"E", "nu", "sig0", "a", "tangent"};
  for (int k = 0; k < 5; ++k)
    if (!std::isfinite(p[k])) return fail(-1, "plane-stress Hosford plasticity: %s must be finite, got %g", names[k], p[k]);
  if (!(p[0] > 0.0)) return fail(-1, "plane-stress Hosford plasticity: E must be > 0, got %g", p[0]);
  if (!(p[1] > -1.0 && p[1] < 1.0)) return fail(-1, "plane-stress Hosford plasticity: nu must lie in (-1, 1), got %g", p[1]);
  if (!(p[2] > 0.0)) return fail(-1, "plane-stress Hosford plasticity: sig0 must be > 0, got %g", p[2]);
  if (!(p[3] >= PSH_A_MIN))
    return fail(-1, "plane-stress Hosford plasticity: the exponent a must be >= 2 (below 2 the Hessian of the yield function is unbounded "
                    "on the axes), got %g", p[3]);
  if (!(p[3] <= PSH_A_MAX))
    return fail(-1, "plane-stress Hosford plasticity: the exponent a must be <= 100 (the largest exponent at which the accuracy was "
                    "measured), got %g", p[3]);
  if (!(p[4] == 0.0 || p[4] == 1.0))
    return fail(-1, "plane-stress Hosford plasticity: tangent must be 0 (the elastic C) or 1 (the algorithmic tangent), got %g", p[4]);
  q.sig0 = p[2];
  q.tol = fmax(q.rtol, 0x1p-49);   // on the last step of the angle, in radians
  return 0;
}

// ---- launchers (defined in the launch section, where the handle is complete) ----
template <int LAW> static void launch_small_strain(const LaunchArgs& a);
static void launch_fefp_voce(const LaunchArgs& a);
static void launch_fefp_linear(const LaunchArgs& a);
static void launch_ramberg_osgood(const LaunchArgs& a);
static void launch_ogden(const LaunchArgs& a);
static void launch_hosford(const LaunchArgs& a);
static void launch_orthotropic(const LaunchArgs& a);
static void launch_single_crystal(const LaunchArgs& a);
static void launch_heat_stationary(const LaunchArgs& a);
static void launch_heat_phase_change(const LaunchArgs& a);
static void launch_heat_stationary_2d(const LaunchArgs& a);
static void launch_heat_phase_change_2d(const LaunchArgs& a);
static void launch_log_strain(const LaunchArgs& a);
static void launch_fs_single_crystal(const LaunchArgs& a);
static void launch_ps_quadratic(const LaunchArgs& a);
static void launch_ps_polygon(const LaunchArgs& a);
template <int LAW> static void launch_plane_strain(const LaunchArgs& a);
template <int HARD> static void launch_plane_stress_j2(const LaunchArgs& a);
static void launch_ps_hosford(const LaunchArgs& a);
static void launch_ogden_pe(const LaunchArgs& a);
static void launch_pe_hosford(const LaunchArgs& a);
static void launch_log_strain_pe(const LaunchArgs& a);

// The device assembly of this file lists its kernels in the order in which host code first names them, and
// tests/test_hosford_build.py pins the digest of that assembly.  These five were first named by dxm_create in this order, which is
// not the order of the rows below (the Voce FeFp law has the lower id): naming them here, ahead of the table, keeps the order.
[[maybe_unused]] static const void* const kKernelOrder[5] = {
    (const void*)small_strain_kernel<LAW_ELASTIC, TL_FULL>, (const void*)small_strain_kernel<LAW_J2_LINEAR, TL_FULL>,
    (const void*)small_strain_kernel<LAW_J2_VOCE, TL_FULL>, (const void*)fefp_kernel<0, 0>, (const void*)fefp_kernel<1, 0>};

// ---- the rows ----
// Grid size, in workgroups per CU (blocks_per_cu).  FeFp: the workgroups that are resident at once (persistent
// grid).  Small strain: 32 = 8 x the resident 4: a grid of exactly-resident workgroups starts all
// waves together and keeps them in lockstep (everybody loads, then everybody stores); workgroups
// that are dispatched as others retire spread those phases, 3-6 % faster at 1e7 points in the fast
// placement mode and 10 % in the slow one (tools/grid_sweep.py, profiles/archive/r01_grid_sweep.jsonl).
// The laws with a local Newton iteration (Voce or traced hardening, FeFp) do a point-dependent amount of work per tile: a
// grid of one workgroup per 256 points (up to 256 per CU, the cap; a grid-stride loop beyond) lets the dispatcher balance
// it -- Voce +3 %, FeFp +2.5 % over the persistent grids above at 1e7 points (profiles/archive/r03_grid_size_by_law.txt); the
// linear-hardening kernel, whose tiles all cost the same, loses 2.5 % with it and keeps 32.

// what every isotropic law answers dxm_set_frame* with
constexpr const char* kNoFrame = "this law is isotropic: a material frame changes nothing in its update, and accepting one would hide a "
                                 "mistake of the caller (frames are read by DXM_LAW_ORTHOTROPIC_ELASTIC and DXM_LAW_SINGLE_CRYSTAL_FCC)";

constexpr void state_field(LawDesc& d, int f, const char* name, int dim, int slot) {
  d.isv_name[f] = name; d.isv_dim[f] = dim; d.isv_slot[f] = slot;
}

// what the small-strain laws of small_strain.hpp share; `coef`: the tangent is c1 1x1 + c2 I + c3 n x n with per-point coefficients
constexpr LawDesc small_strain_law(int id, int n_params, int alg_bytes, const char* kernel, bool coef, void (*launch)(const LaunchArgs&)) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = 6;
  d.n_params = d.n_params_custom = n_params;
  d.alg_bytes = alg_bytes;
  d.kernel = kernel;
  d.set_layouts = d.launch_layouts = coef ? L_ALL : L_FULL | L_SYM;
  d.no_frame = kNoFrame;
  d.launch = launch;
  return d;
}

constexpr void j2_state(LawDesc& d) {
  d.n_isv_fields = d.n_fields = 2;
  state_field(d, 0, "p", 1, 0);
  state_field(d, 1, "epsp", 6, 1);
  d.n_slots = SS_NSLOTS;
}

constexpr LawDesc law_elastic() {
  LawDesc d = small_strain_law(DXM_LAW_ELASTIC_ISO, 2, 384, "small_strain_kernel<0", false, launch_small_strain<LAW_ELASTIC>);
  d.build = build_elastic;
  d.residency_kernel = []() -> const void* { return (const void*)small_strain_kernel<LAW_ELASTIC, TL_FULL>; };
  d.blocks_per_cu = 32;
  d.set_refusal = d.launch_refusal = "the elastic tangent is the constant lambda 1x1 + 2 mu I: there are no per-point coefficients";
  d.no_fields = "the elastic tangent is a constant the host path never downloads";
  return d;
}

constexpr LawDesc law_j2_linear() {
  LawDesc d = small_strain_law(DXM_LAW_J2_LINEAR, 4, 496, "small_strain_kernel<1", true, launch_small_strain<LAW_J2_LINEAR>);
  j2_state(d);
  d.build = build_linear_hardening;
  d.residency_kernel = []() -> const void* { return (const void*)small_strain_kernel<LAW_J2_LINEAR, TL_FULL>; };
  d.blocks_per_cu = 32;
  d.field_kernel = "small_strain_field_kernel<1";
  return d;
}

constexpr LawDesc law_j2_voce() {
  LawDesc d = small_strain_law(DXM_LAW_J2_VOCE, 5, 496, "small_strain_kernel<2", true, launch_small_strain<LAW_J2_VOCE>);
  j2_state(d);
  d.n_params_custom = 9;
  d.build = build_voce_hardening;
  d.residency_kernel = []() -> const void* { return (const void*)small_strain_kernel<LAW_J2_VOCE, TL_FULL>; };
  d.blocks_per_cu = 256;
  d.field_kernel = "small_strain_field_kernel<2";
  return d;
}

// stateless: the elastic law's stream (48 B in, 48 + 288 B out), with per-point tangent coefficients like J2
constexpr LawDesc law_ramberg_osgood() {
  // ramberg_osgood.hip holds the kernels
  LawDesc d = small_strain_law(DXM_LAW_RAMBERG_OSGOOD, 5, 384, "small_strain_kernel<3", true, DXM_STOCK_ONLY(launch_ramberg_osgood));
  d.build = build_ramberg_osgood;
  d.stock_only = "Ramberg-Osgood has no hardening law: it is served by the stock libdxmat, not by a custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(ramberg_osgood_kernel);
  d.blocks_per_cu = RO_BLOCKS_PER_CU;   // DESIGN.md section "Ramberg-Osgood"
  d.no_fields = "Ramberg-Osgood precomputes per-handle Newton constants on the host";
  return d;
}

// F -> PK1.  A launch may also ask for TL_COEF: the 54 building blocks of the tangent per point instead of its 81 entries, which
// the host-buffer form expands; no handle can be set to it
constexpr LawDesc law_fefp(int id, bool voce) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = 9;
  d.n_params = voce ? 5 : 4;
  d.n_params_custom = voce ? 9 : 4;
  d.n_isv_fields = 2;
  d.n_fields = 3;   // field 2 is hidden state: the isochoric inverse plastic right Cauchy-Green tensor
  state_field(d, 0, "p", 1, FEFP_SLOT_P);
  state_field(d, 1, "be_bar", 6, FEFP_SLOT_BE);
  state_field(d, 2, "cp_bar_inv", 6, FEFP_SLOT_CPI);
  d.n_slots = FEFP_NSLOTS;
  // be_bar = Cp^-1 = identity: unstressed natural configuration
  // (demos/jax/finite_strain_elastoplasticity/finite_strain_elastoplasticity.py:181)
  d.unit_fields = 1u << 1 | 1u << 2;
  d.alg_bytes = 976;
  d.kernel = voce ? "fefp_kernel<1" : "fefp_kernel<0";
  d.no_fields = "the FeFp kernels have no registers to spare";
  d.build = voce ? build_voce_hardening : build_linear_hardening;
  if (voce) d.residency_kernel = []() -> const void* { return (const void*)fefp_kernel<1, 0>; };
  else d.residency_kernel = []() -> const void* { return (const void*)fefp_kernel<0, 0>; };
  d.blocks_per_cu = 256;
  d.set_layouts = L_FULL;
  d.launch_layouts = L_FULL | L_COEF;
  d.set_refusal = d.launch_refusal = "the FeFp tangent dP/dF is not symmetric: only DXM_TANGENT_FULL is available";
  d.no_frame = kNoFrame;
  d.launch = voce ? launch_fefp_voce : launch_fefp_linear;
  return d;
}

// Ogden: F in (72 B), PK1 (72) + dP/dF (648) + the isochoric PK2 stress (48) out; the state is written, never read
constexpr LawDesc law_ogden() {
  LawDesc d{};
  d.id = DXM_LAW_OGDEN;
  d.n_grad = d.n_flux = 9;
  d.n_params = d.n_params_custom = 3;
  d.n_isv_fields = d.n_fields = 1;
  state_field(d, 0, "PK2Stress", 6, 0);
  d.n_slots = OGDEN_NSLOTS;
  d.alg_bytes = 840;
  d.kernel = "ogden_kernel";
  d.no_fields = "the Ogden kernel takes its exponents as per-handle constants";
  d.build = build_ogden;
  d.stock_only = "Ogden hyperelasticity has no hardening law: it is served by the stock libdxmat, not by a custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(ogden_kernel_fn);
  d.blocks_per_cu = OGDEN_BLOCKS_PER_CU;   // hyperelastic.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = "the Ogden kernel writes the full 81-entry dP/dF only: no packed tangent record (sym / coef / pack4) exists for this law";
  d.launch_refusal = "the Ogden kernel writes the full 81-entry dP/dF only: no packed tangent record exists for this law";
  d.no_fused = "the Ogden kernel has no fused displacement-gradient form: set option fused_gradient to 0 (F is then evaluated "
               "by the gradient kernel) or pass F as an array";
  d.no_frame = kNoFrame;
  d.launch = DXM_STOCK_ONLY(launch_ogden);   // hyperelastic.hip: F from the (N, 9) array, the full tangent
  return d;
}

// Hosford: strain in (48 B), stress (48) + tangent (288) out; reads p and the hidden plastic strain (56), writes them and the
// elastic strain (104)
constexpr LawDesc law_hosford() {
  LawDesc d{};
  d.id = DXM_LAW_HOSFORD_LINEAR;
  d.n_grad = d.n_flux = 6;
  d.n_params = d.n_params_custom = 5;
  d.n_isv_fields = 2;
  d.n_fields = 3;   // field 2 is hidden state: what the update is driven by (hosford.hpp)
  state_field(d, 0, "ElasticStrain", 6, HF_SLOT_EEL);
  state_field(d, 1, "EquivalentPlasticStrain", 1, HF_SLOT_P);
  state_field(d, 2, "PlasticStrain", 6, HF_SLOT_EP);
  d.n_slots = HF_NSLOTS;
  d.alg_bytes = 544;
  d.kernel = "hosford_kernel";
  d.no_fields = "the Hosford kernel takes its exponent's constants per handle";
  d.build = build_hosford;
  d.stock_only = "Hosford plasticity takes linear hardening only: it is served by the stock libdxmat, not by a custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(hosford_kernel_fn);
  d.blocks_per_cu = HF_BLOCKS_PER_CU;   // hosford.hpp
  d.set_layouts = d.launch_layouts = L_FULL | L_SYM;
  d.set_refusal = "the Hosford tangent is a general symmetric 6x6, not of the form c1 1x1 + c2 I + c3 n x n: there are no coefficients "
                  "(coef / pack4); DXM_TANGENT_FULL and DXM_TANGENT_SYM are available";
  d.launch_refusal = "the Hosford tangent is a general symmetric 6x6: no coefficient record (coef / pack4) exists for this law";
  d.no_fused = "the Hosford kernel has no fused displacement-gradient form: set option fused_gradient to 0 (the strain is then "
               "evaluated by the gradient kernel) or pass the strain as an array";
  d.no_frame = kNoFrame;
  d.launch = DXM_STOCK_ONLY(launch_hosford);   // hosford.hip: strain from the (N, 6) array, the full block or its upper triangle
  return d;
}

// Orthotropic elasticity: strain in (48 B), stress (48) + tangent (288) out, no state; a frame field adds nine 8 B streams
// (dxm_algorithmic_bytes)
constexpr LawDesc law_orthotropic() {
  LawDesc d{};
  d.id = DXM_LAW_ORTHOTROPIC_ELASTIC;
  d.n_grad = d.n_flux = 6;
  d.n_params = d.n_params_custom = 9;
  d.alg_bytes = 384;
  d.kernel = "orthotropic_kernel<0";
  d.frame_kernel[0] = "orthotropic_kernel<1";
  d.frame_kernel[1] = "orthotropic_kernel<2";
  d.no_fields = "per-point stiffness fields are not served for orthotropic elasticity: the host inverts the compliance once per handle";
  d.build = build_orthotropic;
  d.stock_only = "orthotropic elasticity has no hardening law: it is served by the stock libdxmat, not by a custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(orthotropic_kernel_fn);
  d.blocks_per_cu = OR_BLOCKS_PER_CU;   // orthotropic.hpp
  d.set_layouts = d.launch_layouts = L_FULL | L_SYM;
  d.set_refusal = "the orthotropic tangent Q^T C Q is a general symmetric 6x6, not of the form c1 1x1 + c2 I + c3 n x n: there are no "
                  "coefficients (coef / pack4); DXM_TANGENT_FULL and DXM_TANGENT_SYM are available";
  d.launch_refusal = "the orthotropic tangent is a general symmetric 6x6: no coefficient record (coef / pack4) exists for this law";
  d.no_fused = "the orthotropic kernel has no fused displacement-gradient form: set option fused_gradient to 0 (the strain is then "
               "evaluated by the gradient kernel) or pass the strain as an array";
  d.launch = DXM_STOCK_ONLY(launch_orthotropic);   // orthotropic.hip: strain from the (N, 6) array, the handle's frame
  return d;
}

// FCC single-crystal viscoplasticity: strain in (48 B) and slips, cumulated slips, back strains read (288); stress (48), the
// non-symmetric tangent (288) and the four state fields (336) out: 1008 B/point, plus nine 8 B streams with a frame field
constexpr LawDesc law_single_crystal() {
  LawDesc d{};
  d.id = DXM_LAW_SINGLE_CRYSTAL_FCC;
  d.n_grad = d.n_flux = 6;
  d.n_params = d.n_params_custom = 22;
  d.n_isv_fields = d.n_fields = 4;
  state_field(d, 0, "ElasticStrain", 6, SC_SLOT_EEL);
  state_field(d, 1, "ViscoplasticSlip", 12, SC_SLOT_G);
  state_field(d, 2, "EquivalentViscoplasticSlip", 12, SC_SLOT_P);
  state_field(d, 3, "BackStrain", 12, SC_SLOT_A);
  d.n_slots = SC_NSLOTS;
  d.alg_bytes = 1008;
  d.kernel = "single_crystal_kernel<0";
  d.frame_kernel[0] = "single_crystal_kernel<1";
  d.frame_kernel[1] = "single_crystal_kernel<2";
  d.no_fields = "per-point parameter fields are not served for single-crystal viscoplasticity: its constants are formed once per handle";
  d.build = build_single_crystal;
  d.stock_only = "single-crystal viscoplasticity has no isotropic hardening law to replace: it is served by the stock libdxmat, not by a "
                 "custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(single_crystal_kernel_fn);
  d.blocks_per_cu = SC_BLOCKS_PER_CU;   // single_crystal.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = "the single-crystal tangent is not symmetric (interaction hardening): only DXM_TANGENT_FULL is available, no packed "
                  "record (sym / coef / pack4) exists for this law";
  d.launch_refusal = "the single-crystal tangent is not symmetric: only the full 36-entry block exists for this law";
  d.no_fused = "the single-crystal kernel has no fused displacement-gradient form: set option fused_gradient to 0 (the strain is then "
               "evaluated by the gradient kernel) or pass the strain as an array";
  d.launch = DXM_STOCK_ONLY(launch_single_crystal);   // single_crystal.hip: strain from the (N, 6) array, the handle's frame, dt
  d.rate_dependent = true;
  return d;
}

constexpr dxm_tangent_block tangent_block(int row_kind, int row_index, int col_kind, int col_index, int rows, int cols) {
  return dxm_tangent_block{row_kind, row_index, col_kind, col_index, rows, cols};
}

// The two heat-transfer laws (heat_transfer.hip): temperature gradient in (24 B), heat flux (24) and the blocks of the tangent out;
// the temperature is an external state variable, a kernel argument or one more 8 B stream (dxm_algorithmic_bytes)
constexpr LawDesc heat_law(int id, int n_params, const char* kernel) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = 3;
  d.n_params = d.n_params_custom = n_params;
  d.kernel = kernel;
  d.n_ext = 1;
  d.ext_name[0] = "Temperature";
  d.ext_default[0] = 293.15;   // mfront.py:109-110
  d.blocks[0] = tangent_block(DXM_BLOCK_ROW_FLUX, 0, DXM_BLOCK_COL_GRADIENT, 0, 3, 3);
  d.blocks[1] = tangent_block(DXM_BLOCK_ROW_FLUX, 0, DXM_BLOCK_COL_EXTERNAL, 0, 3, 1);
  d.n_blocks = 2;
  d.ct_full = 12;
  d.blocks_per_cu = HT_BLOCKS_PER_CU;   // heat_transfer.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  return d;
}

// counted as 120 B/point: temperature gradient in (24) and tangent out (96); with the flux (24) the kernel moves 144
constexpr LawDesc law_heat_stationary() {
  LawDesc d = heat_law(DXM_LAW_HEAT_STATIONARY, 2, "heat_transfer_kernel<0, 0");
  d.alg_bytes = 120;
  d.ext_kernel = "heat_transfer_kernel<0, 1";
  d.build = build_heat_stationary;
  d.residency_kernel = DXM_STOCK_ONLY(heat_stationary_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_heat_stationary);
  d.no_fields = "per-point parameter fields are not served for stationary heat transfer: A and B are per-handle constants (the "
                "temperature is an external state variable: dxm_set_external_state)";
  d.stock_only = "stationary heat transfer has no hardening law: it is served by the stock libdxmat, not by a custom-hardening build";
  // (one sentence: the host path asks these laws for no other layout than the handle's, so a launch never meets the second check)
  d.set_refusal = d.launch_refusal = "the stationary heat-transfer tangent is two blocks of 9 + 3 entries, not a symmetric 6x6: only "
                                     "DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "stationary heat transfer takes a temperature gradient, not a strain or a deformation gradient: the "
                                   "displacement forms (dxm_integrate_displacement*) do not apply; pass grad(T) as an array";
  d.no_frame = "stationary heat transfer is isotropic (a scalar conductivity): a material frame changes nothing in its update";
  return d;
}

// counted as 136 B/point: gradient in (24), tangent (104) and enthalpy (8) out; with the flux (24) the kernel moves 160.  The
// enthalpy is written, never read
constexpr LawDesc law_heat_phase_change() {
  LawDesc d = heat_law(DXM_LAW_HEAT_PHASE_CHANGE, 7, "heat_transfer_kernel<1, 0");
  d.alg_bytes = 136;
  d.ext_kernel = "heat_transfer_kernel<1, 1";
  d.n_isv_fields = d.n_fields = 1;
  state_field(d, 0, "Enthalpy", 1, 0);
  d.n_slots = 1;
  d.blocks[2] = tangent_block(DXM_BLOCK_ROW_STATE, 0, DXM_BLOCK_COL_EXTERNAL, 0, 1, 1);
  d.n_blocks = 3;
  d.ct_full = 13;
  d.build = build_heat_phase_change;
  d.residency_kernel = DXM_STOCK_ONLY(heat_phase_change_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_heat_phase_change);
  d.no_fields = "per-point parameter fields are not served for heat transfer with phase change: its constants are formed once per "
                "handle (the temperature is an external state variable: dxm_set_external_state)";
  d.stock_only = "heat transfer with phase change has no hardening law: it is served by the stock libdxmat, not by a custom-hardening build";
  d.set_refusal = d.launch_refusal = "the phase-change tangent is three blocks of 9 + 3 + 1 entries, not a symmetric 6x6: only "
                                     "DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "heat transfer with phase change takes a temperature gradient, not a strain or a deformation gradient: "
                                   "the displacement forms (dxm_integrate_displacement*) do not apply; pass grad(T) as an array";
  d.no_frame = "heat transfer with phase change is isotropic (a scalar conductivity): a material frame changes nothing in its update";
  return d;
}

// Logarithmic-strain J2: F in (72 B), PK1 (72) + dP/dF (648) out; reads p and the hidden logarithmic plastic strain (56), writes
// them and the elastic strain (104)
constexpr LawDesc law_log_strain_j2() {
  LawDesc d{};
  d.id = DXM_LAW_LOG_STRAIN_J2;
  d.n_grad = d.n_flux = 9;
  d.n_params = d.n_params_custom = 4;
  d.n_isv_fields = 2;
  d.n_fields = 3;   // field 2 is hidden state: what the update is driven by (log_strain.hpp)
  state_field(d, 0, "ElasticStrain", 6, LS_SLOT_EEL);
  state_field(d, 1, "EquivalentPlasticStrain", 1, LS_SLOT_P);
  state_field(d, 2, "PlasticStrain", 6, LS_SLOT_EP);
  d.n_slots = LS_NSLOTS;
  d.alg_bytes = 952;
  d.kernel = "log_strain_kernel";
  d.no_fields = "the logarithmic-strain plasticity kernel takes its constants per handle";
  d.build = build_log_strain;
  d.stock_only = "logarithmic-strain plasticity takes linear hardening only: it is served by the stock libdxmat, not by a custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(log_strain_kernel_fn);
  d.blocks_per_cu = LS_BLOCKS_PER_CU;   // log_strain.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = "the logarithmic-strain plasticity kernel writes the full 81-entry dP/dF only: no packed tangent record (sym / coef / pack4) "
                  "exists for this law";
  d.launch_refusal = "the logarithmic-strain plasticity kernel writes the full 81-entry dP/dF only: no packed tangent record exists for this law";
  d.no_fused = "the logarithmic-strain plasticity kernel has no fused displacement-gradient form: set option fused_gradient to 0 (F is "
               "then evaluated by the gradient kernel) or pass F as an array";
  d.no_frame = kNoFrame;
  d.launch = DXM_STOCK_ONLY(launch_log_strain);   // log_strain.hip: F from the (N, 9) array, the full tangent
  return d;
}

// Finite-strain FCC single-crystal viscoplasticity: F in (72 B) and the four state fields read (360); PK1 (72), dP/dF (648) and the
// four state fields (360) out: 1512 B/point, plus nine 8 B streams with a frame field.  A yielded point reads its cumulated slips
// and back strains a second time in its Newton round (192 B, cache hits: not counted)
constexpr LawDesc law_fs_single_crystal() {
  LawDesc d{};
  d.id = DXM_LAW_FS_SINGLE_CRYSTAL_FCC;
  d.n_grad = d.n_flux = 9;
  d.n_params = d.n_params_custom = 16;
  d.n_isv_fields = d.n_fields = 4;
  state_field(d, 0, "PlasticSlip", 12, FX_SLOT_G);
  state_field(d, 1, "EquivalentViscoplasticSlip", 12, FX_SLOT_P);
  state_field(d, 2, "BackStrain", 12, FX_SLOT_A);
  state_field(d, 3, "PlasticPartOfTheDeformationGradient", 9, FX_SLOT_FP);
  d.unit_fields = 1u << 3;   // the 9-vector starts with the diagonal: the three slots init_state fills
  d.n_slots = FX_NSLOTS;
  d.alg_bytes = 1512;
  d.kernel = "fs_single_crystal_kernel<0";
  d.frame_kernel[0] = "fs_single_crystal_kernel<1";
  d.frame_kernel[1] = "fs_single_crystal_kernel<2";
  d.no_fields = "per-point parameter fields are not served for finite-strain single-crystal viscoplasticity: its constants are formed "
                "once per handle";
  d.build = build_fs_single_crystal;
  d.stock_only = "finite-strain single-crystal viscoplasticity has no isotropic hardening law to replace: it is served by the stock "
                 "libdxmat, not by a custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(fs_single_crystal_kernel_fn);
  d.blocks_per_cu = FX_BLOCKS_PER_CU;   // fs_single_crystal.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = "the finite-strain single-crystal tangent dP/dF is 81 independent numbers: only DXM_TANGENT_FULL is available, no packed "
                  "record (sym / coef / pack4) exists for this law";
  d.launch_refusal = "the finite-strain single-crystal tangent is 81 independent numbers: only the full block exists for this law";
  d.no_fused = d.no_displacement = "the finite-strain single-crystal kernel takes F as an array: the displacement forms "
                                   "(dxm_integrate_displacement*) and the fused displacement gradient are not served for this law";
  d.launch = DXM_STOCK_ONLY(launch_fs_single_crystal);   // fs_single_crystal.hip: F from the (N, 9) array, the handle's frame, dt
  d.rate_dependent = true;
  return d;
}

// The two plane-stress return mappings (plane_stress.hip): strain in (24 B) and the hidden plastic strain read (24); stress (24),
// the 3x3 tangent (72) and the plastic strain (24) out: 168 B/point.  Strain and stress are 3 wide: on a mesh that is not
// two-dimensional the refusals of the fused and displacement forms are what keeps a 6-wide mesh gradient away from these rows; a
// two-dimensional mesh is asked for plane_kind (the in-plane 3-vector of plane_gradient.hip) and the update kernel runs after it
constexpr LawDesc plane_stress_law(int id, int n_params, const char* kernel) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = 3;
  d.n_params = d.n_params_custom = n_params;
  d.n_isv_fields = 0;
  d.n_fields = 1;   // field 0 is hidden state: what the update is driven by (plane_stress.hpp)
  state_field(d, 0, "PlasticStrain", 3, 0);
  d.n_slots = PS_NSLOTS;
  d.alg_bytes = 168;
  d.kernel = kernel;
  d.blocks_per_cu = PS_BLOCKS_PER_CU;   // plane_stress.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.plane_kind = GRAD_IN_PLANE3;
  return d;
}

constexpr LawDesc law_ps_quadratic() {
  LawDesc d = plane_stress_law(DXM_LAW_PS_QUADRATIC, 5, "plane_stress_kernel<0");
  d.build = build_ps_quadratic;
  d.residency_kernel = DXM_STOCK_ONLY(plane_stress_quadratic_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_ps_quadratic);
  d.no_fields = "per-point parameter fields are not served for the plane-stress quadratic yield set: its constants are formed once per handle";
  d.stock_only = "the plane-stress quadratic yield set is perfectly plastic, it has no hardening law: it is served by the stock libdxmat, "
                 "not by a custom-hardening build";
  d.set_refusal = d.launch_refusal = "the plane-stress tangent is a 3x3 block of 9 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is "
                                     "available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "the plane-stress quadratic yield set takes a 3-wide strain [xx, yy, sqrt(2) xy]: the mesh gradient "
                                   "kernels evaluate 6-wide strains or F, so the displacement forms (dxm_integrate_displacement*) and the "
                                   "fused displacement gradient are not served on a mesh that is not two-dimensional; pass the strain as an array";
  d.no_frame = "the plane-stress quadratic yield set is isotropic: a material frame changes nothing in its update";
  return d;
}

constexpr LawDesc law_ps_polygon() {
  LawDesc d = plane_stress_law(DXM_LAW_PS_POLYGON, 3 + 3 * PS_MAX_PLANES, "plane_stress_kernel<1");
  d.build = build_ps_polygon;
  d.residency_kernel = DXM_STOCK_ONLY(plane_stress_polygon_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_ps_polygon);
  d.no_fields = "per-point parameter fields are not served for the plane-stress polygonal yield set: its half-planes and vertices are "
                "formed once per handle";
  d.stock_only = "the plane-stress polygonal yield set is perfectly plastic, it has no hardening law: it is served by the stock libdxmat, "
                 "not by a custom-hardening build";
  d.set_refusal = d.launch_refusal = "the plane-stress tangent is a 3x3 block of 9 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is "
                                     "available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "the plane-stress polygonal yield set takes a 3-wide strain [xx, yy, sqrt(2) xy]: the mesh gradient "
                                   "kernels evaluate 6-wide strains or F, so the displacement forms (dxm_integrate_displacement*) and the "
                                   "fused displacement gradient are not served on a mesh that is not two-dimensional; pass the strain as an array";
  d.no_frame = "the plane-stress polygonal yield set is a function of the principal stresses: a material frame changes nothing in its update";
  return d;
}

// The plane-strain forms of laws 0 / 1 / 2 (plane_strain.hip): strain in (32 B), stress (32) and the 4x4 tangent (128) out: 192
// B/point; the J2 laws read and write p and the 4-wide plastic strain (40 + 40): 272.  Strain and stress are 4 wide: on a mesh that is
// not two-dimensional the refusals of the fused and displacement forms are what keeps a 6-wide mesh gradient away from these rows; a
// two-dimensional mesh is asked for plane_kind (the 4-vector of plane_gradient.hip) and the update kernel runs after it.
// Grid: 128 workgroups per CU for the elastic and the linear-hardening law, 256 for Voce, from two sweeps at 1e7 points
// (plane_strain.hpp, profiles/r21_plane_strain.md); every other size is UNMEASURED for these kernels
constexpr LawDesc plane_strain_law(int id, int n_params, int alg_bytes, const char* kernel) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = PE_DIM;
  d.n_params = d.n_params_custom = n_params;
  d.alg_bytes = alg_bytes;
  d.kernel = kernel;
  d.blocks_per_cu = PE_BLOCKS_PER_CU;   // plane_strain.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = d.launch_refusal = "the plane-strain tangent is a 4x4 block of 16 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is "
                                     "available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fields = "per-point parameter fields are not served under the plane-strain hypothesis: the field kernels are the 6-wide "
                "DXM_LAW_J2_LINEAR and DXM_LAW_J2_VOCE (embed the strain as [xx, yy, zz, xy, 0, 0] to use them)";
  d.no_fused = d.no_displacement = "the plane-strain laws take a 4-wide strain [xx, yy, zz, sqrt(2) xy]: the mesh gradient kernels "
                                   "evaluate 6-wide strains or F, so the displacement forms (dxm_integrate_displacement*) and the "
                                   "fused displacement gradient are not served on a mesh that is not two-dimensional; pass the strain as an array";
  d.plane_kind = GRAD_PLANE_STRAIN4;
  d.no_frame = kNoFrame;
  d.stock_only = "the plane-strain laws take the stock hardening laws only (linear, Voce): they are served by the stock libdxmat, not by "
                 "a custom-hardening build";
  return d;
}

constexpr void pe_j2_state(LawDesc& d) {
  d.n_isv_fields = d.n_fields = 2;
  state_field(d, 0, "p", 1, 0);
  state_field(d, 1, "epsp", PE_DIM, 1);
  d.n_slots = PE_NSLOTS;
}

constexpr LawDesc law_pe_elastic() {
  LawDesc d = plane_strain_law(DXM_LAW_PE_ELASTIC_ISO, 2, 192, "plane_strain_kernel<0");
  d.build = build_elastic;
  d.residency_kernel = DXM_STOCK_ONLY(plane_strain_elastic_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_plane_strain<PE_ELASTIC>);
  return d;
}

constexpr LawDesc law_pe_j2_linear() {
  LawDesc d = plane_strain_law(DXM_LAW_PE_J2_LINEAR, 4, 272, "plane_strain_kernel<1");
  pe_j2_state(d);
  d.build = build_linear_hardening;
  d.residency_kernel = DXM_STOCK_ONLY(plane_strain_j2_linear_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_plane_strain<PE_J2_LINEAR>);
  return d;
}

constexpr LawDesc law_pe_j2_voce() {
  LawDesc d = plane_strain_law(DXM_LAW_PE_J2_VOCE, 5, 272, "plane_strain_kernel<2");
  pe_j2_state(d);
  d.build = build_voce_hardening;
  d.residency_kernel = DXM_STOCK_ONLY(plane_strain_j2_voce_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_plane_strain<PE_J2_VOCE>);
  d.blocks_per_cu = PE_BLOCKS_PER_CU_VOCE;   // plane_strain.hpp
  return d;
}

// Plane-stress J2 plasticity with linear or Voce hardening (plane_stress_j2.hip): laws 1 / 2 under sig_zz = 0 in the three components
// [xx, yy, sqrt(2) xy] of laws 23 / 24.  Strain in (24 B), p and the in-plane plastic strain read (32); stress (24), the 3x3 tangent
// (72) and the state (32) out: 184 B/point.  The parameters are those of laws 1 / 2 and go through their build functions.  Strain and
// stress are 3 wide: the refusals of the fused and displacement forms govern the meshes that are not two-dimensional, plane_kind the
// two-dimensional ones (see the rows of laws 23 / 24).  No external state variable is declared (n_ext = 0):
// dxm_set_external_state* answers with the library's sentence for every law without one
constexpr LawDesc plane_stress_j2_law(int id, int n_params, const char* kernel) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = 3;
  d.n_params = d.n_params_custom = n_params;
  d.n_isv_fields = d.n_fields = 2;
  state_field(d, 0, "p", 1, 0);
  state_field(d, 1, "epsp", 3, 1);
  d.n_slots = PSJ_NSLOTS;
  d.alg_bytes = 184;
  d.kernel = kernel;
  d.blocks_per_cu = PSJ_BLOCKS_PER_CU;   // plane_stress_j2.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = d.launch_refusal = "the plane-stress tangent is a 3x3 block of 9 entries, not a symmetric 6x6: only DXM_TANGENT_FULL is "
                                     "available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fields = "per-point parameter fields are not served for plane-stress J2 plasticity: the field kernels are the 6-wide "
                "DXM_LAW_J2_LINEAR and DXM_LAW_J2_VOCE, and the plane-stress constants are formed once per handle";
  d.no_fused = d.no_displacement = "plane-stress J2 plasticity takes a 3-wide strain [xx, yy, sqrt(2) xy]: the mesh gradient kernels "
                                   "evaluate 6-wide strains or F, so the displacement forms (dxm_integrate_displacement*) and the "
                                   "fused displacement gradient are not served on a mesh that is not two-dimensional; pass the strain as an array";
  d.plane_kind = GRAD_IN_PLANE3;
  d.no_frame = kNoFrame;
  d.stock_only = "plane-stress J2 plasticity takes the stock hardening laws only (linear, Voce): it is served by the stock libdxmat, not "
                 "by a custom-hardening build";
  return d;
}

constexpr LawDesc law_ps_j2_linear() {
  LawDesc d = plane_stress_j2_law(DXM_LAW_PS_J2_LINEAR, 4, "plane_stress_j2_kernel<1");
  d.build = build_linear_hardening;
  d.residency_kernel = DXM_STOCK_ONLY(plane_stress_j2_linear_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_plane_stress_j2<PSJ_LINEAR>);
  return d;
}

constexpr LawDesc law_ps_j2_voce() {
  LawDesc d = plane_stress_j2_law(DXM_LAW_PS_J2_VOCE, 5, "plane_stress_j2_kernel<2");
  d.build = build_voce_hardening;
  d.residency_kernel = DXM_STOCK_ONLY(plane_stress_j2_voce_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_plane_stress_j2<PSJ_VOCE>);
  return d;
}

// Plane-stress Hosford plasticity (plane_stress_hosford.hip): the streams of laws 23 / 24, 168 B/point, and their hidden 3-wide
// plastic strain.  No external state variable is declared (n_ext = 0): dxm_set_external_state* answers with the library's sentence
constexpr LawDesc law_ps_hosford() {
  LawDesc d{};
  d.id = DXM_LAW_PS_HOSFORD;
  d.n_grad = d.n_flux = 3;
  d.n_params = d.n_params_custom = 5;
  d.n_isv_fields = 0;
  d.n_fields = 1;   // field 0 is hidden state: what the update is driven by (plane_stress_hosford.hpp)
  state_field(d, 0, "PlasticStrain", 3, 0);
  d.n_slots = PSH_NSLOTS;
  d.alg_bytes = 168;
  d.kernel = "plane_stress_hosford_kernel<0";
  d.blocks_per_cu = PSH_BLOCKS_PER_CU;   // plane_stress_hosford.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.build = build_ps_hosford;
  d.residency_kernel = DXM_STOCK_ONLY(plane_stress_hosford_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_ps_hosford);
  d.no_fields = "per-point parameter fields are not served for plane-stress Hosford plasticity: its constants are formed once per handle";
  d.stock_only = "plane-stress Hosford plasticity is perfectly plastic, it has no hardening law: it is served by the stock libdxmat, not by "
                 "a custom-hardening build";
  d.set_refusal = d.launch_refusal = "the plane-stress Hosford tangent is a 3x3 block of 9 entries, not a symmetric 6x6: only "
                                     "DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "plane-stress Hosford plasticity takes a 3-wide strain [xx, yy, sqrt(2) xy]: the mesh gradient kernels "
                                   "evaluate 6-wide strains or F, so the displacement forms (dxm_integrate_displacement*) and the fused "
                                   "displacement gradient are not served on a mesh that is not two-dimensional; pass the strain as an array";
  d.plane_kind = GRAD_IN_PLANE3;
  d.no_frame = "plane-stress Hosford plasticity is a function of the principal stresses: a material frame changes nothing in its update";
  return d;
}

// The two heat-transfer laws under a two-dimensional hypothesis (heat_plane.hip): temperature gradient in (16 B), heat flux (16) and
// the blocks of the tangent out, 2 x 2 | 2 x 1 [| 1 x 1]; parameters, build functions, external state variable and HeatParams are
// those of laws 16 / 17.  nodal_scalar: the displacement forms take the nodal temperature on a scalar mesh
constexpr LawDesc heat_plane_law(int id, int n_params, const char* kernel) {
  LawDesc d{};
  d.id = id;
  d.n_grad = d.n_flux = 2;
  d.n_params = d.n_params_custom = n_params;
  d.kernel = kernel;
  d.ext_kernel = kernel;   // one instantiation reads a uniform temperature or a stream
  d.n_ext = 1;
  d.ext_name[0] = "Temperature";
  d.ext_default[0] = 293.15;   // mfront.py:109-110
  d.blocks[0] = tangent_block(DXM_BLOCK_ROW_FLUX, 0, DXM_BLOCK_COL_GRADIENT, 0, 2, 2);
  d.blocks[1] = tangent_block(DXM_BLOCK_ROW_FLUX, 0, DXM_BLOCK_COL_EXTERNAL, 0, 2, 1);
  d.n_blocks = 2;
  d.ct_full = 6;
  d.blocks_per_cu = HP_BLOCKS_PER_CU;   // heat_plane.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.nodal_scalar = true;
  return d;
}

// counted as 64 B/point: temperature gradient in (16) and tangent out (48); with the flux (16) the kernel moves 80
constexpr LawDesc law_heat_stationary_2d() {
  LawDesc d = heat_plane_law(DXM_LAW_HEAT_STATIONARY_2D, 2, "heat_plane_kernel<0, 0");
  d.alg_bytes = 64;
  d.build = build_heat_stationary;
  d.residency_kernel = DXM_STOCK_ONLY(heat_plane_stationary_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_heat_stationary_2d);
  d.no_fields = "per-point parameter fields are not served for two-dimensional stationary heat transfer: A and B are per-handle "
                "constants (the temperature is an external state variable: dxm_set_external_state)";
  d.stock_only = "two-dimensional stationary heat transfer has no hardening law: it is served by the stock libdxmat, not by a "
                 "custom-hardening build";
  d.set_refusal = d.launch_refusal = "the two-dimensional stationary heat-transfer tangent is two blocks of 4 + 2 entries, not a "
                                     "symmetric 6x6: only DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists "
                                     "for this law";
  d.no_fused = d.no_displacement = "two-dimensional stationary heat transfer takes a temperature gradient, not a strain or a deformation "
                                   "gradient: the displacement forms (dxm_integrate_displacement*) serve it from the nodal temperature "
                                   "on a scalar mesh (dxm_mesh_create_plane_scalar) only; on this mesh pass grad(T) as an array";
  d.no_frame = "two-dimensional stationary heat transfer is isotropic (a scalar conductivity): a material frame changes nothing in its "
               "update";
  return d;
}

// counted as 80 B/point: gradient in (16), tangent (56) and enthalpy (8) out; with the flux (16) the kernel moves 96.  The enthalpy
// is written, never read
constexpr LawDesc law_heat_phase_change_2d() {
  LawDesc d = heat_plane_law(DXM_LAW_HEAT_PHASE_CHANGE_2D, 7, "heat_plane_kernel<1, 0");
  d.alg_bytes = 80;
  d.n_isv_fields = d.n_fields = 1;
  state_field(d, 0, "Enthalpy", 1, 0);
  d.n_slots = 1;
  d.blocks[2] = tangent_block(DXM_BLOCK_ROW_STATE, 0, DXM_BLOCK_COL_EXTERNAL, 0, 1, 1);
  d.n_blocks = 3;
  d.ct_full = 7;
  d.build = build_heat_phase_change;
  d.residency_kernel = DXM_STOCK_ONLY(heat_plane_phase_change_kernel_fn);
  d.launch = DXM_STOCK_ONLY(launch_heat_phase_change_2d);
  d.no_fields = "per-point parameter fields are not served for two-dimensional heat transfer with phase change: its constants are "
                "formed once per handle (the temperature is an external state variable: dxm_set_external_state)";
  d.stock_only = "two-dimensional heat transfer with phase change has no hardening law: it is served by the stock libdxmat, not by a "
                 "custom-hardening build";
  d.set_refusal = d.launch_refusal = "the two-dimensional phase-change tangent is three blocks of 4 + 2 + 1 entries, not a symmetric "
                                     "6x6: only DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "two-dimensional heat transfer with phase change takes a temperature gradient, not a strain or a "
                                   "deformation gradient: the displacement forms (dxm_integrate_displacement*) serve it from the nodal "
                                   "temperature on a scalar mesh (dxm_mesh_create_plane_scalar) only; on this mesh pass grad(T) as an array";
  d.no_frame = "two-dimensional heat transfer with phase change is isotropic (a scalar conductivity): a material frame changes nothing "
               "in its update";
  return d;
}

// Ogden under the plane-strain hypothesis (ogden_plane.hip): the 5-wide F in (40 B), PK1 (40) + the 5x5 dP/dF (200) + the isochoric PK2
// stress as [xx, yy, zz, sqrt(2) xy] (32) out: 312 B/point; the state is written, never read.  Parameters, their checks and the kernel's
// record are those of law 7 (build_ogden).  No external state variable is declared (n_ext = 0)
constexpr LawDesc law_ogden_pe() {
  LawDesc d{};
  d.id = DXM_LAW_OGDEN_PE;
  d.n_grad = d.n_flux = OGP_DIM;
  d.n_params = d.n_params_custom = 3;
  d.n_isv_fields = d.n_fields = 1;
  state_field(d, 0, "PK2Stress", OGP_NSLOTS, 0);
  d.n_slots = OGP_NSLOTS;
  d.alg_bytes = 312;
  d.kernel = "ogden_plane_kernel";
  d.no_fields = "per-point parameter fields are not served for plane-strain Ogden hyperelasticity: the kernel takes its exponents as "
                "per-handle constants";
  d.build = build_ogden;
  d.stock_only = "plane-strain Ogden hyperelasticity has no hardening law: it is served by the stock libdxmat, not by a custom-hardening "
                 "build";
  d.residency_kernel = DXM_STOCK_ONLY(ogden_plane_kernel_fn);
  d.blocks_per_cu = OGP_BLOCKS_PER_CU;   // ogden_plane.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = d.launch_refusal = "the plane-strain Ogden tangent dP/dF is a 5x5 block of 25 entries, not a symmetric 6x6: only "
                                     "DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "plane-strain Ogden hyperelasticity takes the 5-wide deformation gradient [F00, F11, F22, F01, F10]: "
                                   "the mesh gradient kernels produce the 9-wide F, so the displacement forms "
                                   "(dxm_integrate_displacement*) and the fused displacement gradient are not served; pass the 5-wide F "
                                   "[1 + H00, 1 + H11, 1, H01, H10] of the displacement gradient H as an array";
  d.no_frame = "plane-strain Ogden hyperelasticity is isotropic (a function of the principal stretches): a material frame changes "
               "nothing in its update";
  d.launch = DXM_STOCK_ONLY(launch_ogden_pe);   // ogden_plane.hip: F from the (N, 5) array, the full 5x5 tangent
  return d;
}

// Hosford under the plane-strain hypothesis (hosford_plane.hip): law 10 in the four components [xx, yy, zz, sqrt(2) xy].  Strain in
// (32 B), p and the hidden 4-wide plastic strain read (40); stress (32), the 4x4 tangent (128) and the nine state slots (72) out: 304
// B/point.  Parameters, their checks and the kernel's record are those of law 10 (build_hosford).  On a two-dimensional mesh the
// displacement forms run the plane gradient kernel (plane_kind) and then the update kernel, as laws 26-28 do
constexpr LawDesc law_pe_hosford() {
  // what the plane-strain rows share: the widths, L_FULL only, plane_kind = GRAD_PLANE_STRAIN4, kNoFrame; the sentences are this law's own
  LawDesc d = plane_strain_law(DXM_LAW_PE_HOSFORD_LINEAR, 5, 304, "hosford_plane_kernel");
  static_assert(HFP_DIM == PE_DIM, "the 4-wide strain of the plane-strain rows");
  d.n_isv_fields = 2;
  d.n_fields = 3;   // field 2 is hidden state: what the update is driven by (hosford_plane.hpp)
  state_field(d, 0, "ElasticStrain", HFP_DIM, HFP_SLOT_EEL);
  state_field(d, 1, "EquivalentPlasticStrain", 1, HFP_SLOT_P);
  state_field(d, 2, "PlasticStrain", HFP_DIM, HFP_SLOT_EP);
  d.n_slots = HFP_NSLOTS;
  d.no_fields = "per-point parameter fields are not served for plane-strain Hosford plasticity: the kernel takes its exponent's "
                "constants per handle";
  d.build = build_hosford;
  d.stock_only = "plane-strain Hosford plasticity takes linear hardening only: it is served by the stock libdxmat, not by a "
                 "custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(hosford_plane_kernel_fn);
  d.blocks_per_cu = HFP_BLOCKS_PER_CU;   // hosford_plane.hpp
  d.set_refusal = d.launch_refusal = "the plane-strain Hosford tangent is a general symmetric 4x4 block of 16 entries, not a symmetric 6x6 "
                                     "and not of the form c1 1x1 + c2 I + c3 n x n: only DXM_TANGENT_FULL is available, no packed record "
                                     "(sym / coef / pack4) exists for this law";
  d.no_fused = d.no_displacement = "plane-strain Hosford plasticity takes a 4-wide strain [xx, yy, zz, sqrt(2) xy]: the mesh gradient "
                                   "kernels evaluate 6-wide strains or F, so the displacement forms (dxm_integrate_displacement*) and the "
                                   "fused displacement gradient are not served on a mesh that is not "
                                   "two-dimensional; pass the strain as an array";
  d.launch = DXM_STOCK_ONLY(launch_pe_hosford);   // hosford_plane.hip: strain from the (N, 4) array, the full 4x4 tangent
  return d;
}

// Logarithmic-strain J2 under the plane-strain hypothesis (log_strain_plane.hip): the 5-wide F in (40 B), p and the hidden 4-wide
// logarithmic plastic strain read (40); PK1 (40), the 5x5 dP/dF (200) and the nine state slots (72) out: 392 B/point.  Parameters, their
// checks and the kernel's record are those of law 19 (build_log_strain).  F comes as an array: the row names no plane gradient kind
constexpr LawDesc law_log_strain_pe() {
  LawDesc d{};
  d.id = DXM_LAW_LOG_STRAIN_PE;
  d.n_grad = d.n_flux = LSP_DIM;
  d.n_params = d.n_params_custom = 4;
  d.n_isv_fields = 2;
  d.n_fields = 3;   // field 2 is hidden state: what the update is driven by (log_strain_plane.hpp)
  state_field(d, 0, "ElasticStrain", LSP_SYM, LSP_SLOT_EEL);
  state_field(d, 1, "EquivalentPlasticStrain", 1, LSP_SLOT_P);
  state_field(d, 2, "PlasticStrain", LSP_SYM, LSP_SLOT_EP);
  d.n_slots = LSP_NSLOTS;
  d.alg_bytes = 392;
  d.kernel = "log_strain_plane_kernel";
  d.no_fields = "per-point parameter fields are not served for plane-strain logarithmic-strain plasticity: the kernel takes its constants "
                "per handle";
  d.build = build_log_strain;
  d.stock_only = "plane-strain logarithmic-strain plasticity takes linear hardening only: it is served by the stock libdxmat, not by a "
                 "custom-hardening build";
  d.residency_kernel = DXM_STOCK_ONLY(log_strain_plane_kernel_fn);
  d.blocks_per_cu = LSP_BLOCKS_PER_CU;   // log_strain_plane.hpp
  d.set_layouts = d.launch_layouts = L_FULL;
  d.set_refusal = d.launch_refusal = "the plane-strain logarithmic-strain plasticity tangent dP/dF is a 5x5 block of 25 entries, not a "
                                     "symmetric 6x6: only DXM_TANGENT_FULL is available, no packed record (sym / coef / pack4) exists for "
                                     "this law";
  d.no_fused = d.no_displacement = "plane-strain logarithmic-strain plasticity takes the 5-wide deformation gradient "
                                   "[F00, F11, F22, F01, F10]: the mesh gradient kernels produce the 9-wide F, so the displacement forms "
                                   "(dxm_integrate_displacement*) and the fused displacement gradient are not served; pass the 5-wide F "
                                   "[1 + H00, 1 + H11, 1, H01, H10] of the displacement gradient H as an array";
  d.no_frame = "plane-strain logarithmic-strain plasticity is isotropic (Hooke, Mises): a material frame changes nothing in its update";
  d.launch = DXM_STOCK_ONLY(launch_log_strain_pe);   // log_strain_plane.hip: F from the (N, 5) array, the full 5x5 tangent
  return d;
}

// positional: row i is law id i; ids 6, 8, 9, 11, 13, 15, 18, 20, 22, 25, 29, 32, 34, 37, 39 and 41 are not assigned and stay empty rows (law_known).
// The rows through id 40 keep the text they had (tests/test_hosford_plane_cpu.py pins the last line of this initialiser); the ids
// after them are appended by law_table() below
static constexpr LawDesc kLawsThrough40[41] = {
    law_elastic(), law_j2_linear(), law_j2_voce(), law_fefp(DXM_LAW_FEFP_J2_VOCE, true), law_fefp(DXM_LAW_FEFP_J2_LINEAR, false),
    law_ramberg_osgood(), {}, law_ogden(), {}, {}, law_hosford(), {}, law_orthotropic(), {}, law_single_crystal(), {},
    law_heat_stationary(), law_heat_phase_change(), {}, law_log_strain_j2(), {}, law_fs_single_crystal(), {},
    law_ps_quadratic(), law_ps_polygon(), {}, law_pe_elastic(), law_pe_j2_linear(), law_pe_j2_voce(), {},
    law_ps_j2_linear(), law_ps_j2_voce(), {}, law_ps_hosford(),
    {}, law_heat_stationary_2d(), law_heat_phase_change_2d(),
    {}, law_ogden_pe(),
    {}, law_pe_hosford(),
};
struct LawTable {
  LawDesc row[DXM_LAW_COUNT];
};
constexpr LawTable law_table() {
  LawTable t{};
  for (int i = 0; i < 41; ++i) t.row[i] = kLawsThrough40[i];
  t.row[DXM_LAW_LOG_STRAIN_PE] = law_log_strain_pe();   // id 41 stays an empty row
  return t;
}
static constexpr LawTable kLawTable = law_table();
static constexpr const LawDesc (&kLaws)[DXM_LAW_COUNT] = kLawTable.row;

constexpr bool rows_in_place() {
  for (int i = 0; i < DXM_LAW_COUNT; ++i)
    if (kLaws[i].kernel && kLaws[i].id != i) return false;
  return true;
}
static_assert(rows_in_place(), "each row of kLaws sits at the index of its DXM_LAW_* id");
static_assert(!kLaws[6].kernel && !kLaws[8].kernel && !kLaws[9].kernel && !kLaws[11].kernel && !kLaws[13].kernel && !kLaws[15].kernel &&
                  !kLaws[18].kernel && !kLaws[20].kernel && !kLaws[22].kernel && !kLaws[25].kernel && !kLaws[29].kernel &&
                  !kLaws[32].kernel && !kLaws[34].kernel && !kLaws[37].kernel && !kLaws[39].kernel && !kLaws[41].kernel,
              "ids 6, 8, 9, 11, 13, 15, 18, 20, 22, 25, 29, 32, 34, 37, 39 and 41 are not assigned");

static bool law_known(int law) { return law >= 0 && law < DXM_LAW_COUNT && kLaws[law].kernel != nullptr; }

// parameters a law takes in THIS build: a custom-hardening build takes [E, nu, sig0, c0..c5] for the two "voce" slots
static int n_params_of(const LawDesc& d) { return kCustomBuild ? d.n_params_custom : d.n_params; }

// what the mesh gradient kernel evaluates for the law: 1 the deformation gradient F (9 components), 0 the small strain (6); on a
// two-dimensional mesh the row's plane_kind where it has one
static int gradient_kind(const LawDesc& d, bool on_2d_mesh) { return on_2d_mesh && d.plane_kind ? d.plane_kind : d.n_grad == 9 ? 1 : 0; }

static int tangent_size(const dxm_material* m);

static int isv_total(const LawDesc& d) {
  int t = 0;
  for (int f = 0; f < d.n_isv_fields; ++f) t += d.isv_dim[f];
  return t;
}

// ------------------------------------------------------------------------------------------
// host side that needs no GPU (worker pool, tangent rebuilds, chunk planner, locked-range table, row moves, upload-route
// state machine): host_side.hpp, shared with the sanitizer harness of the CPU test suite
// ------------------------------------------------------------------------------------------
using dxm_host::HostPool;
using dxm_host::expand_coef_tangent;
using dxm_host::expand_pack4_tangent;
using dxm_host::expand_fefp_tangent;
using dxm_host::fill_const_tangent;
using dxm_host::CtRoute;
using dxm_host::Route;
static_assert(dxm_host::THIRD == SS_THIRD && dxm_host::FEFP_RECORD == FEFP_REC, "host rebuilds and kernels share these constants");

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
constexpr int DXM_MAX_CHUNKS = dxm_host::MAX_CHUNKS;
constexpr int DXM_RING = dxm_host::RING;   // slots of the page-locked staging ring

struct dxm_material {
  int law = 0;
  int device = 0;
  int64_t n = 0;
  int64_t ld = 0;  // SoA leading dimension (n rounded up to 256, plus a 32-double stagger)
  LawParams prm{};
  std::vector<double> raw_params;
  int maxit = 25;
  double rtol = 1e-14;
  double* state[2] = {nullptr, nullptr};  // [n_slots][ld] each
  double* state_base = nullptr;           // one allocation holds s0 and s1
  size_t s1_skew = 0;
  bool s1_alias = false;  // after advance()/revert() s1 == s0 until the next integrate: no copy is made
  BlockStats* d_stats = nullptr;
  BlockStats* h_stats = nullptr;   // page-locked landing of the block records (no DMA into pageable memory)
  int stats_capacity = 0;
  int last_grid = 0;                      // stats records written by the last integrate
  hipStream_t pipe_stream = nullptr;      // second stream of the chunk-pipelined host path
  hipStream_t down_stream2 = nullptr;     // option split_streams: the second of the two download streams (pipe_stream is the first)
  // completion of the last launch: an event owned by the handle, recorded on the caller's stream (the
  // stream itself may be gone by the time the handle is asked to wait: e.g. a torch side stream)
  hipEvent_t last_event = nullptr;
  bool last_event_recorded = false;       // false while the last launch was stream-captured (no event then)
  bool launched = false;
  hipStream_t own_stream = nullptr;
  // launch configuration identity (dxm_launch_generation): epoch changes with parameters / layout /
  // placement / options, parity with every advance that swaps the two state buffers
  uint64_t epoch = 0;
  int parity = 0;
  // options (dxm_set_option)
  bool opt_pipeline = true;               // chunk-pipelined host path
  bool opt_split_streams = true;          // host path, page-locked gradient: uploads + kernels on one stream, downloads on two others (else: whole chunks alternate on two)
  int opt_packed_transfer = 2;            // host path: 0 move the full tangent; 1 its 9 coefficients (J2) / 54 building blocks (FeFp), block rebuilt
                                          // on the host; 2 (small strain) only (c1, c2, c3, w), the direction rebuilt from the stress
  bool opt_fused_gradient = true;         // displacement form: evaluate the gradient inside the update kernel
  bool opt_staged_gradient = true;        // hex8 gradient kernel: nodal data through LDS
  bool opt_verbose = false;
  dxm_host::UploadChooser up;             // option register_input (host path, pageable gradient array): 2 page-lock it for the call (DMA upload), 0 stage it, 1 measure and keep the faster
  int last_upload = DXM_UPLOAD_NONE;      // dxm_stats.upload of the last host-buffer call
  int opt_host_threads = 16;
  int opt_pageable_dma = 0;   // 1: hand pageable host arrays to the runtime (faster uploads; see upload_from_host)
  int64_t opt_packed_min_points = 32768;   // below: waking the workers costs what the bytes save (r02_hostpath_v2.jsonl)
  int opt_max_chunks = DXM_MAX_CHUNKS;
  HostPool* pool = nullptr;
  double* h_coef = nullptr;               // page-locked landing area of the tangent coefficients, h_coef_per_point doubles per point
  int h_coef_per_point = 0;
  double* h_flux = nullptr;               // page-locked (n, 6) landing area of the stress (dxm_integrate_rows)
  double* h_isv = nullptr;                // page-locked landing area of the bound state fields in the rows forms, field after field
  double elastic_lm[2] = {0.0, 0.0};      // lambda, mu handed to the constant-block fill
  hipEvent_t chunk_done[DXM_MAX_CHUNKS] = {};
  hipEvent_t kernel_done[DXM_MAX_CHUNKS] = {};   // option split_streams: what the download stream waits for, per chunk
  int num_cu = 256;
  int blocks_per_cu = 5;
  int tangent_layout = 0;    // DXM_TANGENT_FULL (36 / 81) | DXM_TANGENT_SYM (21) | DXM_TANGENT_COEF (9)
  // host-path staging (device side), allocated on first dxm_integrate
  double* d_grad = nullptr;
  double* d_flux = nullptr;
  // option keep_initial_io: gradient / flux of the initial state s0, kept by swapping with d_grad / d_flux at dxm_advance
  double* d_grad0 = nullptr;
  double* d_flux0 = nullptr;
  int io1_valid = 0;          // bit 0: d_grad holds the gradient of s1, bit 1: d_flux its flux (a completed host-buffer call)
  int io0_valid = 0;          // the same for d_grad0 / d_flux0 and s0
  int opt_keep_initial_io = 0;
  double* d_isv = nullptr;
  double* isv_out[DXM_MAX_STATE_FIELDS] = {};   // dxm_bind_isv_output: host rows the host-buffer forms deliver each field of s1 into
  double* d_isv_fields = nullptr;   // field-major scratch of those deliveries in a call that ALSO fills isv_aos (d_isv holds the AoS rows then)
  double* d_ct = nullptr;
  double* d_field = nullptr;  // (n, <= 6) AoS scratch for set/get_state of one field
  // host-buffer form, strain in ordinary memory: page-locked ring the kernels read the chunks from (zero-copy)
  double* h_grad_ring = nullptr;
  int64_t ring_slot_doubles = 0;
  hipEvent_t ring_done[DXM_RING] = {};
  int opt_stage_ahead = 3;
  double unregister_ms = 0.0;   // what releasing the call-scoped page-lock of the gradient array took in the last call
  // per-point parameter fields (dxm_set_param_field; the two small-strain J2 laws): bit i of pf_mask = params[i] is a field.
  // The kernels read streams of KERNEL parameters; E and nu fields are kept as given too, (lambda, mu) being functions of both
  int pf_mask = 0;
  double* pf_law[2] = {nullptr, nullptr};   // device copies of the E / nu fields, n doubles each
  double* pf_stream[PF_COUNT] = {};         // device streams (lambda, mu, sig0, h1, h2), n doubles each; null = uniform
  // material frame (dxm_set_frame*; the laws whose row has no `no_frame`): 0 none (identity), 1 uniform, 2 one per Gauss point
  double dt = 0.0;                          // the time increment of the call in progress (the rate-dependent laws; take_dt)
  // external state variables (dxm_set_external_state*; LawDesc::n_ext): 0 uniform (a kernel argument), 1 field (the handle's own
  // device copy, n doubles, allocated by the first field and kept until dxm_destroy: rewriting a field keeps its address)
  int ext_kind[DXM_MAX_EXTERNAL_STATE] = {};
  double ext_uniform[DXM_MAX_EXTERNAL_STATE] = {};
  double* ext_field[DXM_MAX_EXTERNAL_STATE] = {};
  // the nodal forms of the laws with LawDesc::nodal_scalar, for the duration of one call: 0 none, 1 the update kernel evaluates the
  // field at its points from nodal_src, 2 it reads the value stream d_nodal_value the scalar gradient kernel wrote.  The handle's own
  // external state above is neither read nor changed by such a call
  int nodal_mode = 0;
  ScalarSource nodal_src{};
  double* d_nodal_value = nullptr;          // n doubles, allocated by the first such call without a fused gradient
  int frame_kind = 0;
  Frame9 frame_uniform{};
  double* frame_streams = nullptr;          // the field as nine SoA streams of ld doubles each (the kernel reads 8 B per lane)
  // clean-tile stamps (the J2 laws; small_strain_clean.hpp): stamps[t] == clean_stamp means that tile t holds
  // the same bytes in state[0] and state[1].  Whoever writes either buffer without maintaining them calls bump_clean_stamp first
  uint32_t* stamps = nullptr;               // ceil(ld / 64) words, zeroed at dxm_create
  uint32_t clean_stamp = 1;                 // never 0
  bool stamps_stale = false;                // the counter wrapped: no stamp is believed until the next eager launch has zeroed them
  bool opt_elide_clean_state = true;
  mutable bool state_exposed = false;       // dxm_state_ptr handed out an address: the plain kernels from then on
  // packed copy of s0 (the J2 laws; host_side.hpp: PackEpoch): a read-side cache of state[0] for the clean
  // kernels, allocated by the first launch that builds it (+56 B/point while it exists), dropped at any time without changing a result
  unsigned long long* pack_mask = nullptr;  // ceil(n / 64) words: bit l = point l of the tile has a slot that is not bit-zero
  double* pack_buf = nullptr;               // ceil(n / 64) x 7 x 64 doubles: the tile's k kept points, slot c of the r-th at c k + r
  dxm_host::PackEpoch pack;
  hipStream_t pack_stream = nullptr;        // where the last launch that wrote or read the copy went
  bool pack_touched = false;                // ... if there was one
  bool pack_failed = false;                 // the allocation failed: the handle carries on without (until the option is set again)
  bool opt_pack_old_state = true;
};

static int sync_last(dxm_material* m);
static int pf_refresh_elastic(dxm_material* m, hipStream_t st);

// Called BEFORE anything but a clean kernel writes either state buffer (and by whoever learns of a write it could not see): all
// stamps turn stale at once.  Launches still in flight may go on writing the old value, which is stale too.
// s0_kept: the writer is known to leave state[0] alone (a replayed graph: the update kernel writes s1 only), the packed copy of s0
// stays; everybody else moves the s0 epoch on with the stamp.
static void bump_clean_stamp(dxm_material* m, bool s0_kept = false) {
  if (!m->stamps) return;
  if (!s0_kept) m->pack.move();
  bool wrapped = false;
  m->clean_stamp = dxm_host::next_clean_stamp(m->clean_stamp, &wrapped);
  if (wrapped) m->stamps_stale = true;
}
static int64_t stamp_words(const dxm_material* m) { return (m->ld + 63) / 64; }

// the packed copy is given back (no launch may be reading it: the caller has waited, or hipFree does)
static void free_pack(dxm_material* m) {
  if (m->pack_mask) { (void)hipFree(m->pack_mask); m->pack_mask = nullptr; }
  if (m->pack_buf) { (void)hipFree(m->pack_buf); m->pack_buf = nullptr; }
  m->pack.move();
  m->pack_touched = false;
}
// both arrays, when a launch first builds the copy.  False: no memory for them -- the HIP error is consumed, the handle goes on without
static bool reserve_pack(dxm_material* m) {
  if (m->pack_mask && m->pack_buf) return true;
  const size_t nt = (size_t)((m->n + WAVE - 1) / WAVE);
  if (hipMalloc(&m->pack_mask, sizeof(unsigned long long) * nt) == hipSuccess &&
      hipMalloc(&m->pack_buf, sizeof(double) * 7 * WAVE * nt) == hipSuccess)
    return true;
  (void)hipGetLastError();
  free_pack(m);
  m->pack_failed = true;
  return false;
}

static void free_state(dxm_material* m) {
  free_pack(m);
  if (m->stamps) { (void)hipFree(m->stamps); m->stamps = nullptr; }
  if (!m->state_base) return;
  (void)hipFree(m->state_base);
  m->state_base = nullptr;
}

static int build_params(dxm_material* m, const double* p, int np) {
  const LawDesc& d = kLaws[m->law];
  const int expect = n_params_of(d);
  if (np != expect) return fail(-1, "law %d expects %d parameters, got %d", m->law, expect, np);
  LawParams q{};
  q.maxit = m->maxit;
  q.rtol = m->rtol;
  if (int rc = d.build(p, q)) return rc;
  m->prm = q;
  m->raw_params.assign(p, p + np);
  return 0;
}

// What every dxm_integrate* form does with its dt: a rate-dependent law keeps it for its launches (a captured graph bakes it in),
// every other law ignores it as it always has.  A null handle is reported by the form itself.
static int take_dt(dxm_material* m, double dt) {
  if (!m || !kLaws[m->law].rate_dependent) return 0;
  if (!std::isfinite(dt) || dt < 0.0) return fail(-1, "law %d is rate-dependent: dt must be finite and >= 0, got %g", m->law, dt);
  m->dt = dt;
  return 0;
}

// the widest state field: the AoS scratch of dxm_set_state / dxm_get_state holds one field
static int widest_field(const LawDesc& d) {
  int w = 6;
  for (int f = 0; f < d.n_fields; ++f) w = d.isv_dim[f] > w ? d.isv_dim[f] : w;
  return w;
}

static int tangent_size(const dxm_material* m) {
  const LawDesc& d = kLaws[m->law];
  if (m->tangent_layout == DXM_TANGENT_SYM) return d.n_flux * (d.n_flux + 1) / 2;
  if (m->tangent_layout == DXM_TANGENT_COEF) return 9;
  if (m->tangent_layout == DXM_TANGENT_PACK4) return 4;
  return ct_full_of(d);
}

// ------------------------------------------------------------------------------------------
// small helper kernels (not on the hot path)
// ------------------------------------------------------------------------------------------
__global__ void fill_slot_kernel(double* dst, int64_t count, double value) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dst[i] = value;
}

struct PackMap { int n; int slot[16]; };

// SoA state -> AoS (n, total) internal-state-variable array (jaxmat.py:46-58 `_hcat_mixed`).
// Strain chunks from the page-locked ring to HBM: a copy kernel on a few workgroups (the PCIe link, not the CUs, bounds
// it), so that the rest of the chip stays free for the update kernel and the downloads of the other stream.
__global__ void __launch_bounds__(256) ring_upload_kernel(const double2_t* __restrict__ src, double2_t* __restrict__ dst, int64_t n16) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n16; k += (int64_t)gridDim.x * blockDim.x)
    dst[k] = __builtin_nontemporal_load(src + k);
}

__global__ void pack_isv_kernel(const double* __restrict__ soa, int64_t ld, int64_t n,
                                double* __restrict__ aos, PackMap map) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = n * map.n;
  if (t >= total) return;
  const int64_t i = t / map.n;
  const int k = (int)(t - i * map.n);
  aos[t] = soa[(int64_t)map.slot[k] * ld + i];
}

// AoS (n, map.n) -> SoA state slots (set_initial_state_dict upload).
__global__ void unpack_isv_kernel(double* __restrict__ soa, int64_t ld, int64_t n,
                                  const double* __restrict__ aos, PackMap map) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = n * map.n;
  if (t >= total) return;
  const int64_t i = t / map.n;
  const int k = (int)(t - i * map.n);
  soa[(int64_t)map.slot[k] * ld + i] = aos[t];
}

// ------------------------------------------------------------------------------------------
// ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int dxm_abi_version(void) { return DXM_ABI_VERSION; }

int dxm_has_custom_hardening(void) { return kCustomBuild ? 1 : 0; }

const char* dxm_last_error(void) { return g_last_error.c_str(); }

int dxm_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(-2, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int dxm_law_blocks_get(int law, dxm_law_blocks* out) {
  if (!law_known(law) || !out) return fail(-1, "unknown law id %d", law);
  const LawDesc& d = kLaws[law];
  memset(out, 0, sizeof(*out));
  out->n_external = d.n_ext;
  for (int k = 0; k < d.n_ext; ++k) {
    out->external_name[k] = d.ext_name[k];
    out->external_default[k] = d.ext_default[k];
  }
  out->n_blocks = d.n_blocks ? d.n_blocks : 1;
  if (d.n_blocks) {
    for (int b = 0; b < d.n_blocks; ++b) out->block[b] = d.blocks[b];
  } else {
    out->block[0] = tangent_block(DXM_BLOCK_ROW_FLUX, 0, DXM_BLOCK_COL_GRADIENT, 0, d.n_flux, d.n_grad);
  }
  out->tangent_width = ct_full_of(d);
  return 0;
}

int dxm_law_info_get(int law, dxm_law_info* out) {
  if (!law_known(law) || !out) return fail(-1, "unknown law id %d", law);
  const LawDesc& d = kLaws[law];
  memset(out, 0, sizeof(*out));
  out->n_grad = d.n_grad;
  out->n_flux = d.n_flux;
  out->n_params = n_params_of(d);
  out->n_isv_fields = d.n_isv_fields;
  for (int f = 0; f < DXM_MAX_STATE_FIELDS; ++f) {
    out->isv_dim[f] = d.isv_dim[f];
    out->isv_name[f] = d.isv_name[f];
  }
  out->n_isv_total = isv_total(d);
  out->algorithmic_bytes_per_point = d.alg_bytes;
  return 0;
}

static int init_state(dxm_material* m) {
  const LawDesc& d = kLaws[m->law];
  if (d.n_slots == 0) return 0;
  const size_t bytes = (size_t)d.n_slots * m->ld * sizeof(double);
  for (int w = 0; w < 2; ++w) {
    HIP_TRY(hipMemsetAsync(m->state[w], 0, bytes, m->own_stream));
    for (int f = 0; f < d.n_fields; ++f) {
      if (!(d.unit_fields & (1u << f))) continue;
      for (int s = d.isv_slot[f]; s < d.isv_slot[f] + 3; ++s) {   // the diagonal of the identity
        const int blocks = (int)((m->ld + 255) / 256);
        hipLaunchKernelGGL(fill_slot_kernel, dim3(blocks), dim3(256), 0, m->own_stream,
                           m->state[w] + (size_t)s * m->ld, m->ld, 1.0);
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(m->own_stream));
  return 0;
}

dxm_material* dxm_create(int law, const double* params, int n_params, int64_t npoints, int device) {
  if (!law_known(law)) { fail(-1, "unknown law id %d", law); return nullptr; }
  if (npoints < 0) { fail(-1, "negative point count"); return nullptr; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    fail(-2, "no usable HIP device (hipGetDeviceCount: %s, count %d); libdxmat has no CPU fallback",
         hipGetErrorString(e), ndev);
    return nullptr;
  }
  if (device < 0 || device >= ndev) { fail(-1, "device %d out of range [0,%d)", device, ndev); return nullptr; }
  const LawDesc& d = kLaws[law];
  // a library built for a user-supplied hardening law carries the hardening kernels only
  if (kCustomBuild && d.stock_only) { fail(-1, "%s", d.stock_only); return nullptr; }
  dxm_material* m = new dxm_material();
  m->law = law;
  m->device = device;
  m->n = npoints;
  for (int k = 0; k < kLaws[law].n_ext; ++k) m->ext_uniform[k] = kLaws[law].ext_default[k];
  // SoA leading dimension: N rounded up to 256 plus 32 doubles.  With a slot stride that is a
  // multiple of 2 KiB the s0 read streams and s1 write streams of all slots stay congruent and the
  // kernel falls into a slow mode (0.91 vs 0.83 ms at 1e7 points, bimodal by allocation address);
  // a 256 B stagger per slot removes it (profiles/archive/r01_tune_state_stride.txt).
  m->ld = ((npoints + 255) / 256) * 256 + 32;
  auto bail = [&](void) -> dxm_material* { dxm_destroy(m); return nullptr; };
  if (build_params(m, params, n_params) != 0) return bail();
  DeviceGuard guard(device);
  if (!guard.ok) { fail(-2, "hipSetDevice(%d) failed", device); return bail(); }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->num_cu = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&m->last_event, hipEventDisableTiming) != hipSuccess) {
    fail(-2, "hipStreamCreate / hipEventCreate failed"); return bail();
  }
  if (d.n_slots > 0) {
    const size_t bytes = (size_t)d.n_slots * m->ld * sizeof(double);
    {
      if (hipMalloc(&m->state_base, 2 * bytes + m->s1_skew) != hipSuccess) {
        fail(-3, "hipMalloc of %zu state bytes failed", 2 * bytes + m->s1_skew); return bail();
      }
      m->state[0] = m->state_base;
      m->state[1] = reinterpret_cast<double*>(reinterpret_cast<char*>(m->state_base) + bytes + m->s1_skew);
    }
  }
  // grid size, in workgroups per CU: the row's figure (the paragraphs at kLaws), else the residency of its kernel
  {
    // residency from the kernel's own resources (the occupancy API over-reports on ROCm 7.2):
    // waves/SIMD by allocated VGPRs (512-entry file, granule 8), workgroups by LDS (160 KiB/CU)
    hipFuncAttributes fa;
    if (d.residency_kernel && hipFuncGetAttributes(&fa, d.residency_kernel()) == hipSuccess && fa.numRegs > 0) {
      const int alloc = ((fa.numRegs + 7) / 8) * 8;
      int waves_simd = 512 / alloc;
      if (waves_simd > 8) waves_simd = 8;
      int by_vgpr = waves_simd * 4 / WAVES_PER_BLOCK;
      int by_lds = fa.sharedSizeBytes > 0 ? (int)(160 * 1024 / fa.sharedSizeBytes) : 8;
      int occ = by_vgpr < by_lds ? by_vgpr : by_lds;
      if (occ < 1) occ = 1;
      m->blocks_per_cu = occ;
    }
    if (d.blocks_per_cu) m->blocks_per_cu = d.blocks_per_cu;
  }
  // one record per workgroup and launch.  A single launch has at most num_cu * 256 workgroups (the largest grid
  // dxm_set_option("blocks_per_cu") allows); the chunked host path appends the records of up to DXM_MAX_CHUNKS
  // launches, each of min(ceil(chunk / 256), num_cu * blocks_per_cu) workgroups: never more than one record per
  // 256 points plus one partial block per chunk
  m->stats_capacity = dxm_host::stats_capacity(m->num_cu, npoints);
  if (hipMalloc(&m->d_stats, sizeof(BlockStats) * m->stats_capacity) != hipSuccess) {
    fail(-3, "hipMalloc of stats failed"); return bail();
  }
  if (init_state(m) != 0) return bail();
#ifndef DXM_CUSTOM_HARDENING
  if (law == DXM_LAW_J2_LINEAR || law == DXM_LAW_J2_VOCE) {
    const size_t bytes = sizeof(uint32_t) * (size_t)stamp_words(m);
    if (hipMalloc(&m->stamps, bytes) != hipSuccess || hipMemset(m->stamps, 0, bytes) != hipSuccess) {
      fail(-3, "hipMalloc / hipMemset of %zu stamp bytes failed", bytes); return bail();
    }
  }
#endif
  g_last_error.clear();
  return m;
}

int dxm_destroy(dxm_material* m) {
  if (!m) return 0;
  RelaxedCaptureMode relaxed;
  DeviceGuard guard(m->device);
  (void)sync_last(m);
  delete m->pool;
  if (m->h_coef) (void)hipHostFree(m->h_coef);
  if (m->h_flux) (void)hipHostFree(m->h_flux);
  if (m->h_isv) (void)hipHostFree(m->h_isv);
  for (hipEvent_t e : m->chunk_done) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->kernel_done) if (e) (void)hipEventDestroy(e);
  if (m->last_event) (void)hipEventDestroy(m->last_event);
  free_state(m);
  if (m->d_stats) (void)hipFree(m->d_stats);
  if (m->h_stats) (void)hipHostFree(m->h_stats);
  if (m->d_grad) (void)hipFree(m->d_grad);
  if (m->d_flux) (void)hipFree(m->d_flux);
  if (m->d_grad0) (void)hipFree(m->d_grad0);
  if (m->d_flux0) (void)hipFree(m->d_flux0);
  if (m->d_isv) (void)hipFree(m->d_isv);
  if (m->d_isv_fields) (void)hipFree(m->d_isv_fields);
  if (m->d_ct) (void)hipFree(m->d_ct);
  if (m->d_field) (void)hipFree(m->d_field);
  if (m->h_grad_ring) (void)hipHostFree(m->h_grad_ring);
  for (double* q : m->pf_law) if (q) (void)hipFree(q);
  for (double* q : m->pf_stream) if (q) (void)hipFree(q);
  if (m->frame_streams) (void)hipFree(m->frame_streams);
  for (double* q : m->ext_field) if (q) (void)hipFree(q);
  if (m->d_nodal_value) (void)hipFree(m->d_nodal_value);
  for (hipEvent_t e : m->ring_done) if (e) (void)hipEventDestroy(e);
  if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
  if (m->pipe_stream) (void)hipStreamDestroy(m->pipe_stream);
  if (m->down_stream2) (void)hipStreamDestroy(m->down_stream2);
  delete m;
  return 0;
}

int64_t dxm_npoints(const dxm_material* m) { return m ? m->n : -1; }
int dxm_law(const dxm_material* m) { return m ? m->law : -1; }

int dxm_set_params(dxm_material* m, const double* params, int n_params) {
  if (!m || !params) return fail(-1, "null argument");
  if (int rc = build_params(m, params, n_params)) return rc;   // nothing changed: captured graphs stay valid
  ++m->epoch;
  // bound parameter fields stay bound; (lambda, mu) streams made of one field and one uniform value follow the new value
  if (m->pf_mask & 3) {
    DEVICE_GUARD(m);
    if (int rc = sync_last(m)) return rc;
    if (int rc = pf_refresh_elastic(m, m->own_stream)) return rc;
    HIP_TRY(hipStreamSynchronize(m->own_stream));
  }
  return 0;
}

int dxm_set_tangent_layout(dxm_material* m, int layout) {
  if (!m) return fail(-1, "null handle");
  if (layout != DXM_TANGENT_FULL && layout != DXM_TANGENT_SYM && layout != DXM_TANGENT_COEF && layout != DXM_TANGENT_PACK4)
    return fail(-1, "unknown tangent layout %d", layout);
  const LawDesc& d = kLaws[m->law];
  if (!(d.set_layouts & (1u << layout))) return fail(-1, "%s", d.set_refusal);
  m->tangent_layout = layout;
  ++m->epoch;
  return 0;
}

int dxm_tangent_size(const dxm_material* m) { return m ? tangent_size(m) : -1; }

int dxm_set_newton(dxm_material* m, int maxit, double rtol) {
  if (!m) return fail(-1, "null handle");
  if (maxit < 1 || !(rtol > 0.0)) return fail(-1, "invalid Newton controls maxit=%d rtol=%g", maxit, rtol);
  m->maxit = maxit;
  m->rtol = rtol;
  if (int rc = build_params(m, m->raw_params.data(), (int)m->raw_params.size())) return rc;
  ++m->epoch;
  return 0;
}

static int check_field(const dxm_material* m, int which, int field) {
  if (!m) return fail(-1, "null handle");
  if (which != DXM_S0 && which != DXM_S1) return fail(-1, "state selector must be DXM_S0 or DXM_S1");
  const LawDesc& d = kLaws[m->law];
  if (field < 0 || field >= d.n_fields) return fail(-1, "law %d has no state field %d", m->law, field);
  return 0;
}

// Wait for the last launch on the handle.  The event belongs to the handle; if the last launch went
// into a stream capture (no event can be recorded there) the whole device is waited for.
static int sync_last(dxm_material* m) {
  if (!m->launched) return 0;
  if (m->last_event_recorded) {
    HIP_TRY(hipEventSynchronize(m->last_event));
  } else {
    HIP_TRY(hipDeviceSynchronize());
  }
  return 0;
}

static double* state_of(const dxm_material* m, int which) {
  return m->state[(which == DXM_S1 && !m->s1_alias) ? 1 : 0];
}

// A write to s1 while it is served from s0 needs its own storage first.
static int materialize_s1(dxm_material* m) {
  if (!m->s1_alias) return 0;
  const LawDesc& d = kLaws[m->law];
  bump_clean_stamp(m);   // (the copy makes the buffers equal, the writer that asked for it then changes one of them)
  if (d.n_slots > 0)
    HIP_TRY(hipMemcpy(m->state[1], m->state[0], (size_t)d.n_slots * m->ld * sizeof(double),
                      hipMemcpyDeviceToDevice));
  m->s1_alias = false;
  return 0;
}


// No DMA to or from pageable memory.  The runtime page-locks such a range on the fly and keeps the mapping in a cache
// keyed by address; when the owner has freed that memory since and a later allocation lands on the same address, the
// cached mapping is stale and the copy dies with "Memory access fault by GPU ... on address <host address>" -- as a
// write into a read-only page (download into a range once pinned as an upload source) or as a read through a dead
// mapping (upload).  Seen about once in 25 runs of the GPU test suite, whose tests allocate and free large numpy
// arrays all the time, as QuadratureMap.update does with its gradient arrays.  So: page-locked or registered memory
// is used directly; anything else goes through this page-locked staging (two halves in flight) and a CPU copy.
constexpr size_t BOUNCE_BYTES = 16u << 20;
// Host ranges this library has page-locked itself (dxm_host_alloc, dxm_host_register): start -> bytes.
static dxm_host::LockedTable g_locked;
static std::atomic<int> g_query_foreign{1};   // ask the runtime about pointers that are not in the table (option "query_foreign_pointers")
static void note_locked(const void* p, size_t bytes) { g_locked.note(p, bytes); }
static void forget_locked(const void* p) { g_locked.forget(p); }
static bool in_locked_table(const void* host, size_t bytes) { return g_locked.contains(host, bytes); }
static bool page_locked_byte(const void* host) {
  hipPointerAttribute_t attr{};
  const bool locked = host && hipPointerGetAttributes(&attr, host) == hipSuccess && attr.type == hipMemoryTypeHost;
  (void)hipGetLastError();   // "not a registered pointer" is the expected answer for ordinary memory
  return locked;
}
// Both ends of [host, host + bytes): an array that starts inside a registered / page-locked block but extends past it
// (a view into a larger buffer, a dxm_host_register of a shorter length) must take the staged route too.
static bool page_locked(const void* host, size_t bytes) {
  if (!host) return false;
  if (in_locked_table(host, bytes)) return true;
  if (!g_query_foreign.load()) return false;
  if (!page_locked_byte(host)) return false;
  return bytes <= 1 || page_locked_byte(static_cast<const char*>(host) + bytes - 1);
}
struct Staging {
  char* buf = nullptr;
  hipEvent_t done[2] = {nullptr, nullptr};
};
static std::mutex g_staging_mu[64];   // one per device: handles on different GPUs stage concurrently
static Staging g_staging[64];
static int current_device_index(int* dev) {
  HIP_TRY(hipGetDevice(dev));
  if (*dev < 0 || *dev >= 64) return fail(-1, "device index %d out of range", *dev);
  return 0;
}
static int staging_for_current_device(Staging** out) {
  int dev = 0;
  if (int rc = current_device_index(&dev)) return rc;
  Staging& s = g_staging[dev];
  if (!s.buf) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.buf), 2 * BOUNCE_BYTES, hipHostMallocDefault));
    for (hipEvent_t& e : s.done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  *out = &s;
  return 0;
}
static size_t chunk_size(size_t c, size_t nchunks, size_t bytes) { return c + 1 < nchunks ? BOUNCE_BYTES : bytes - c * BOUNCE_BYTES; }

// device -> caller-owned host memory; complete on return
static int download_to_host(void* host, const void* dev, size_t bytes, hipStream_t st) {
  if (bytes == 0) return 0;
  if (page_locked(host, bytes)) {
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  int devi = 0;
  if (int rc = current_device_index(&devi)) return rc;
  std::lock_guard<std::mutex> lk(g_staging_mu[devi]);
  Staging* s = nullptr;
  if (int rc = staging_for_current_device(&s)) return rc;
  const size_t nchunks = (bytes + BOUNCE_BYTES - 1) / BOUNCE_BYTES;
  for (size_t c = 0; c <= nchunks; ++c) {
    if (c < nchunks) {
      HIP_TRY(hipMemcpyAsync(s->buf + (c & 1) * BOUNCE_BYTES, static_cast<const char*>(dev) + c * BOUNCE_BYTES,
                             chunk_size(c, nchunks, bytes), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipEventRecord(s->done[c & 1], st));
    }
    if (c > 0) {   // the previous chunk lands while this one is in flight
      HIP_TRY(hipEventSynchronize(s->done[(c - 1) & 1]));
      memcpy(static_cast<char*>(host) + (c - 1) * BOUNCE_BYTES, s->buf + ((c - 1) & 1) * BOUNCE_BYTES, chunk_size(c - 1, nchunks, bytes));
    }
  }
  return 0;
}

// caller-owned host memory -> device; the host range may be reused on return (the device copy is complete too)
static int upload_from_host(void* dev, const void* host, size_t bytes, hipStream_t st) {
  if (bytes == 0) return 0;
  if (page_locked(host, bytes)) {
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  int devi = 0;
  if (int rc = current_device_index(&devi)) return rc;
  std::lock_guard<std::mutex> lk(g_staging_mu[devi]);
  Staging* s = nullptr;
  if (int rc = staging_for_current_device(&s)) return rc;
  const size_t nchunks = (bytes + BOUNCE_BYTES - 1) / BOUNCE_BYTES;
  for (size_t c = 0; c < nchunks; ++c) {
    if (c >= 2) HIP_TRY(hipEventSynchronize(s->done[c & 1]));   // this half has left for the device
    memcpy(s->buf + (c & 1) * BOUNCE_BYTES, static_cast<const char*>(host) + c * BOUNCE_BYTES, chunk_size(c, nchunks, bytes));
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(dev) + c * BOUNCE_BYTES, s->buf + (c & 1) * BOUNCE_BYTES, chunk_size(c, nchunks, bytes),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->done[c & 1], st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int dxm_set_state(dxm_material* m, int which, int field, const double* host_aos) {
  if (int rc = check_field(m, which, field)) return rc;
  if (!host_aos) return fail(-1, "null host pointer");
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  const LawDesc& d = kLaws[m->law];
  const int dim = d.isv_dim[field];
  const int64_t n = m->n;
  if (n == 0) return 0;
  // s1 served from s0 (after advance / revert) gets its own storage before EITHER is written: writing s1 must not
  // touch s0, and writing s0 must not change what s1 shows (the reference rebinds `data_manager.s0` and leaves s1
  // alone, generic.py:200-201 / jaxmat.py:205-206; found by tests/test_gpu_fuzz_protocol.py: advance, set, advance)
  if (int rc = materialize_s1(m)) return rc;
  // upload the AoS block and transpose on the device (a host-side transposition of 6 x 1e7
  // doubles costs more than the PCIe transfer)
  if (!m->d_field) HIP_TRY(hipMalloc(&m->d_field, sizeof(double) * n * widest_field(d)));
  PackMap map{};
  map.n = dim;
  for (int c = 0; c < dim; ++c) map.slot[c] = d.isv_slot[field] + c;
  hipStream_t st = m->own_stream;
  if (int rc = upload_from_host(m->d_field, host_aos, sizeof(double) * n * dim, st)) return rc;
  const int blocks = (int)((n * dim + 255) / 256);
  bump_clean_stamp(m);   // one of the two buffers changes
  hipLaunchKernelGGL(unpack_isv_kernel, dim3(blocks), dim3(256), 0, st, state_of(m, which), m->ld, n,
                     m->d_field, map);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int dxm_get_state(dxm_material* m, int which, int field, double* host_aos) {
  if (int rc = check_field(m, which, field)) return rc;
  if (!host_aos) return fail(-1, "null host pointer");
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  const LawDesc& d = kLaws[m->law];
  const int dim = d.isv_dim[field];
  const int64_t n = m->n;
  if (n == 0) return 0;
  if (!m->d_field) HIP_TRY(hipMalloc(&m->d_field, sizeof(double) * n * widest_field(d)));
  PackMap map{};
  map.n = dim;
  for (int c = 0; c < dim; ++c) map.slot[c] = d.isv_slot[field] + c;
  hipStream_t st = m->own_stream;
  const int blocks = (int)((n * dim + 255) / 256);
  hipLaunchKernelGGL(pack_isv_kernel, dim3(blocks), dim3(256), 0, st, state_of(m, which), m->ld, n,
                     m->d_field, map);
  HIP_TRY(hipGetLastError());
  return download_to_host(host_aos, m->d_field, sizeof(double) * n * dim, st);
}

int dxm_advance(dxm_material* m) {
  if (!m) return fail(-1, "null handle");
  // s0 <- s1 (generic.py:212-213 copies, jaxmat.py:39-40 aliases).  Done by swapping the two
  // device buffers; until the next integrate rewrites s1 in full, s1 reads are served from s0
  // (QuadratureMap.advance reads the final state right after update(): quadrature_map.py:355-356).
  if (!m->s1_alias) {
    double* t = m->state[0];
    m->state[0] = m->state[1];
    m->state[1] = t;
    m->s1_alias = true;
    m->parity ^= 1;   // launches now read / write the other buffer: dxm_launch_generation changes
    m->pack.move();   // state[0] is the other buffer: a new s0 epoch (the packed copy of the old s0 is not read again)
    // Gradient and flux of the accepted state stay on the device as those of s0 (option keep_initial_io): the buffers the
    // last host-buffer call filled become d_grad0 / d_flux0 and the next call fills the other pair -- no copy.  Without a
    // new state in between (advance twice, advance after revert: s1 is served from s0 and this branch is not entered) s0
    // keeps what it has.  A state that came from a form of call without host arrays (device pointers; a fused displacement
    // for the gradient) or that got its own storage back after revert (dxm_set_state: materialize_s1) brings NO copies
    // along, and s0 then holds none (io0_valid below): the Python layer's lazy s0 mirrors are settled before this call.
    if (m->opt_keep_initial_io && m->io1_valid) {
      if (m->io1_valid & 1) { double* g = m->d_grad0; m->d_grad0 = m->d_grad; m->d_grad = g; }
      if (m->io1_valid & 2) { double* f = m->d_flux0; m->d_flux0 = m->d_flux; m->d_flux = f; }
    }
    // the copies held for the state that has just been replaced belong to nobody now: s0 holds what the accepted state
    // brought along and nothing else (a state accepted from a device-pointer call brings nothing)
    m->io0_valid = m->opt_keep_initial_io ? m->io1_valid : 0;
    m->io1_valid = 0;
  }
  return 0;
}

// which copies the handle holds for state `which`: s1 shows those of s0 while it is served from it (after advance / revert)
static int io_mask(const dxm_material* m, int which) { return (which == DXM_S0 || m->s1_alias) ? m->io0_valid : m->io1_valid; }

int dxm_io_held(const dxm_material* m, int which) {
  if (!m || (which != DXM_S0 && which != DXM_S1)) return -1;
  return io_mask(m, which);
}

int dxm_get_io(dxm_material* m, int which, int kind, double* host_aos) {
  if (!m) return fail(-1, "null handle");
  if (which != DXM_S0 && which != DXM_S1) return fail(-1, "state selector must be DXM_S0 or DXM_S1");
  if (kind != 0 && kind != 1) return fail(-1, "kind must be 0 (gradient) or 1 (flux)");
  if (!(io_mask(m, which) & (1 << kind)))
    return fail(-1, "the %s of that state is not held on the device (a host-buffer integrate; for s0 also option keep_initial_io before dxm_advance)", kind ? "flux" : "gradient");
  if (m->n == 0) return 0;
  if (!host_aos) return fail(-1, "null host pointer");
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  const LawDesc& d = kLaws[m->law];
  const bool first = which == DXM_S0 || m->s1_alias;
  const double* src = kind ? (first ? m->d_flux0 : m->d_flux) : (first ? m->d_grad0 : m->d_grad);
  return download_to_host(host_aos, src, sizeof(double) * m->n * (kind ? d.n_flux : d.n_grad), m->own_stream);
}

int dxm_revert(dxm_material* m) {
  if (!m) return fail(-1, "null handle");
  m->s1_alias = true;  // s1 <- s0 (generic.py:215-216, jaxmat.py:42-43)
  m->io1_valid = 0;    // d_grad / d_flux belong to the state that was dropped
  return 0;
}

}  // extern "C"

// ---- launch -------------------------------------------------------------------------------
// The launchers of the rows of kLaws: one launch each over the point range of a LaunchArgs record.
template <int LAW>
static void launch_small_strain(const LaunchArgs& a) {
  dxm_material* m = a.m;
  const int grid = a.grid, tl = a.tl;
  const hipStream_t st = a.st;
  const int64_t cnt = a.cnt;
  const double* grad = a.grad;
  double *flux = a.flux, *ct = a.ct;
  const double* s0 = m->state[0] + a.off;
  double* s1 = m->state[1] + a.off;
  BlockStats* bs = m->d_stats + a.stats_off;
  const MeshSource none{};
  const MeshSource& src = a.fused ? *a.fused : none;
  const int g = a.fused ? a.fused->kind : 0;   // where the strain comes from: array / hex8 x 8 / tet4 / Lagrange simplex
  // J2 kernels: 2.25 KiB of unused dynamic LDS on top of the static 30.1 KiB keep FOUR workgroups (16 waves) per CU.  The
  // linear-hardening kernel needs 95 VGPRs since the flow direction of the tangent comes from the stress (it was 103):
  // a fifth wave per SIMD would fit and costs 0.65 % (0.8169 vs 0.8116 / 0.8123 ms per 1e7 points in one process,
  // profiles/archive/r03_j2_ab_pack4.jsonl); the elastic kernel keeps its five.
  constexpr int dyn_lds = LAW == LAW_ELASTIC ? 0 : 2304;
  // the J2 laws: the kernel that leaves unchanged tiles' state where it is, or the plain one behind a moved-on stamp
  // (dxm_host::choose_state_launch holds the rule; every writer of the state buffers is listed in DESIGN.md section 2)
  if constexpr (ss_has_state<LAW>) {
    if (m->stamps) {
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
      const bool capturing = cap != hipStreamCaptureStatusNone;
      if (m->stamps_stale && !capturing && m->opt_elide_clean_state && !m->state_exposed) {
        // every stamp value has been used: start over from zeroed stamps, behind whatever this handle still has in flight
        if (sync_last(m) == 0 && hipMemsetAsync(m->stamps, 0, sizeof(uint32_t) * (size_t)stamp_words(m), st) == hipSuccess) {
          m->stamps_stale = false;
          m->clean_stamp = 1;
        } else {
          (void)hipGetLastError();
        }
      }
      dxm_host::StateLaunchFlags f{};
      f.has_stamps = true;
      f.option = m->opt_elide_clean_state;
      f.fields = m->pf_mask != 0;
      f.frame = m->frame_kind != 0;
      f.fused = a.fused != nullptr;
      f.whole_tiles = dxm_host::covers_whole_tiles(a.off, cnt, m->n);
      f.capturing = capturing;
      f.exposed = m->state_exposed;
      f.stamps_stale = m->stamps_stale;
      // the packed copy of s0: none for a handle whose state address is out (and what it held is given back)
      if (m->state_exposed && (m->pack_buf || m->pack_mask)) free_pack(m);
      f.pack_option = m->opt_pack_old_state && !m->pack_failed;
      f.full_range = a.off == 0 && cnt == m->n;
      f.chunk_of_host_call = a.host_chunk;
      f.epoch_launches = m->pack.launches;
      f.built = m->pack.built;
      f.ordered = !m->pack_touched || st == m->pack_stream || (m->launched && m->last_event_recorded);
      dxm_host::StateLaunch how = dxm_host::choose_state_launch(f);
#ifndef DXM_CUSTOM_HARDENING
      using dxm_host::StateLaunch;
      if (how == StateLaunch::clean_build || how == StateLaunch::clean_use) {
        // the arrays on first use; behind the last launch that touched the copy where that one went to another stream
        bool ok = f.ordered && (how == StateLaunch::clean_use || reserve_pack(m));
        if (ok && m->pack_touched && st != m->pack_stream && hipStreamWaitEvent(st, m->last_event, 0) != hipSuccess) {
          (void)hipGetLastError();
          ok = false;
        }
        if (ok && small_strain_packed_launch(how == StateLaunch::clean_build ? 1 : 2, LAW, tl, grid, dyn_lds, st, m->prm, cnt, grad, s0, s1,
                                             m->ld, flux, ct, bs, m->stamps, m->clean_stamp, m->pack_mask, m->pack_buf)) {
          m->pack.note(f, how);
          m->pack_stream = st;
          m->pack_touched = true;
          return;
        }
        how = StateLaunch::clean;   // no memory, no such instantiation, no way to order it: the kernel without the copy
      }
      if (how == StateLaunch::clean &&
          small_strain_clean_launch(LAW, tl, grid, dyn_lds, st, m->prm, cnt, grad, s0, s1, m->ld, flux, ct, bs, m->stamps + a.off / WAVE,
                                    m->clean_stamp)) {
        m->pack.note(f, how);
        return;
      }
#endif
      bump_clean_stamp(m);
    }
  }
#ifndef DXM_CUSTOM_HARDENING
  if constexpr (LAW != LAW_ELASTIC) {
    if (m->pf_mask) {   // param_fields.hip: the streams advance with the range like the state slots
      ParamStreams pf{};
      for (int k = 0; k < PF_COUNT; ++k) pf.p[k] = m->pf_stream[k] ? m->pf_stream[k] + a.off : nullptr;
      param_fields_launch(LAW, tl, g, grid, dyn_lds, st, m->prm, pf, cnt, grad, s0, s1, m->ld, flux, ct, bs, src);
      return;
    }
  }
#endif
#define DXM_LAUNCH_SS(TL, G)                                                                              \
  hipLaunchKernelGGL((small_strain_kernel<LAW, TL, G>), dim3(grid), dim3(BLOCK), dyn_lds, st, m->prm, cnt, grad, s0, s1, \
                     m->ld, flux, ct, bs, src)
#define DXM_LAUNCH_SS_G(TL) do { if (g == 0) DXM_LAUNCH_SS(TL, 0); else if (g == 1) DXM_LAUNCH_SS(TL, 1); \
                                 else if (g == 2) DXM_LAUNCH_SS(TL, 2); else DXM_LAUNCH_SS(TL, 3); } while (0)
  if (tl == TL_SYM) DXM_LAUNCH_SS_G(TL_SYM);
  else if (tl == TL_FULL) DXM_LAUNCH_SS_G(TL_FULL);
  else if constexpr (ss_has_coef<LAW>) { if (tl == TL_PACK4) DXM_LAUNCH_SS_G(TL_PACK4); else DXM_LAUNCH_SS_G(TL_COEF); }
#undef DXM_LAUNCH_SS_G
#undef DXM_LAUNCH_SS
}

// voce: Voce hardening (or the traced law of a custom-hardening build); else linear hardening
static void launch_fefp(const LaunchArgs& a, bool voce) {
  dxm_material* m = a.m;
  const int grid = a.grid;
  const hipStream_t st = a.st;
  const int64_t cnt = a.cnt;
  const double* grad = a.grad;
  double *flux = a.flux, *ct = a.ct;
  const double* s0 = m->state[0] + a.off;
  double* s1 = m->state[1] + a.off;
  BlockStats* bs = m->d_stats + a.stats_off;
  const MeshSource none{};
  const MeshSource& fsrc = a.fused ? *a.fused : none;
  const int g = a.fused ? a.fused->kind : 0;
#define DXM_LAUNCH_FEFP(HARD, G, T) \
  hipLaunchKernelGGL((fefp_kernel<HARD, G, T>), dim3(grid), dim3(BLOCK), 0, st, m->prm, cnt, grad, s0, s1, m->ld, flux, ct, bs, fsrc)
#define DXM_LAUNCH_FEFP_G(HARD, T) do { if (g == 0) DXM_LAUNCH_FEFP(HARD, 0, T); else if (g == 1) DXM_LAUNCH_FEFP(HARD, 1, T); \
                                       else if (g == 2) DXM_LAUNCH_FEFP(HARD, 2, T); else DXM_LAUNCH_FEFP(HARD, 3, T); } while (0)
  // tl == TL_COEF: the 54 building blocks of the tangent per point instead of its 81 entries (host-buffer form)
  if (a.tl == TL_COEF) { if (voce) DXM_LAUNCH_FEFP_G(1, 1); else DXM_LAUNCH_FEFP_G(0, 1); }
  else                 { if (voce) DXM_LAUNCH_FEFP_G(1, 0); else DXM_LAUNCH_FEFP_G(0, 0); }
#undef DXM_LAUNCH_FEFP_G
#undef DXM_LAUNCH_FEFP
}
static void launch_fefp_voce(const LaunchArgs& a) { launch_fefp(a, true); }
static void launch_fefp_linear(const LaunchArgs& a) { launch_fefp(a, false); }

#ifndef DXM_CUSTOM_HARDENING
static void launch_ramberg_osgood(const LaunchArgs& a) {
  const MeshSource none{};
  ramberg_osgood_launch(a.tl, a.fused ? a.fused->kind : 0, a.grid, a.st, a.m->prm, a.cnt, a.grad, a.flux, a.ct,
                        a.m->d_stats + a.stats_off, a.fused ? *a.fused : none);
}

static void launch_ogden(const LaunchArgs& a) {
  dxm_material* m = a.m;
  ogden_launch(a.grid, a.st, m->prm, a.cnt, a.grad, m->state[1] + a.off, m->ld, a.flux, a.ct, m->d_stats + a.stats_off);
}

static void launch_ogden_pe(const LaunchArgs& a) {
  dxm_material* m = a.m;
  ogden_plane_launch(a.grid, a.st, m->prm, a.cnt, a.grad, m->state[1] + a.off, m->ld, a.flux, a.ct, m->d_stats + a.stats_off);
}

static void launch_pe_hosford(const LaunchArgs& a) {
  dxm_material* m = a.m;
  hosford_plane_launch(a.grid, a.st, m->prm, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                       m->d_stats + a.stats_off);
}

static void launch_log_strain_pe(const LaunchArgs& a) {
  dxm_material* m = a.m;
  log_strain_plane_launch(a.grid, a.st, m->prm, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                          m->d_stats + a.stats_off);
}

static void launch_hosford(const LaunchArgs& a) {
  dxm_material* m = a.m;
  hosford_launch(a.tl, a.grid, a.st, m->prm, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                 m->d_stats + a.stats_off);
}

static void launch_log_strain(const LaunchArgs& a) {
  dxm_material* m = a.m;
  log_strain_launch(a.grid, a.st, m->prm, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                    m->d_stats + a.stats_off);
}

static void launch_fs_single_crystal(const LaunchArgs& a) {
  dxm_material* m = a.m;
  const double* p = m->raw_params.data();   // 16 values (build_fs_single_crystal)
  const OrthoStiffness s = ortho_load(m->prm);
  FxParams sp{};
  sp.c11 = s.c[0]; sp.c12 = s.c[1]; sp.g2 = s.g2[0];
  sp.n = p[3]; sp.K = p[4]; sp.tau0 = p[5]; sp.b = p[7]; sp.d = p[8]; sp.C = p[9];
  for (int k = 0; k < 6; ++k) sp.qh[k] = p[6] * p[10 + k];
  sp.dt = a.dt;
  fs_single_crystal_launch(m->frame_kind, a.grid, a.st, m->prm, sp, a.cnt, a.grad, m->frame_uniform,
                           m->frame_streams ? m->frame_streams + a.off : nullptr, m->ld, m->state[0] + a.off, m->state[1] + a.off, m->ld,
                           a.flux, a.ct, m->d_stats + a.stats_off);
}

static void launch_orthotropic(const LaunchArgs& a) {
  dxm_material* m = a.m;
  // the frame streams advance with the range like the state slots
  orthotropic_launch(m->frame_kind, a.tl, a.grid, a.st, m->prm, a.cnt, a.grad, m->frame_uniform,
                     m->frame_streams ? m->frame_streams + a.off : nullptr, m->ld, a.flux, a.ct, m->d_stats + a.stats_off);
}

static void launch_single_crystal(const LaunchArgs& a) {
  dxm_material* m = a.m;
  const double* p = m->raw_params.data();   // 22 values (build_single_crystal)
  ScParams sp{};
  sp.n = p[9]; sp.K = p[10]; sp.tau0 = p[11]; sp.b = p[13]; sp.d = p[14]; sp.C = p[15];
  for (int k = 0; k < 6; ++k) sp.qh[k] = p[12] * p[16 + k];
  sp.guard = 1.1 * sp.K;
  sp.floor_f = 1e-12 * ortho_load(m->prm).c[0];
  sp.dt = a.dt;
  single_crystal_launch(m->frame_kind, a.grid, a.st, m->prm, sp, a.cnt, a.grad, m->frame_uniform,
                        m->frame_streams ? m->frame_streams + a.off : nullptr, m->ld, m->state[0] + a.off, m->state[1] + a.off, m->ld,
                        a.flux, a.ct, m->d_stats + a.stats_off);
}

// the external state variable of the range: the field advances with it like the state slots
static HeatParams heat_params_stationary(const dxm_material* m) {
  HeatParams hp{};
  hp.p[HT_A] = m->raw_params[0];
  hp.p[HT_B] = m->raw_params[1];
  return hp;
}
static void launch_heat_stationary(const LaunchArgs& a) {
  dxm_material* m = a.m;
  const HeatParams hp = heat_params_stationary(m);
  heat_transfer_launch(HT_STATIONARY, a.grid, a.st, hp, a.cnt, a.grad, m->ext_uniform[0], m->ext_kind[0] ? m->ext_field[0] + a.off : nullptr,
                       nullptr, a.flux, a.ct, m->d_stats + a.stats_off);
}

// what both phase-change kernels read (heat_transfer.hpp: HeatParams): each entry a parameter or one individually rounded operation
static HeatParams heat_params_phase_change(const dxm_material* m) {
#pragma clang fp contract(off)
  const double* p = m->raw_params.data();   // [Tm, ks, cs, kl, cl, dhsl, Tsmooth] (build_heat_phase_change)
  const double Tm = p[0], ks = p[1], cs = p[2], kl = p[3], cl = p[4], dhsl = p[5], Tsm = p[6];
  HeatParams hp{};
  const double half = Tsm / 2;
  hp.p[HT_TS] = Tm - half;
  hp.p[HT_TL] = Tm + half;
  hp.p[HT_KS] = ks; hp.p[HT_KL] = kl; hp.p[HT_CS] = cs; hp.p[HT_CL] = cl;
  hp.p[HT_DK] = kl - ks;
  hp.p[HT_TSM] = Tsm;
  const double c_mean = (cs + cl) / 2, c_latent = dhsl / Tsm;
  hp.p[HT_CTR] = c_mean + c_latent;
  hp.p[HT_NSLOPE] = -(kl - ks) / Tsm;
  hp.p[HT_DHSL] = dhsl;
  hp.p[HT_CSTS] = cs * hp.p[HT_TS];
  const double cc = (cs + cl) * Tsm;
  hp.p[HT_HL3] = cc / 2;
  return hp;
}
static void launch_heat_phase_change(const LaunchArgs& a) {
  dxm_material* m = a.m;
  const HeatParams hp = heat_params_phase_change(m);
  heat_transfer_launch(HT_PHASE_CHANGE, a.grid, a.st, hp, a.cnt, a.grad, m->ext_uniform[0], m->ext_kind[0] ? m->ext_field[0] + a.off : nullptr,
                       m->state[1] + a.off, a.flux, a.ct, m->d_stats + a.stats_off);
}

// The 2-wide laws (heat_plane.hip) on the same records.  In a nodal call (dxm_material::nodal_mode) the temperature of a point is
// the field's: evaluated by the kernel itself from the mesh (1), or the stream the scalar gradient kernel wrote beside the
// gradient (2); the handle's own external state is not read then
static void launch_heat_plane(int law, const HeatParams& hp, const LaunchArgs& a, double* enthalpy) {
  dxm_material* m = a.m;
  const double* tfield = m->ext_kind[0] ? m->ext_field[0] + a.off : nullptr;
  ScalarSource src = m->nodal_src;
  src.point0 = a.off;
  if (m->nodal_mode == 2) tfield = m->d_nodal_value + a.off;
  heat_plane_launch(law, a.grid, a.st, hp, a.cnt, a.grad, m->ext_uniform[0], tfield, m->nodal_mode == 1 ? &src : nullptr, enthalpy, a.flux,
                    a.ct, m->d_stats + a.stats_off);
}
static void launch_heat_stationary_2d(const LaunchArgs& a) { launch_heat_plane(HT_STATIONARY, heat_params_stationary(a.m), a, nullptr); }
static void launch_heat_phase_change_2d(const LaunchArgs& a) {
  launch_heat_plane(HT_PHASE_CHANGE, heat_params_phase_change(a.m), a, a.m->state[1] + a.off);
}

// the plane-stress stiffness as cvxpy_materials.py:16-18 forms it, and its eigenvalues: what every plane-stress launcher puts into
// its kernel's record, each entry one or two individually rounded operations
struct PsStiffness { double c11, c12, c33, CA, CB; };   // CA = E/(1-nu), CB = E/(1+nu)
static PsStiffness ps_stiffness(double E, double nu) {
#pragma clang fp contract(off)
  const double c0 = E / (1.0 - nu * nu);
  return {c0, c0 * nu, c0 * (1.0 - nu), E / (1.0 - nu), E / (1.0 + nu)};
}
// the constants both plane-stress kernels read
static void ps_elastic_constants(PsParams& q, double E, double nu) {
  const PsStiffness k = ps_stiffness(E, nu);
  q.p[PS_C11] = k.c11; q.p[PS_C12] = k.c12; q.p[PS_C33] = k.c33;
  q.p[PS_E] = E; q.p[PS_NU] = nu;
  q.p[PS_CA] = k.CA; q.p[PS_CB] = k.CB;
}

static void launch_ps_quadratic(const LaunchArgs& a) {
#pragma clang fp contract(off)
  dxm_material* m = a.m;
  const double* p = m->raw_params.data();   // [E, nu, sig0, q, tangent] (build_ps_quadratic)
  PsParams q{};
  ps_elastic_constants(q, p[0], p[1]);
  q.p[PS_QC] = p[3];
  q.p[PS_SIG0] = p[2];
  q.p[PS_TOL] = m->prm.tol;
  q.p[PS_KMAX] = fmax(fmax(0.5 * q.p[PS_CA], 1.5 * q.p[PS_CB]), p[3] * q.p[PS_CB]);
  q.p[PS_SIG0SQ] = p[2] * p[2];
  q.maxit = m->prm.maxit;
  plane_stress_launch(PS_QUADRATIC, p[4] != 0.0, a.grid, a.st, q, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                      m->d_stats + a.stats_off);
}

static void launch_ps_polygon(const LaunchArgs& a) {
#pragma clang fp contract(off)
  dxm_material* m = a.m;
  const double* p = m->raw_params.data();   // [E, nu, M, (n1, n2, d) x 4] (build_ps_polygon)
  PsParams q{};
  ps_elastic_constants(q, p[0], p[1]);
  const int M = (int)p[2];
  q.planes = M;
  constexpr double eps = 2.220446049250313e-16;
  for (int k = 0; k < M; ++k) {
    const double* r = p + 3 + 3 * k;
    double* pl = q.p + PS_PLANE + k * PS_PLANE_REC;
    pl[PL_N1] = r[0]; pl[PL_N2] = r[1]; pl[PL_D] = r[2];
    // w = M^-1 n with M^-1 = [[C11, C12], [C12, C11]], the stiffness of the principal values
    pl[PL_W1] = q.p[PS_C11] * r[0] + q.p[PS_C12] * r[1];
    pl[PL_W2] = q.p[PS_C12] * r[0] + q.p[PS_C11] * r[1];
    pl[PL_NW] = r[0] * pl[PL_W1] + r[1] * pl[PL_W2];
    pl[PL_SLACK] = (8.0 * eps) * r[2];
  }
  // the vertices: intersections of two non-parallel rows at which every other row holds (to 64 eps d: three rows through one point)
  int nv = 0;
  for (int i = 0; i < M; ++i)
    for (int j = i + 1; j < M; ++j) {
      const double* ri = p + 3 + 3 * i;
      const double* rj = p + 3 + 3 * j;
      const double det = ri[0] * rj[1] - ri[1] * rj[0];
      if (det == 0.0) continue;
      const double x = (ri[2] * rj[1] - rj[2] * ri[1]) / det, y = (ri[0] * rj[2] - rj[0] * ri[2]) / det;
      bool adm = std::isfinite(x) && std::isfinite(y);
      for (int k = 0; k < M; ++k) {
        const double* rk = p + 3 + 3 * k;
        if (k != i && k != j) adm = adm && ((rk[0] * x + rk[1] * y) - rk[2] <= (64.0 * eps) * rk[2]);
      }
      if (adm) { q.p[PS_VERTEX + 2 * nv] = x; q.p[PS_VERTEX + 2 * nv + 1] = y; ++nv; }
    }
  q.vertices = nv;
  plane_stress_launch(PS_POLYGON, 0, a.grid, a.st, q, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                      m->d_stats + a.stats_off);
}
// the record of the handle's law is the 6-wide law's (build_elastic / build_linear_hardening / build_voce_hardening)
template <int LAW> static void launch_plane_strain(const LaunchArgs& a) {
  dxm_material* m = a.m;
  const bool state = LAW != PE_ELASTIC;
  plane_strain_launch(LAW, a.grid, a.st, m->prm, a.cnt, a.grad, state ? m->state[0] + a.off : nullptr, state ? m->state[1] + a.off : nullptr,
                      m->ld, a.flux, a.ct, m->d_stats + a.stats_off);
}
// the record of the handle's law is the 6-wide law's (build_linear_hardening / build_voce_hardening); the plane-stress constants are
// formed here from E and nu, each entry a few individually rounded operations (plane_stress_j2.hpp: PsJ2Params)
template <int HARD> static void launch_plane_stress_j2(const LaunchArgs& a) {
#pragma clang fp contract(off)
  dxm_material* m = a.m;
  const PsStiffness k = ps_stiffness(m->raw_params[0], m->raw_params[1]);
  PsJ2Params q{};
  q.law = m->prm;
  q.c11 = k.c11; q.c12 = k.c12; q.c33 = k.c33;
  q.CA = k.CA; q.CB = k.CB;
  q.ka = q.CA / 3.0;
  q.kmax = fmax(q.ka, q.CB);
  q.kmin = fmin(q.ka, q.CB);
  plane_stress_j2_launch(HARD, a.grid, a.st, q, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                         m->d_stats + a.stats_off);
}
// what the kernel reads (plane_stress_hosford.hpp: PshParams): each entry a parameter or a few individually rounded operations
static void launch_ps_hosford(const LaunchArgs& a) {
#pragma clang fp contract(off)
  dxm_material* m = a.m;
  const double* p = m->raw_params.data();   // [E, nu, sig0, a, tangent] (build_ps_hosford)
  const double E = p[0], nu = p[1];
  const PsStiffness k = ps_stiffness(E, nu);
  PshParams q{};
  q.p[PSH_C11] = k.c11; q.p[PSH_C12] = k.c12; q.p[PSH_C33] = k.c33;
  q.p[PSH_E] = E; q.p[PSH_NU] = nu;
  q.p[PSH_SQA] = sqrt(k.CA);   // sqrt(E / (1 - nu)), sqrt(E / (1 + nu)): the quotient rounded, then the root
  q.p[PSH_SQB] = sqrt(k.CB);
  q.p[PSH_SIG0] = p[2];
  q.p[PSH_A] = p[3];
  q.p[PSH_AM1] = p[3] - 1.0;
  q.p[PSH_AM2] = p[3] - 2.0;
  q.p[PSH_INVA] = 1.0 / p[3];
  q.p[PSH_TOL] = m->prm.tol;
  q.p[PSH_CB] = k.CB;
  constexpr double eps4 = 4.0 * 2.220446049250313e-16;
  q.p[PSH_KLO] = pow(0.5, q.p[PSH_INVA]) * (1.0 - eps4);
  q.p[PSH_KHI] = pow(1.5, q.p[PSH_INVA]) * (1.0 + eps4);
  q.maxit = m->prm.maxit;
  plane_stress_hosford_launch(p[4] != 0.0, a.grid, a.st, q, a.cnt, a.grad, m->state[0] + a.off, m->state[1] + a.off, m->ld, a.flux, a.ct,
                              m->d_stats + a.stats_off);
}
#endif

// tl: tangent layout of THIS launch (LaunchArgs)
static int launch_range(dxm_material* m, int64_t off, int64_t cnt, const double* grad, double* flux,
                        double* ct, hipStream_t st, int stats_off, int* grid_out,
                        const MeshSource* fused, int tl, bool host_chunk = true) {
  if (((uintptr_t)grad | (uintptr_t)flux | (uintptr_t)ct) & 15)
    return fail(-1, "gradient / flux / tangent device arrays must be 16-byte aligned");
  m->io1_valid = 0;   // s1 is being rewritten; a host-buffer call that completes sets it again
  static_assert(WAVE * WAVES_PER_BLOCK == 256, "dxm_host::launch_grid counts workgroups of 256 points");
  const int64_t blocks = dxm_host::launch_grid(cnt, m->num_cu, m->blocks_per_cu);
  if (stats_off + blocks > m->stats_capacity) return fail(-1, "internal: stats buffer too small");
  const int grid = (int)blocks;
  const LawDesc& d = kLaws[m->law];
  if (!d.launch) return fail(-1, "law %d not launchable", m->law);
  if (fused && d.no_fused) return fail(-1, "%s", d.no_fused);
  if (!(d.launch_layouts & (1u << tl))) return fail(-1, "%s", d.launch_refusal);
  d.launch(LaunchArgs{m, grid, st, off, cnt, grad, flux, ct, stats_off, fused, tl, m->dt, host_chunk});
  HIP_TRY(hipGetLastError());
  *grid_out = grid;
  return 0;
}

static int launch(dxm_material* m, const double* grad, double* flux, double* ct, hipStream_t st,
                  const MeshSource* fused = nullptr) {
  if (m->n == 0) { m->last_grid = 0; return 0; }
  int grid = 0;
  if (int rc = launch_range(m, 0, m->n, grad, flux, ct, st, 0, &grid, fused, m->tangent_layout, false)) return rc;
  m->last_grid = grid;
  m->launched = true;
  m->s1_alias = false;  // the kernel rewrites every slot of s1
  // completion marker owned by the handle (not recordable while the stream is being captured into a graph)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  m->last_event_recorded = false;
  if (cap == hipStreamCaptureStatusNone) {
    HIP_TRY(hipEventRecord(m->last_event, st));
    m->last_event_recorded = true;
  }
  return 0;
}

extern "C" {

int dxm_integrate_device(dxm_material* m, const double* grad_dev, double dt, double* flux_dev,
                         double* ct_dev, void* hip_stream) {
  if (!m) return fail(-1, "null handle");
  if (int rc = take_dt(m, dt)) return rc;   // read by the rate-dependent laws only; QuadratureMap never forwards dt (quadrature_map.py:321)
  if (m->n > 0 && (!grad_dev || !flux_dev || !ct_dev)) return fail(-1, "null device pointer");
  DEVICE_GUARD(m);
  return launch(m, grad_dev, flux_dev, ct_dev, (hipStream_t)hip_stream);
}

int dxm_get_stats(dxm_material* m, dxm_stats* stats) {
  if (!m) return fail(-1, "null handle");
  dxm_stats s{};
  s.n_points = m->n;
  if (m->launched && m->last_grid > 0) {
    DEVICE_GUARD(m);
    if (int rc = sync_last(m)) return rc;
    if (!m->h_stats) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_stats), sizeof(BlockStats) * m->stats_capacity, hipHostMallocDefault));
    HIP_TRY(hipMemcpy(m->h_stats, m->d_stats, sizeof(BlockStats) * m->last_grid, hipMemcpyDeviceToHost));
    for (int k = 0; k < m->last_grid; ++k) {
      const BlockStats& b = m->h_stats[k];
      s.n_plastic += (int64_t)b.n_plastic;
      s.n_not_converged += (int64_t)b.n_not_converged;
      s.n_nan += (int64_t)b.n_nan;
      if ((int32_t)b.max_iters > s.max_local_iters) s.max_local_iters = (int32_t)b.max_iters;
    }
  }
  if (stats) *stats = s;
  if (s.n_not_converged > 0)
    return (int)(s.n_not_converged > 0x7fffffff ? 0x7fffffff : s.n_not_converged);
  return 0;
}

static int pack_isv_range(dxm_material* m, int which, int64_t off, int64_t cnt, double* isv_aos_dev,
                          hipStream_t st) {
  const LawDesc& d = kLaws[m->law];
  const int total = isv_total(d);
#ifndef DXM_CUSTOM_HARDENING
  if (total > (int)(sizeof(PackMap::slot) / sizeof(int))) {   // wider than the slot map: served where the visible fields are consecutive slots
    int next = d.isv_slot[0];
    for (int f = 0; f < d.n_isv_fields; ++f) {
      if (d.isv_slot[f] != next) return fail(-1, "internal: %d visible state numbers exceed the slot map and are not in consecutive slots", total);
      next += d.isv_dim[f];
    }
    pack_consecutive_slots(state_of(m, which) + off, m->ld, cnt, d.isv_slot[0], total, isv_aos_dev, st);
    HIP_TRY(hipGetLastError());
    return 0;
  }
#endif
  PackMap map{};
  map.n = total;
  int k = 0;
  for (int f = 0; f < d.n_isv_fields; ++f)
    for (int c = 0; c < d.isv_dim[f]; ++c) map.slot[k++] = d.isv_slot[f] + c;
  const int64_t work = cnt * total;
  const int blocks = (int)((work + 255) / 256);
  hipLaunchKernelGGL(pack_isv_kernel, dim3(blocks), dim3(256), 0, st, state_of(m, which) + off, m->ld,
                     cnt, isv_aos_dev, map);
  HIP_TRY(hipGetLastError());
  return 0;
}

// one user-visible field of s1 for the point range [off, off + cnt): AoS (cnt, dim) at dst_dev
static int pack_isv_field_range(dxm_material* m, int field, int64_t off, int64_t cnt, double* dst_dev, hipStream_t st) {
  const LawDesc& d = kLaws[m->law];
  PackMap map{};
  map.n = d.isv_dim[field];
  for (int c = 0; c < map.n; ++c) map.slot[c] = d.isv_slot[field] + c;
  const int blocks = (int)((cnt * map.n + 255) / 256);
  hipLaunchKernelGGL(pack_isv_kernel, dim3(blocks), dim3(256), 0, st, m->state[1] + off, m->ld, cnt, dst_dev, map);
  HIP_TRY(hipGetLastError());
  return 0;
}

int dxm_bind_isv_output(dxm_material* m, int field, double* host_aos) {
  if (!m) return fail(-1, "null handle");
  const LawDesc& d = kLaws[m->law];
  if (field < 0 || field >= d.n_isv_fields) return fail(-1, "state field %d out of range", field);
  if (host_aos && m->n > 0 && !page_locked(host_aos, sizeof(double) * m->n * d.isv_dim[field]))
    return fail(-1, "the array must be page-locked (dxm_host_alloc / dxm_host_register): it is written by DMA inside the chunk pipeline");
  m->isv_out[field] = host_aos;
  return 0;
}

int dxm_isv_device(dxm_material* m, int which, double* isv_aos_dev, void* hip_stream) {
  if (!m) return fail(-1, "null handle");
  if (which != DXM_S0 && which != DXM_S1) return fail(-1, "state selector must be DXM_S0 or DXM_S1");
  const LawDesc& d = kLaws[m->law];
  const int total = isv_total(d);
  if (total == 0 || m->n == 0) return 0;
  if (!isv_aos_dev) return fail(-1, "null device pointer");
  DEVICE_GUARD(m);
  return pack_isv_range(m, which, 0, m->n, isv_aos_dev, (hipStream_t)hip_stream);
}

static int ensure_host_path_buffers(dxm_material* m, bool need_grad = true) {
  const LawDesc& d = kLaws[m->law];
  const int64_t n = m->n;
  const int total = isv_total(d);
  if (need_grad && !m->d_grad) HIP_TRY(hipMalloc(&m->d_grad, sizeof(double) * n * d.n_grad));
  if (!m->d_flux) HIP_TRY(hipMalloc(&m->d_flux, sizeof(double) * n * d.n_flux));
  if (!m->d_ct) HIP_TRY(hipMalloc(&m->d_ct, sizeof(double) * n * ct_full_of(d)));  // sized for the full layout
  if (total > 0 && !m->d_isv) HIP_TRY(hipMalloc(&m->d_isv, sizeof(double) * n * total));
  return 0;
}

}  // extern "C"

// What a host-buffer call is asked to do (dxm_host::plan_transfer decides from it).  One pointer query per array; the rows forms
// land flux and tangent in the library's own page-locked areas and ask about neither.
static dxm_host::TransferRequest transfer_request(const dxm_material* m, const double* flux_aos, const double* isv_aos, const double* ct_aos,
                                                  bool staged_grad, bool fused, bool rows) {
  const LawDesc& d = kLaws[m->law];
  const int64_t n = m->n;
  dxm_host::TransferRequest r{};
  r.law = d.id; r.n_grad = d.n_grad; r.n_flux = d.n_flux; r.n_isv_fields = d.n_isv_fields;
  for (int f = 0; f < d.n_isv_fields; ++f) {
    r.isv_dim[f] = d.isv_dim[f];
    if (m->isv_out[f]) r.bound_fields |= 1u << f;
  }
  r.layout = m->tangent_layout; r.tangent_size = tangent_size(m); r.n = n;
  r.plain_blocks = d.n_blocks > 1;
  r.flux = flux_aos != nullptr; r.isv_aos = isv_aos != nullptr; r.ct = ct_aos != nullptr;
  r.rows = rows; r.staged_grad = staged_grad; r.fused = fused;
  const bool any = m->opt_pageable_dma;
  r.flux_locked = any || (!rows && page_locked(flux_aos, sizeof(double) * n * d.n_flux));
  r.isv_locked = any || page_locked(isv_aos, sizeof(double) * n * isv_total(d));
  r.ct_locked = any || (!rows && page_locked(ct_aos, sizeof(double) * n * r.tangent_size));
  r.packed_transfer = m->opt_packed_transfer; r.packed_min_points = m->opt_packed_min_points;
  r.split_streams = m->opt_split_streams; r.pipeline = m->opt_pipeline; r.max_chunks = m->opt_max_chunks;
  return r;
}

// The streams, page-locked landing areas, worker pool, events, staging ring and field scratch a plan names (the device arrays
// every call uses: ensure_host_path_buffers).  A regrown area is forgotten by the handle before it is freed: a failed free must
// not leave a pointer for dxm_destroy to free again.
static int ensure_plan_buffers(dxm_material* m, const dxm_host::TransferPlan& plan) {
  const LawDesc& d = kLaws[m->law];
  const int64_t n = m->n;
  const int total = isv_total(d);
  if (!m->pipe_stream) HIP_TRY(hipStreamCreateWithFlags(&m->pipe_stream, hipStreamNonBlocking));
  if (m->opt_split_streams && !m->down_stream2) HIP_TRY(hipStreamCreateWithFlags(&m->down_stream2, hipStreamNonBlocking));
  if (plan.need_pool) {
    if (plan.need_h_coef && m->h_coef_per_point < plan.land) {
      double* old = m->h_coef;
      m->h_coef = nullptr;
      m->h_coef_per_point = 0;
      if (old) HIP_TRY(hipHostFree(old));
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_coef), sizeof(double) * n * plan.land, hipHostMallocDefault));
      m->h_coef_per_point = plan.land;
    }
    if (plan.need_h_flux && !m->h_flux) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_flux), sizeof(double) * n * d.n_flux, hipHostMallocDefault));
    if (plan.need_h_isv && !m->h_isv) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_isv), sizeof(double) * n * total, hipHostMallocDefault));
    if (!m->pool || (int)m->pool->threads.size() != m->opt_host_threads) {
      delete m->pool;
      m->pool = new HostPool(m->opt_host_threads);
    }
    m->elastic_lm[0] = m->prm.lambda;
    m->elastic_lm[1] = m->prm.mu;
  }
  for (int c = 0; c < plan.chunks.nchunks; ++c) {
    if (!m->chunk_done[c]) HIP_TRY(hipEventCreateWithFlags(&m->chunk_done[c], hipEventDisableTiming));
    if (plan.split && !m->kernel_done[c]) HIP_TRY(hipEventCreateWithFlags(&m->kernel_done[c], hipEventDisableTiming));
  }
  if (plan.req.staged_grad) {
    const int64_t need = plan.chunks.csize * d.n_grad;
    if (m->ring_slot_doubles < need) {
      double* old = m->h_grad_ring;
      m->h_grad_ring = nullptr;
      m->ring_slot_doubles = 0;
      if (old) HIP_TRY(hipHostFree(old));
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->h_grad_ring), sizeof(double) * need * DXM_RING, hipHostMallocDefault));
      m->ring_slot_doubles = need;
    }
    for (hipEvent_t& e : m->ring_done) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (plan.fields_own_scratch && !m->d_isv_fields) HIP_TRY(hipMalloc(&m->d_isv_fields, sizeof(double) * n * total));
  return 0;
}

// Host-buffer form, shared by dxm_integrate and dxm_integrate_displacement.
//   upload(off, cnt, stream) enqueues whatever produces m->d_grad[off .. off+cnt) on `stream`.
// Large batches are cut into chunks (multiples of 256 points): the H2D and the kernel of chunk c+1 overlap the D2H of
// chunk c (PCIe is full duplex and the bytes coming back dominate).  Page-locked gradient arrays: up to 24 chunks, uploads +
// kernels on one stream, downloads on two others (option split_streams, see below); staged uploads and the displacement
// forms: up to 64 whole chunks alternating on two streams.  Each chunk is one launch over a point range; its block-stat
// records are appended after the previous chunk's.
//
// What crosses PCIe on the way back, per point: the flux (48 / 72 B), the tangent, and -- only when the
// caller passes a destination -- the internal state variables (they are consumed at advance(), not per
// Newton iteration: the Python layer fetches them on demand).  For the small-strain laws with the full
// (N, 6, 6) tangent requested, the kernel writes the 9 coefficients of the tangent instead of its 36
// entries, 72 instead of 288 B/point are moved into a page-locked landing area and worker threads rebuild
// the block in the caller's array chunk by chunk, behind the transfer of the following chunks
// (bit-identical to the full kernel; the elastic block is a constant and is only filled in).
// host_grad: the caller's gradient array when it is in ordinary (pageable) memory, else nullptr.  It is never handed
// to the runtime: worker threads copy chunk c into slot c % 8 of a page-locked ring and a small copy kernel moves it to
// HBM over PCIe (what the runtime's own pageable path does with its staging buffers; no DMA engine is shared with the
// downloads).
template <class Upload>
static int run_and_download(dxm_material* m, Upload upload, double* flux_aos, double* isv_aos,
                            double* ct_aos, dxm_stats* stats, const MeshSource* fused = nullptr,
                            const double* host_grad = nullptr, const int64_t* rows = nullptr) {
  const auto t_enter = std::chrono::steady_clock::now();
  const LawDesc& d = kLaws[m->law];
  const int64_t n = m->n;
  const int total = isv_total(d);
  const dxm_host::TransferRequest r = transfer_request(m, flux_aos, isv_aos, ct_aos, host_grad != nullptr, fused != nullptr, rows != nullptr);
  const dxm_host::TransferPlan plan = dxm_host::plan_transfer(r);
  const int nchunks = plan.chunks.nchunks;
  const int64_t csize = plan.chunks.csize;
  if (int rc = ensure_plan_buffers(m, plan)) return rc;
  double* const field_scratch = plan.fields_own_scratch ? m->d_isv_fields : m->d_isv;
  int stats_off = 0, issued = 0, submitted = 0;
  hipStream_t streams[2] = {m->own_stream, m->pipe_stream};
  // An early return (a failing HIP call part-way through the chunk loop) leaves kernels, ring copies and downloads of
  // the earlier chunks in flight on both streams, into the caller's arrays: wait for them before returning, so that the
  // caller may free or reuse its arrays, and leave the handle as after a launch whose completion is unknown.
  struct InFlight {
    dxm_material* m;
    bool completed = false;
    ~InFlight() {
      if (completed) return;
      (void)hipStreamSynchronize(m->own_stream);
      if (m->pipe_stream) (void)hipStreamSynchronize(m->pipe_stream);
      if (m->down_stream2) (void)hipStreamSynchronize(m->down_stream2);
      (void)hipGetLastError();
      m->launched = true;
      m->last_event_recorded = false;   // sync_last falls back to the whole device
      m->s1_alias = false;              // parts of s1 have been rewritten
      m->last_grid = 0;
    }
  } inflight{m};
  // no worker may still be writing into the caller's array when this function returns, error paths included
  struct PoolDrain {
    HostPool* p;
    ~PoolDrain() {
      if (!p) return;
      for (int t = 0; t < 64; ++t) p->wait_copy(t);   // staging copies still read the caller's gradient array
      p->wait();
    }
  } drain{plan.need_pool ? m->pool : nullptr};
  if (plan.ct == CtRoute::fill) m->pool->submit(m->elastic_lm, ct_aos, n, 0);   // nothing to wait for
  const dxm_host::ChunkTargets targets{flux_aos, ct_aos, m->h_coef, m->h_flux, m->h_isv, m->isv_out, rows, m->elastic_lm};
  // chunk p of the caller's pageable gradient array -> its ring slot, by the worker threads, asynchronously
  auto stage_chunk = [&](int p) -> int {
    const int64_t o = (int64_t)p * csize;
    if (!host_grad || p >= nchunks || o >= n) return 0;
    if (p >= DXM_RING) HIP_TRY(hipEventSynchronize(m->ring_done[dxm_host::ring_slot(p)]));   // the copy kernel of chunk p - DXM_RING has read this slot
    m->pool->copy_async(host_grad + o * d.n_grad, m->h_grad_ring + (int64_t)dxm_host::ring_slot(p) * m->ring_slot_doubles,
                        sizeof(double) * ((n - o) < csize ? (n - o) : csize) * d.n_grad, p);
    return 0;
  };
  double ms_wait_copy = 0.0, ms_first_copy = 0.0;   // option verbose: time the issue loop spent waiting for staging copies
  const int ahead = m->opt_stage_ahead;
  for (int p = 0; p < ahead; ++p) if (int rc = stage_chunk(p)) return rc;
  for (int c = 0; c < nchunks; ++c) {
    const int64_t off = plan.chunks.offset(c);
    if (off >= n) break;
    const int64_t cnt = plan.chunks.count(c, n);
    hipStream_t st = plan.split ? m->own_stream : streams[c & 1];                         // upload + kernels of this chunk
    hipStream_t sd = plan.split ? ((c & 1) ? m->down_stream2 : m->pipe_stream) : st;      // its downloads (split: two download streams take turns)
    if (int rc = upload(off, cnt, st)) return rc;
    const double* gptr = fused ? m->d_flux : m->d_grad + off * d.n_grad;
    if (host_grad) {
      const int slot = dxm_host::ring_slot(c);
      double* dst = m->h_grad_ring + (int64_t)slot * m->ring_slot_doubles;
      if (int rc = stage_chunk(c + ahead)) return rc;   // keep `ahead` chunks ahead of the launches
      {
        const auto tw = std::chrono::steady_clock::now();
        m->pool->wait_copy(c);
        const double w = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw).count();
        ms_wait_copy += w;
        if (c == 0) ms_first_copy = w;
      }
      // page-locked host memory is addressable from the device under the same pointer
      const int64_t n16 = cnt * d.n_grad / 2;      // cnt is a multiple of 256 except in the last chunk; n_grad 6 or 9:
      const int64_t tail = cnt * d.n_grad - 2 * n16;   // an odd count leaves one double for a plain copy
      // (on the chunk's own stream: a third stream carrying all uploads ahead of the kernels was measured at 46-62 ms per
      // 1e7 points against 31-33, profiles/archive/r03_hostpath_fresh_array.md)
      hipLaunchKernelGGL(ring_upload_kernel, dim3(32), dim3(256), 0, st, reinterpret_cast<const double2_t*>(dst),
                         reinterpret_cast<double2_t*>(m->d_grad + off * d.n_grad), n16);
      if (tail) HIP_TRY(hipMemcpyAsync(m->d_grad + off * d.n_grad + 2 * n16, dst + 2 * n16, sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(m->ring_done[slot], st));   // the slot is free once the copy kernel has read it
    }
    int grid = 0;
    MeshSource src{};
    if (fused) { src = *fused; src.point0 = off; }
    if (int rc = launch_range(m, off, cnt, gptr, m->d_flux + off * d.n_flux,
                              m->d_ct + off * plan.nt, st, stats_off, &grid, fused ? &src : nullptr, plan.tl))
      return rc;
    stats_off += grid;
    // device side of the chunk first (pack kernels of the internal state variables included), then its downloads (split: on
    // one of the two download streams, behind the chunk's kernel_done event)
    if (plan.isv != Route::none) {
      // the kernel wrote state[1]; s1_alias is cleared below, address it directly
      const bool alias = m->s1_alias;
      m->s1_alias = false;
      int rc = pack_isv_range(m, DXM_S1, off, cnt, m->d_isv + off * total, st);
      m->s1_alias = alias;
      if (rc) return rc;
    }
    // the bound state fields (dxm_bind_isv_output: the x.array of the ISV Functions), field after field
    for (int f = 0; f < d.n_isv_fields; ++f)
      if (m->isv_out[f])
        if (int rc = pack_isv_field_range(m, f, off, cnt, field_scratch + dxm_host::field_slice(r, f, off), st)) return rc;
    if (plan.split) {
      HIP_TRY(hipEventRecord(m->kernel_done[c], st));
      HIP_TRY(hipStreamWaitEvent(sd, m->kernel_done[c], 0));
    }
    if (plan.flux == Route::dma || plan.flux == Route::rows)
      HIP_TRY(hipMemcpyAsync((plan.flux == Route::rows ? m->h_flux : flux_aos) + off * d.n_flux, m->d_flux + off * d.n_flux,
                             sizeof(double) * cnt * d.n_flux, hipMemcpyDeviceToHost, sd));
    if (plan.ct == CtRoute::dma || plan.ct_lands()) {
      double* dst = plan.ct == CtRoute::dma ? ct_aos + off * plan.nt : m->h_coef + off * plan.np;
      HIP_TRY(hipMemcpyAsync(dst, m->d_ct + off * plan.nt, sizeof(double) * cnt * plan.nt, hipMemcpyDeviceToHost, sd));
    }
    if (plan.isv == Route::dma)
      HIP_TRY(hipMemcpyAsync(isv_aos + off * total, m->d_isv + off * total, sizeof(double) * cnt * total, hipMemcpyDeviceToHost, sd));
    for (int f = 0; f < d.n_isv_fields; ++f) {
      if (!m->isv_out[f]) continue;
      const int64_t at = dxm_host::field_slice(r, f, off);
      double* land = plan.fields == Route::rows ? m->h_isv + at : m->isv_out[f] + off * d.isv_dim[f];
      HIP_TRY(hipMemcpyAsync(land, field_scratch + at, sizeof(double) * cnt * d.isv_dim[f], hipMemcpyDeviceToHost, sd));
    }
    HIP_TRY(hipEventRecord(m->chunk_done[c], sd));
    issued = c + 1;
    // a pageable upload blocks this thread for its whole duration, so earlier chunks land while the later ones are
    // still being issued: hand them to the workers now, not after the loop
    if (plan.chunk_jobs)
      while (submitted < issued && hipEventQuery(m->chunk_done[submitted]) == hipSuccess) dxm_host::submit_chunk(*m->pool, plan, targets, submitted++);
  }
  (void)hipGetLastError();   // hipEventQuery reports "not ready" through the error state
  m->last_grid = stats_off;
  m->launched = true;
  m->s1_alias = false;  // every slot of s1 has been rewritten
  // the chunks complete in issue order on their streams; rebuild each block as soon as it has landed
  const auto t_issued = std::chrono::steady_clock::now();
  auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
  for (int c = 0; c < issued; ++c) {
    HIP_TRY(hipEventSynchronize(m->chunk_done[c]));
    if (m->opt_verbose && (c % 8 == 7 || c == 0)) fprintf(stderr, "[dxm host path] chunk %d landed at +%.2f ms after issue (issue loop took %.2f ms)\n", c, ms_since(t_issued), std::chrono::duration<double, std::milli>(t_issued - t_enter).count());
    if (plan.chunk_jobs && c >= submitted) {
      dxm_host::submit_chunk(*m->pool, plan, targets, c);
      submitted = c + 1;
    }
  }
  // destinations in ordinary (pageable) memory were left out above: they are filled through the page-locked staging now
  // (download_to_host; slower, and only a C caller that did not use dxm_host_alloc / dxm_host_register gets here)
  if (plan.flux == Route::staged)
    if (int rc = download_to_host(flux_aos, m->d_flux, sizeof(double) * n * d.n_flux, m->own_stream)) return rc;
  if (plan.isv == Route::staged)
    if (int rc = download_to_host(isv_aos, m->d_isv, sizeof(double) * n * total, m->own_stream)) return rc;
  if (plan.ct == CtRoute::staged)
    if (int rc = download_to_host(ct_aos, m->d_ct, sizeof(double) * n * plan.nt, m->own_stream)) return rc;
  HIP_TRY(hipEventRecord(m->last_event, m->own_stream));   // everything of this call is complete already
  m->last_event_recorded = true;
  const auto t_landed = std::chrono::steady_clock::now();
  if (plan.packed) m->pool->wait();
  if (m->opt_verbose && host_grad) fprintf(stderr, "[dxm host path] %d chunks of %lld points; issue loop waited %.2f ms for staging copies (first chunk %.2f ms)\n", nchunks, (long long)csize, ms_wait_copy, ms_first_copy);
  if (m->opt_verbose) fprintf(stderr, "[dxm host path] all landed at +%.2f ms, workers done %.2f ms later\n", std::chrono::duration<double, std::milli>(t_landed - t_issued).count(), ms_since(t_landed));
  inflight.completed = true;
  m->io1_valid = (fused ? 0 : 1) | 2;   // d_grad (unless the strain never existed as an array) and d_flux are those of s1
  const auto t_stats = std::chrono::steady_clock::now();
  const int rc_stats = dxm_get_stats(m, stats);
  if (stats) stats->upload = host_grad ? DXM_UPLOAD_STAGED : m->last_upload;
  if (m->opt_verbose) fprintf(stderr, "[dxm host path] status records summed in %.3f ms; %.2f ms since entry\n", ms_since(t_stats), ms_since(t_enter));
  return rc_stats;
}

extern "C" {

// upload_choice: 0 = this call had no choice to make (page-locked input, small batch, option off), else the way the pageable
// gradient array went up (1 page-locked for the call + DMA, 2 staged by the worker threads); see integrate_host below
static int integrate_host_impl(dxm_material* m, const double* grad_aos, double* flux_aos, double* isv_aos, double* ct_aos,
                               dxm_stats* stats, const int64_t* rows, int* upload_choice) {
  const LawDesc& d = kLaws[m->law];
  const int64_t n = m->n;
  DEVICE_GUARD(m);
  // a page-locked gradient array is uploaded by DMA; so is a pageable one if the caller asked for it (option pageable_dma)
  const auto t_in = std::chrono::steady_clock::now();
  bool locked_in = m->opt_pageable_dma || page_locked(grad_aos, sizeof(double) * n * d.n_grad);
  // An array in ordinary memory is page-locked HERE, for the duration of this call, and uploaded by DMA like a page-locked
  // one: registering a 480 MB array takes ~1 ms (profiles/archive/r03_hostpath_register.md) where staging it through the ring
  // costs the worker threads 5-10 ms of a 24 ms call.  This is not the runtime's implicit path for pageable memory (whose
  // cache of on-the-fly mappings outlives the caller's array: DESIGN.md section 1): the range is unregistered before this
  // function returns, error paths included, while the caller still owns the array.  A refusal (a range that overlaps a
  // registered one, memory that cannot be pinned) falls back to the staging ring.
  struct TempRegistration {
    void* p = nullptr;
    dxm_material* m = nullptr;
    ~TempRegistration() {
      if (!p) return;
      const auto t0 = std::chrono::steady_clock::now();
      forget_locked(p);
      (void)hipHostUnregister(p);
      (void)hipGetLastError();
      m->unregister_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (m->opt_verbose) fprintf(stderr, "[dxm host path] releasing the page-lock of the gradient array took %.3f ms\n", m->unregister_ms);
    }
  } temp;
  temp.m = m;
  if (!locked_in && (size_t)n * d.n_grad * sizeof(double) >= ((size_t)1 << 20)) {
    // Which of the two is faster depends on the host (where the caller's pages sit relative to the GPU, what else runs on the
    // machine): the handle measures it (dxm_host::UploadChooser, option register_input).
    const int way = m->up.choose();   // 0: option off, 1: page-lock for the call, 2: stage through the ring
    *upload_choice = way;
    if (way == 1) {
      void* p = const_cast<double*>(grad_aos);
      const size_t bytes = sizeof(double) * n * d.n_grad;
      const auto t0 = std::chrono::steady_clock::now();
      if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) {
        temp.p = p;
        locked_in = true;
        // 0.9 ms per 480 MB on transparent huge pages (what numpy asks for), 7-17 ms on 4 KiB pages, where the whole call
        // then takes 43 instead of 28 ms: such arrays go through the staging ring for the next 20 calls, then one more try
        const double ms_lock = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (m->opt_verbose) fprintf(stderr, "[dxm host path] page-locking the gradient array took %.3f ms (releasing it after the previous call: %.3f ms)\n", ms_lock, m->unregister_ms);
        m->up.registered(ms_lock + m->unregister_ms, bytes);   // what the previous call paid to release its range counts too
      } else {
        (void)hipGetLastError();
        m->up.refused();
        *upload_choice = 2;
      }
    }
  }
  m->last_upload = m->opt_pageable_dma ? DXM_UPLOAD_RUNTIME : (temp.p ? DXM_UPLOAD_REGISTERED : (locked_in ? DXM_UPLOAD_PAGE_LOCKED : DXM_UPLOAD_STAGED));
  const auto t_q = std::chrono::steady_clock::now();
  if (int rc = ensure_host_path_buffers(m)) return rc;
  if (int rc = sync_last(m)) return rc;
  if (m->opt_verbose)
    fprintf(stderr, "[dxm host path] classifying the gradient pointer took %.3f ms, buffers + wait for the previous call %.3f ms\n",
            std::chrono::duration<double, std::milli>(t_q - t_in).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_q).count());
  const int ng = d.n_grad;
  auto upload = [&](int64_t off, int64_t cnt, hipStream_t st) -> int {
    if (locked_in)
      HIP_TRY(hipMemcpyAsync(m->d_grad + off * ng, grad_aos + off * ng, sizeof(double) * cnt * ng,
                             hipMemcpyHostToDevice, st));
    return 0;
  };
  return run_and_download(m, upload, flux_aos, isv_aos, ct_aos, stats, nullptr, locked_in ? nullptr : grad_aos, rows);
}

static int integrate_host(dxm_material* m, const double* grad_aos, double* flux_aos, double* isv_aos, double* ct_aos,
                          dxm_stats* stats, const int64_t* rows) {
  if (!m) return fail(-1, "null handle");
  if (m->n == 0) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return 0;
  }
  if (!grad_aos) return fail(-1, "null gradient pointer");
  int way = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = integrate_host_impl(m, grad_aos, flux_aos, isv_aos, ct_aos, stats, rows, &way);
  if (rc < 0) return rc;
  // the adaptive choice between page-locking the caller's gradient array for the call and staging it (see above)
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const bool changed = m->up.record(way, ms);
  if (m->opt_verbose && way && m->up.opt == 1 && (changed || m->up.calls == 5))
    fprintf(stderr, "[dxm host path] gradient upload: page-locked for the call %.2f ms, staged %.2f ms per call -> %s\n",
            m->up.ms[1], m->up.ms[2], m->up.pref == 1 ? "page-locking" : "staging");
  return rc;
}

int dxm_integrate(dxm_material* m, const double* grad_aos, double dt, double* flux_aos,
                  double* isv_aos, double* ct_aos, dxm_stats* stats) {
  if (int rc = take_dt(m, dt)) return rc;
  return integrate_host(m, grad_aos, flux_aos, isv_aos, ct_aos, stats, nullptr);
}

int dxm_integrate_rows(dxm_material* m, const double* grad_aos, double dt, double* flux_rows, double* ct_rows,
                       const int64_t* rows, dxm_stats* stats) {
  if (!m) return fail(-1, "null handle");
  if (int rc = take_dt(m, dt)) return rc;
  if (m->n > 0 && (!flux_rows || !ct_rows || !rows)) return fail(-1, "dxm_integrate_rows needs the flux array, the tangent array and the row index");
  return integrate_host(m, grad_aos, flux_rows, nullptr, ct_rows, stats, rows);
}

void* dxm_host_alloc(uint64_t bytes) {
  void* p = nullptr;
  if (bytes == 0) bytes = 8;
  hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    fail(-3, "hipHostMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
    return nullptr;
  }
  note_locked(p, bytes);
  return p;
}

int dxm_host_free(void* p) {
  if (p) {
    RelaxedCaptureMode relaxed;
    forget_locked(p);
    HIP_TRY(hipHostFree(p));
  }
  return 0;
}

// ---- gradient evaluation on device ----------------------------------------------------------
struct dxm_mesh {
  int nodes_per_cell = 8;   // 8: trilinear hexahedron, 4: linear tetrahedron, 0: Lagrange simplex (fields below)
  int device = 0;
  int64_t n_nodes = 0, n_cells = 0;
  int64_t u_len = 0;        // doubles in the displacement vector (3 per node; tdim per dof for a Lagrange simplex)
  QuadPoints qp{};
  double* d_coords = nullptr;
  int32_t* d_conn = nullptr;
  double* d_u = nullptr;
  hipEvent_t grad_done = nullptr;
  // Lagrange simplex: geometry through d_conn (tdim + 1 vertices per cell), displacement through its own dofmap
  int tdim = 3, nd = 0;
  int64_t n_dofs = 0;
  int32_t* d_dofmap = nullptr;
  double* d_dphi = nullptr;
  // two-dimensional meshes (tdim 2): what plane_gradient.hip reads.  geom_nv vertices per cell in d_conn and the reference derivatives
  // of the geometry's shape functions at the Gauss points, (nqp, geom_nv, 2): the caller's for dxm_mesh_create_plane, the constant
  // table of the affine triangle for dxm_mesh_create_simplex.  plane: made by dxm_mesh_create_plane (no in-kernel gradient form)
  int geom_nv = 0;
  double* d_gdphi = nullptr;
  bool plane = false;
  // a SCALAR field on a plane mesh (dxm_mesh_create_plane_scalar): one value per dof, and the values of the field's shape functions
  // at the Gauss points, (nqp, nd), beside their derivatives.  Read by heat_plane.hip only: every kind of dxm_mesh_gradient_device refuses
  bool scalar = false;
  double* d_phi = nullptr;
  // a meridian mesh (dxm_mesh_create_axisymmetric): column 0 of the coordinates is r, column 1 is z.  A displacement mesh with the
  // value tables of the field (d_phi) and of the geometry (d_gphi, (nqp, geom_nv)) beside the derivative tables: what
  // axisym_gradient.hip reads for the hoop term u_r / r.  Every kind of dxm_mesh_gradient_device refuses
  bool axisym = false;
  double* d_gphi = nullptr;
};

// triangles through dxm_mesh_create_simplex, triangles and quadrilaterals through dxm_mesh_create_plane
static bool mesh_2d(const dxm_mesh* mesh) { return mesh->nodes_per_cell == 0 && mesh->tdim == 2; }

static dxm_mesh* mesh_create(int npc, const double* coords, int64_t n_nodes, const int32_t* conn,
                             int64_t n_cells, const double* qpoints, int nqp, int device) {
  if (!coords || !conn || n_nodes <= 0 || n_cells <= 0 || nqp <= 0 || nqp > 27 || (npc == 8 && !qpoints)) {
    fail(-1, "invalid mesh arguments");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    fail(-2, "no usable HIP device %d (libdxmat has no CPU fallback)", device);
    return nullptr;
  }
  for (int64_t k = 0; k < n_cells * npc; ++k)
    if (conn[k] < 0 || conn[k] >= n_nodes) { fail(-1, "connectivity entry %lld out of range", (long long)k); return nullptr; }
  dxm_mesh* mesh = new dxm_mesh();
  mesh->nodes_per_cell = npc;
  mesh->device = device;
  mesh->n_nodes = n_nodes;
  mesh->n_cells = n_cells;
  mesh->u_len = 3 * n_nodes;
  mesh->qp.nqp = nqp;
  if (qpoints)
    for (int q = 0; q < nqp; ++q)
      for (int d = 0; d < 3; ++d) mesh->qp.xi[q][d] = qpoints[3 * q + d];
  DeviceGuard guard(device);
  bool ok = guard.ok;
  ok = ok && hipMalloc(&mesh->d_coords, sizeof(double) * 3 * n_nodes) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_conn, sizeof(int32_t) * npc * n_cells) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_u, sizeof(double) * 3 * n_nodes) == hipSuccess;
  ok = ok && upload_from_host(mesh->d_coords, coords, sizeof(double) * 3 * n_nodes, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_conn, conn, sizeof(int32_t) * npc * n_cells, nullptr) == 0;
  if (!ok) {
    fail(-3, "device allocation / upload of the mesh failed");
    dxm_mesh_destroy(mesh);
    return nullptr;
  }
  return mesh;
}

dxm_mesh* dxm_mesh_create_hex8(const double* coords, int64_t n_nodes, const int32_t* conn,
                               int64_t n_cells, const double* qpoints, int nqp, int device) {
  return mesh_create(8, coords, n_nodes, conn, n_cells, qpoints, nqp, device);
}

dxm_mesh* dxm_mesh_create_tet4(const double* coords, int64_t n_nodes, const int32_t* conn,
                               int64_t n_cells, int nqp, int device) {
  return mesh_create(4, coords, n_nodes, conn, n_cells, nullptr, nqp, device);
}

dxm_mesh* dxm_mesh_create_simplex(int tdim, const double* coords, int64_t n_vertices, const int32_t* geom_conn,
                                  int64_t n_cells, const int32_t* dofmap, int nd, int64_t n_dofs,
                                  const double* dphi, int nqp, int device) {
  if ((tdim != 2 && tdim != 3) || !coords || !geom_conn || !dofmap || !dphi || n_vertices <= 0 || n_cells <= 0 ||
      nd < tdim + 1 || nd > 64 || n_dofs <= 0 || nqp <= 0 || nqp > 64) {
    fail(-1, "invalid simplex mesh arguments");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    fail(-2, "no usable HIP device %d (libdxmat has no CPU fallback)", device);
    return nullptr;
  }
  const int nv = tdim + 1;
  for (int64_t k = 0; k < n_cells * nv; ++k)
    if (geom_conn[k] < 0 || geom_conn[k] >= n_vertices) { fail(-1, "geometry connectivity entry %lld out of range", (long long)k); return nullptr; }
  for (int64_t k = 0; k < n_cells * nd; ++k)
    if (dofmap[k] < 0 || dofmap[k] >= n_dofs) { fail(-1, "dofmap entry %lld out of range", (long long)k); return nullptr; }
  // a flat or inverted reference map would put Inf / NaN into every gradient of the cell
  for (int64_t c = 0; c < n_cells; ++c) {
    const double* X0 = coords + 3 * (int64_t)geom_conn[c * nv];
    double A[9];
    for (int d = 0; d < tdim; ++d) {
      const double* Xd = coords + 3 * (int64_t)geom_conn[c * nv + d + 1];
      for (int a = 0; a < tdim; ++a) A[a * 3 + d] = Xd[a] - X0[a];
    }
    const double det = tdim == 2 ? A[0] * A[4] - A[1] * A[3]
                                 : A[0] * (A[4] * A[8] - A[5] * A[7]) + A[1] * (A[5] * A[6] - A[3] * A[8]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (!(det != 0.0) || !std::isfinite(det)) { fail(-1, "cell %lld is degenerate (zero volume)", (long long)c); return nullptr; }
  }
  dxm_mesh* mesh = new dxm_mesh();
  mesh->nodes_per_cell = 0;
  mesh->device = device;
  mesh->n_nodes = n_vertices;
  mesh->n_cells = n_cells;
  mesh->qp.nqp = nqp;
  mesh->tdim = tdim;
  mesh->nd = nd;
  mesh->n_dofs = n_dofs;
  mesh->u_len = (int64_t)tdim * n_dofs;
  DeviceGuard guard(device);
  bool ok = guard.ok;
  ok = ok && hipMalloc(&mesh->d_coords, sizeof(double) * 3 * n_vertices) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_conn, sizeof(int32_t) * nv * n_cells) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_dofmap, sizeof(int32_t) * nd * n_cells) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_dphi, sizeof(double) * nqp * nd * tdim) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_u, sizeof(double) * mesh->u_len) == hipSuccess;
  ok = ok && upload_from_host(mesh->d_coords, coords, sizeof(double) * 3 * n_vertices, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_conn, geom_conn, sizeof(int32_t) * nv * n_cells, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_dofmap, dofmap, sizeof(int32_t) * nd * n_cells, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_dphi, dphi, sizeof(double) * nqp * nd * tdim, nullptr) == 0;
  if (tdim == 2) {   // kinds 2 and 3 run through plane_gradient.hip: the affine triangle's table, the same at every point
    std::vector<double> gd((size_t)nqp * 6);
    for (int q = 0; q < nqp; ++q) {
      const double t[6] = {-1.0, -1.0, 1.0, 0.0, 0.0, 1.0};
      std::copy(t, t + 6, gd.begin() + 6 * q);
    }
    mesh->geom_nv = 3;
    ok = ok && hipMalloc(&mesh->d_gdphi, sizeof(double) * gd.size()) == hipSuccess;
    ok = ok && upload_from_host(mesh->d_gdphi, gd.data(), sizeof(double) * gd.size(), nullptr) == 0;
  }
  if (!ok) {
    fail(-3, "device allocation / upload of the mesh failed");
    dxm_mesh_destroy(mesh);
    return nullptr;
  }
  return mesh;
}

// dxm_mesh_create_plane (components 2, phi null), dxm_mesh_create_plane_scalar (components 1, with the value table phi) and
// dxm_mesh_create_axisymmetric (components 2, axisym: with the value tables phi and geom_phi)
static dxm_mesh* plane_mesh_create(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                   const int32_t* dofmap, int nd, int64_t n_dofs, const double* geom_dphi, const double* phi,
                                   const double* dphi, int nqp, int device, int components, bool axisym = false,
                                   const double* geom_phi = nullptr) {
  const bool scalar = components == 1;
  // every check runs on the host before a device is asked for: the kernels are never launched on indices that were not checked
  if (nv != 3 && nv != 4) {
    fail(-1, "a plane mesh has nv = 3 (triangles) or nv = 4 (bilinear quadrilaterals) vertices per cell, not %d", nv);
    return nullptr;
  }
  if (!coords || !geom_conn || !dofmap || !geom_dphi || !dphi || (scalar && !phi) || (axisym && (!phi || !geom_phi)) || n_vertices <= 0 || n_cells <= 0 || nd < nv ||
      nd > PLANE_GRAD_MAX_ND || n_dofs <= 0 || nqp <= 0 || nqp > PLANE_GRAD_MAX_NQP) {
    fail(-1, "invalid plane mesh arguments");
    return nullptr;
  }
  if (scalar) {   // a NaN in a table would reach every point: the values, then the field's derivatives, then the geometry's
    const struct { const char* name; const double* tab; int64_t len; } tabs[3] = {
        {"phi", phi, (int64_t)nqp * nd}, {"dphi", dphi, (int64_t)nqp * nd * 2}, {"geom_dphi", geom_dphi, (int64_t)nqp * nv * 2}};
    for (const auto& t : tabs)
      for (int64_t k = 0; k < t.len; ++k)
        if (!std::isfinite(t.tab[k])) { fail(-1, "table %s: entry %lld is not finite", t.name, (long long)k); return nullptr; }
  }
  for (int64_t k = 0; k < n_cells * nv; ++k)
    if (geom_conn[k] < 0 || geom_conn[k] >= n_vertices) { fail(-1, "geometry connectivity entry %lld out of range", (long long)k); return nullptr; }
  for (int64_t k = 0; k < n_cells * nd; ++k)
    if (dofmap[k] < 0 || dofmap[k] >= n_dofs) { fail(-1, "dofmap entry %lld out of range", (long long)k); return nullptr; }
  // det J at every Gauss point: zero or not finite puts Inf / NaN into the gradient, a change of sign within a cell is a cell that
  // folds over (a bow-tie quadrilateral).  One sign per cell, not per mesh: the cells of a dolfinx mesh are numbered either way round
  for (int64_t c = 0; c < n_cells; ++c) {
    double sign = 0.0;
    for (int q = 0; q < nqp; ++q) {
      double J[4] = {0.0, 0.0, 0.0, 0.0};
      for (int v = 0; v < nv; ++v) {
        const double* X = coords + 3 * (int64_t)geom_conn[c * nv + v];
        const double* t = geom_dphi + ((int64_t)q * nv + v) * 2;
        J[0] += X[0] * t[0]; J[1] += X[0] * t[1];
        J[2] += X[1] * t[0]; J[3] += X[1] * t[1];
      }
      const double det = J[0] * J[3] - J[1] * J[2];
      if (!(det != 0.0) || !std::isfinite(det)) {
        fail(-1, "cell %lld is degenerate: det J is zero or not finite at Gauss point %d", (long long)c, q);
        return nullptr;
      }
      if (sign == 0.0) sign = det;
      if ((det > 0.0) != (sign > 0.0)) {
        fail(-1, "cell %lld is folded over (a bow-tie quadrilateral?): det J changes sign at Gauss point %d", (long long)c, q);
        return nullptr;
      }
    }
  }
  if (axisym) {   // after det J: a NaN in a table would reach every point; then r at every Gauss point, the divisor of the hoop term
    const struct { const char* name; const double* tab; int64_t len; } tabs[4] = {
        {"phi", phi, (int64_t)nqp * nd}, {"dphi", dphi, (int64_t)nqp * nd * 2}, {"geom_phi", geom_phi, (int64_t)nqp * nv},
        {"geom_dphi", geom_dphi, (int64_t)nqp * nv * 2}};
    for (const auto& t : tabs)
      for (int64_t k = 0; k < t.len; ++k)
        if (!std::isfinite(t.tab[k])) { fail(-1, "table %s: entry %lld is not finite", t.name, (long long)k); return nullptr; }
    for (int64_t c = 0; c < n_cells; ++c)
      for (int q = 0; q < nqp; ++q) {
        double rad = 0.0;
        for (int v = 0; v < nv; ++v) rad += coords[3 * (int64_t)geom_conn[c * nv + v]] * geom_phi[(int64_t)q * nv + v];
        if (!(rad > 0.0) || !std::isfinite(rad)) {
          fail(-1, "cell %lld: r = %g at Gauss point %d: an axisymmetric mesh lies on one side of the axis (r > 0 at every Gauss "
                   "point), with no Gauss point on it", (long long)c, rad, q);
          return nullptr;
        }
      }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    fail(-2, "no usable HIP device %d (libdxmat has no CPU fallback)", device);
    return nullptr;
  }
  dxm_mesh* mesh = new dxm_mesh();
  mesh->nodes_per_cell = 0;
  mesh->plane = true;
  mesh->scalar = scalar;
  mesh->axisym = axisym;
  mesh->device = device;
  mesh->n_nodes = n_vertices;
  mesh->n_cells = n_cells;
  mesh->qp.nqp = nqp;
  mesh->tdim = 2;
  mesh->nd = nd;
  mesh->geom_nv = nv;
  mesh->n_dofs = n_dofs;
  mesh->u_len = components * n_dofs;
  DeviceGuard guard(device);
  bool ok = guard.ok;
  ok = ok && hipMalloc(&mesh->d_coords, sizeof(double) * 3 * n_vertices) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_conn, sizeof(int32_t) * nv * n_cells) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_dofmap, sizeof(int32_t) * nd * n_cells) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_gdphi, sizeof(double) * nqp * nv * 2) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_dphi, sizeof(double) * nqp * nd * 2) == hipSuccess;
  ok = ok && hipMalloc(&mesh->d_u, sizeof(double) * mesh->u_len) == hipSuccess;
  ok = ok && upload_from_host(mesh->d_coords, coords, sizeof(double) * 3 * n_vertices, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_conn, geom_conn, sizeof(int32_t) * nv * n_cells, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_dofmap, dofmap, sizeof(int32_t) * nd * n_cells, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_gdphi, geom_dphi, sizeof(double) * nqp * nv * 2, nullptr) == 0;
  ok = ok && upload_from_host(mesh->d_dphi, dphi, sizeof(double) * nqp * nd * 2, nullptr) == 0;
  if (scalar || axisym) {
    ok = ok && hipMalloc(&mesh->d_phi, sizeof(double) * nqp * nd) == hipSuccess;
    ok = ok && upload_from_host(mesh->d_phi, phi, sizeof(double) * nqp * nd, nullptr) == 0;
  }
  if (axisym) {
    ok = ok && hipMalloc(&mesh->d_gphi, sizeof(double) * nqp * nv) == hipSuccess;
    ok = ok && upload_from_host(mesh->d_gphi, geom_phi, sizeof(double) * nqp * nv, nullptr) == 0;
  }
  if (!ok) {
    fail(-3, "device allocation / upload of the mesh failed");
    dxm_mesh_destroy(mesh);
    return nullptr;
  }
  return mesh;
}

dxm_mesh* dxm_mesh_create_plane(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                const int32_t* dofmap, int nd, int64_t n_dofs, const double* geom_dphi, const double* dphi, int nqp,
                                int device) {
  return plane_mesh_create(coords, n_vertices, geom_conn, nv, n_cells, dofmap, nd, n_dofs, geom_dphi, nullptr, dphi, nqp, device, 2);
}

dxm_mesh* dxm_mesh_create_plane_scalar(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                       const int32_t* dofmap, int nd, int64_t n_dofs, const double* geom_dphi, const double* phi,
                                       const double* dphi, int nqp, int device) {
  return plane_mesh_create(coords, n_vertices, geom_conn, nv, n_cells, dofmap, nd, n_dofs, geom_dphi, phi, dphi, nqp, device, 1);
}

dxm_mesh* dxm_mesh_create_axisymmetric(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                       const int32_t* dofmap, int nd, int64_t n_dofs, const double* geom_phi, const double* geom_dphi,
                                       const double* phi, const double* dphi, int nqp, int device) {
  return plane_mesh_create(coords, n_vertices, geom_conn, nv, n_cells, dofmap, nd, n_dofs, geom_dphi, phi, dphi, nqp, device, 2, true,
                           geom_phi);
}

int dxm_mesh_destroy(dxm_mesh* mesh) {
  if (!mesh) return 0;
  RelaxedCaptureMode relaxed;
  DeviceGuard guard(mesh->device);
  if (mesh->d_coords) (void)hipFree(mesh->d_coords);
  if (mesh->d_conn) (void)hipFree(mesh->d_conn);
  if (mesh->d_u) (void)hipFree(mesh->d_u);
  if (mesh->d_dofmap) (void)hipFree(mesh->d_dofmap);
  if (mesh->d_dphi) (void)hipFree(mesh->d_dphi);
  if (mesh->d_gdphi) (void)hipFree(mesh->d_gdphi);
  if (mesh->d_phi) (void)hipFree(mesh->d_phi);
  if (mesh->d_gphi) (void)hipFree(mesh->d_gphi);
  if (mesh->grad_done) (void)hipEventDestroy(mesh->grad_done);
  delete mesh;
  return 0;
}

int64_t dxm_mesh_npoints(const dxm_mesh* mesh) { return mesh ? mesh->n_cells * mesh->qp.nqp : -1; }
int64_t dxm_mesh_displacement_size(const dxm_mesh* mesh) { return mesh ? mesh->u_len : -1; }

static MeshSource mesh_source(const dxm_mesh* mesh, const double* u_dev);

int dxm_mesh_gradient_device(dxm_mesh* mesh, const double* u_dev, int kind, double* grad_dev,
                             void* hip_stream) {
  if (!mesh || !u_dev || !grad_dev) return fail(-1, "null argument");
  if (mesh->scalar)
    return fail(-1, "a scalar mesh (dxm_mesh_create_plane_scalar) holds one value per dof, not a displacement: it has no strain or "
                    "deformation gradient of any kind; dxm_mesh_scalar_gradient_device evaluates grad(T) and T on it");
  if (mesh->axisym)
    return fail(-1, "an axisymmetric mesh (dxm_mesh_create_axisymmetric) has a hoop term u_r / r in every strain and deformation "
                    "gradient, which none of these kinds holds: dxm_mesh_axisymmetric_gradient_device evaluates its four kinds");
  if (kind < 0 || kind > 3)
    return fail(-1, "gradient kind must be 0 (strain), 1 (F), 2 (plane-strain 4-vector) or 3 (in-plane 3-vector)");
  if (kind >= 2 && !mesh_2d(mesh))
    return fail(-1, "gradient kinds 2 (plane-strain 4-vector) and 3 (in-plane 3-vector) are evaluated on two-dimensional meshes only "
                    "(dxm_mesh_create_plane, dxm_mesh_create_simplex with tdim 2): this mesh is three-dimensional");
  DEVICE_GUARD(mesh);
  const int64_t npts = mesh->n_cells * mesh->qp.nqp;
  const int blocks = (int)((npts + 255) / 256);
  hipStream_t st = (hipStream_t)hip_stream;
  if (mesh->plane || kind >= 2) {   // plane_gradient.hip: every kind on a plane mesh, kinds 2 and 3 on triangles of either constructor
#ifdef DXM_CUSTOM_HARDENING
    return fail(-1, "the plane gradient kernels (a mesh of dxm_mesh_create_plane; gradient kinds 2 and 3) are served by the stock "
                    "libdxmat, not by a custom-hardening build, which is dxmat.hip alone");
#else
    HIP_TRY(plane_gradient_launch(kind, st, mesh->d_coords, mesh->d_conn, mesh->geom_nv, mesh->d_dofmap, mesh->nd, mesh->d_gdphi,
                                  mesh->d_dphi, mesh->qp.nqp, mesh->n_cells, u_dev, grad_dev));
#endif
  } else if (mesh->nodes_per_cell == 0) {
    const MeshSource src = mesh_source(mesh, u_dev);
    if (kind == 0) hipLaunchKernelGGL(simplex_gradient_kernel<0>, dim3(blocks), dim3(256), 0, st, src, grad_dev);
    else hipLaunchKernelGGL(simplex_gradient_kernel<1>, dim3(blocks), dim3(256), 0, st, src, grad_dev);
  } else if (mesh->nodes_per_cell == 4) {
    if (kind == 0)
      hipLaunchKernelGGL(tet4_gradient_kernel<0>, dim3(blocks), dim3(256), 0, st, mesh->d_coords, mesh->d_conn,
                         u_dev, mesh->n_cells, mesh->qp.nqp, grad_dev);
    else
      hipLaunchKernelGGL(tet4_gradient_kernel<1>, dim3(blocks), dim3(256), 0, st, mesh->d_coords, mesh->d_conn,
                         u_dev, mesh->n_cells, mesh->qp.nqp, grad_dev);
  } else if (mesh->qp.nqp >= 4) {   // nodal data staged through LDS once per cell
    if (kind == 0)
      hipLaunchKernelGGL(hex8_gradient_staged_kernel<0>, dim3(blocks), dim3(256), 0, st, mesh->d_coords, mesh->d_conn,
                         u_dev, mesh->n_cells, mesh->qp, grad_dev);
    else
      hipLaunchKernelGGL(hex8_gradient_staged_kernel<1>, dim3(blocks), dim3(256), 0, st, mesh->d_coords, mesh->d_conn,
                         u_dev, mesh->n_cells, mesh->qp, grad_dev);
  } else if (kind == 0) {
    hipLaunchKernelGGL(hex8_gradient_kernel<0>, dim3(blocks), dim3(256), 0, st, mesh->d_coords, mesh->d_conn,
                       u_dev, mesh->n_cells, mesh->qp, grad_dev);
  } else {
    hipLaunchKernelGGL(hex8_gradient_kernel<1>, dim3(blocks), dim3(256), 0, st, mesh->d_coords, mesh->d_conn,
                       u_dev, mesh->n_cells, mesh->qp, grad_dev);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// kind of in-kernel gradient evaluation this mesh allows: 1 hex8 x 8 points, 2 tet4, 3 Lagrange simplex, 0 none (a plane mesh: its
// gradient kernel runs on its own)
static int fused_kind(const dxm_mesh* mesh) {
  if (mesh->plane) return 0;
  if (mesh->nodes_per_cell == 8) return mesh->qp.nqp == 8 ? 1 : 0;
  if (mesh->nodes_per_cell == 0) return 3;
  return mesh->nodes_per_cell == 4 ? 2 : 0;
}
static MeshSource mesh_source(const dxm_mesh* mesh, const double* u_dev) {
  MeshSource src{};
  src.coords = mesh->d_coords; src.conn = mesh->d_conn; src.u = u_dev; src.ncells = mesh->n_cells; src.point0 = 0;
  src.kind = fused_kind(mesh); src.nqp = mesh->qp.nqp;
  src.dofmap = mesh->d_dofmap; src.dphi = mesh->d_dphi; src.nd = mesh->nd; src.tdim = mesh->tdim;
  if (src.kind == 1)
    for (int q = 0; q < 8; ++q)
      for (int a = 0; a < 3; ++a) src.xi[q][a] = mesh->qp.xi[q][a];
  return src;
}
static bool fusable(const dxm_mesh* mesh) { return fused_kind(mesh) != 0; }

// ---- a scalar field on a plane mesh: grad(T) and T at the Gauss points, and the nodal forms of the laws that read them ----------
#ifndef DXM_CUSTOM_HARDENING
static ScalarSource scalar_source(const dxm_mesh* mesh, const double* t_dev) {
  ScalarSource s{};
  s.coords = mesh->d_coords; s.conn = mesh->d_conn; s.dofmap = mesh->d_dofmap; s.gdphi = mesh->d_gdphi; s.phi = mesh->d_phi;
  s.dphi = mesh->d_dphi; s.t = t_dev; s.point0 = 0; s.nqp = mesh->qp.nqp; s.nv = mesh->geom_nv; s.nd = mesh->nd;
  return s;
}
#endif

int dxm_mesh_scalar_gradient_device(dxm_mesh* mesh, const double* t_dev, double* grad_dev, double* value_dev, void* hip_stream) {
  if (!mesh || !t_dev || !grad_dev) return fail(-1, "null argument");
  if (!mesh->scalar)
    return fail(-1, "dxm_mesh_scalar_gradient_device needs a scalar mesh (dxm_mesh_create_plane_scalar): this mesh carries a "
                    "displacement, whose gradients dxm_mesh_gradient_device evaluates");
  if ((uintptr_t)grad_dev & 15) return fail(-1, "the gradient device array must be 16-byte aligned");
#ifdef DXM_CUSTOM_HARDENING
  return fail(-1, "the scalar gradient kernel (a mesh of dxm_mesh_create_plane_scalar) is served by the stock libdxmat, not by a "
                  "custom-hardening build, which is dxmat.hip alone");
#else
  DEVICE_GUARD(mesh);
  HIP_TRY(scalar_gradient_launch((hipStream_t)hip_stream, scalar_source(mesh, t_dev), mesh->n_cells * mesh->qp.nqp, grad_dev, value_dev));
  return 0;
#endif
}

// ---- a meridian mesh: the gradients with the hoop term u_r / r, and the displacement forms of the laws that read them -------------
int dxm_mesh_axisymmetric_gradient_device(dxm_mesh* mesh, const double* u_dev, int kind, double* grad_dev, double* radius_dev,
                                          void* hip_stream) {
  if (!mesh || !u_dev || !grad_dev) return fail(-1, "null argument");
  if (!mesh->axisym)
    return fail(-1, "dxm_mesh_axisymmetric_gradient_device needs an axisymmetric mesh (dxm_mesh_create_axisymmetric): the gradients "
                    "of this mesh are those of dxm_mesh_gradient_device");
  if (kind < 0 || kind > 3)
    return fail(-1, "axisymmetric gradient kind must be 0 (4-vector [rr, zz, tt, sqrt(2) rz]), 1 (5-wide F), 2 (6-wide strain) or 3 "
                    "(9-wide F)");
  if ((kind == 0 || kind == 2) && ((uintptr_t)grad_dev & 15))
    return fail(-1, "the gradient device array must be 16-byte aligned for axisymmetric gradient kinds 0 and 2");
#ifdef DXM_CUSTOM_HARDENING
  return fail(-1, "the axisymmetric gradient kernels (a mesh of dxm_mesh_create_axisymmetric) are served by the stock libdxmat, not by "
                  "a custom-hardening build, which is dxmat.hip alone");
#else
  DEVICE_GUARD(mesh);
  AxisymSource s{};
  s.coords = mesh->d_coords; s.conn = mesh->d_conn; s.dofmap = mesh->d_dofmap; s.gphi = mesh->d_gphi; s.gdphi = mesh->d_gdphi;
  s.phi = mesh->d_phi; s.dphi = mesh->d_dphi; s.u = u_dev;
  s.npts = mesh->n_cells * mesh->qp.nqp; s.nqp = mesh->qp.nqp; s.nv = mesh->geom_nv; s.nd = mesh->nd;
  HIP_TRY(axisym_gradient_launch(kind, (hipStream_t)hip_stream, s, grad_dev, radius_dev));
  return 0;
#endif
}

// which kind the law's row asks an axisymmetric mesh for (*kind), or the refusal of the pairing, the handle left as it was.  The slots
// of MGIS's axisymmetric hypothesis are those of its plane-strain one, so the 4-wide rows take kind 0 and the 6- / 9-wide laws the
// embedded kinds; the rows are told apart by what they state themselves, not by their ids
static int axisym_pairing(const dxm_material* m, const dxm_mesh* mesh, int* kind) {
  const LawDesc& d = kLaws[m->law];
  if (d.nodal_scalar)
    return fail(-1, "an axisymmetric mesh (dxm_mesh_create_axisymmetric) carries a displacement (u_r, u_z): the two-dimensional "
                    "heat-transfer laws read a scalar field and take a scalar mesh (dxm_mesh_create_plane_scalar) or grad(T) as an "
                    "array, not this mesh (law %d)", m->law);
  if (d.plane_kind == GRAD_IN_PLANE3)
    return fail(-1, "plane stress and axisymmetry exclude each other: law %d takes the in-plane 3-vector [xx, yy, sqrt(2) xy] and has no "
                    "hoop component, an axisymmetric mesh (dxm_mesh_create_axisymmetric) serves the 4-wide plane-strain rows and the "
                    "6- and 9-wide laws", m->law);
  if (d.no_displacement && !d.plane_kind) return fail(-1, "%s", d.no_displacement);   // as on every other mesh (the 5-wide rows: kind 1, then the array form)
  if (mesh->device != m->device) return fail(-1, "mesh and material live on different devices");
  if (dxm_mesh_npoints(mesh) != m->n) return fail(-1, "mesh has %lld Gauss points, material %lld",
                                                   (long long)dxm_mesh_npoints(mesh), (long long)m->n);
  *kind = d.plane_kind == GRAD_PLANE_STRAIN4 ? AXI_STRAIN4 : d.n_grad == 9 ? AXI_F9 : AXI_STRAIN6;
  if (d.n_grad != AXISYM_GRAD_WIDTH[*kind])   // the scratch array holds rows of n_grad doubles: no kernel writes a wider row into it
    return fail(-1, "law %d reads a gradient of %d components: an axisymmetric mesh evaluates rows of 4, 6 or 9 for the displacement forms",
                m->law, d.n_grad);
  return 0;
}

// dxm_integrate_displacement / _rows on an axisymmetric mesh: the gradient kernel into the handle's scratch, then the update kernel
// (no fused form: fused_gradient makes no difference)
static int integrate_axisym_host(dxm_material* m, dxm_mesh* mesh, const double* u_host, double* flux_aos, double* isv_aos, double* ct_aos,
                                 dxm_stats* stats, const int64_t* rows) {
  int kind = 0;
  if (int rc = axisym_pairing(m, mesh, &kind)) return rc;
  DEVICE_GUARD(m);
  m->last_upload = DXM_UPLOAD_NONE;   // no gradient array crosses PCIe in this form
  if (int rc = ensure_host_path_buffers(m, true)) return rc;
  hipStream_t st = m->own_stream;
  if (int rc = sync_last(m)) return rc;
  if (int rc = upload_from_host(mesh->d_u, u_host, sizeof(double) * mesh->u_len, st)) return rc;
  if (int rc = dxm_mesh_axisymmetric_gradient_device(mesh, mesh->d_u, kind, m->d_grad, nullptr, st)) return rc;
  // the displacement upload and the gradient array are produced on own_stream; chunks on the second stream wait for it
  if (!mesh->grad_done) HIP_TRY(hipEventCreateWithFlags(&mesh->grad_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(mesh->grad_done, st));
  auto upload = [&](int64_t, int64_t, hipStream_t s) -> int {
    if (s != st) HIP_TRY(hipStreamWaitEvent(s, mesh->grad_done, 0));
    return 0;
  };
  return run_and_download(m, upload, flux_aos, isv_aos, ct_aos, stats, nullptr, nullptr, rows);
}

// dxm_integrate_displacement_device on an axisymmetric mesh: two kernels on the caller's stream through the handle's gradient scratch
static int integrate_axisym_device(dxm_material* m, dxm_mesh* mesh, const double* u_dev, double dt, double* flux_dev, double* ct_dev,
                                   void* hip_stream) {
  int kind = 0;
  if (int rc = axisym_pairing(m, mesh, &kind)) return rc;
  if (int rc = take_dt(m, dt)) return rc;
  if (m->n > 0 && (!u_dev || !flux_dev || !ct_dev)) return fail(-1, "null device pointer");
  DEVICE_GUARD(m);
  if (!m->d_grad) HIP_TRY(hipMalloc(&m->d_grad, sizeof(double) * m->n * kLaws[m->law].n_grad));
  if (int rc = dxm_mesh_axisymmetric_gradient_device(mesh, u_dev, kind, m->d_grad, nullptr, hip_stream)) return rc;
  return launch(m, m->d_grad, flux_dev, ct_dev, (hipStream_t)hip_stream);
}

// a scalar mesh and a law that reads a scalar field belong together: every other pairing is refused, the handle left as it was
static bool nodal_pairing(const dxm_material* m, const dxm_mesh* mesh) { return mesh->scalar || kLaws[m->law].nodal_scalar; }
static int nodal_refusal(const dxm_material* m, const dxm_mesh* mesh) {
  const LawDesc& d = kLaws[m->law];
  if (!mesh->scalar) return fail(-1, "%s", d.no_displacement);   // a law of a scalar field on a mesh that carries a displacement
  if (!d.nodal_scalar) {
    if (d.no_displacement && !d.plane_kind) return fail(-1, "%s", d.no_displacement);   // as on every other mesh
    return fail(-1, "a scalar mesh (dxm_mesh_create_plane_scalar) carries a temperature, not a displacement: it serves the "
                    "two-dimensional heat-transfer laws (DXM_LAW_HEAT_STATIONARY_2D, DXM_LAW_HEAT_PHASE_CHANGE_2D) only, not law %d",
                m->law);
  }
  if (mesh->device != m->device) return fail(-1, "mesh and material live on different devices");
  if (dxm_mesh_npoints(mesh) != m->n) return fail(-1, "mesh has %lld Gauss points, material %lld",
                                                   (long long)dxm_mesh_npoints(mesh), (long long)m->n);
  return 0;
}

#ifndef DXM_CUSTOM_HARDENING
// the nodal mode of the handle lasts for one call
struct NodalCall {
  dxm_material* m;
  NodalCall(dxm_material* m_, const dxm_mesh* mesh, const double* t_dev, int mode) : m(m_) {
    m->nodal_src = scalar_source(mesh, t_dev);
    m->nodal_mode = mode;
  }
  ~NodalCall() { m->nodal_mode = 0; m->nodal_src = ScalarSource{}; }
};

// fused_gradient 0: grad(T) and T into the handle's scratch on st, for the update kernel that follows there
static int nodal_scratch(dxm_material* m, const dxm_mesh* mesh, const double* t_dev, hipStream_t st) {
  if (!m->d_grad) HIP_TRY(hipMalloc(&m->d_grad, sizeof(double) * m->n * kLaws[m->law].n_grad));
  if (!m->d_nodal_value) HIP_TRY(hipMalloc(&m->d_nodal_value, sizeof(double) * m->n));
  HIP_TRY(scalar_gradient_launch(st, scalar_source(mesh, t_dev), m->n, m->d_grad, m->d_nodal_value));
  return 0;
}
#endif

// dxm_integrate_displacement / _rows with the nodal temperature t_host (n_dofs doubles) in place of a displacement
static int integrate_nodal_host(dxm_material* m, dxm_mesh* mesh, const double* t_host, double* flux_aos, double* isv_aos, double* ct_aos,
                                dxm_stats* stats, const int64_t* rows) {
  if (int rc = nodal_refusal(m, mesh)) return rc;
#ifdef DXM_CUSTOM_HARDENING
  return fail(-1, "%s", kLaws[m->law].stock_only);
#else
  if (m->n == 0) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return 0;
  }
  DEVICE_GUARD(m);
  m->last_upload = DXM_UPLOAD_NONE;   // no gradient array crosses PCIe in this form
  const bool fuse = m->opt_fused_gradient;   // T and grad(T) evaluated inside the update kernel
  if (int rc = ensure_host_path_buffers(m, true)) return rc;   // (the chunks address d_grad by offset in either mode)
  hipStream_t st = m->own_stream;
  if (int rc = sync_last(m)) return rc;
  if (int rc = upload_from_host(mesh->d_u, t_host, sizeof(double) * mesh->u_len, st)) return rc;
  if (!fuse)
    if (int rc = nodal_scratch(m, mesh, mesh->d_u, st)) return rc;
  // the upload (and the scratch) are produced on own_stream; chunks on the second stream wait for it
  if (!mesh->grad_done) HIP_TRY(hipEventCreateWithFlags(&mesh->grad_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(mesh->grad_done, st));
  auto upload = [&](int64_t, int64_t, hipStream_t s) -> int {
    if (s != st) HIP_TRY(hipStreamWaitEvent(s, mesh->grad_done, 0));
    return 0;
  };
  NodalCall call(m, mesh, mesh->d_u, fuse ? 1 : 2);
  const int rc = run_and_download(m, upload, flux_aos, isv_aos, ct_aos, stats, nullptr, nullptr, rows);
  if (fuse) m->io1_valid &= ~1;   // grad(T) never existed as an array
  return rc;
#endif
}

// dxm_integrate_displacement_device with the nodal temperature t_dev in place of a displacement
static int integrate_nodal_device(dxm_material* m, dxm_mesh* mesh, const double* t_dev, double dt, double* flux_dev, double* ct_dev,
                                  void* hip_stream) {
  if (int rc = nodal_refusal(m, mesh)) return rc;
#ifdef DXM_CUSTOM_HARDENING
  return fail(-1, "%s", kLaws[m->law].stock_only);
#else
  if (int rc = take_dt(m, dt)) return rc;
  if (m->n > 0 && (!t_dev || !flux_dev || !ct_dev)) return fail(-1, "null device pointer");
  DEVICE_GUARD(m);
  hipStream_t st = (hipStream_t)hip_stream;
  if (m->opt_fused_gradient) {   // one kernel: no gradient array, no temperature array
    NodalCall call(m, mesh, t_dev, 1);
    return launch(m, flux_dev /* unused, only checked for alignment */, flux_dev, ct_dev, st);
  }
  // two kernels on the caller's stream through the handle's scratch
  if (m->n > 0)
    if (int rc = nodal_scratch(m, mesh, t_dev, st)) return rc;
  NodalCall call(m, mesh, t_dev, 2);
  return launch(m, m->d_grad, flux_dev, ct_dev, st);
#endif
}

static int integrate_displacement_host(dxm_material* m, dxm_mesh* mesh, const double* u_host, double* flux_aos, double* isv_aos,
                                       double* ct_aos, dxm_stats* stats, const int64_t* rows) {
  if (!m || !mesh || !u_host) return fail(-1, "null argument");
  if (mesh->axisym) return integrate_axisym_host(m, mesh, u_host, flux_aos, isv_aos, ct_aos, stats, rows);   // a meridian mesh: its own gradient kernel
  if (nodal_pairing(m, mesh)) return integrate_nodal_host(m, mesh, u_host, flux_aos, isv_aos, ct_aos, stats, rows);   // a scalar field's nodal values
  const bool plane_law = kLaws[m->law].plane_kind && mesh_2d(mesh);   // a 2-D law on a 2-D mesh: gradient kernel, then update kernel
  if (kLaws[m->law].no_displacement && !plane_law) return fail(-1, "%s", kLaws[m->law].no_displacement);
  if (mesh->device != m->device) return fail(-1, "mesh and material live on different devices");
  if (dxm_mesh_npoints(mesh) != m->n) return fail(-1, "mesh has %lld Gauss points, material %lld",
                                                   (long long)dxm_mesh_npoints(mesh), (long long)m->n);
  DEVICE_GUARD(m);
  m->last_upload = DXM_UPLOAD_NONE;   // no gradient array crosses PCIe in this form
  const bool fuse = m->opt_fused_gradient && fusable(mesh) && !plane_law;   // gradient evaluated inside the update kernel
  if (int rc = ensure_host_path_buffers(m, !fuse)) return rc;
  hipStream_t st = m->own_stream;
  if (int rc = sync_last(m)) return rc;
  if (int rc = upload_from_host(mesh->d_u, u_host, sizeof(double) * mesh->u_len, st)) return rc;
  MeshSource src{};
  if (fuse) {
    src = mesh_source(mesh, mesh->d_u);
  } else {
    if (int rc = dxm_mesh_gradient_device(mesh, mesh->d_u, gradient_kind(kLaws[m->law], mesh_2d(mesh)), m->d_grad, st)) return rc;
  }
  // the displacement upload (and the gradient array) are produced on own_stream; chunks on the second stream wait for it
  if (!mesh->grad_done) HIP_TRY(hipEventCreateWithFlags(&mesh->grad_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(mesh->grad_done, st));
  auto upload = [&](int64_t, int64_t, hipStream_t s) -> int {
    if (s != st) HIP_TRY(hipStreamWaitEvent(s, mesh->grad_done, 0));
    return 0;
  };
  return run_and_download(m, upload, flux_aos, isv_aos, ct_aos, stats, fuse ? &src : nullptr, nullptr, rows);
}

int dxm_integrate_displacement(dxm_material* m, dxm_mesh* mesh, const double* u_host, double dt,
                               double* flux_aos, double* isv_aos, double* ct_aos, dxm_stats* stats) {
  if (int rc = take_dt(m, dt)) return rc;
  return integrate_displacement_host(m, mesh, u_host, flux_aos, isv_aos, ct_aos, stats, nullptr);
}

int dxm_integrate_displacement_rows(dxm_material* m, dxm_mesh* mesh, const double* u_host, double dt, double* flux_rows,
                                    double* ct_rows, const int64_t* rows, dxm_stats* stats) {
  if (!m) return fail(-1, "null argument");
  if (int rc = take_dt(m, dt)) return rc;
  if (m->n > 0 && (!flux_rows || !ct_rows || !rows)) return fail(-1, "dxm_integrate_displacement_rows needs the flux array, the tangent array and the row index");
  return integrate_displacement_host(m, mesh, u_host, flux_rows, nullptr, ct_rows, stats, rows);
}

int dxm_integrate_displacement_device(dxm_material* m, dxm_mesh* mesh, const double* u_dev, double dt,
                                      double* flux_dev, double* ct_dev, void* hip_stream) {
  if (!m || !mesh) return fail(-1, "null argument");
  if (mesh->axisym) return integrate_axisym_device(m, mesh, u_dev, dt, flux_dev, ct_dev, hip_stream);   // a meridian mesh: its own gradient kernel
  if (nodal_pairing(m, mesh)) return integrate_nodal_device(m, mesh, u_dev, dt, flux_dev, ct_dev, hip_stream);   // a scalar field's nodal values
  const bool plane_law = kLaws[m->law].plane_kind && mesh_2d(mesh);   // the 2-D laws have no fused form: the option makes no difference
  if (kLaws[m->law].no_displacement && !plane_law) return fail(-1, "%s", kLaws[m->law].no_displacement);
  if (int rc = take_dt(m, dt)) return rc;
  if (mesh->device != m->device) return fail(-1, "mesh and material live on different devices");
  if (dxm_mesh_npoints(mesh) != m->n) return fail(-1, "mesh has %lld Gauss points, material %lld",
                                                   (long long)dxm_mesh_npoints(mesh), (long long)m->n);
  if (m->n > 0 && (!u_dev || !flux_dev || !ct_dev)) return fail(-1, "null device pointer");
  DEVICE_GUARD(m);
  hipStream_t st = (hipStream_t)hip_stream;
  const LawDesc& d = kLaws[m->law];
  if (m->opt_fused_gradient && fusable(mesh) && !plane_law) {   // one kernel: no gradient array at all
    const MeshSource src = mesh_source(mesh, u_dev);
    return launch(m, flux_dev /* unused, only checked for alignment */, flux_dev, ct_dev, st, &src);
  }
  // two kernels on the caller's stream through the handle's gradient scratch
  if (!m->d_grad) HIP_TRY(hipMalloc(&m->d_grad, sizeof(double) * m->n * d.n_grad));
  if (int rc = dxm_mesh_gradient_device(mesh, u_dev, gradient_kind(d, mesh_2d(mesh)), m->d_grad, hip_stream)) return rc;
  return launch(m, m->d_grad, flux_dev, ct_dev, st);
}

const double* dxm_state_ptr(const dxm_material* m, int which, int field, int comp) {
  if (check_field(m, which, field)) return nullptr;
  const LawDesc& d = kLaws[m->law];
  if (comp < 0 || comp >= d.isv_dim[field]) { fail(-1, "component out of range"); return nullptr; }
  m->state_exposed = true;   // what is written through the address is not seen here: no state store is elided from now on
  return state_of(m, which) + (size_t)(d.isv_slot[field] + comp) * m->ld;
}

int dxm_clean_tiles(dxm_material* m, int64_t* clean, int64_t* tiles) {
  if (!m || !clean || !tiles) return fail(-1, "null argument");
  *clean = *tiles = 0;
  if (!m->stamps || m->n == 0) return 0;
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  const int64_t nt = (m->n + WAVE - 1) / WAVE;
  *tiles = nt;
  // a handle that launches the plain kernels only (option off, address handed out) has no clean tile in use
  if (!m->opt_elide_clean_state || m->state_exposed || m->stamps_stale) return 0;
  std::vector<uint32_t> host((size_t)nt);
  if (int rc = download_to_host(host.data(), m->stamps, sizeof(uint32_t) * (size_t)nt, m->own_stream)) return rc;   // pageable: through the page-locked staging
  int64_t c = 0;
  for (uint32_t v : host) c += v == m->clean_stamp;
  *clean = c;
  return 0;
}

int dxm_packed_state(dxm_material* m, int64_t* tiles_packed, int64_t* points_kept) {
  if (!m || !tiles_packed || !points_kept) return fail(-1, "null argument");
  *tiles_packed = *points_kept = 0;
  if (!m->pack.built || !m->pack_mask || !m->opt_pack_old_state || m->state_exposed || m->n == 0) return 0;
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  const int64_t nt = (m->n + WAVE - 1) / WAVE;
  std::vector<unsigned long long> host((size_t)nt);
  if (int rc = download_to_host(host.data(), m->pack_mask, sizeof(unsigned long long) * (size_t)nt, m->own_stream)) return rc;
  int64_t kept = 0;
  for (unsigned long long v : host) kept += __builtin_popcountll(v);
  *tiles_packed = nt;
  *points_kept = kept;
  return 0;
}

const char* dxm_kernel_name(const dxm_material* m) {
  if (!m) return "";
  if (m->frame_kind) return kLaws[m->law].frame_kernel[m->frame_kind - 1];
  for (int k : m->ext_kind) if (k) return kLaws[m->law].ext_kernel;
  return m->pf_mask ? kLaws[m->law].field_kernel : kLaws[m->law].kernel;
}

int dxm_expand_tangent_device(const double* coef_dev, int64_t npoints, double* ct_dev, int device, void* hip_stream) {
  if (npoints < 0) return fail(-1, "negative point count");
  if (npoints == 0) return 0;
  if (!coef_dev || !ct_dev) return fail(-1, "null device pointer");
  if (((uintptr_t)coef_dev | (uintptr_t)ct_dev) & 15) return fail(-1, "coefficient / tangent device arrays must be 16-byte aligned");
  DeviceGuard guard(device);
  if (!guard.ok) return fail(-2, "hipSetDevice(%d) failed", device);
  const int64_t tiles = (npoints + WAVE - 1) / WAVE;
  int64_t blocks = (tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(expand_tangent_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, npoints, coef_dev, ct_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

int dxm_expand_tangent_pack4_device(const double* flux_dev, const double* pack_dev, int64_t npoints, double* ct_dev, int device,
                                    void* hip_stream) {
  if (npoints < 0) return fail(-1, "negative point count");
  if (npoints == 0) return 0;
  if (!flux_dev || !pack_dev || !ct_dev) return fail(-1, "null device pointer");
  if (((uintptr_t)flux_dev | (uintptr_t)pack_dev | (uintptr_t)ct_dev) & 15) return fail(-1, "stress / pack / tangent device arrays must be 16-byte aligned");
  DeviceGuard guard(device);
  if (!guard.ok) return fail(-2, "hipSetDevice(%d) failed", device);
  const int64_t tiles = (npoints + WAVE - 1) / WAVE;
  int64_t blocks = (tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(expand_pack4_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, npoints, flux_dev, pack_dev, ct_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- per-point parameter fields -----------------------------------------------------------------------
}  // extern "C"

// (lambda, mu) streams from the E / nu fields and uniform values as they stand; both streams exist while either is a field
static int pf_refresh_elastic(dxm_material* m, hipStream_t st) {
#ifndef DXM_CUSTOM_HARDENING
  if (!(m->pf_mask & 3) || m->n == 0) return 0;
  param_fields_elastic_streams(m->n, m->pf_law[0], m->raw_params[0], m->pf_law[1], m->raw_params[1], m->pf_stream[PF_LAMBDA],
                               m->pf_stream[PF_MU], st);
  HIP_TRY(hipGetLastError());
#endif
  return 0;
}

static int pf_check(const dxm_material* m, int idx) {
  if (!m) return fail(-1, "null handle");
  if (kCustomBuild) return fail(-1, "per-point parameter fields are served by the stock libdxmat, not by a custom-hardening build");
  const LawDesc& d = kLaws[m->law];
  if (!d.field_kernel)
    return fail(-1, "per-point parameter fields exist for DXM_LAW_J2_LINEAR and DXM_LAW_J2_VOCE only (law %d: %s)", m->law, d.no_fields);
  if (idx < 0 || idx >= d.n_params) return fail(-1, "law %d has no parameter %d", m->law, idx);
  return 0;
}

// where parameter idx (>= 2) of the J2 laws goes: [E, nu, sig0, H] / [E, nu, sig0, sigu, b]
static int pf_stream_of(int idx) { return idx == 2 ? PF_SIG0 : idx == 3 ? PF_H1 : PF_H2; }

// device storage a bind of parameter idx needs and does not have yet: allocated before anything is changed
static int pf_reserve(dxm_material* m, int idx) {
  const size_t bytes = sizeof(double) * (size_t)(m->n > 0 ? m->n : 1);
  double** want[3] = {nullptr, nullptr, nullptr};
  if (idx < 2) { want[0] = &m->pf_law[idx]; want[1] = &m->pf_stream[PF_LAMBDA]; want[2] = &m->pf_stream[PF_MU]; }
  else want[0] = &m->pf_stream[pf_stream_of(idx)];
  double* fresh[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; ++k) {
    if (!want[k] || *want[k]) continue;
    if (hipMalloc(&fresh[k], bytes) != hipSuccess) {
      (void)hipGetLastError();
      for (double* q : fresh) if (q) (void)hipFree(q);
      return fail(-3, "hipMalloc of a %zu-byte parameter stream failed", bytes);
    }
  }
  for (int k = 0; k < 3; ++k) if (fresh[k]) *want[k] = fresh[k];
  return 0;
}

// back to the uniform value of dxm_set_params (the launch before must be complete: the streams are freed)
static int pf_unbind(dxm_material* m, int idx, hipStream_t st) {
  if (!(m->pf_mask & (1 << idx))) return 0;
  m->pf_mask &= ~(1 << idx);
  ++m->epoch;
  if (idx >= 2) {
    double*& q = m->pf_stream[pf_stream_of(idx)];
    HIP_TRY(hipFree(q));
    q = nullptr;
    return 0;
  }
  HIP_TRY(hipFree(m->pf_law[idx]));
  m->pf_law[idx] = nullptr;
  if (m->pf_mask & 3) {
    if (int rc = pf_refresh_elastic(m, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  for (int k : {PF_LAMBDA, PF_MU}) { HIP_TRY(hipFree(m->pf_stream[k])); m->pf_stream[k] = nullptr; }
  return 0;
}

extern "C" {

int dxm_set_param_field(dxm_material* m, int param_index, const double* host_values) {
  if (int rc = pf_check(m, param_index)) return rc;
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  if (!host_values) return pf_unbind(m, param_index, m->own_stream);
  // the rules build_params applies to the scalar, per point; E and nu are constrained one by one, so a partner field needs no look
  for (int64_t i = 0; i < m->n; ++i) {
    const double v = host_values[i];
    if (!std::isfinite(v)) return fail(-1, "parameter %d is not finite at point %lld (%g)", param_index, (long long)i, v);
    if (param_index == 0 && !(v > 0.0)) return fail(-1, "invalid elastic constant E=%g at point %lld", v, (long long)i);
    if (param_index == 1 && !(v > -1.0 && v < 0.5)) return fail(-1, "invalid elastic constant nu=%g at point %lld", v, (long long)i);
  }
  if (int rc = pf_reserve(m, param_index)) return rc;
  double* dst = param_index < 2 ? m->pf_law[param_index] : m->pf_stream[pf_stream_of(param_index)];
  if (int rc = upload_from_host(dst, host_values, sizeof(double) * (size_t)m->n, m->own_stream)) return rc;
  m->pf_mask |= 1 << param_index;
  ++m->epoch;
  if (param_index < 2) {
    if (int rc = pf_refresh_elastic(m, m->own_stream)) return rc;
    HIP_TRY(hipStreamSynchronize(m->own_stream));
  }
  return 0;
}

int dxm_set_param_field_device(dxm_material* m, int param_index, const double* dev_values, void* hip_stream) {
  if (int rc = pf_check(m, param_index)) return rc;
  DEVICE_GUARD(m);
  hipStream_t st = (hipStream_t)hip_stream;
  if (!dev_values) {
    if (int rc = sync_last(m)) return rc;
    return pf_unbind(m, param_index, st);
  }
  // the last launch may still read the streams from another stream: this one waits for it, the host does not
  if (m->launched && m->last_event_recorded) HIP_TRY(hipStreamWaitEvent(st, m->last_event, 0));
  else if (int rc = sync_last(m)) return rc;
  if (int rc = pf_reserve(m, param_index)) return rc;
  double* dst = param_index < 2 ? m->pf_law[param_index] : m->pf_stream[pf_stream_of(param_index)];
  if (m->n > 0) HIP_TRY(hipMemcpyAsync(dst, dev_values, sizeof(double) * (size_t)m->n, hipMemcpyDeviceToDevice, st));
  m->pf_mask |= 1 << param_index;
  ++m->epoch;
  if (param_index < 2) return pf_refresh_elastic(m, st);
  return 0;
}

int dxm_param_field_mask(const dxm_material* m) { return m ? m->pf_mask : -1; }

// ---- material frames -----------------------------------------------------------------------------------
static int frame_check(const dxm_material* m) {
  if (!m) return fail(-1, "null handle");
  const LawDesc& d = kLaws[m->law];
  if (d.no_frame) return fail(-1, "law %d takes no material frame: %s", m->law, d.no_frame);
  return 0;
}

// finite and orthonormal: max |R R^T - I| <= 1e-8
static int frame_valid(const double* r, long long point) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(r[k])) {
      if (point < 0) return fail(-1, "the frame is not finite (entry %d is %g)", k, r[k]);
      return fail(-1, "the frame of point %lld is not finite (entry %d is %g)", point, k, r[k]);
    }
  double worst = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double v = r[3 * i] * r[3 * j] + r[3 * i + 1] * r[3 * j + 1] + r[3 * i + 2] * r[3 * j + 2] - (i == j ? 1.0 : 0.0);
      worst = std::max(worst, std::fabs(v));
    }
  if (worst <= 1e-8) return 0;
  if (point < 0) return fail(-1, "the frame is not orthonormal: max |R R^T - I| = %g (allowed 1e-8)", worst);
  return fail(-1, "the frame of point %lld is not orthonormal: max |R R^T - I| = %g (allowed 1e-8)", point, worst);
}

static int frame_reserve(dxm_material* m) {
  if (m->frame_streams) return 0;
  if (hipMalloc(&m->frame_streams, sizeof(double) * 9 * (size_t)m->ld) != hipSuccess) {
    (void)hipGetLastError();
    m->frame_streams = nullptr;
    return fail(-3, "hipMalloc of the %zu-byte frame streams failed", sizeof(double) * 9 * (size_t)m->ld);
  }
  return 0;
}

// the field is dropped (the launch before must be complete: the streams are freed)
static int frame_release(dxm_material* m) {
  if (!m->frame_streams) return 0;
  double* q = m->frame_streams;
  m->frame_streams = nullptr;
  HIP_TRY(hipFree(q));
  return 0;
}

int dxm_set_frame(dxm_material* m, const double* r9) {
  if (int rc = frame_check(m)) return rc;
  if (r9)
    if (int rc = frame_valid(r9, -1)) return rc;
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  if (int rc = frame_release(m)) return rc;
  m->frame_kind = r9 ? 1 : 0;
  if (r9) memcpy(m->frame_uniform.r, r9, sizeof(m->frame_uniform.r));
  ++m->epoch;
  return 0;
}

int dxm_set_frame_field(dxm_material* m, const double* host_aos) {
  if (int rc = frame_check(m)) return rc;
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  if (!host_aos) {
    if (m->frame_kind != 2) return 0;
    if (int rc = frame_release(m)) return rc;
    m->frame_kind = 0;
    ++m->epoch;
    return 0;
  }
  for (int64_t i = 0; i < m->n; ++i)
    if (int rc = frame_valid(host_aos + 9 * i, (long long)i)) return rc;
#ifndef DXM_CUSTOM_HARDENING
  if (int rc = frame_reserve(m)) return rc;
  if (m->n > 0) {
    // the (n, 9) rows go up as they are and are transposed into the streams on the device, once
    double* aos = nullptr;
    HIP_TRY(hipMalloc(&aos, sizeof(double) * 9 * (size_t)m->n));
    int rc = upload_from_host(aos, host_aos, sizeof(double) * 9 * (size_t)m->n, m->own_stream);
    if (rc == 0) {
      orthotropic_frames_to_streams(m->n, aos, m->frame_streams, m->ld, m->own_stream);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(m->own_stream) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(-2, "transposing the frame field on the device failed");
      }
    }
    (void)hipFree(aos);
    if (rc) return rc;
  }
#endif
  m->frame_kind = 2;
  ++m->epoch;
  return 0;
}

int dxm_set_frame_field_device(dxm_material* m, const double* dev_aos, void* hip_stream) {
  if (int rc = frame_check(m)) return rc;
  if (!dev_aos) return dxm_set_frame_field(m, nullptr);
  DEVICE_GUARD(m);
  hipStream_t st = (hipStream_t)hip_stream;
  // the last launch may still read the streams from another stream: this one waits for it, the host does not
  if (m->launched && m->last_event_recorded) HIP_TRY(hipStreamWaitEvent(st, m->last_event, 0));
  else if (int rc = sync_last(m)) return rc;
#ifndef DXM_CUSTOM_HARDENING
  if (int rc = frame_reserve(m)) return rc;
  orthotropic_frames_to_streams(m->n, dev_aos, m->frame_streams, m->ld, st);
  HIP_TRY(hipGetLastError());
#endif
  m->frame_kind = 2;
  ++m->epoch;
  return 0;
}

int dxm_frame_kind(const dxm_material* m) { return m ? m->frame_kind : -1; }

// ---- external state variables --------------------------------------------------------------------------
static int ext_check(const dxm_material* m, int index) {
  if (!m) return fail(-1, "null handle");
  const LawDesc& d = kLaws[m->law];
  if (d.n_ext == 0)
    return fail(-1, "law %d has no external state variable: its update reads the gradient, its parameters and its own state only "
                    "(DXM_LAW_HEAT_STATIONARY and DXM_LAW_HEAT_PHASE_CHANGE read a Temperature)", m->law);
  if (index < 0 || index >= d.n_ext) return fail(-1, "law %d has no external state variable %d", m->law, index);
  return 0;
}

static int ext_reserve(dxm_material* m, int index) {
  if (m->ext_field[index]) return 0;
  const size_t bytes = sizeof(double) * (size_t)(m->n > 0 ? m->n : 1);
  if (hipMalloc(&m->ext_field[index], bytes) != hipSuccess) {
    (void)hipGetLastError();
    m->ext_field[index] = nullptr;
    return fail(-3, "hipMalloc of a %zu-byte external-state field failed", bytes);
  }
  return 0;
}

static void ext_set_kind(dxm_material* m, int index, int kind) {
  if (m->ext_kind[index] == kind) return;
  m->ext_kind[index] = kind;
  ++m->epoch;   // the launches read another argument from now on
}

int dxm_set_external_state(dxm_material* m, int index, const double* host_values) {
  if (int rc = ext_check(m, index)) return rc;
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  if (!host_values) { ext_set_kind(m, index, 0); return 0; }
  const char* name = kLaws[m->law].ext_name[index];
  for (int64_t i = 0; i < m->n; ++i)
    if (!std::isfinite(host_values[i])) return fail(-1, "%s is not finite at point %lld (%g)", name, (long long)i, host_values[i]);
  if (int rc = ext_reserve(m, index)) return rc;
  if (int rc = upload_from_host(m->ext_field[index], host_values, sizeof(double) * (size_t)m->n, m->own_stream)) return rc;
  ext_set_kind(m, index, 1);
  return 0;
}

int dxm_set_external_state_uniform(dxm_material* m, int index, double value) {
  if (int rc = ext_check(m, index)) return rc;
  if (!std::isfinite(value)) return fail(-1, "%s must be finite, got %g", kLaws[m->law].ext_name[index], value);
  if (m->ext_kind[index] == 0 && m->ext_uniform[index] == value) return 0;   // nothing changed: captured launches stay valid
  m->ext_uniform[index] = value;
  m->ext_kind[index] = 0;
  ++m->epoch;
  return 0;
}

int dxm_set_external_state_device(dxm_material* m, int index, const double* dev_values, void* hip_stream) {
  if (int rc = ext_check(m, index)) return rc;
  if (!dev_values) return dxm_set_external_state(m, index, nullptr);
  DEVICE_GUARD(m);
  hipStream_t st = (hipStream_t)hip_stream;
  // the last launch may still read the field from another stream: this one waits for it, the host does not
  if (m->launched && m->last_event_recorded) HIP_TRY(hipStreamWaitEvent(st, m->last_event, 0));
  else if (int rc = sync_last(m)) return rc;
  if (int rc = ext_reserve(m, index)) return rc;
  if (m->n > 0) HIP_TRY(hipMemcpyAsync(m->ext_field[index], dev_values, sizeof(double) * (size_t)m->n, hipMemcpyDeviceToDevice, st));
  ext_set_kind(m, index, 1);
  return 0;
}

int dxm_external_state_kind(const dxm_material* m, int index) {
  if (!m || index < 0 || index >= kLaws[m->law].n_ext) return -1;
  return m->ext_kind[index];
}

int dxm_algorithmic_bytes(const dxm_material* m) {
  if (!m) return -1;
  int bytes = kLaws[m->law].alg_bytes;
  for (const double* q : m->pf_stream) if (q) bytes += 8;
  if (m->frame_kind == 2) bytes += 9 * 8;   // the nine frame streams
  for (int k : m->ext_kind) if (k) bytes += 8;   // an external state variable held as a field
  return bytes;
}

int dxm_notify_replay(dxm_material* m) {
  if (!m) return fail(-1, "null handle");
  m->launched = true;
  m->last_event_recorded = false;   // nothing of the replay is known here: waits fall back to the device
  m->s1_alias = false;              // the replayed kernel rewrote every slot of s1
  bump_clean_stamp(m, true);        // ... without maintaining the stamps; it read s0 and left it as it was: the packed copy stays
  return 0;
}

uint64_t dxm_launch_generation(const dxm_material* m) { return m ? (m->epoch << 1) | (uint64_t)m->parity : 0; }

int dxm_set_option(dxm_material* m, const char* name, double value) {
  if (!m || !name) return fail(-1, "null argument");
  const std::string k(name);
  const bool on = value != 0.0;
  if (k == "pipeline") m->opt_pipeline = on;
  else if (k == "split_streams") m->opt_split_streams = on;
  else if (k == "packed_transfer") {
    if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(-1, "packed_transfer must be 0, 1 or 2");
    m->opt_packed_transfer = (int)value;
  }
  else if (k == "fused_gradient") m->opt_fused_gradient = on;
  else if (k == "verbose") m->opt_verbose = on;
  else if (k == "stage_ahead") {
    if (!(value >= 1 && value <= DXM_RING - 2)) return fail(-1, "stage_ahead must be in [1, %d]", DXM_RING - 2);
    m->opt_stage_ahead = (int)value;
  }
  else if (k == "register_input") {
    if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(-1, "register_input must be 0, 1 or 2");
    m->up.set_option((int)value);
  }
  else if (k == "keep_initial_io") m->opt_keep_initial_io = on;
  else if (k == "pageable_dma") m->opt_pageable_dma = value != 0.0;
  else if (k == "query_foreign_pointers") g_query_foreign.store(on ? 1 : 0);   // process-wide
  else if (k == "packed_min_points") {
    if (!(value >= 0 && value <= 1e12)) return fail(-1, "packed_min_points must be >= 0");
    m->opt_packed_min_points = (int64_t)value;
  }
  else if (k == "host_threads") {
    if (!(value >= 1 && value <= 256)) return fail(-1, "host_threads must be in [1, 256]");
    m->opt_host_threads = (int)value;
  } else if (k == "max_chunks") {
    if (!(value >= 1 && value <= DXM_MAX_CHUNKS)) return fail(-1, "max_chunks must be in [1, %d]", DXM_MAX_CHUNKS);
    m->opt_max_chunks = (int)value;
  } else if (k == "blocks_per_cu") {
    if (!(value >= 1 && value <= 256)) return fail(-1, "blocks_per_cu must be in [1, 256]");
    m->blocks_per_cu = (int)value;
  } else if (k == "elide_clean_state") {
    m->opt_elide_clean_state = on;
    bump_clean_stamp(m);
  } else if (k == "pack_old_state") {
    if (!on && (m->pack_buf || m->pack_mask)) {   // off: the copy is given back, behind whatever still reads it
      DEVICE_GUARD(m);
      if (int rc = sync_last(m)) return rc;
      free_pack(m);
    }
    m->opt_pack_old_state = on;
    m->pack_failed = false;
    m->pack.move();
  } else {
    return fail(-1, "unknown option '%s'", name);
  }
  ++m->epoch;
  return 0;
}

int dxm_isv_host(dxm_material* m, int which, double* isv_aos) {
  if (!m) return fail(-1, "null handle");
  if (which != DXM_S0 && which != DXM_S1) return fail(-1, "state selector must be DXM_S0 or DXM_S1");
  const LawDesc& d = kLaws[m->law];
  const int total = isv_total(d);
  if (total == 0 || m->n == 0) return 0;
  if (!isv_aos) return fail(-1, "null host pointer");
  DEVICE_GUARD(m);
  if (int rc = sync_last(m)) return rc;
  if (!m->d_isv) HIP_TRY(hipMalloc(&m->d_isv, sizeof(double) * m->n * total));
  if (int rc = pack_isv_range(m, which, 0, m->n, m->d_isv, m->own_stream)) return rc;
  return download_to_host(isv_aos, m->d_isv, sizeof(double) * m->n * total, m->own_stream);
}

int dxm_host_copy(void* dst, const void* src, uint64_t bytes, int threads) {
  if (bytes == 0) return 0;
  if (!dst || !src) return fail(-1, "null host pointer");
  dxm_host::host_copy(dst, src, bytes, threads);
  return 0;
}

// rows of `width` doubles moved through an index on several threads (utils.py:136-143 `array[index] = values`)
static int move_rows(bool scatter, double* dst, const double* src, const int64_t* rows, int64_t n, int width, int threads) {
  if (n <= 0 || width <= 0) return 0;
  if (!dst || !src || !rows) return fail(-1, "null host pointer");
  dxm_host::move_rows(scatter, dst, src, rows, n, width, threads);
  return 0;
}

int dxm_host_scatter_rows(double* dst, const double* src, const int64_t* rows, int64_t n, int width, int threads) {
  return move_rows(true, dst, src, rows, n, width, threads);
}

int dxm_host_gather_rows(double* dst, const double* src, const int64_t* rows, int64_t n, int width, int threads) {
  return move_rows(false, dst, src, rows, n, width, threads);
}

int dxm_host_index_range(const int64_t* rows, int64_t n, int threads, int64_t* lo, int64_t* hi) {
  if (!lo || !hi) return fail(-1, "null result pointer");
  if (n > 0 && !rows) return fail(-1, "null index");
  dxm_host::index_min_max(rows, n, threads, lo, hi);
  return 0;
}

int dxm_host_register(void* p, uint64_t bytes) {
  if (!p || bytes == 0) return fail(-1, "null / empty host range");
  hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // (a range that is registered already, memory that cannot be pinned: the caller falls back)
    return fail(-3, "hipHostRegister(%p, %llu) failed: %s", p, (unsigned long long)bytes, hipGetErrorString(e));
  }
  note_locked(p, bytes);
  return 0;
}

int dxm_host_unregister(void* p) {
  if (p) {
    RelaxedCaptureMode relaxed;
    forget_locked(p);
    HIP_TRY(hipHostUnregister(p));
  }
  return 0;
}

}  // extern "C"
