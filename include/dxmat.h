/*
 * dxmat.h -- C ABI of libdxmat.so, the MI355X (gfx950) batched constitutive-update engine.
 *
 * This is the drop-in boundary for ONE path of bleyerj/dolfinx_materials: the per-Gauss-point
 * constitutive update reached through
 *     NonlinearMaterialProblem._constitutive_update   (dolfinx_materials/solvers.py:173-176)
 *  -> QuadratureMap.update()                          (dolfinx_materials/quadrature_map.py:297-334)
 *  -> material.integrate(gradients)                   (dolfinx_materials/jaxmat.py:208-234,
 *                                                      dolfinx_materials/generic.py:176-189)
 *  -> batched_constitutive_update = vmap(jacfwd(constitutive_update))
 *                                                     (dolfinx_materials/jaxmat.py:147-155)
 *
 * The reference has no FFI of its own (its boundary is the duck-typed Python `Material` protocol);
 * the Python classes in dolfinx_materials_amd/ implement that protocol on top of these entry
 * points through ctypes.  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *   - all floating point data is IEEE fp64;
 *   - "AoS" = row-major (npoints, dim), component fastest: the memory layout of a dolfinx
 *     quadrature Function (dolfinx_materials/utils.py:98-104, :136-143);
 *   - symmetric tensors are Mandel 6-vectors, non-symmetric ones 9-vectors in the order
 *     [11,22,33,12,21,13,31,23,32] (dolfinx_materials/utils.py:146-190);
 *   - the tangent is Ct[i][j] = d flux_i / d gradient_j, row-major (npoints, nflux*ngrad)
 *     (dolfinx_materials/quadrature_map.py:83-105, :334);
 *   - int return codes: 0 = ok, > 0 = number of points whose local Newton did not converge,
 *     < 0 = hard error (message from dxm_last_error());
 *   - HIP graphs: the device-pointer entry points are capturable.  A captured launch bakes in the two
 *     state buffers (advance() swaps them on the host) and the parameters, so a graph is valid only while
 *     dxm_launch_generation() returns the value it had at capture time; the value comes back when the
 *     buffers swap back (two graphs, captured at consecutive increments, serve a whole load history);
 *   - one handle per (material, device); a handle is not thread-safe (the reference calls the path
 *     from the PETSc SNES callback on one thread: dolfinx_materials/solvers.py:72); successive
 *     device-pointer launches on one handle must be ordered on the same HIP stream (advance()
 *     and revert() only swap pointers on the host);
 *   - there is NO CPU fallback: every entry point that computes fails with a negative code when no
 *     HIP device is usable;
 *   - the library exports what this header declares and nothing else (tests/test_abi.py).  The placement search and launch
 *     timing of ABI 3-5 are gone (profiles/r05_placement_decision.md: a search rescued 4 of 12 slow leases); the matrix-free
 *     assembly kernels of the stand-in FE loop are examples/csrc/dxmfem.hip (examples/libdxmfem.so), not product.
 */
#ifndef DXMAT_H
#define DXMAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXM_ABI_VERSION 6   /* 6: dxm_tune_placement, dxm_time_device, the dxm_mesh_* assembly operators and the options "tune_verbose" /
                             *    "tune_max_skip_bytes" removed (there is no dxmat_experimental.h any more); option "verbose" */

/* Constitutive laws (what `behavior.constitutive_update` is in jaxmat.py:163). */
enum {
  /* sigma = C:eps, Ct = C.  Replaces python_materials/elasticity.py:21-24.
   * params = [E, nu] */
  DXM_LAW_ELASTIC_ISO = 0,
  /* small-strain J2, linear isotropic hardening R(p) = sig0 + H p, implicit radial return +
   * consistent tangent.  Spec: tests/mfront/IsotropicLinearHardeningPlasticity.mfront:49-77.
   * params = [E, nu, sig0, H] */
  DXM_LAW_J2_LINEAR = 1,
  /* small-strain J2, Voce hardening R(p) = sig0 + (sigu - sig0)(1 - exp(-b p))
   * (jaxmat vonMisesIsotropicHardening + VoceHardening as constructed in
   * demos/jax/elastoplasticity/plane_elastoplasticity.py:60-73).
   * params = [E, nu, sig0, sigu, b] */
  DXM_LAW_J2_VOCE = 2,
  /* finite-strain FeFp J2 plasticity with Voce hardening, gradient F (9), flux PK1 (9)
   * (jaxmat FeFpJ2Plasticity as constructed in tests/test_FeFp_jax.py:7-20).
   * params = [E, nu, sig0, sigu, b] */
  DXM_LAW_FEFP_J2_VOCE = 3,
  /* the same finite-strain law with linear hardening R(p) = sig0 + H p.
   * params = [E, nu, sig0, H] */
  DXM_LAW_FEFP_J2_LINEAR = 4,
  /* small-strain Ramberg-Osgood nonlinear elasticity, no internal state
   * (tests/mfront/RambergOsgoodNonLinearElasticity.mfront): eps_e = sqrt(2/3 dev(eps):dev(eps)),
   * sigma = K tr(eps) 1 + sig_e ne with ne = 2 dev(eps) / (3 max(eps_e, 1e-12)), sig_e the root of
   * sig_e / (3 mu) + beta (sig_e / sig0)^n = eps_e, beta = alpha sig0 / E (3 mu eps_e below eps_e = 1e-12).
   * Local Newton per point under dxm_set_newton(maxit, rtol): stops when |step| <= rtol sig_e.
   * dxm_stats: n_plastic = points on the Newton branch (eps_e >= 1e-12), max_local_iters = the most Newton
   * iterations of a point, n_not_converged = points that reached maxit, n_nan as for J2.
   * Tangent layouts "sym", "coef" and "pack4" as for J2.  Not served by a custom-hardening build.
   * params = [E, nu, sig0, alpha, n] with sig0 > 0, alpha > 0, n >= 1 */
  DXM_LAW_RAMBERG_OSGOOD = 5,
  /* finite-strain Ogden hyperelasticity, gradient F (9), flux PK1 (9), full 81-entry dP/dF
   * (demos/mfront/hyperelasticity/Ogden.mfront): stored energy
   * W(F) = (mu / alpha) (J^(-alpha/3) sum_i c_i^(alpha/2) - 3) + K/2 (J - 1)^2, c_i the eigenvalues of C = F^T F, J = det F.
   * One internal state variable, PK2Stress (6, MFront vector convention): the isochoric part of the second Piola-Kirchhoff
   * stress, written by every update, never read, zero initially.  Points with det F <= 0 give NaN outputs and count in
   * dxm_stats.n_nan; n_plastic, n_not_converged and max_local_iters are 0 (closed form, no local iteration).
   * Only DXM_TANGENT_FULL; the displacement forms evaluate the gradient in a kernel of its own (no fused kernel for this
   * law: with option fused_gradient on they are refused).  The host-buffer forms download the 81 entries as they are.
   * Not served by a custom-hardening build.
   * params = [alpha, mu, K] with alpha != 0, mu > 0, K > 0 */
  DXM_LAW_OGDEN = 7,   /* id 6 is not assigned: the library answers it with "unknown law id", as ABI 6 always has */
  /* small-strain Hosford plasticity with linear isotropic hardening R(p) = R0 + H p (the reference's
   * IsotropicPlasticHosfordFlowLinear behaviour): equivalent stress (1/2 (|s1-s2|^a + |s1-s3|^a + |s2-s3|^a))^(1/a) of the
   * principal stresses, associated flow, implicit update with a local Newton per plastic point (dxm_set_newton: stops when every
   * residual, as a stress, is <= max(tol, rtol seq_trial)); a = 2 and a = 4 are von Mises.  Plain Newton from the trial state:
   * converges for seq_trial / R <= 3 with a <= 10 and <= 1.5 with a = 20; points beyond that may stop at maxit and
   * are counted in dxm_stats.n_not_converged (and n_nan if their outputs are not finite), never silently.
   * Internal state variables ElasticStrain (6; written by every update) and EquivalentPlasticStrain (1); the strain handed in is
   * the TOTAL strain, so the update is driven by a hidden state field 2, the plastic strain (6): dxm_set_state / dxm_get_state
   * address it, a state set through field 0 alone does not change the next update.
   * The tangent is a general symmetric 6x6: DXM_TANGENT_FULL and DXM_TANGENT_SYM; _COEF and _PACK4 are refused.  No per-point
   * parameter fields, no fused displacement gradient (option fused_gradient 0), not served by a custom-hardening build.
   * params = [E, nu, R0, H, a] with R0 > 0, H >= 0, a >= 2 */
  DXM_LAW_HOSFORD_LINEAR = 10,   /* ids 8 and 9 are not assigned */
  /* small-strain orthotropic elasticity in a material frame (the orthotropic form of the reference's StandardElasticity brick,
   * tests/mfront/MericCailletaudSingleCrystalViscoPlasticity.mfront:18-28, driven through a rotated frame in
   * tests/uniaxial_tension.py:59-68).  In the material frame, Mandel [11, 22, 33, sqrt2 12, sqrt2 13, sqrt2 23]:
   * sigma_m = C eps_m, C block-diagonal: its 3x3 normal block is the inverse of the compliance S11 = 1/E1, S22 = 1/E2, S33 = 1/E3,
   * S12 = -nu12/E1, S13 = -nu13/E1, S23 = -nu23/E2 (symmetric), its shear diagonal 2 G12, 2 G13, 2 G23.  No internal state.
   * FRAME CONVENTION (dxm_set_frame*): R is 3x3 row-major and its ROWS are the material axes in global coordinates, so
   * eps_m = R eps R^T, sigma = R^T sigma_m R and Ct = Q^T C Q with Q(R) the orthogonal 6x6 Mandel image of R -- the matrix
   * tests/uniaxial_tension.py:61-66 builds for a material turned by +angle about z, nine numbers per point as rotation_func.x.array
   * holds them.  (This reading is not pinned against mgis_bv.rotate*: MGIS was not available.)  Gradient, flux and tangent of every
   * call are GLOBAL: the rotation is inside the kernel.  Without a frame the kernel computes C eps and C with no rotation at all.
   * The tangent is a general symmetric 6x6: DXM_TANGENT_FULL and DXM_TANGENT_SYM; _COEF and _PACK4 are refused.  No per-point
   * parameter fields, no fused displacement gradient (option fused_gradient 0), not served by a custom-hardening build.
   * dxm_stats: n_nan counts points with a non-finite stress or tangent; n_plastic, n_not_converged, max_local_iters are 0.
   * params = [E1, E2, E3, nu12, nu23, nu13, G12, G23, G13], all finite, E_i > 0, G_ij > 0, compliance positive definite */
  DXM_LAW_ORTHOTROPIC_ELASTIC = 12,   /* id 11 is not assigned */
  /* small-strain FCC single-crystal viscoplasticity (the reference's MericCailletaudSingleCrystalViscoPlasticity behaviour,
   * restated from its equations; DESIGN.md section "Single-crystal viscoplasticity" lists them).  Orthotropic stiffness and the
   * FRAME CONVENTION of DXM_LAW_ORTHOTROPIC_ELASTIC (dxm_set_frame*; gradient, flux and tangent are global).  Twelve {111}<01-1>
   * systems in the library's own order (plane-major over (1,1,1), (-1,1,1), (1,-1,1), (1,1,-1)): MFront's numbering is not pinned,
   * so the slip fields compare with MFront's up to a permutation and sign of systems; stress and tangent do not depend on it.
   * RATE-DEPENDENT: the only law that reads the dt of dxm_integrate* (finite, >= 0, else the call fails; dt = 0 is the elastic
   * response).  A graph captured around dxm_integrate_device bakes the dt of the capture in.
   * State, all in the material frame: ElasticStrain (6, written by every update, read by none), ViscoplasticSlip (12),
   * EquivalentViscoplasticSlip (12), BackStrain (12).  The plastic strain is sum g_i mu_i: a frame that changes while g != 0 is
   * the caller's business.  The tangent is NOT symmetric: DXM_TANGENT_FULL only.  No per-point parameter fields, no fused
   * displacement gradient (option fused_gradient 0), not served by a custom-hardening build.
   * dxm_stats: n_plastic counts points with any f_i > 0 at the trial state; n_not_converged those that reach the iteration cap of
   * dxm_set_newton (whose rtol is the absolute bound on the slip residuals) or whose trial state trips the f_i > 1.1 K guard -- such
   * a point writes its elastic trial stress and Q^T D Q and keeps the state bits it read; max_local_iters counts halvings too.
   * params = [E1, E2, E3, nu12, nu23, nu13, G12, G23, G13, n, K, tau0, Q, b, d, C, h_self, h_coplanar, h_Hirth, h_collinear,
   * h_glissile, h_Lomer]: all finite, the first nine as for DXM_LAW_ORTHOTROPIC_ELASTIC, n >= 1, K > 0, tau0, b, d, C >= 0 */
  DXM_LAW_SINGLE_CRYSTAL_FCC = 14,   /* id 13 is not assigned */
  /* stationary nonlinear heat transfer (the reference's demos/mfront/heat_transfer/StationaryHeatTransfer.mfront, restated from its
   * equations).  Gradient TemperatureGradient g (3), flux HeatFlux j (3), one EXTERNAL state variable Temperature T (the value at
   * the end of the step, MFront's T + dT; dxm_set_external_state*): k = 1 / (A + B T), j = -k g.  The tangent has TWO blocks
   * (dxm_law_blocks_get), 12 doubles per point in this order: (HeatFlux, TemperatureGradient) 3x3 = -k I row-major with its six
   * zeros written, then (HeatFlux, Temperature) 3x1 = B k^2 g.  No internal state.  A + B T <= 0 is not refused (MFront does not
   * refuse it either): A + B T = 0 gives non-finite results, counted in n_nan.  The gradient is 3 wide whatever the dimension of
   * the problem: a 2-D caller pads grad(T) with a zero; 2-component hypotheses are not served.
   * DXM_TANGENT_FULL only; no material frame, no per-point parameter fields, none of the displacement forms
   * (dxm_integrate_displacement*), not served by a custom-hardening build.
   * dxm_stats: n_nan counts points with a non-finite flux or tangent entry; n_plastic, n_not_converged, max_local_iters are 0.
   * dxm_law_info.algorithmic_bytes_per_point counts 120 (gradient 24 + tangent 96; the flux, 24 more, is written too), 136 for the
   * phase-change law (+ 8 of tangent + 8 of Enthalpy); dxm_algorithmic_bytes adds 8 with a temperature per point.
   * params = [A, B], finite */
  DXM_LAW_HEAT_STATIONARY = 16,   /* id 15 is not assigned */
  /* heat transfer with a smoothed solid/liquid phase change (demos/mfront/heat_transfer/HeatTransferPhaseChange.mfront, its lines
   * 41-56).  Gradient, flux and external state variable as for DXM_LAW_HEAT_STATIONARY.  With Ts = Tm - Tsmooth/2 and
   * Tl = Tm + Tsmooth/2, each formed on the host by one rounded operation and compared against as doubles:
   *   T < Ts:  k = ks, c = cs, h = cs T, k' = 0
   *   T > Tl:  k = kl, c = cl, h = cl (T - Tl) + dhsl + cs Ts + (cs + cl) Tsmooth / 2, k' = 0
   *   else:    k = ks + (kl - ks)(T - Ts)/Tsmooth, c = (cs + cl)/2 + dhsl/Tsmooth, h = cs Ts + c (T - Ts), k' = -(kl - ks)/Tsmooth
   * j = -k g.  One internal state variable, Enthalpy h (1): every update writes it and none reads it.  THREE blocks, 13 doubles
   * per point: (HeatFlux, TemperatureGradient) = -k I (9), (HeatFlux, Temperature) = k' g (3), (Enthalpy, Temperature) = c (1).
   * Restrictions and dxm_stats as for DXM_LAW_HEAT_STATIONARY (n_nan also counts a non-finite Enthalpy).
   * params = [Tm, ks, cs, kl, cl, dhsl, Tsmooth], finite, Tsmooth > 0 */
  DXM_LAW_HEAT_PHASE_CHANGE = 17,
  /* finite-strain logarithmic-strain J2 plasticity with linear hardening (the reference's
   * demos/mfront/finite_strain_elastoplasticity/LogarithmicStrainPlasticity.mfront, restated from its equations): gradient F (9),
   * flux PK1 (9), full 81-entry dP/dF.  The Hencky strain E = 1/2 log(F^T F) goes through the small-strain radial return of
   * DXM_LAW_J2_LINEAR (Hooke, Mises, R(p) = s0 + H0 p) and its stress T is mapped back to PK1 by the derivatives of the tensor
   * logarithm (DESIGN.md section "Logarithmic-strain J2 plasticity"); closed form, no local iteration.
   * Internal state variables ElasticStrain (6; written by every update) and EquivalentPlasticStrain (1), MFront vector
   * convention; the gradient handed in is the TOTAL F, so the update is driven by a hidden state field 2, the logarithmic
   * plastic strain (6): dxm_set_state / dxm_get_state address it, a state set through field 0 alone does not change the next
   * update.  Points with det F <= 0 or a non-finite F give NaN outputs and count in dxm_stats.n_nan; n_plastic counts the points
   * that yield; n_not_converged and max_local_iters are 0.
   * Only DXM_TANGENT_FULL; no material frame, no per-point parameter fields, no fused displacement gradient (option
   * fused_gradient 0), not served by a custom-hardening build.
   * params = [E, nu, s0, H0] with E > 0, -1 < nu < 0.5, s0 > 0, H0 >= 0, all finite */
  DXM_LAW_LOG_STRAIN_J2 = 19,   /* id 18 is not assigned */
  /* finite-strain FCC single-crystal viscoplasticity (the reference's FCCMericCailletaudFiniteStrainSingleCrystalViscoPlasticity
   * behaviour, restated from its equations; DESIGN.md section "Finite-strain single-crystal viscoplasticity" lists them).
   * Gradient F (9), flux PK1 (9), tangent dP/dF (81 independent numbers), 9-vectors as for DXM_LAW_OGDEN.  Multiplicative
   * F = Fe Fp, cubic stiffness of E, nu, G, St-Venant-Kirchhoff elasticity in the intermediate configuration, the twelve
   * {111}<01-1> systems of DXM_LAW_SINGLE_CRYSTAL_FCC in the same order with mu_i = m_i x n_i (not symmetrised), Norton flow,
   * interaction hardening and Armstrong-Frederick back strain as there; dFp^-1 = (I - sum dg_i mu_i) / det^(1/3).
   * FRAME CONVENTION of DXM_LAW_ORTHOTROPIC_ELASTIC (dxm_set_frame*): F_m = R F R^T, P = R^T P_m R; gradient, flux and tangent
   * are global, the state lives in the material frame.
   * RATE-DEPENDENT like DXM_LAW_SINGLE_CRYSTAL_FCC: dt finite and >= 0, else the call fails; dt = 0 is the elastic response.
   * State, all visible, all carried: PlasticSlip (12), EquivalentViscoplasticSlip (12), BackStrain (12),
   * PlasticPartOfTheDeformationGradient (9, the identity after dxm_create).  MFront's other variables (ElasticStrain, the elastic
   * part of F, ResolvedShearStress) are functions of F and this state.  MFront's entry names, its numbering of the systems and its
   * det^(1/3) normalisation are not pinned (MFront is absent).
   * DXM_TANGENT_FULL only.  No per-point parameter fields, no fused displacement gradient, no displacement forms, not served
   * by a custom-hardening build.
   * dxm_stats: n_plastic counts points with any f_i > 0 at the trial state; n_not_converged those that reach the iteration cap of
   * dxm_set_newton (whose rtol is the absolute bound on the slip residuals): such a point writes its elastic trial response
   * (St-Venant-Kirchhoff about the old Fp) and keeps the state bits it read; max_local_iters counts step halvings too (a step is
   * halved while the largest slip residual grows or is not finite).
   * params = [E, nu, G, n, K, tau0, Q, b, d, C, h_self, h_coplanar, h_Hirth, h_collinear, h_glissile, h_Lomer]: all finite,
   * E, G, K > 0, -1 < nu < 0.5, n >= 1, tau0, b, d, C >= 0 */
  DXM_LAW_FS_SINGLE_CRYSTAL_FCC = 21,   /* id 20 is not assigned */
  /* plane-stress return mapping onto a quadratic yield set, perfectly plastic (the reference's PlaneStressvonMises,
   * demos/cvxpy/cvxpy_materials.py:89-93, with its update :38-51, without the conic program).  Gradient Strain (3) and flux
   * Stress (3) are [xx, yy, sqrt(2) xy] (Kelvin-Mandel); C = E/(1-nu^2) [[1, nu, 0], [nu, 1, 0], [0, 0, 1-nu]] (:16-18).
   *   s_tr = C (eps - epsp_n),   s = argmin 1/2 (t - s_tr)^T C^-1 (t - s_tr) over K = {t^T Q t <= sig0^2},
   *   Q = [[1, -1/2, 0], [-1/2, 1, 0], [0, 0, q]].
   * q = 1 is the reference's matrix, which is NOT von Mises in Mandel components (the weight of its third component is its own);
   * q = 3/2 is von Mises.  The projection is a scalar monotone Newton on one multiplier (DESIGN.md section "Plane-stress return
   * mapping"), ended on the residual sqrt(s^T Q s) - sig0 <= rtol sig0 of dxm_set_newton.
   * No user-visible internal state (the reference's state is Strain and Stress, the gradient and the flux of s0).  ONE HIDDEN
   * state field 0, PlasticStrain (3) = eps - C^-1 s: dxm_set_state / dxm_get_state address it; a yielded point writes it, an
   * elastic point writes back the bits it read.  A caller that sets a Strain / Stress state sets epsp_n = eps_n - C^-1 s_n.
   * tangent = 0 writes C at every point (the reference's); tangent = 1 writes the algorithmic tangent of a yielded point,
   * A - (A n)(A n)^T / (n^T A n) with A = (C^-1 + l Q)^-1 and n = Q s, and C at an elastic one.  9 entries, row-major.
   * DXM_TANGENT_FULL only; no material frame, no per-point parameter fields, not served by a custom-hardening build.  The
   * displacement forms (dxm_integrate_displacement*) are served on two-dimensional meshes (dxm_mesh_create_plane,
   * dxm_mesh_create_simplex with tdim 2): the gradient kernel writes kind 3 of dxm_mesh_gradient_device, then this law's kernel runs;
   * there is no fused form and option fused_gradient makes no difference.  On any other mesh they are refused.
   * dxm_stats: n_plastic counts the projected points; max_local_iters is the largest number of Newton steps a point took before
   * its residual met the bound; n_not_converged counts the points that reached the cap of dxm_set_newton (they write their last
   * iterate); n_nan counts points with a non-finite stress, state or (tangent = 1) tangent entry.
   * algorithmic_bytes_per_point = 168: strain 24 + state 24 in, stress 24 + tangent 72 + state 24 out.
   * params = [E, nu, sig0, q, tangent], all finite, E > 0, -1 < nu < 1, sig0 > 0, q > 0, tangent 0 or 1 */
  DXM_LAW_PS_QUADRATIC = 23,   /* id 22 is not assigned */
  /* plane-stress return mapping onto a polygonal yield set in the plane of the two principal stresses, perfectly plastic (the
   * reference's Rankine, cvxpy_materials.py:54-65, and L1Rankine, :68-86).  Conventions, update, hidden state and restrictions as
   * for DXM_LAW_PS_QUADRATIC.  K = {n_k . (sI, sII) <= d_k, k < M}, M <= 4, in the UNORDERED principal-stress plane: d_k > 0 (the
   * origin strictly inside), no zero normal, and the list closed under the exchange of the principal stresses (the mirror
   * (n2, n1, d) of every row is a row, exactly), else dxm_create refuses.  Trial and answer are coaxial: the answer is the
   * nearest, in the energy norm, of the projections onto the rows' lines that keep the other rows and of the set's vertices.
   * Rankine(ft, fc): (1,0,ft), (0,1,ft), (-1,0,fc), (0,-1,fc).  L1Rankine, a = (1/ft-1/fc)/2, b = (1/ft+1/fc)/2: (1,1,ft),
   * (-1,-1,fc), (a+b,a-b,1), (a-b,a+b,1).  The tangent written is C (no consistent tangent for this law).
   * dxm_stats: n_plastic counts the projected points; there is no local iteration: max_local_iters = n_not_converged = 0; n_nan as
   * for DXM_LAW_PS_QUADRATIC.
   * params = [E, nu, M, n1_0, n2_0, d_0, ..., n1_3, n2_3, d_3]: always 15 numbers, the rows past M are not read */
  DXM_LAW_PS_POLYGON = 24,
  /* The plane-strain hypothesis of DXM_LAW_ELASTIC_ISO / DXM_LAW_J2_LINEAR / DXM_LAW_J2_VOCE (the reference's
   * MFrontMaterial(..., hypothesis="plane_strain"), dolfinx_materials/mfront.py:33-37): the same three updates in the four
   * components a plane-strain state has.  Gradient Strain (4) and flux Stress (4) are [xx, yy, zz, sqrt(2) xy]
   * (utils.py:146-150 for a 2x2 tensor); eps_zz is read like any other component (a plane-strain caller passes 0) and sig_zz is
   * returned.  The tangent is the 4x4 block d Stress / d Strain, 16 entries, row-major: the rows and columns [0, 1, 2, 3] of the
   * 6-wide law's block (whose out-of-plane rest is zero for such a state).  DXM_TANGENT_FULL only.
   * State of the two J2 laws: field 0 p (1), field 1 epsp (4, the same order), 5 SoA slots; the elastic law has none.
   * Parameters, validation, dxm_set_newton and dxm_stats as for the 6-wide law of the same name.
   * No per-point parameter fields, no material frame, no external state variable, not served by a custom-hardening build.  The
   * displacement forms are served on two-dimensional meshes as for DXM_LAW_PS_QUADRATIC, through kind 2 of
   * dxm_mesh_gradient_device (eps_zz = 0.0 exactly); on any other mesh they are refused.
   * algorithmic_bytes_per_point = 192 (strain 32 in, stress 32 + tangent 128 out) / 272 (+ state 40 in, 40 out) / 272.
   * params = [E, nu] / [E, nu, sig0, H] / [E, nu, sig0, sigu, b] */
  DXM_LAW_PE_ELASTIC_ISO = 26,   /* id 25 is not assigned */
  DXM_LAW_PE_J2_LINEAR = 27,
  DXM_LAW_PE_J2_VOCE = 28,
  /* (the table ended here, with DXM_LAW_COUNT = 29, before ids 30 and 31)
   * Plane-stress J2 plasticity with isotropic hardening: the backward-Euler update of DXM_LAW_J2_LINEAR / DXM_LAW_J2_VOCE (Hooke,
   * von Mises, associated flow, R(p) linear or Voce) under sig_zz = sig_xz = sig_yz = 0, what the reference's
   * demos/jax/elastoplasticity/_plane_stress_elastoplasticity.py obtains with eps_zz as an extra unknown of the global problem.
   * Gradient Strain (3) and flux Stress (3) are [xx, yy, sqrt(2) xy], the convention of DXM_LAW_PS_QUADRATIC.
   * State: field 0 p (1), field 1 epsp (3, the in-plane plastic strain in the same components), 4 SoA slots; epsp_zz =
   * -(epsp_xx + epsp_yy) is implied and not stored; eps_zz = -nu/E (s_xx + s_yy) - (epsp_xx + epsp_yy) follows from the outputs.
   * The update is one scalar equation in the multiplier dg of epsp - epsp_n = dg P s, g(dg) = seq(dg) - R(p_n + 2/3 dg seq(dg)) = 0,
   * solved by a bracketed Newton (DESIGN.md section "Plane-stress J2 plasticity") and ended on |g| <= max(rtol max(|sig0|, 2e-8 mu),
   * rtol seq_trial) of dxm_set_newton; both hardening laws iterate.
   * The tangent is one 3x3 block, 9 entries, row-major, exactly symmetric: the consistent (algorithmic) tangent at a yielded point,
   * the plane-stress C = E/(1-nu^2) [[1, nu, 0], [nu, 1, 0], [0, 0, 1-nu]] at an elastic one.  DXM_TANGENT_FULL only.
   * No per-point parameter fields, no material frame, no external state variable, not served by a custom-hardening build.  The
   * displacement forms are served on two-dimensional meshes as for DXM_LAW_PS_QUADRATIC (kind 3); on any other mesh they are refused.
   * dxm_stats: n_plastic counts the yielded points; max_local_iters is the largest number of Newton steps a point took before its
   * residual met the bound; n_not_converged counts the points that reached the cap of dxm_set_newton (they write their last
   * iterate); n_nan counts points with a non-finite stress, state or tangent entry (a non-finite strain takes the elastic path and
   * keeps its state bits).
   * algorithmic_bytes_per_point = 184: strain 24 + state 32 in, stress 24 + tangent 72 + state 32 out.
   * params = [E, nu, sig0, H] / [E, nu, sig0, sigu, b], validated as for DXM_LAW_J2_LINEAR / DXM_LAW_J2_VOCE */
  DXM_LAW_PS_J2_LINEAR = 30,   /* id 29 is not assigned */
  DXM_LAW_PS_J2_VOCE = 31,
  /* (the table ended here, with DXM_LAW_COUNT = 32, before id 33)
   * Plane-stress Hosford plasticity, perfectly plastic (the reference's PlaneStressHosford, demos/cvxpy/cvxpy_materials.py:96-110,
   * without the conic program).  Conventions, update, hidden state field PlasticStrain (3) and restrictions as for
   * DXM_LAW_PS_QUADRATIC, with the yield set
   *   K = {phi(t) <= sig0},   phi(t) = ((|t_I|^a + |t_II|^a + |t_I - t_II|^a) / 2)^(1/a),   t_I, t_II the principal values.
   * a = 2 is plane-stress von Mises (DXM_LAW_PS_QUADRATIC with q = 3/2).  Trial and answer are coaxial; in the scaled principal
   * plane the projection is ONE bracketed scalar root in the polar angle th of the boundary's first-quadrant arc, solved by Newton
   * inside the bracket [0, pi/2] with a bisection safeguard (DESIGN.md section "Plane-stress Hosford plasticity"), ended when the
   * step just taken is at most max(rtol, 2^-49) radians (dxm_set_newton).  Every iterate lies on the yield surface by construction.
   * tangent = 0 writes C at every point (the reference's); tangent = 1 writes the algorithmic tangent of a yielded point (exactly
   * symmetric), and C at an elastic one.  9 entries, row-major.  DXM_TANGENT_FULL only; no material frame, no per-point parameter
   * fields, no external state variable, not served by a custom-hardening build.  The displacement forms are served on
   * two-dimensional meshes as for DXM_LAW_PS_QUADRATIC (kind 3); on any other mesh they are refused.
   * dxm_stats: n_plastic counts the projected points; max_local_iters is the largest number of steps of the angle a point took;
   * n_not_converged counts the points that reached the cap of dxm_set_newton (they write their last iterate, which is admissible);
   * n_nan counts points with a non-finite stress, state or (tangent = 1) tangent entry (a non-finite trial is not projected).
   * algorithmic_bytes_per_point = 168: strain 24 + state 24 in, stress 24 + tangent 72 + state 24 out.
   * params = [E, nu, sig0, a, tangent], all finite, E > 0, -1 < nu < 1, sig0 > 0, 2 <= a <= 100, tangent 0 or 1 */
  DXM_LAW_PS_HOSFORD = 33,   /* id 32 is not assigned */
  /* (before ids 35 and 36 the table ended here, with DXM_LAW_COUNT = 34
   * and DXM_ABI_VERSION 6, which stays)
   * DXM_LAW_HEAT_STATIONARY and DXM_LAW_HEAT_PHASE_CHANGE under a two-dimensional hypothesis: what the reference's heat-transfer
   * demos ask for (demos/mfront/heat_transfer/nonlinear_heat_transfer.py:247 and phase_change.py:265 load their law with
   * hypothesis="plane_strain" and register ufl.grad(T) as a 2-wide TemperatureGradient).  Gradient TemperatureGradient (2) =
   * [dT/dx, dT/dy], flux HeatFlux (2); the external state variable Temperature with the setters and the default of the 3-wide laws;
   * the phase-change law has the internal state variable Enthalpy (1).  Parameters and their validation are those of the 3-wide law.
   * Tangent, DXM_TANGENT_FULL only, the blocks of dxm_law_blocks_get one after the other: (HeatFlux, TemperatureGradient) 2 x 2 =
   * [-k, 0, 0, -k] with both zeros written, (HeatFlux, Temperature) 2 x 1, and for the phase-change law (Enthalpy, Temperature) 1 x 1:
   * 6 / 7 doubles per point.  The arithmetic is that of the 3-wide kernels, operation for operation: flux, tangent entries, enthalpy
   * and dxm_stats.n_nan equal those of the 3-wide law on [g0, g1, 0] bit for bit.
   * No material frame, no per-point parameter fields, not served by a custom-hardening build.
   * THE DISPLACEMENT FORMS (dxm_integrate_displacement, _rows, _device) take these laws with a scalar mesh
   * (dxm_mesh_create_plane_scalar) and the NODAL TEMPERATURE vector in place of the displacement: gradient and temperature of a
   * point are those of the interpolated field, T = sum_m T_m phi_m and grad(T) = Ji^T sum_m T_m dphi_m.  In these calls the handle's
   * own external state (uniform value or field, dxm_set_external_state*) is neither read nor changed.  With option fused_gradient 1
   * (default) the update kernel evaluates both at its own points and no gradient or temperature array exists; with 0 the kernel of
   * dxm_mesh_scalar_gradient_device fills scratch arrays owned by the handle and the update kernel reads them on the same stream:
   * both deliver the same bits.  Refused, with a sentence and the handle left as it was: these laws with a mesh that carries a
   * displacement, any other law with a scalar mesh, a mesh whose number of Gauss points is not the handle's.
   * algorithmic_bytes_per_point = 64 (gradient 16 + tangent 48; the flux, 16 more, is written too) / 80 (+ 8 of tangent + 8 of
   * Enthalpy); dxm_algorithmic_bytes adds 8 with a temperature per point.
   * params = [A, B] / [Tm, ks, cs, kl, cl, dhsl, Tsmooth] */
  DXM_LAW_HEAT_STATIONARY_2D = 35,   /* id 34 is not assigned */
  DXM_LAW_HEAT_PHASE_CHANGE_2D = 36,
  /* (before id 38 the table ended here, with
   * DXM_LAW_COUNT = 37
   * and DXM_ABI_VERSION 6, which stays)
   * DXM_LAW_OGDEN under the plane-strain hypothesis: what MFrontMaterial(lib, "Ogden", hypothesis="plane_strain") exchanges.
   * Gradient DeformationGradient (5) = [F00, F11, F22, F01, F10], the 5-vector utils.py:168-172 builds from a 2x2 tensor with its
   * out-of-plane stretch; flux FirstPiolaKirchhoffStress (5) in the same order; tangent dP/dF 5 x 5, row-major, 25 doubles per
   * point.  BY DEFINITION the law is DXM_LAW_OGDEN evaluated on F9 = [F00, F11, F22, F01, F10, 0, 0, 0, 0], of which are kept:
   * components 0..4 of PK1 (the other four are exactly zero for such an F), rows and columns 0..4 of the 9 x 9 dP/dF (the dropped
   * cross derivatives vanish by the reflection z -> -z) and the components [xx, yy, zz, sqrt(2) xy] of the internal state variable
   * PK2Stress (4, MFront's 2-D symmetric tensor; the isochoric part of S, written by every update, never read, zero initially).
   * F22 is read like the other components: a plane-strain caller passes 1.0, the law does not assume it.
   * dxm_stats: n_nan counts the points with J = F22 (F00 F11 - F01 F10) <= 0 or a non-finite input, whose outputs are NaN as for
   * DXM_LAW_OGDEN; n_plastic, n_not_converged and max_local_iters are 0 (closed form: C = F^T F is a 2 x 2 block and F22^2, one
   * rotation diagonalises it).
   * Only DXM_TANGENT_FULL; the host-buffer forms download the 25 entries as they are and the rows forms move them.  Refused, with a
   * sentence of the law's own and the handle left as it was: packed tangent layouts, per-point parameter fields, material frames,
   * the fused displacement gradient and the displacement forms on every mesh (the mesh gradient kernels produce the 9-wide F: pass
   * [1 + H00, 1 + H11, 1, H01, H10] as an array).  Not served by a custom-hardening build.
   * algorithmic_bytes_per_point = 312: F 40 in, PK1 40 + tangent 200 + state 32 out (DXM_LAW_OGDEN on the embedded F: 840).
   * params = [alpha, mu, K] as DXM_LAW_OGDEN, with its checks */
  DXM_LAW_OGDEN_PE = 38,   /* id 37 is not assigned */
  /* (before id 40 the table ended here, with
   * DXM_LAW_COUNT = 39
   * and DXM_ABI_VERSION 6, which stays)
   * DXM_LAW_HOSFORD_LINEAR under the plane-strain hypothesis: the matrix of the reference's multi-material demo on its plane mesh.
   * Gradient Strain (4) and flux Stress (4), both [xx, yy, zz, sqrt(2) xy]; one tangent block, 4 x 4, row-major, 16 doubles per
   * point: a general symmetric matrix, not of the form c1 1x1 + c2 I + c3 n x n.  BY DEFINITION the law is DXM_LAW_HOSFORD_LINEAR
   * evaluated on the strain [xx, yy, zz, sqrt(2) xy, 0, 0], of which are kept: components 0..3 of the stress, the elastic and the
   * plastic strain (the out-of-plane shears are exactly zero for such a strain) and rows and columns 0..3 of the 6 x 6 tangent (its
   * coupling to the out-of-plane shears vanishes).  eps_zz is read like the other components (a plane-strain caller passes 0) and
   * sig_zz is returned, as DXM_LAW_PE_* do.
   * Internal state variables ElasticStrain (4; written by every update, read by none) and EquivalentPlasticStrain (1); the update
   * is driven by the hidden state field 2, the plastic strain (4), addressed by dxm_set_state / dxm_get_state exactly as for
   * DXM_LAW_HOSFORD_LINEAR: 9 SoA slots.
   * dxm_stats and dxm_set_newton: as DXM_LAW_HOSFORD_LINEAR (residuals as stresses, <= max(tol, rtol seq_trial); n_plastic,
   * n_not_converged, n_nan, max_local_iters), with its Newton domain.
   * Only DXM_TANGENT_FULL; the host-buffer forms download the 16 entries as they are and the rows forms move them.  On a
   * two-dimensional mesh (dxm_mesh_create_plane) the displacement forms evaluate the 4-wide strain and then run the update kernel.
   * Refused, with a sentence of the law's own and the handle left as it was: packed tangent layouts, per-point parameter fields,
   * material frames, external state variables, the fused displacement gradient and the displacement forms on a mesh that is not
   * two-dimensional.  Not served by a custom-hardening build.
   * algorithmic_bytes_per_point = 304: strain 32 + state 40 in, stress 32 + tangent 128 + state 72 out (DXM_LAW_HOSFORD_LINEAR on
   * the embedded strain: 544).
   * params = [E, nu, R0, H, a] as DXM_LAW_HOSFORD_LINEAR, with its checks */
  DXM_LAW_PE_HOSFORD_LINEAR = 40,   /* id 39 is not assigned */
  /* (before id 42 the table ended here, with
   * DXM_LAW_COUNT = 41
   * and DXM_ABI_VERSION 6, which stays)
   * DXM_LAW_LOG_STRAIN_J2 under the plane-strain hypothesis: what MFrontMaterial(lib, "LogarithmicStrainPlasticity",
   * hypothesis="plane_strain") exchanges.  Gradient DeformationGradient (5) = [F00, F11, F22, F01, F10], the 5-vector
   * utils.py:168-172 builds from a 2x2 tensor with its out-of-plane stretch; flux FirstPiolaKirchhoffStress (5) in the same order;
   * tangent dP/dF 5 x 5, row-major, 25 doubles per point.  BY DEFINITION the law is DXM_LAW_LOG_STRAIN_J2 evaluated on
   * F9 = [F00, F11, F22, F01, F10, 0, 0, 0, 0] and an old plastic strain without out-of-plane shears, of which are kept: components
   * 0..4 of PK1 (the other four are exactly zero for such a state), rows and columns 0..4 of the 9 x 9 dP/dF (the dropped cross
   * derivatives vanish by the reflection z -> -z) and the components [xx, yy, zz, sqrt(2) xy] of the symmetric tensors.  F22 is read
   * like the other components: a plane-strain caller passes 1.0, the law does not assume it.  Closed form, no local iteration: one
   * rotation diagonalises the 2 x 2 block of C = F^T F, one first and two second divided differences of the logarithm remain.
   * Internal state variables ElasticStrain (4; written by every update, read by none) and EquivalentPlasticStrain (1); the
   * gradient handed in is the TOTAL F, so the update is driven by the hidden state field 2, the logarithmic plastic strain (4),
   * addressed by dxm_set_state / dxm_get_state exactly as for DXM_LAW_LOG_STRAIN_J2: 9 SoA slots.
   * dxm_stats: n_nan counts the points with J = F22 (F00 F11 - F01 F10) <= 0 or a non-finite F, whose outputs are all NaN;
   * n_plastic counts the points that yield; n_not_converged and max_local_iters are 0.
   * Only DXM_TANGENT_FULL; the host-buffer forms download the 25 entries as they are and the rows forms move them.  Refused, with a
   * sentence of the law's own and the handle left as it was: packed tangent layouts, per-point parameter fields, material frames,
   * the fused displacement gradient and the displacement forms on every mesh (the mesh gradient kernels produce the 9-wide F: pass
   * [1 + H00, 1 + H11, 1, H01, H10] as an array).  Not served by a custom-hardening build.
   * algorithmic_bytes_per_point = 392: F 40 + state 40 in, PK1 40 + tangent 200 + state 72 out (DXM_LAW_LOG_STRAIN_J2 on the
   * embedded F: 952).
   * params = [E, nu, s0, H0] as DXM_LAW_LOG_STRAIN_J2, with its checks */
  DXM_LAW_LOG_STRAIN_PE = 42,   /* id 41 is not assigned */
  DXM_LAW_COUNT = 43
};

/* Which state: s0 = beginning of the increment, s1 = end (generic.py:204-216, jaxmat.py:30-43). */
enum { DXM_S0 = 0, DXM_S1 = 1 };

#define DXM_MAX_STATE_FIELDS 4

typedef struct dxm_law_info {
  int32_t n_grad;         /* gradient size (6 strain / 9 F)              jaxmat.py:166-175 */
  int32_t n_flux;         /* flux size (6 stress / 9 PK1)                jaxmat.py:177-186 */
  int32_t n_params;       /* number of material parameters                                 */
  int32_t n_isv_fields;   /* number of user-visible internal state variables               */
  int32_t isv_dim[DXM_MAX_STATE_FIELDS];      /* size of each (scalar = 1)  jaxmat.py:188-193 */
  const char* isv_name[DXM_MAX_STATE_FIELDS]; /* e.g. "p", "epsp", "be_bar"                   */
  int32_t n_isv_total;    /* sum of isv_dim = columns of the isv array of integrate()      */
  int32_t algorithmic_bytes_per_point; /* 384 / 496 / 496 / 976    */
} dxm_law_info;

/* Per-batch status of the last integrate (the reference only has host-side NaN asserts,
 * quadrature_map.py:322-324, and no local-Newton report on the JAX path). */
typedef struct dxm_stats {
  int64_t n_points;
  int64_t n_plastic;        /* points that took the plastic branch */
  int64_t n_not_converged;  /* local Newton hit maxit              */
  int64_t n_nan;            /* points with a non-finite flux, isv or tangent (quadrature_map.py:322-324) */
  int32_t max_local_iters;
  int32_t upload;   /* host-buffer form: how the gradient reached the GPU in this call -- DXM_UPLOAD_* below; 0 otherwise */
} dxm_stats;

typedef struct dxm_material dxm_material; /* opaque handle */

/* ---- library / device ------------------------------------------------------------------- */
int dxm_abi_version(void);
/* 1 if this library was built with -DDXM_CUSTOM_HARDENING (a user-supplied isotropic hardening law
 * R(p), dR/dp compiled into the DXM_LAW_J2_VOCE / DXM_LAW_FEFP_J2_VOCE kernels; those laws then
 * take params = [E, nu, sig0, c0..c5]), 0 for the stock library. */
int dxm_has_custom_hardening(void);
/* Message of the last failing call on this thread ("" if none). */
const char* dxm_last_error(void);
/* Number of HIP devices, or < 0 if the HIP runtime cannot be initialised. */
int dxm_device_count(void);
int dxm_law_info_get(int law, dxm_law_info* out);

/* External state variables and tangent blocks of a law (generic.py:141-146 `tangent_blocks`, quadrature_map.py:84-105).  The
 * tangent array of DXM_TANGENT_FULL holds the blocks one after the other, each rows x cols row-major, tangent_width doubles per
 * point.  A block's row is a flux (row_index 0) or internal state field row_index of dxm_law_info; its column the gradient
 * (col_index 0) or external state variable col_index.  External state variables are scalars.  The laws without one report the
 * single block n_flux x n_grad and n_external = 0. */
#define DXM_MAX_EXTERNAL_STATE 2
#define DXM_MAX_TANGENT_BLOCKS 4
enum { DXM_BLOCK_ROW_FLUX = 0, DXM_BLOCK_ROW_STATE = 1 };
enum { DXM_BLOCK_COL_GRADIENT = 0, DXM_BLOCK_COL_EXTERNAL = 1 };
typedef struct dxm_tangent_block {
  int32_t row_kind, row_index;   /* DXM_BLOCK_ROW_* */
  int32_t col_kind, col_index;   /* DXM_BLOCK_COL_* */
  int32_t rows, cols;
} dxm_tangent_block;
typedef struct dxm_law_blocks {
  int32_t n_external;                                  /* number of external state variables */
  int32_t n_blocks;
  int32_t tangent_width;                               /* sum of rows * cols = dxm_tangent_size of a DXM_TANGENT_FULL handle */
  int32_t reserved;
  const char* external_name[DXM_MAX_EXTERNAL_STATE];   /* e.g. "Temperature" */
  double external_default[DXM_MAX_EXTERNAL_STATE];     /* the uniform value after dxm_create */
  dxm_tangent_block block[DXM_MAX_TANGENT_BLOCKS];
} dxm_law_blocks;
int dxm_law_blocks_get(int law, dxm_law_blocks* out);

/* ---- life cycle: Material.set_data_manager(ngauss)  (generic.py:172-174, jaxmat.py:195-197,
 *      quadrature_map.py:231-233) ---------------------------------------------------------- */
/* Allocates device-resident SoA state s0/s1 for npoints Gauss points on `device` and
 * initialises it (p = 0, epsp = 0, be_bar = identity; cf. behavior.init_state, jaxmat.py:35). */
dxm_material* dxm_create(int law, const double* params, int n_params, int64_t npoints, int device);
/* dxm_destroy, dxm_mesh_destroy, dxm_host_free and dxm_host_unregister may be called while another stream of the application is
 * being captured on the calling thread (a garbage collector's finalizer inside a graph capture): they run in the thread's relaxed
 * capture mode and leave that capture valid. */
int dxm_destroy(dxm_material* m);
int64_t dxm_npoints(const dxm_material* m);
int dxm_law(const dxm_material* m);
/* Material.update_material_property (generic.py:119-120): replace the parameter vector. */
int dxm_set_params(dxm_material* m, const double* params, int n_params);
/* Per-point parameter fields, DXM_LAW_J2_LINEAR and DXM_LAW_J2_VOCE of the stock library (what the reference's
 * QuadratureMap.update_material_properties hands to update_material_property when a property is a Function or an expression:
 * one value per Gauss point, quadrature_map.py:160-172).  param_index indexes the law's parameter vector ([E, nu, sig0, H] /
 * [E, nu, sig0, sigu, b]); host_values holds npoints doubles, of which the library keeps its own device copy; NULL returns the
 * parameter to the uniform value of dxm_set_params.  Every value is checked with the rules dxm_set_params applies to the
 * scalar (finite; E > 0; -1 < nu < 0.5); a refusal returns < 0, names the first offending point and leaves the handle as it
 * was.  The kernels read streams of lambda, mu, sig0, h1, h2 (8 B/point each): a varying E or nu binds both lambda and mu.
 * dxm_set_params keeps working for the parameters that stay uniform and does not unbind a field.  The other laws refuse
 * (< 0, message); so does a custom-hardening build. */
int dxm_set_param_field(dxm_material* m, int param_index, const double* host_values);
/* The same from npoints doubles in device memory on the handle's device; asynchronous on hip_stream (the copy, and for E / nu
 * the kernel that forms lambda and mu); dev_values is not referenced once the call is complete on that stream.  Launches that
 * are to see the field go to the same stream or are ordered after it by the caller.  The values are NOT checked: a value that
 * makes an update non-finite shows in dxm_stats.n_nan.  NULL unbinds, as above (that form waits for the last launch). */
int dxm_set_param_field_device(dxm_material* m, int param_index, const double* dev_values, void* hip_stream);
/* bit i = parameter i is a field */
int dxm_param_field_mask(const dxm_material* m);
/* Material frames, DXM_LAW_ORTHOTROPIC_ELASTIC (convention: at the law).  A handle has no frame after dxm_create (identity).
 * dxm_set_frame: one frame for every point, r9 = 3x3 row-major, passed to the kernel as an argument; NULL: back to no frame.
 * dxm_set_frame_field: one frame per Gauss point, host_aos (npoints, 9) as rotation_func.x.array holds them; the library keeps its
 * own device copy (nine streams, transposed once here); NULL unbinds (back to no frame).  Both check every frame -- finite, and
 * max |R R^T - I| <= 1e-8 -- and a refusal returns < 0, names the first offending point and leaves the handle as it was.
 * dxm_set_frame_field_device: the same from (npoints, 9) doubles in device memory on the handle's device, asynchronous on
 * hip_stream and ordered like dxm_set_param_field_device; the frames are NOT checked; dev_aos is not referenced once the call is
 * complete on that stream; NULL unbinds (that form waits for the last launch).
 * In the rows forms (dxm_integrate_rows) the frame of point i is row i of the handle's field, not row rows[i].
 * Every other law refuses all three (< 0, message): a frame changes nothing for an isotropic law.
 * dxm_frame_kind: 0 none, 1 uniform, 2 field (negative: null handle). */
int dxm_set_frame(dxm_material* m, const double* r9);
int dxm_set_frame_field(dxm_material* m, const double* host_aos);
int dxm_set_frame_field_device(dxm_material* m, const double* dev_aos, void* hip_stream);
int dxm_frame_kind(const dxm_material* m);
/* External state variables (dxm_law_blocks_get: DXM_LAW_HEAT_STATIONARY and DXM_LAW_HEAT_PHASE_CHANGE have one, Temperature,
 * index 0).  The handle holds ONE value per variable and point, the value at the end of the step (MGIS keeps a pair s0 / s1; the
 * served laws read nothing else).  After dxm_create every variable is uniform at its default (Temperature: 293.15, mfront.py:109-110).
 * dxm_set_external_state: host_values holds npoints doubles, of which the handle keeps its own device copy; writing the values
 * again reuses that allocation at the same address; NULL returns to the uniform value.  dxm_set_external_state_uniform: one value
 * for every point, a kernel argument.  Both refuse a non-finite value (< 0, the message names it and the first offending point)
 * and leave the handle as it was.  dxm_set_external_state_device: npoints doubles in device memory on the handle's device,
 * asynchronous on hip_stream and ordered like dxm_set_param_field_device; the values are NOT checked; dev_values is not
 * referenced once the call is complete on that stream; NULL returns to the uniform value (that form waits for the last launch).
 * dxm_launch_generation moves when a uniform value or the kind changes, NOT when a field is rewritten in place: a captured launch
 * bakes in the field's address, not its contents.  In chunked launches and in the rows forms the value of point i is entry i of
 * the handle's field (not entry rows[i]).  Laws without an external state variable refuse all of these (< 0, message).
 * dxm_external_state_kind: 0 uniform, 1 field (negative: null handle, no such variable). */
int dxm_set_external_state(dxm_material* m, int index, const double* host_values);
int dxm_set_external_state_uniform(dxm_material* m, int index, double value);
int dxm_set_external_state_device(dxm_material* m, int index, const double* dev_values, void* hip_stream);
int dxm_external_state_kind(const dxm_material* m, int index);
/* Bytes per point the handle's update kernel moves as it is configured now: dxm_law_info.algorithmic_bytes_per_point plus 8
 * per bound kernel-parameter stream, plus 72 while a frame field is bound, plus 8 per external state variable held as a field. */
int dxm_algorithmic_bytes(const dxm_material* m);
/* Tangent layout integrate writes, doubles per point:
 *   DXM_TANGENT_FULL   n_flux*n_grad (36 / 81), row-major: what `jacobian_flatten` holds (quadrature_map.py:83-105); for a law
 *                      with several blocks their widths' sum (dxm_law_blocks.tangent_width: 12 / 13 for the heat-transfer laws);
 *   DXM_TANGENT_SYM    21 upper-triangle entries (i <= j), small-strain laws (symmetric tangent);
 *                      Hosford and orthotropic elasticity: the host-buffer forms of a DXM_TANGENT_FULL handle move these 21 and
 *                      mirror them on the host;
 *   DXM_TANGENT_COEF   9 = (c1, c2, c3, n[0..5]) of Ct = c1 1x1 + c2 I + c3 n x n, J2 laws and Ramberg-Osgood
 *                      (tests/mfront/IsotropicLinearHardeningPlasticity.mfront:66-69 with M expanded);
 *   DXM_TANGENT_PACK4  4 = (c1, c2, c3, w), J2 laws and Ramberg-Osgood: the kernels form n = dev(stress) w, so the stress of the same update
 *                      and these four rebuild the block bit for bit (dxm_expand_tangent_pack4_device). */
/* dxm_stats.upload */
enum { DXM_UPLOAD_NONE = 0, DXM_UPLOAD_PAGE_LOCKED = 1 /* the caller's array was page-locked already: DMA */,
       DXM_UPLOAD_REGISTERED = 2 /* page-locked by the library for the duration of the call: DMA */,
       DXM_UPLOAD_STAGED = 3 /* copied chunk by chunk into the library's page-locked ring by the worker threads */,
       DXM_UPLOAD_RUNTIME = 4 /* option pageable_dma: handed to the runtime's own pageable path */ };
enum { DXM_TANGENT_FULL = 0, DXM_TANGENT_SYM = 1, DXM_TANGENT_COEF = 2, DXM_TANGENT_PACK4 = 3 };
int dxm_set_tangent_layout(dxm_material* m, int layout);
/* doubles per point of the tangent array integrate writes (36 / 21 / 9 / 81). */
int dxm_tangent_size(const dxm_material* m);
/* Local Newton controls (Voce / traced hardening, FeFp): at most maxit iterations, stop when
 *   |r| <= max(tol, rtol * sigma_eq_trial),   tol = rtol * max(|sig0|, 2e-8 mu)
 * (an absolute floor from the initial yield stress -- or from the shear modulus when sig0 is 0 -- and a relative term that
 * follows the trial von Mises stress of the point: csrc/small_strain.hpp, csrc/dxm_common.hpp J2Params.tol / .rtol).
 * FeFp solves two equations: the same bound on the yield residual (as a Kirchhoff stress) AND |det(be_bar) - 1| <= 1e-14.
 * Points that stop at maxit are counted in dxm_stats.n_not_converged (and are the positive return value of the integrate calls). */
int dxm_set_newton(dxm_material* m, int maxit, double rtol);

/* ---- state: set_initial_state_dict / get_initial_state_dict / get_final_state_dict
 *      (generic.py:194-201, jaxmat.py:199-206; consumers quadrature_map.py:279,294,356-360) -- */
/* host AoS (npoints, isv_dim[field]) -> device SoA of state `which` */
int dxm_set_state(dxm_material* m, int which, int field, const double* host_aos);
/* device SoA -> host AoS (npoints, isv_dim[field]) */
int dxm_get_state(dxm_material* m, int which, int field, double* host_aos);
/* DataManager.update(): s0 <- s1   (generic.py:212-213, jaxmat.py:39-40; quadrature_map.py:355) */
int dxm_advance(dxm_material* m);
/* DataManager.revert(): s1 <- s0   (generic.py:215-216, jaxmat.py:42-43) */
int dxm_revert(dxm_material* m);
/* Gradient and flux of a state (generic.py:194-201: get_initial_state_dict()["Strain"] / ["Stress"]) from the device copies
 * of the last HOST-BUFFER call: dxm_get_io(m, which, kind, host_aos) downloads the gradient (kind 0) or flux (kind 1),
 * (npoints, n_grad | n_flux).  With option "keep_initial_io" dxm_advance keeps the copies of the accepted state as those of s0
 * (a pointer swap).  A state accepted from a call without host arrays (device pointers; a fused displacement for the gradient)
 * holds no copy.  dxm_io_held(m, which): bit 0 = a gradient is held for that state, bit 1 = a flux (negative: bad arguments). */
int dxm_io_held(const dxm_material* m, int which);
int dxm_get_io(dxm_material* m, int which, int kind, double* host_aos);

/* ---- the hot path: Material.integrate(gradients, dt)  (jaxmat.py:208-234, generic.py:176-189;
 *      consumer quadrature_map.py:321) ------------------------------------------------------ */
/* Host-buffer form (what QuadratureMap hands over): grad_aos (npoints, n_grad) in host memory;
 * writes flux_aos (npoints, n_flux), isv_aos (npoints, n_isv_total) and ct_aos
 * (npoints, n_flux*n_grad) to host memory (any of the three may be NULL to skip its download; the ISVs
 * are only needed at advance() and can be fetched later with dxm_isv_host).
 * Reads state s0, writes state s1.  Synchronous.  `stats` may be NULL. */
int dxm_integrate(dxm_material* m, const double* grad_aos, double dt, double* flux_aos,
                  double* isv_aos, double* ct_aos, dxm_stats* stats);
/* The same for a QuadratureMap over a SUBSET of the cells (quadrature_map.py:66-73 with `cells`; one map per material in a
 * multi-material problem): grad_aos (npoints, n_grad) are the map's own points as above, but flux_rows / ct_rows are the BASES of
 * the quadrature Functions over ALL cells and point i belongs in their row rows[i] (the `dofs` index the map built once,
 * quadrature_map.py:231-233) -- what `_update_vals(field, values, cells)` does with a fancy assignment per array per update
 * (utils.py:136-143).  Of each point 80 B cross PCIe into the library's page-locked landing areas and the worker threads that
 * rebuild the (6, 6) blocks store them, and the stress, straight into their rows; the caller's arrays need not be page-locked.
 * (The elastic law's constant block is filled in by the same threads, the FeFp laws move their 54 building blocks + 9 stress
 * components per point.)  A handle with a packed tangent layout (DXM_TANGENT_SYM / _COEF / _PACK4): ct_rows has dxm_tangent_size
 * doubles per row, the kernel's own 21 / 9 / 4 numbers land and are moved to their rows as they are -- nothing is rebuilt.  The index
 * holds each row once and is NOT range-checked here (dxm_host_index_range is the check; the Python layer runs it per call);
 * internal state variables: bound with dxm_bind_isv_output they are delivered into their rows by the same call, else
 * dxm_isv_host / dxm_get_state when needed. */
int dxm_integrate_rows(dxm_material* m, const double* grad_aos, double dt, double* flux_rows, double* ct_rows,
                       const int64_t* rows, dxm_stats* stats);
/* Device-pointer form: all three arrays are device memory on the handle's device (e.g. torch
 * tensors' data_ptr()); the kernel is enqueued on `hip_stream` (a hipStream_t, NULL = default
 * stream) and the call returns without synchronising.  Returns 0 or < 0. */
int dxm_integrate_device(dxm_material* m, const double* grad_dev, double dt, double* flux_dev,
                         double* ct_dev, void* hip_stream);
/* Waits for the last integrate on the handle and returns its status (same code as dxm_integrate). */
int dxm_get_stats(dxm_material* m, dxm_stats* stats);
/* Packs the user-visible ISVs of state `which` into a device AoS (npoints, n_isv_total) array,
 * enqueued on hip_stream (the `_hcat_mixed` of jaxmat.py:46-58, :227-229, on device). */
int dxm_isv_device(dxm_material* m, int which, double* isv_aos_dev, void* hip_stream);
/* Device address of component `comp` of SoA state field `field` (npoints contiguous doubles).
 * The library cannot see what is written through such an address.  A handle whose state address was handed out (S0 or S1,
 * any field) therefore stops eliding state stores for good (option "elide_clean_state" below): from this call on its launches use
 * the kernel that rewrites s1 in full, and dxm_clean_tiles reports no clean tile. */
const double* dxm_state_ptr(const dxm_material* m, int which, int field, int comp);
/* The J2 laws: how many 64-point tiles of the handle are currently known to hold the same bytes in both state buffers (*clean), of
 * how many (*tiles = ceil(npoints / 64)); a launch with option "elide_clean_state" skips the state store of such a tile while no point
 * of it yields.  Waits for the last launch.  Other laws (and a custom-hardening build) report 0 of 0.  Returns 0 or < 0. */
int dxm_clean_tiles(dxm_material* m, int64_t* clean, int64_t* tiles);
/* The J2 laws: the packed copy of s0 that option "pack_old_state" keeps for the update kernel.  While a valid copy exists -- a launch
 * of the present load step has built it, and nothing may have changed s0 since -- *tiles_packed = ceil(npoints / 64), the tiles it
 * covers, and *points_kept the points held in it: those with a slot of s0 that is not bit-zero.  0 and 0 when there is no valid copy
 * (none built yet since the last dxm_advance / dxm_set_state / plain launch, option off, a state address handed out, other laws).
 * Waits for the last launch.  Returns 0 or < 0. */
int dxm_packed_state(dxm_material* m, int64_t* tiles_packed, int64_t* points_kept);
/* Rebuild full tangents from their coefficient form on the device: coef_dev (npoints, 9) as written with
 * DXM_TANGENT_COEF -> ct_dev (npoints, 36), the block DXM_TANGENT_FULL writes, bit for bit; asynchronous on
 * hip_stream of `device`.  For consumers that move the 72 B/point form (e.g. across xGMI: an all-gather of
 * coefficients followed by this kernel instead of an all-gather of 288 B/point blocks) and need the full block. */
int dxm_expand_tangent_device(const double* coef_dev, int64_t npoints, double* ct_dev, int device, void* hip_stream);
/* The same from the 32 B/point form: flux_dev (npoints, 6) the stress and pack_dev (npoints, 4) the (c1, c2, c3, w) of the
 * same update (DXM_TANGENT_PACK4) -> ct_dev (npoints, 36), bit for bit what DXM_TANGENT_FULL writes.  An all-gather of
 * stress + this form moves 80 instead of 120 (coefficients) or 336 (full blocks) B/point across xGMI. */
int dxm_expand_tangent_pack4_device(const double* flux_dev, const double* pack_dev, int64_t npoints, double* ct_dev, int device,
                                    void* hip_stream);
/* Name of the HIP kernel integrate launches for this handle (for profile filtering).  A J2 handle whose launches elide state stores
 * (option "elide_clean_state") runs the same tile body as small_strain_clean_kernel<law, layout>; the name reported stays that of the
 * plain kernel. */
const char* dxm_kernel_name(const dxm_material* m);
/* Identity of the launch configuration: changes whenever a launch captured into a HIP graph before would
 * no longer do what a fresh call does -- dxm_advance (the two state buffers swap: the low bit flips and
 * flips back at the next advance), dxm_set_params / dxm_set_newton / dxm_set_tangent_layout /
 * dxm_set_param_field(_device) / dxm_set_frame / dxm_set_frame_field(_device) / dxm_set_external_state* (a changed kind or uniform value) / dxm_set_option and anything else that moves the resident state (the upper bits increase).  Replay a captured graph only while the
 * value equals the one read at capture time.  dxm_revert does not change it. */
uint64_t dxm_launch_generation(const dxm_material* m);
/* Tell the handle that the caller has replayed a HIP graph containing a launch of this handle: the replay
 * is invisible to the library, but it rewrote state s1 (so the next dxm_advance must swap the buffers) and
 * the flux / tangent / stats.  Call after every replay, before dxm_advance / dxm_get_stats / dxm_get_state. */
int dxm_notify_replay(dxm_material* m);
/* Per-handle options (no environment variables are read by the library):
 *   "pipeline"       1 | 0   host-buffer form: chunked upload / kernel / download on several streams (default 1)
 *   "split_streams"  1 | 0   how the chunks use the streams when the gradient array is page-locked (DMA uploads).  1 (default):
 *                            uploads and kernels of all chunks on one stream, the downloads of chunk c on one of two others
 *                            behind an event (7 sqrt(npoints / 1e6) chunks, truncated, at least 1 and at most 24): the device-to-host direction, 80-136 B/point against 48 up, does
 *                            not wait behind uploads queued on its own stream.  0: whole chunks alternate between two streams
 *                            (rounds 1-5; still what staged uploads and the displacement forms use)
 *   "max_chunks"     1..64   upper bound on the chunks of that pipeline (default 64)
 *   "packed_transfer" 2|1|0  host-buffer form, full tangent layout, >= packed_min_points.  1: move the 9 coefficients
 *                            of Ct = c1 1x1 + c2 I + c3 n x n (72 instead of 288 B/point; nothing for the elastic
 *                            law) / for the FeFp laws the 54 building blocks of the 9x9 tangent (432 instead of
 *                            648 B/point), and rebuild the block on the host with the kernel's own expression.
 *                            2 (default): the J2 laws move (c1, c2, c3, w) only, 32 B/point -- the kernels build
 *                            the tangent with n = dev(stress) w, so the host rebuilds n from the stress it receives
 *                            anyway (needs a flux destination in page-locked / registered memory, else as 1); FeFp
 *                            as 1.  0: the full block crosses PCIe.  All three deliver the same bits.  A J2 handle with the
 *                            DXM_TANGENT_SYM layout: 2 moves (c1, c2, c3, w) as well and the workers rebuild its 21 entries
 *                            (32 instead of 168 B/point over PCIe); 1 | 0 download the kernel's 21 entries
 *   "register_input" 2 | 1 | 0  host-buffer form, gradient array in ordinary (pageable) memory.  2: page-locked for the
 *                            duration of the call (hipHostRegister ... hipHostUnregister before the call returns) and
 *                            uploaded by DMA: ~1 ms per 480 MB on transparent huge pages (numpy's default).  Arrays on
 *                            4 KiB pages register slowly (7-17 ms): after three such registrations in a row the handle
 *                            stages the next 20 calls.  0: always staged through the page-locked ring by the worker
 *                            threads.  1 (default): the handle measures -- calls 2-5 alternate between the two, the
 *                            faster (by the whole call; page-locking wins within 5 %) is kept and the other one is
 *                            tried again once in 32 calls; which one wins depends on the host (2-3 ms either way on
 *                            most, 5-9 ms for staging on some).  dxm_stats.upload reports what each call did
 *   "keep_initial_io" 0 | 1  dxm_advance keeps the device copies of gradient and flux of the accepted state as those of
 *                            s0 (dxm_get_io above); default 0
 *   "query_foreign_pointers" 1 | 0  (process-wide) host pointers that this library did not page-lock itself
 *                            (dxm_host_alloc / dxm_host_register) are looked up with hipPointerGetAttributes (1,
 *                            default) or treated as pageable and staged (0)
 *   "packed_min_points" >= 0 batch size from which packed_transfer applies (default 32768: below, waking the
 *                            worker threads costs what the bytes save)
 *   "pageable_dma"   0 | 1   host-buffer form: 1 hands gradient / result arrays in ordinary (pageable) memory to the
 *                            runtime's own transfer path instead of staging them through page-locked memory.  Faster
 *                            (the strain upload then costs the host nothing), but exposed to the runtime's cache of
 *                            on-the-fly page-locked ranges: with host arrays that are freed and reallocated between
 *                            calls, about one process in 25 of the test suite died with "Memory access fault by GPU"
 *                            (DESIGN.md section 1).  Default 0
 *   "host_threads"   1..256  worker threads of that rebuild and of the staging copies (default 16)
 *   "fused_gradient" 1 | 0   displacement forms: evaluate the gradient inside the update kernel where the mesh
 *                            allows (default 1)
 *   "blocks_per_cu"  1..256  grid size of the update kernel in workgroups per CU (default 32 small strain,
 *                            the resident 2 for FeFp)
 *   "elide_clean_state" 1 | 0  the J2 laws (uniform parameters, strain-array forms): a 64-point tile without a yielding point
 *                            stores into s1 exactly the bits it read from s0; 1 (default) skips that store where the handle knows
 *                            that s1 holds them already (one 32-bit stamp per tile), 56 of 496 B/point for
 *                            such a tile.  Results and both state buffers are bit for bit those of 0.  Launches captured into a
 *                            HIP graph, launches with parameter fields or a fused gradient, and every launch after dxm_state_ptr
 *                            use the kernel of 0; a replayed graph must be reported with dxm_notify_replay as before
 *   "pack_old_state" 1 | 0   the J2 laws, where "elide_clean_state" applies and the launch covers all points of the handle (device-
 *                            pointer form): s0 does not change between the updates of one load step, and a point that has never
 *                            yielded holds seven zeros there.  With 1 the second such launch since s0 last changed also writes a
 *                            packed copy of s0 -- per 64-point tile one 64-bit mask and the slots of the points that are not all
 *                            bit-zero -- and the later ones read that copy instead of s0: 56 B less per never-yielded point.
 *                            Results and both state buffers are bit for bit those of 0.  The copy costs +56 B/point of device memory
 *                            from its first build on (without it if that allocation fails); dxm_advance, dxm_set_state, a launch
 *                            of another form and dxm_state_ptr (for good) end its validity, dxm_revert and dxm_notify_replay do
 *                            not; 0 frees it (default 1; dxm_packed_state reports)
 *   "verbose"        0 | 1   host-buffer form: log the chunk timeline, page-locking and upload-mode decisions to stderr (default 0) */
int dxm_set_option(dxm_material* m, const char* name, double value);
/* get_initial_state_dict / get_final_state_dict without a device array of the caller: packs the
 * user-visible ISVs of state `which` and downloads them into host memory (npoints, n_isv_total).  This is
 * how the Python layer serves the `isv` array of integrate() on first access (jaxmat.py:227-229). */
int dxm_isv_host(dxm_material* m, int which, double* isv_aos);
/* QuadratureMap.update writes every internal state variable into its quadrature Function after each integrate
 * (quadrature_map.py:332, :343-348: `_update_vals(isv, isv_vals[:, buff:buff+dim], cells)`).  Bind the memory of such a Function --
 * C-contiguous (npoints, dim) rows of field `field`, page-locked by dxm_host_alloc / dxm_host_register -- and the host-buffer
 * forms (dxm_integrate, dxm_integrate_displacement, ..._rows) deliver that field of the final state into it chunk by chunk inside
 * their transfer pipeline: the caller finds the Functions written when the call returns, without a second pass over the state.
 * NULL unbinds (do so before un-page-locking the array).  The device-pointer forms do not deliver.
 * In the rows forms (dxm_integrate_rows, dxm_integrate_displacement_rows) the bound pointer is, like their flux / tangent arguments,
 * the BASE of the Function over all cells: the field of point i goes to its row rows[i] (stored by the worker threads from the
 * library's own page-locked landing area).  A handle serves either kind of call with a given binding, not both. */
int dxm_bind_isv_output(dxm_material* m, int field, double* host_aos);

/* ---- pinned host memory for the host-buffer form --------------------------------------------
 * integrate() returns arrays owned by the material (the reference returns views of its state
 * manager: generic.py:185-189); allocating them page-locked lets the D2H copies run at full PCIe
 * rate without the runtime's staging copy.  Returns NULL on failure.
 * Output arrays in ordinary (pageable) memory are accepted everywhere, but the library never lets the GPU write into
 * them directly: they are filled through its own page-locked staging and a CPU copy, after the transfers of the call
 * (slower; and not subject to the runtime's cache of on-the-fly page-locked ranges -- DESIGN.md section 1). */
void* dxm_host_alloc(uint64_t bytes);
int dxm_host_free(void* p);
/* Page-lock an existing host range in place (e.g. the `x.array` of the dolfinx quadrature Functions that
 * QuadratureMap.update scatters into, quadrature_map.py:331-334, utils.py:136-143), so that integrate()
 * can deliver straight into it at full PCIe rate; undo with dxm_host_unregister before the memory is freed. */
/* bytes from src to dst (host memory, non-overlapping) on `threads` threads (<= 0: 8): a 480 MB numpy copy takes 50 ms on one
 * core; the Python layer snapshots bound gradient / flux arrays with this when an increment is accepted. */
int dxm_host_copy(void* dst, const void* src, uint64_t bytes, int threads);
/* Rows of `width` doubles through an index on `threads` threads (<= 0: 8), host memory, no overlap between dst and src:
 * scatter: dst[rows[i]] = src[i]; gather: dst[i] = src[rows[i]] for i < n.  What a QuadratureMap over a SUBSET of the cells does
 * with every array per update (utils.py:136-143 `array[index] = values`, quadrature_map.py:271 `_get_vals(f)[self.dofs]`);
 * the index holds each row once (the caller's responsibility, as in the reference) and is not range-checked. */
int dxm_host_scatter_rows(double* dst, const double* src, const int64_t* rows, int64_t n, int width, int threads);
int dxm_host_gather_rows(double* dst, const double* src, const int64_t* rows, int64_t n, int width, int threads);
/* Smallest and largest entry of such an index on `threads` threads (<= 0: 8): the range check that dxm_integrate_rows and the
 * two calls above leave to the caller (~1 ms per 1e7 entries).  n == 0: *lo = INT64_MAX, *hi = INT64_MIN. */
int dxm_host_index_range(const int64_t* rows, int64_t n, int threads, int64_t* lo, int64_t* hi);
int dxm_host_register(void* p, uint64_t bytes);
int dxm_host_unregister(void* p);

/* ---- gradient evaluation on device (the step before the path; hex8, tet4, Lagrange simplices of any order) --
 * Replaces, for the device-resident flow, QuadratureExpression.eval -> fem.Expression.eval
 * (quadrature_function.py:45-51; consumer quadrature_map.py:247-253): only the displacement
 * vector crosses PCIe, the (npoints, n_grad) gradient array is produced in HBM in the layout
 * the constitutive kernels read (point = cell * nqp + q). */
typedef struct dxm_mesh dxm_mesh; /* opaque: device copies of coordinates and connectivity */
/* coords (n_nodes,3) fp64, conn (n_cells,8) int32 with the corner order
 * (-,-,-)(+,-,-)(+,+,-)(-,+,-)(-,-,+)(+,-,+)(+,+,+)(-,+,+); qpoints (nqp,3) in [-1,1]^3, nqp <= 27. */
dxm_mesh* dxm_mesh_create_hex8(const double* coords, int64_t n_nodes, const int32_t* conn,
                               int64_t n_cells, const double* qpoints, int nqp, int device);
/* First-order tetrahedra: conn (n_cells,4); the gradient is constant per cell and repeated at the
 * cell's nqp Gauss points (point = cell * nqp + q). */
dxm_mesh* dxm_mesh_create_tet4(const double* coords, int64_t n_nodes, const int32_t* conn,
                               int64_t n_cells, int nqp, int device);
/* Lagrange displacement of any order on STRAIGHT-SIDED simplices (tdim 3: tetrahedra, tdim 2: triangles, embedded as
 * plane strain: eps_zz = 0 / F_zz = 1) -- the P2 spaces of the reference's demos
 * (demos/jax/finite_strain_elastoplasticity/finite_strain_elastoplasticity.py:115-117 tet10 with 4 points,
 * demos/jax/elastoplasticity/plane_elastoplasticity.py:96-100 tri6 with 3 points).  The geometry map is affine and
 * comes from the tdim+1 vertices of each cell: coords (n_vertices,3) [dolfinx geometry.x is 3-wide in 2-D too],
 * geom_conn (n_cells, tdim+1).  The displacement has its own dofmap (n_cells, nd) into a vector of n_dofs blocks of tdim
 * components [u.x.array of a (tdim,)-shaped space], and dphi (nqp, nd, tdim) holds the reference derivatives
 * d N_m / d xi_d of its nd shape functions at the nqp quadrature points, in the dofmap's local ordering
 * [basix: element.tabulate(1, points)[1:, :, :, 0] transposed to (point, dof, direction)]. */
dxm_mesh* dxm_mesh_create_simplex(int tdim, const double* coords, int64_t n_vertices, const int32_t* geom_conn,
                                  int64_t n_cells, const int32_t* dofmap, int nd, int64_t n_dofs,
                                  const double* dphi, int nqp, int device);
/* Lagrange displacement of any order on triangles (nv = 3) or bilinear quadrilaterals (nv = 4), two components per dof.
 * Geometry from the nv vertices of a cell through geom_dphi (nqp, nv, 2), the reference derivatives of the geometry's shape
 * functions at the Gauss points; the field through its own dofmap (n_cells, nd) and dphi (nqp, nd, 2).  Both tables refer to the
 * same reference coordinates.  coords (n_vertices, 3), third column ignored.  Point c * nqp + q is Gauss point q of cell c.
 * nd <= 64, nqp <= 64.  Checked on the host, in this order, before a device is asked for: the arguments; every geom_conn and
 * dofmap entry in range; det J finite, not zero and of one sign within each cell at every Gauss point (the message names the
 * cell; a bow-tie quadrilateral is refused here).  The mesh answers every kind of dxm_mesh_gradient_device (kinds 0 and 1 embedded
 * as for triangles above); the displacement forms run its gradient kernel on its own, then the update kernel (no fused form).
 * A custom-hardening build creates such a mesh but refuses its gradient, and kinds 2 and 3 on any mesh: those kernels are the
 * stock library's. */
dxm_mesh* dxm_mesh_create_plane(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                const int32_t* dofmap, int nd, int64_t n_dofs,
                                const double* geom_dphi, const double* dphi, int nqp, int device);
/* A SCALAR Lagrange field (a temperature) of any order on the same cells: ONE value per dof, dxm_mesh_displacement_size = n_dofs.
 * phi (nqp, nd) holds the values of the field's nd shape functions at the Gauss points beside their derivatives dphi (nqp, nd, 2);
 * the other arguments, the bounds and the host-side checks are those of dxm_mesh_create_plane, in the same order and with the same
 * sentences (arguments; indices; det J; the device), all reached without a GPU; after the arguments it also refuses a table entry
 * (phi, dphi, geom_dphi) that is not finite.  The mesh serves dxm_mesh_scalar_gradient_device and, with DXM_LAW_HEAT_STATIONARY_2D /
 * DXM_LAW_HEAT_PHASE_CHANGE_2D, the displacement forms, which then take the nodal temperature; it refuses every kind of
 * dxm_mesh_gradient_device.  A custom-hardening build creates such a mesh and refuses both uses. */
dxm_mesh* dxm_mesh_create_plane_scalar(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                       const int32_t* dofmap, int nd, int64_t n_dofs,
                                       const double* geom_dphi, const double* phi, const double* dphi, int nqp, int device);
/* An AXISYMMETRIC mesh: the same cells in the meridian half plane, column 0 of coords is r, column 1 is z, and the two components
 * per dof are (u_r, u_z).  Under MGIS's axisymmetric hypothesis a symmetric tensor is [rr, zz, tt, sqrt(2) rz] and F is
 * [F_rr, F_zz, F_tt, F_rz, F_zr]: the slots of the plane-strain hypothesis, with the hoop terms eps_tt = u_r / r, F_tt = 1 + u_r / r
 * where plane strain has 0 and 1.  So the hypothesis lives on the MESH: a DXM_LAW_PE_* handle, or a 6- / 9-wide one, on this mesh is
 * the axisymmetric law.  The arguments are those of dxm_mesh_create_plane plus the VALUES of the shape functions at the Gauss
 * points: geom_phi (nqp, nv) of the geometry's (for r) and phi (nqp, nd) of the field's (for u_r).  Checked on the host, in this
 * order and with the sentences of dxm_mesh_create_plane, before a device is asked for: the arguments; the indices; det J; every
 * entry of the four tables finite; r = sum_v r_v geom_phi[q][v] finite and > 0 at every Gauss point (the message names the cell: the
 * mesh must lie on one side of the axis, with no Gauss point on it); the device last.  dxm_mesh_displacement_size = 2 n_dofs.
 * The mesh serves dxm_mesh_axisymmetric_gradient_device and the displacement forms; it refuses every kind of
 * dxm_mesh_gradient_device and dxm_mesh_scalar_gradient_device.  Straight-sided (first-order) cells only.  A custom-hardening build
 * creates such a mesh and refuses its gradient. */
dxm_mesh* dxm_mesh_create_axisymmetric(const double* coords, int64_t n_vertices, const int32_t* geom_conn, int nv, int64_t n_cells,
                                       const int32_t* dofmap, int nd, int64_t n_dofs,
                                       const double* geom_phi, const double* geom_dphi, const double* phi, const double* dphi,
                                       int nqp, int device);
int dxm_mesh_destroy(dxm_mesh* mesh);
int64_t dxm_mesh_npoints(const dxm_mesh* mesh);
/* doubles in the displacement vector the mesh expects (3 per node; tdim per dof for dxm_mesh_create_simplex; 2 per dof for
 * dxm_mesh_create_plane and dxm_mesh_create_axisymmetric; 1 per dof for dxm_mesh_create_plane_scalar) */
int64_t dxm_mesh_displacement_size(const dxm_mesh* mesh);
/* kind 0: Mandel strain (6); kind 1: deformation gradient F = I + grad u (9); on two-dimensional meshes only
 * (dxm_mesh_create_plane, dxm_mesh_create_simplex with tdim 2; any other mesh refuses them), with H[i][a] = du_i / dX_a and
 * r = sqrt(2)/2: kind 2 the plane-strain 4-vector [H00, H11, 0.0, r (H01 + H10)] of DXM_LAW_PE_*, kind 3 the in-plane 3-vector
 * [H00, H11, r (H01 + H10)] of the plane-stress laws.  u_dev: device (dxm_mesh_displacement_size doubles); grad_dev: device
 * (npoints, 6|9|4|3).  Asynchronous on hip_stream. */
int dxm_mesh_gradient_device(dxm_mesh* mesh, const double* u_dev, int kind, double* grad_dev,
                             void* hip_stream);
/* On a scalar mesh: grad(T) = Ji^T sum_m T_m dphi_m into grad_dev (npoints, 2; 16-byte aligned) and, unless value_dev is NULL,
 * T = sum_m T_m phi_m into value_dev (npoints) at the Gauss points, from the nodal values t_dev (n_dofs doubles); point c * nqp + q
 * is Gauss point q of cell c.  All device memory; asynchronous on hip_stream.  Every operation is individually rounded, the sums
 * run in the dofmap's local order: the update kernels of the nodal forms evaluate the same text and deliver the same bits.  A mesh
 * that carries a displacement refuses (< 0, message); a refused call writes nothing. */
int dxm_mesh_scalar_gradient_device(dxm_mesh* mesh, const double* t_dev, double* grad_dev, double* value_dev, void* hip_stream);
/* On an axisymmetric mesh (dxm_mesh_create_axisymmetric; any other mesh is refused: its gradients are those of
 * dxm_mesh_gradient_device), with H[i][a] = du_i / dX_a in (r, z), hoop = u_r / r and s = sqrt(2)/2; the kinds are numbered by this
 * entry point alone:
 *   kind 0: [H00, H11, hoop, s (H01 + H10)]                                 (npoints, 4)  the strain of the DXM_LAW_PE_* rows
 *   kind 1: [1 + H00, 1 + H11, 1 + hoop, H01, H10]                          (npoints, 5)  the F of DXM_LAW_OGDEN_PE / DXM_LAW_LOG_STRAIN_PE
 *   kind 2: [H00, H11, hoop, s (H01 + H10), 0, 0]                           (npoints, 6)  the Mandel strain of the 6-wide laws
 *   kind 3: [1 + H00, 1 + H11, 1 + hoop, H01, H10, 0, 0, 0, 0]              (npoints, 9)  the F of the 9-wide laws
 * u_dev (2 n_dofs doubles) and grad_dev are device memory; grad_dev 16-byte aligned for kinds 0 and 2.  Unless radius_dev is NULL,
 * r at the Gauss points goes into radius_dev (npoints): the measure of the hypothesis is 2 pi r w |det J|.  Asynchronous on
 * hip_stream and capturable.  The sums run in the tables' local order (products fused with their sums, as in the plane gradient
 * kernels): a restatement in that order agrees at rounding level.  A refused call (< 0, message) writes nothing.
 * The displacement forms below accept such a mesh: this kernel fills the handle's scratch array, the update kernel follows on the
 * same stream (no fused form; the option fused_gradient makes no difference).  The kind follows the law's gradient width: the
 * 4-wide plane-strain rows kind 0, the 6-wide laws kind 2, the 9-wide laws kind 3.  Refused, the handle left usable: the 3-wide
 * plane-stress rows (plane stress and axisymmetry exclude each other), the heat-transfer laws (a scalar mesh), DXM_LAW_OGDEN_PE and
 * DXM_LAW_LOG_STRAIN_PE (their rows' own sentence: evaluate kind 1, then call the array form), every law that takes no displacement
 * on any mesh, a device mismatch and a point-count mismatch. */
int dxm_mesh_axisymmetric_gradient_device(dxm_mesh* mesh, const double* u_dev, int kind, double* grad_dev, double* radius_dev,
                                          void* hip_stream);
/* dxm_integrate with the gradient computed on the device from the host displacement vector
 * u_host (dxm_mesh_displacement_size doubles): uploads u, evaluates the law's gradient, runs the constitutive update,
 * downloads flux / isv / tangent (any may be NULL).  mesh npoints must equal the handle's. */
int dxm_integrate_displacement(dxm_material* m, dxm_mesh* mesh, const double* u_host, double dt,
                               double* flux_aos, double* isv_aos, double* ct_aos, dxm_stats* stats);
/* The same with the results delivered into rows of larger arrays, as dxm_integrate_rows does: `mesh` holds the cells of ONE
 * material's map (connectivity restricted to its cells, coordinates / displacement vector of the whole mesh), flux_rows /
 * ct_rows are the quadrature Functions over all cells, point i goes to their row rows[i]. */
int dxm_integrate_displacement_rows(dxm_material* m, dxm_mesh* mesh, const double* u_host, double dt, double* flux_rows,
                                    double* ct_rows, const int64_t* rows, dxm_stats* stats);

/* Device-resident form of dxm_integrate_displacement: u_dev (dxm_mesh_displacement_size doubles), flux_dev, ct_dev are device
 * arrays, the call is asynchronous on hip_stream and capturable like dxm_integrate_device.  For
 * hexahedra with 8 Gauss points per cell, for tetrahedra and for Lagrange simplices the gradient is evaluated inside the
 * update kernel (no strain / deformation-gradient array is written or read); otherwise (every law on a plane mesh, the 4-wide
 * and 3-wide laws on any two-dimensional mesh) the gradient kernel fills a scratch array owned by the handle and the update
 * kernel follows on the same stream. */
int dxm_integrate_displacement_device(dxm_material* m, dxm_mesh* mesh, const double* u_dev, double dt,
                                      double* flux_dev, double* ct_dev, void* hip_stream);


#ifdef __cplusplus
}
#endif
#endif /* DXMAT_H */
