// Small-strain FCC single-crystal viscoplasticity (the reference's MericCailletaudSingleCrystalViscoPlasticity behaviour, restated
// from its equations) with a material frame per handle or per Gauss point, for gfx950.  Gradient: strain (6), flux: stress (6),
// Mandel [11, 22, 33, sqrt2 12, sqrt2 13, sqrt2 23]; the tangent is a full 6x6 that is NOT symmetric (interaction hardening).
//
// The law, in the material frame (rows of R = material axes; eps_m = Q eps, sigma = Q^T sigma_m, Ct = Q^T Ct_m Q as in
// orthotropic.hip): orthotropic stiffness D, twelve {111}<01-1> systems with mu_i = Mandel(sym(s_i x n_i)) (single_crystal.hpp),
// unknowns the twelve slip increments dg of an implicit step (theta = 1) of length dt:
//   eel_tr = eps_m - sum g_i mu_i,  sigma = D (eel_tr - sum dg_i mu_i),  tau_i = sigma . mu_i = tau_tr_i - sum_j M_ij dg_j,
//   r_i = tau0 + Q sum_j h_ij (1 - exp(-b (p_j + |dg_j|))),   da_i = (dg_i - d a_i |dg_i|) / (1 + d |dg_i|),   x_i = C (a_i + da_i),
//   f_i = max(|tau_i - x_i| - r_i, 0),  s_i = sgn(tau_i - x_i),   residual  fg_i = dg_i - dt (f_i / K)^n s_i,
//   J_ij = delta_ij + dt dv_i (M_ij + C dda_i delta_ij + s_i Q b h_ij exp(-b (p_j + |dg_j|)) sgn(dg_j)),
//   dv_i = n (f_i / K)^n / max(f_i, 1e-12 D_00),  dda_i = (1 - d a_i sgn(dg_i)) / (1 + d |dg_i|)^2     (sgn(0) = -1 as in the file),
//   Ct_m = D - B^T J^-1 W B,  B_i = D mu_i,  W = diag(dt dv);     state: g += dg, p += |dg|, a += da, eel.
// Newton from dg = 0; an iterate with any f_i > 1.1 K is rejected and the last step halved (at dg = 0 there is none: the point
// writes its elastic trial and keeps its state bits); stop at max |fg_i| <= rtol, then apply the correction of the factorisation
// the tangent needs anyway.
//
// Mapping.  Around the Newton: one thread per point, one wave per tile of 64, the tile I/O as the shared text of tile_rows6_*.hpp
// and stage_full36_store.hpp.  The Newton itself: ONE LANE PER SLIP SYSTEM, 16 lanes per point (12 working), four points per round,
// rounds over the tile's points with any f_i > 0.  A lane holds its row of [J | fg | 6 tangent right-hand sides] (19 doubles);
// Gauss-Jordan with partial pivoting needs no row swap (the pivot row is the unused lane with the largest entry, found and read
// by shuffles within the 16-lane row).  Wave-private LDS only, no s_barrier inside the tile loop.
#include "single_crystal.hpp"

namespace dxm {

__device__ __forceinline__ double sc_push(double v, int dst_lane) {   // lane dst_lane receives v (a permutation within the wave)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_ds_permute(dst_lane << 2, lo);
  hi = __builtin_amdgcn_ds_permute(dst_lane << 2, hi);
  return __hiloint2double(hi, lo);
}

// entry (a, k) of the material-frame stiffness
#define SC_D(a, k) (((a) < 3 && (k) < 3) ? A[(a)][(k)] : (((a) == (k)) ? C.g2[((a) < 3 ? 0 : (a) - 3)] : 0.0))

template <int FRAME>
__global__ void __launch_bounds__(SC_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
single_crystal_kernel(const LawParams prm, const ScParams sp, const int64_t n, const double* __restrict__ eps, const Frame9 uniform,
                      const double* __restrict__ frames, const int64_t ldf, const double* __restrict__ s0, double* __restrict__ s1,
                      const int64_t ld, double* __restrict__ sig, double* __restrict__ ct, BlockStats* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double lds_all[SC_WAVES * SC_LDS_PER_WAVE];
  __shared__ double sys_tab[16 * SC_SYS];   // per slip system: B_i (6), row i of M (12), row i of Q h (12)
  __shared__ double dmat[36];               // the material-frame stiffness, row-major
  __shared__ unsigned long long red[4 * SC_WAVES];
  static_assert(SC_LDS_BYTES == sizeof(lds_all) + sizeof(sys_tab) + sizeof(dmat) + sizeof(red), "single_crystal.hpp states the LDS of the kernel");

  int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  double* t36 = lds_all + wid * SC_LDS_PER_WAVE;                   // 64 x 36 tangent entries
  double* hand = t36 + WAVE * 36;                                  // 4 x SC_ROUND hand-over words
  double2_t* stage2 = reinterpret_cast<double2_t*>(t36);           // strain in / stress out staging: the head of the same region

  const int64_t ntiles = (n + WAVE - 1) / WAVE;
  const int64_t tile_stride = (int64_t)gridDim.x * SC_WAVES;
  unsigned long long c_plastic = 0, c_notconv = 0, c_nan = 0, c_maxit = 0;

  const OrthoStiffness C = ortho_load(prm);
  const double A[3][3] = {{C.c[0], C.c[1], C.c[2]}, {C.c[1], C.c[4], C.c[5]}, {C.c[2], C.c[5], C.c[8]}};
  const double SQ2 = 1.4142135623730950488;

  // ---- the slip system of this lane in the Newton rounds: B_i = D mu_i, row i of M = mu D mu^T and of Q h ------------------
  const int li = threadIdx.x & 15;
  const int grp = (threadIdx.x >> 4) & 3;
  if (threadIdx.x < 16) {
    double Bi[6], Mrow[SC_NSYS], QHrow[SC_NSYS];
    double mui[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < SC_NSYS; ++i)
#pragma unroll
      for (int c = 0; c < 6; ++c) mui[c] = (li == i) ? SC.mu[i][c] : mui[c];
#pragma unroll
    for (int a = 0; a < 3; ++a) Bi[a] = __builtin_fma(A[a][2], mui[2], __builtin_fma(A[a][1], mui[1], A[a][0] * mui[0]));
#pragma unroll
    for (int s = 0; s < 3; ++s) Bi[3 + s] = C.g2[s] * mui[3 + s];
#pragma unroll
    for (int j = 0; j < SC_NSYS; ++j) {
      double t = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c)
        if (SC.mu[j][c] != 0.0) t = __builtin_fma(Bi[c], SC.mu[j][c], t);
      Mrow[j] = t;
      double q = 0.0;
#pragma unroll
      for (int i = 0; i < SC_NSYS; ++i) q = (li == i) ? sp.qh[SC.cls[i][j]] : q;
      QHrow[j] = q;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) sys_tab[li * SC_SYS + c] = Bi[c];
#pragma unroll
    for (int j = 0; j < SC_NSYS; ++j) { sys_tab[li * SC_SYS + 6 + j] = Mrow[j]; sys_tab[li * SC_SYS + 18 + j] = QHrow[j]; }
  }
  if (threadIdx.x >= 64 && threadIdx.x < 64 + 36) {
    double v = 0.0;
#pragma unroll
    for (int eidx = 0; eidx < 36; ++eidx) v = ((int)threadIdx.x - 64 == eidx) ? SC_D(eidx / 6, eidx % 6) : v;
    dmat[threadIdx.x - 64] = v;
  }
  __syncthreads();   // once, ahead of the tile loop
  // read through an opaque copy of this address wherever they are used: hoisted out of the Newton loop the 30 doubles cost 60 VGPRs
  const double* const sys_row = sys_tab + li * SC_SYS;
#define SC_SYS_ROW(name)       \
  const double* name = sys_row; \
  asm volatile("" : "+v"(name))

  for (int64_t tile = (int64_t)blockIdx.x * SC_WAVES + wid; tile < ntiles; tile += tile_stride) {
    const int64_t base = tile * WAVE;
    const int npts = (n - base) < WAVE ? (int)(n - base) : WAVE;
    // per-lane invariants are re-derived per tile from an opaque copy (small_strain.hpp: hoisted, they cost registers over the whole body)
    asm volatile("" : "+v"(lane));
    lane &= WAVE - 1;
    const bool valid = lane < npts;

    // ---- 1. coalesced strain load (3 x 1 KiB per wave) into LDS; the frame of the point ------------------------------
    double e[6];
#include "tile_rows6_load.hpp"
    double R[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    auto load_frame = [&]() {
      if constexpr (FRAME == OR_FRAME_FIELD) {
        if (valid) {
#pragma unroll
          for (int k = 0; k < 9; ++k) R[k / 3][k % 3] = stream_load<3>(frames + ((int64_t)k * ldf + base) + (unsigned)lane);
        }
      } else if constexpr (FRAME == OR_FRAME_UNIFORM) {
        // an opaque copy per use: the 36 entries of Q are not carried over the rounds in registers
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          double r = uniform.r[k];
          asm volatile("" : "+v"(r));
          R[k / 3][k % 3] = r;
        }
      }
    };
    load_frame();
    wave_lds_sync();
#include "tile_rows6_take.hpp"
    wave_lds_sync();   // the staging region is the head of the tangent records written below

    // state slot accesses: a wave-uniform base and the lane as a 32-bit offset (42 + 36 per-lane 64-bit addresses cost the registers)
    // `sl` is the lane, as an opaque copy per phase: the 64-bit addresses of one phase are not kept for the next (36 of them
    // carried over the rounds cost 72 VGPRs)
    int sl = lane;
    auto load0 = [&](int slot) { return stream_load<3>(s0 + ((int64_t)slot * ld + base) + (unsigned)sl); };
    auto store1 = [&](int slot, double v) { stream_store<1>(s1 + ((int64_t)slot * ld + base) + (unsigned)sl, v); };
    // the Mandel image of R, row I (recomputed where it is needed: 36 entries are not carried over the Newton rounds)
    auto Qrow = [&](int I, double* q) {
#pragma unroll
      for (int K = 0; K < 6; ++K) {
        const int i = SI[I], j = SJ[I], k = SI[K], l = SJ[K];
        if (I < 3 && K < 3) q[K] = R[i][k] * R[i][k];
        else if (I < 3) q[K] = SQ2 * (R[i][k] * R[i][l]);
        else if (K < 3) q[K] = SQ2 * (R[i][k] * R[j][k]);
        else q[K] = __builtin_fma(R[i][k], R[j][l], R[i][l] * R[j][k]);
      }
    };
    // the trial elastic strain of the point in the material frame, from the strain and the slips of s0
    auto trial_strain = [&](const double* g, double* et) {
      if constexpr (FRAME == OR_FRAME_NONE) {
#pragma unroll
        for (int c = 0; c < 6; ++c) et[c] = e[c];
      } else {
#pragma unroll
        for (int I = 0; I < 6; ++I) {
          double q[6];
          Qrow(I, q);
          double t = q[0] * e[0];
#pragma unroll
          for (int K = 1; K < 6; ++K) t = __builtin_fma(q[K], e[K], t);
          et[I] = t;
        }
      }
#pragma unroll
      for (int i = 0; i < SC_NSYS; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c)
          if (SC.mu[i][c] != 0.0) et[c] = __builtin_fma(-g[i], SC.mu[i][c], et[c]);
    };
    auto stiffness = [&](const double* v, double* out) {
#pragma unroll
      for (int a = 0; a < 3; ++a) out[a] = __builtin_fma(A[a][2], v[2], __builtin_fma(A[a][1], v[1], A[a][0] * v[0]));
#pragma unroll
      for (int s = 0; s < 3; ++s) out[3 + s] = C.g2[s] * v[3 + s];
    };

    int ro = lane * 36;   // opaque: every access is base + small immediate
    asm volatile("" : "+v"(ro));
    double* rec = t36 + ro;

    // ---- 2. trial state: resolved shear stresses against the hardened thresholds at dg = 0 ----------------------------
    bool plastic = false;
    {
      double et[6];
      {
        double g[SC_NSYS];
#pragma unroll
        for (int i = 0; i < SC_NSYS; ++i) g[i] = valid ? load0(SC_SLOT_G + i) : 0.0;
        trial_strain(g, et);
      }
      __builtin_amdgcn_sched_barrier(0);   // phase after phase: scheduled together, the loads of all of them are in flight at once
      double om[SC_NSYS];   // 1 - exp(-b p_j)
#pragma unroll
      for (int j = 0; j < SC_NSYS; ++j) {
        const double p = valid ? load0(SC_SLOT_P + j) : 0.0;
        om[j] = 1.0 - exp(-sp.b * p);
      }
      __builtin_amdgcn_sched_barrier(0);
      // system after system, rolled: tau_i = B_i . eel_tr and row i of Q h come from the workgroup's table
#pragma unroll 1
      for (int i = 0; i < SC_NSYS; ++i) {
        const double* sr = sys_tab + i * SC_SYS;
        double tau = sr[0] * et[0];
#pragma unroll
        for (int c = 1; c < 6; ++c) tau = __builtin_fma(sr[c], et[c], tau);
        double r = sp.tau0;
#pragma unroll
        for (int j = 0; j < SC_NSYS; ++j) r = __builtin_fma(sr[18 + j], om[j], r);
        const double a = valid ? load0(SC_SLOT_A + i) : 0.0;
        plastic = plastic || (fabs(tau - sp.C * a) - r > 0.0);
        rec[i] = tau;   // parked in the point's own record until its round
      }
      plastic = plastic && valid;
    }
    wave_lds_sync();

    // ---- 3. Newton rounds: four yielded points at a time, one lane per slip system -----------------------------------
    double dg[SC_NSYS];
#pragma unroll
    for (int i = 0; i < SC_NSYS; ++i) dg[i] = 0.0;
    int status = 0;   // 1: iteration cap, 2: the guard tripped at dg = 0
    unsigned iters = 0;
    const unsigned long long pm = __ballot(plastic);
    const int nyield = __popcll(pm);
    const int rank = __popcll(pm & ((1ull << lane) - 1ull));
    for (int r0 = 0; r0 < nyield; r0 += 4) {
      int owner = -1;   // the tile-local point of this 16-lane row
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned long long mk = __ballot(plastic && rank == r0 + k);
        const int o = mk ? __ffsll((long long)mk) - 1 : -1;
        owner = (grp == k) ? o : owner;
      }
      const bool work = owner >= 0 && li < SC_NSYS;
      const double tau_tr = work ? t36[owner * 36 + li] : 0.0;
      const double p_i = work ? s0[(int64_t)(SC_SLOT_P + li) * ld + base + owner] : 0.0;
      const double a_i = work ? s0[(int64_t)(SC_SLOT_A + li) * ld + base + owner] : 0.0;
      wave_lds_sync();   // the records are rewritten below

      double dgi = 0.0, step = 0.0;
      double X6[6] = {0, 0, 0, 0, 0, 0};   // row i of J^-1 W B at the accepted iterate
      unsigned it = 0;
      int st_g = 0;
      bool done = owner < 0;
      const int sh = lane & 48;
      for (;;) {
        // everybody's increment and hardening exponential
        const double adg = fabs(dgi);
        const double Ei = exp(-sp.b * (p_i + adg));
        double row[19];   // my row of [J | fg | W B]; first the hardening part of J_ij without its factor s_i b
        SC_SYS_ROW(sys1);
        const double* Mrow = sys1 + 6;
        const double* QHrow = sys1 + 18;
        double tau = tau_tr, r = sp.tau0;
#pragma unroll
        for (int j = 0; j < SC_NSYS; ++j) {
          const double dgj = __shfl(dgi, j, 16), Ej = __shfl(Ei, j, 16);
          const double qh = QHrow[j];
          tau = __builtin_fma(-Mrow[j], dgj, tau);
          r = __builtin_fma(qh, 1.0 - Ej, r);
          row[j] = qh * Ej * (dgj > 0.0 ? 1.0 : -1.0);
        }
        const double sgi = dgi > 0.0 ? 1.0 : -1.0;
        const double den = 1.0 / (1.0 + sp.d * adg);
        const double da = (dgi - sp.d * a_i * adg) * den;
        const double y = tau - sp.C * (a_i + da);
        const double s = y > 0.0 ? 1.0 : -1.0;
        const double f = work ? fmax(fabs(y) - r, 0.0) : 0.0;
        const double fk = f > 0.0 ? exp(sp.n * log(f / sp.K)) : 0.0;   // (f / K)^n
        const double fg = work ? dgi - sp.dt * fk * s : 0.0;
        const bool guard = ((__ballot(f > sp.guard) >> sh) & 0xffffull) != 0;
        const bool conv = ((__ballot(!(fabs(fg) <= prm.rtol)) >> sh) & 0xffffull) == 0;

        const double w = sp.dt * (sp.n * fk / fmax(f, sp.floor_f));
        const double dda = (1.0 - sp.d * a_i * sgi) * den * den;
        SC_SYS_ROW(sys2);
#pragma unroll
        for (int j = 0; j < SC_NSYS; ++j) {
          double t = sys2[6 + j] + s * sp.b * row[j];
          if (li == j) t += sp.C * dda;
          row[j] = (li == j ? 1.0 : 0.0) + w * t;
        }
        row[12] = fg;
#pragma unroll
        for (int k = 0; k < 6; ++k) row[13 + k] = w * sys2[k];
        if (!work) {   // an idle row: the unit row of its own column, nothing on the right
#pragma unroll
          for (int k = 0; k < 19; ++k) row[k] = (k < SC_NSYS && k == li) ? 1.0 : 0.0;
        }

        // Gauss-Jordan over the 16-lane row: the pivot of column c is the unused lane with the largest entry.  The row is shifted
        // left by one entry per column, so that the pivot column is entry 0 in every pass of a loop that stays rolled (unrolled,
        // the twelve passes cost some 90 VGPRs more); after the twelve passes fg is entry 0 and the right-hand sides 1..6
        bool used = li >= SC_NSYS;
        int mycol = li;
        double mypiv = 1.0;
#pragma unroll 1
        for (int c = 0; c < SC_NSYS; ++c) {
          double v = used ? -1.0 : fabs(row[0]);
          int who = li;
#pragma unroll
          for (int m = 8; m > 0; m >>= 1) {
            const double ov = __shfl_xor(v, m, 16);
            const int ow = __shfl_xor(who, m, 16);
            if (ov > v || (ov == v && ow < who)) { v = ov; who = ow; }
          }
          const bool me = li == who;
          if (me) { used = true; mycol = c; mypiv = row[0]; }
          const double piv = __shfl(row[0], who, 16);
          const double fac = me ? 0.0 : row[0] / piv;
#pragma unroll
          for (int k = 1; k < 19; ++k) {
            const double pk = __shfl(row[k], who, 16);
            row[k - 1] = __builtin_fma(-fac, pk, row[k]);
          }
          row[18] = 0.0;
        }
        // unknown mycol sits in this lane: hand each solution to the lane of its system
        const int dst = (lane & 48) | (mycol & 15);
        const double ipiv = 1.0 / mypiv;
        const double delta = sc_push(row[0] * ipiv, dst);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double x = sc_push(row[1 + k] * ipiv, dst);
          X6[k] = (!done && !guard) ? x : X6[k];   // the accepted iterate is the last one that gets here
        }

        if (!done) {
          if (guard) {
            if (it == 0) { st_g = 2; done = true; }   // no step to halve: the integration fails here
            else {
              step *= 0.5;
              dgi -= step;
              ++it;
              if (it >= (unsigned)prm.maxit) { st_g = 1; done = true; }
            }
          } else {
            step = -delta;
            dgi += step;
            if (conv || it >= (unsigned)prm.maxit) {
              if (!conv) st_g = 1;
              done = true;
            } else {
              ++it;
            }
          }
        }
        if (__ballot(!done) == 0) break;
      }
      if (!work) dgi = 0.0;

      // Ct_m = D - sum_i B_i x X_i: every lane of the row ends with the sums; lane e % 12 writes entry e.  Row by row, rolled
      {
        SC_SYS_ROW(Bi);
        const double* dm = dmat;   // opaque like the row: hoisted out of the tile loop the 36 entries cost 72 VGPRs
        asm volatile("" : "+v"(dm));
#pragma unroll 1
        for (int a = 0; a < 6; ++a) {
          const double ba = Bi[a];
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            double t = ba * X6[k];
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) t += __shfl_xor(t, m, 16);
            const int eidx = a * 6 + k;
            if (work && li == eidx % SC_NSYS) t36[owner * 36 + eidx] = dm[eidx] - t;
          }
        }
      }
      if (work) hand[grp * SC_ROUND + li] = dgi;
      if (owner >= 0 && li == 12) hand[grp * SC_ROUND + 12] = (double)st_g;
      if (owner >= 0 && li == 13) hand[grp * SC_ROUND + 13] = (double)it;
      wave_lds_sync();
      if (plastic && rank >= r0 && rank < r0 + 4) {
        const double* h = hand + (rank - r0) * SC_ROUND;
#pragma unroll
        for (int i = 0; i < SC_NSYS; ++i) dg[i] = h[i];
        status = (int)h[12];
        iters = (unsigned)h[13];
      }
      wave_lds_sync();
    }

    // ---- 4. new state, stress and the tangent in the global axes, one thread per point ------------------------------
    double sg[6];
    double cchk = 0.0;   // sum of everything the point writes
    asm volatile("" : "+v"(sl));
    // strain and frame are read again (L2 hits), not carried over the rounds: 30 VGPRs that the Newton needs
    if (valid) {
      const double2_t* ge = reinterpret_cast<const double2_t*>(eps + (base + (unsigned)lane) * 6);
      const double2_t a = ge[0], b = ge[1], c = ge[2];
      e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y; e[4] = c.x; e[5] = c.y;
    }
    load_frame();
    __builtin_amdgcn_sched_barrier(0);
    {
      const bool moved = plastic && status != 2;
      double g[SC_NSYS];
#pragma unroll
      for (int i = 0; i < SC_NSYS; ++i) g[i] = valid ? load0(SC_SLOT_G + i) : 0.0;
      double et[6], sm[6];
      trial_strain(g, et);
#pragma unroll
      for (int i = 0; i < SC_NSYS; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c)
          if (SC.mu[i][c] != 0.0) et[c] = __builtin_fma(-dg[i], SC.mu[i][c], et[c]);
      stiffness(et, sm);
      __builtin_amdgcn_sched_barrier(0);
      if (valid) {
#pragma unroll
        for (int i = 0; i < SC_NSYS; ++i) {
          const double p = load0(SC_SLOT_P + i);
          const double a = load0(SC_SLOT_A + i);
          const double adg = fabs(dg[i]);
          const double da = (dg[i] - sp.d * a * adg) / (1.0 + sp.d * adg);
          const double gn = moved ? g[i] + dg[i] : g[i], pn = moved ? p + adg : p, an = moved ? a + da : a;
          store1(SC_SLOT_G + i, gn);
          store1(SC_SLOT_P + i, pn);
          store1(SC_SLOT_A + i, an);
          cchk += gn + pn + an;
          __builtin_amdgcn_sched_barrier(0);   // system after system: issued together the 24 loads cost 48 VGPRs
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double v = et[c];
          if (status == 2) v = load0(SC_SLOT_EEL + c);   // a failed integration leaves the bits it found
          store1(SC_SLOT_EEL + c, v);
          cchk += v;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (!plastic) {
        const double* dm = dmat;
        asm volatile("" : "+v"(dm));
#pragma unroll
        for (int eidx = 0; eidx < 36; ++eidx) rec[eidx] = dm[eidx];
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (FRAME == OR_FRAME_NONE) {
#pragma unroll
        for (int c = 0; c < 6; ++c) sg[c] = sm[c];
#pragma unroll
        for (int eidx = 0; eidx < 36; ++eidx) cchk += rec[eidx];
      } else {
        double Q[6][6];
#pragma unroll
        for (int I = 0; I < 6; ++I) Qrow(I, Q[I]);
#pragma unroll
        for (int K = 0; K < 6; ++K) {
          double t = Q[0][K] * sm[0];
#pragma unroll
          for (int r = 1; r < 6; ++r) t = __builtin_fma(Q[r][K], sm[r], t);
          sg[K] = t;
        }
        // Ct = Q^T Ct_m Q in place: rows first (Y = Ct_m Q), then columns (Ct[:, K] = Q^T Y[:, K])
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double mr[6];
#pragma unroll
          for (int c = 0; c < 6; ++c) mr[c] = rec[6 * r + c];
#pragma unroll
          for (int K = 0; K < 6; ++K) {
            double t = mr[0] * Q[0][K];
#pragma unroll
            for (int c = 1; c < 6; ++c) t = __builtin_fma(mr[c], Q[c][K], t);
            rec[6 * r + K] = t;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int K = 0; K < 6; ++K) {
          double yc[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) yc[r] = rec[6 * r + K];
#pragma unroll
          for (int I = 0; I < 6; ++I) {
            double t = Q[0][I] * yc[0];
#pragma unroll
            for (int r = 1; r < 6; ++r) t = __builtin_fma(Q[r][I], yc[r], t);
            rec[6 * I + K] = t;
            cchk += t;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) cchk += sg[c];
    }
    if (valid && plastic) {
      ++c_plastic;
      if (status != 0) ++c_notconv;
      c_maxit = iters > c_maxit ? iters : c_maxit;
    }
    if (valid && !(fabs(cchk) <= 1.79769313486231570e308)) ++c_nan;
    wave_lds_sync();

    // ---- 5. tangent, in output order from the staged records; 6. the stress through the head of the same region ------
#include "stage_full36_store.hpp"
    wave_lds_sync();
    stage2[lane * 3 + 0] = double2_t{sg[0], sg[1]};
    stage2[lane * 3 + 1] = double2_t{sg[2], sg[3]};
    stage2[lane * 3 + 2] = double2_t{sg[4], sg[5]};
    wave_lds_sync();
#include "tile_rows6_store.hpp"
    wave_lds_sync();   // the LDS region is rewritten by the next tile
  }

  // store_block_stats (dxm_common.hpp) for a workgroup of SC_WAVES waves
  c_plastic = wave_sum(c_plastic);
  c_notconv = wave_sum(c_notconv);
  c_nan = wave_sum(c_nan);
  c_maxit = wave_max(c_maxit);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    red[wid * 4 + 0] = c_plastic; red[wid * 4 + 1] = c_notconv; red[wid * 4 + 2] = c_nan; red[wid * 4 + 3] = c_maxit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    BlockStats bs = {0, 0, 0, 0};
    for (int w = 0; w < SC_WAVES; ++w) {
      bs.n_plastic += red[w * 4 + 0];
      bs.n_not_converged += red[w * 4 + 1];
      bs.n_nan += red[w * 4 + 2];
      bs.max_iters = red[w * 4 + 3] > bs.max_iters ? red[w * 4 + 3] : bs.max_iters;
    }
    stats[blockIdx.x] = bs;
  }
}
#undef SC_D
#undef SC_SYS_ROW

__global__ void __launch_bounds__(256) pack_consecutive_slots_kernel(const double* __restrict__ soa, int64_t ld, int64_t n, int first, int width,
                                                                  double* __restrict__ aos) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * width) return;
  const int64_t i = t / width;
  const int k = (int)(t - i * width);
  aos[t] = soa[(int64_t)(first + k) * ld + i];
}

const void* single_crystal_kernel_fn() { return (const void*)single_crystal_kernel<OR_FRAME_NONE>; }

void single_crystal_launch(int frame, int grid, hipStream_t st, const LawParams& prm, const ScParams& sp, int64_t cnt, const double* grad,
                           const Frame9& uniform, const double* frames, int64_t ldf, const double* s0, double* s1, int64_t ld, double* flux,
                           double* ct, BlockStats* bs) {
#define DXM_LAUNCH_SC(F) \
  hipLaunchKernelGGL((single_crystal_kernel<F>), dim3(grid), dim3(SC_BLOCK), 0, st, prm, sp, cnt, grad, uniform, frames, ldf, s0, s1, ld, flux, ct, bs)
  if (frame == OR_FRAME_FIELD) DXM_LAUNCH_SC(OR_FRAME_FIELD);
  else if (frame == OR_FRAME_UNIFORM) DXM_LAUNCH_SC(OR_FRAME_UNIFORM);
  else DXM_LAUNCH_SC(OR_FRAME_NONE);
#undef DXM_LAUNCH_SC
}

void pack_consecutive_slots(const double* soa, int64_t ld, int64_t n, int first, int width, double* aos, hipStream_t st) {
  if (n <= 0 || width <= 0) return;
  const int64_t blocks = (n * width + 255) / 256;
  hipLaunchKernelGGL(pack_consecutive_slots_kernel, dim3((unsigned)blocks), dim3(256), 0, st, soa, ld, n, first, width, aos);
}

}  // namespace dxm
