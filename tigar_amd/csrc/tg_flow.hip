// The incompressible Navier-Stokes law AT THE QUADRATURE POINTS, equal-order velocity and pressure with SUPG / PSPG / LSIC
// stabilisation (Bazilevs et al., CMAME 197 (2007) 173-201, without the cross- and Reynolds-stress terms): from the point
// values and Cartesian gradients of (u_1 .. u_nsd, p) to the source and flux of the weak residual
//   R(v, q) = int s_i v_i + F_iK d_K v_i + s_p q + F_pK d_K q dx
// and their exact derivative, so that a Newton step uploads nothing.
//
// nsd = 2 or 3, nF = nsd + 1 fields (the pressure last), rho and mu constants, nu = mu / rho.  With a = c_a u + a0 (a0: the
// history part of a time integrator, null = 0), f the body force per unit mass (null = 0) and G the element metric of
// tg_quad_metric:
//   r_i   = rho (a_i + u_L d_L u_i - f_i) + d_i p             the strong momentum residual WITHOUT its viscous part
//   tau_M = (dt4 + u . G u + C_I nu^2 G:G)^(-1/2)             dt4 = 4 / dt^2 (0 for a steady problem)
//   tau_C = 1 / (tau_M tr G)
//   s_i   = rho (a_i + u_L d_L u_i - f_i)
//   F_iK  = mu (d_K u_i + d_i u_K) - p d_iK + tau_M u_K r_i + rho tau_C (d_L u_L) d_iK
//   s_p   = d_L u_L                                           F_pK = (tau_M / rho) r_K
// The viscous part of r needs Cartesian second derivatives and is left out: the stabilisation is consistent up to
// O(tau_M mu lap u) only, which limits the spatial order to about 2.
//
// Point arrays are component-major:
//   U      field i                  at i npts + q                                    (i < nF)
//   gradU  d U_i / d x_K            at (i nsd + K) npts + q
//   a0, f  component i              at i npts + q                                    (i < nsd)
//   G      G_KL                     at (K nsd + L) npts + q
//   s      s_i                      at i npts + q            F   F_iK  at (i nsd + K) npts + q
//   A      A_iKjL = d F_iK / d (d_L U_j)   at (((i nF + j) nsd + K) nsd + L) npts + q
//   b      b_iKj  = d F_iK / d U_j         at ((i nF + j) nsd + K) npts + q
//   c      c_ijL  = d s_i / d (d_L U_j)    at ((i nF + j) nsd + L) npts + q
//   M      m_ij   = d s_i / d U_j          at (i nF + j) npts + q
//   tau    tau_M at q, tau_C at npts + q
// the layouts tg_coef_transform_system and tg_quad_load_flux read.  The tangent is the exact derivative, tau included:
// d tau_M / d u_j = -tau_M^3 (G u)_j,  d tau_C / d u_j = -(tau_C / tau_M) d tau_M / d u_j  (G symmetric).
//
// One thread per point, the kernel templated on <NSD>: every index is a compile-time constant and every entry is stored as
// it is formed (no array of the 256 + 64 + 64 + 16 tangent values per thread).  Dense blocks: the entries that are zero by
// structure are written as zeros.  No atomics, no reduction: the same bits in every run and for every subset of outputs.
#include "tg_common.h"
#include <cmath>

struct tg_flow_args {
  int64_t npts;
  double rho, mu, ca, dt4, CI;
  const double *U, *gradU, *a0, *f, *G;      // a0, f may be null
  double *s, *F, *A, *b, *c, *M, *tau;       // any of them may be null
};

#define TG_FLOW_BLOCK 256

// the law at point q
template <int NSD>
__device__ __forceinline__ void tg_flow_point(const tg_flow_args &W, const int64_t q) {
  constexpr int NF = NSD + 1;
  const int64_t npts = W.npts;
  const double rho = W.rho, mu = W.mu, ca = W.ca;
  double u[NSD], H[NSD][NSD], gp[NSD], G[NSD][NSD];
  const double p = W.U[(int64_t)NSD * npts + q];
#pragma unroll
  for (int i = 0; i < NSD; i++) {
    u[i] = W.U[(int64_t)i * npts + q];
    gp[i] = W.gradU[(int64_t)(NSD * NSD + i) * npts + q];
#pragma unroll
    for (int K = 0; K < NSD; K++) {
      H[i][K] = W.gradU[(int64_t)(i * NSD + K) * npts + q];
      G[i][K] = W.G[(int64_t)(i * NSD + K) * npts + q];
    }
  }
  // the momentum without and with the pressure gradient, the divergence
  double sm[NSD], r[NSD], div = 0.0;
#pragma unroll
  for (int i = 0; i < NSD; i++) {
    double acc = ca * u[i] + (W.a0 ? W.a0[(int64_t)i * npts + q] : 0.0) - (W.f ? W.f[(int64_t)i * npts + q] : 0.0);
#pragma unroll
    for (int L = 0; L < NSD; L++) acc = fma(u[L], H[i][L], acc);
    sm[i] = rho * acc;
    r[i] = sm[i] + gp[i];
    div += H[i][i];
  }
  // the stabilisation parameters and their derivatives with respect to u
  double Gu[NSD], uGu = 0.0, GG = 0.0, trG = 0.0;
#pragma unroll
  for (int K = 0; K < NSD; K++) {
    double acc = 0.0;
#pragma unroll
    for (int L = 0; L < NSD; L++) {
      acc = fma(G[K][L], u[L], acc);
      GG = fma(G[K][L], G[K][L], GG);
    }
    Gu[K] = acc;
    uGu = fma(u[K], acc, uGu);
    trG += G[K][K];
  }
  const double nu = mu / rho;
  const double tM = 1.0 / sqrt(W.dt4 + uGu + W.CI * (nu * nu) * GG);
  const double tC = 1.0 / (tM * trG);
  double dtM[NSD], dtC[NSD];
#pragma unroll
  for (int j = 0; j < NSD; j++) {
    dtM[j] = -(tM * tM * tM) * Gu[j];
    dtC[j] = -(tC / tM) * dtM[j];
  }
  if (W.tau) {
    W.tau[q] = tM;
    W.tau[npts + q] = tC;
  }
  if (W.s) {
#pragma unroll
    for (int i = 0; i < NSD; i++) W.s[(int64_t)i * npts + q] = sm[i];
    W.s[(int64_t)NSD * npts + q] = div;
  }
  if (W.F) {
#pragma unroll
    for (int i = 0; i < NSD; i++)
#pragma unroll
      for (int K = 0; K < NSD; K++) {
        double v = mu * (H[i][K] + H[K][i]) + tM * (u[K] * r[i]);
        if (i == K) v += rho * tC * div - p;
        W.F[(int64_t)(i * NSD + K) * npts + q] = v;
      }
#pragma unroll
    for (int K = 0; K < NSD; K++) W.F[(int64_t)(NSD * NSD + K) * npts + q] = (tM / rho) * r[K];
  }
  if (W.M) {           // m_ij = d s_i / d U_j: rho (c_a d_ij + d_j u_i) among the velocities, zero in the pressure row and column
#pragma unroll
    for (int i = 0; i < NF; i++)
#pragma unroll
      for (int j = 0; j < NF; j++)
        W.M[(int64_t)(i * NF + j) * npts + q] = (i < NSD && j < NSD) ? rho * (H[i < NSD ? i : 0][j < NSD ? j : 0] + (i == j ? ca : 0.0)) : 0.0;
  }
  if (W.c) {           // c_ijL = d s_i / d (d_L U_j): rho u_L d_ij (momentum), d_jL (continuity)
#pragma unroll
    for (int i = 0; i < NF; i++)
#pragma unroll
      for (int j = 0; j < NF; j++)
#pragma unroll
        for (int L = 0; L < NSD; L++) {
          double v = 0.0;
          if (i < NSD && i == j) v = rho * u[L];
          if (i == NSD && j == L) v = 1.0;
          W.c[(int64_t)((i * NF + j) * NSD + L) * npts + q] = v;
        }
  }
  if (W.b) {           // b_iKj = d F_iK / d U_j
#pragma unroll
    for (int i = 0; i < NF; i++)
#pragma unroll
      for (int j = 0; j < NF; j++)
#pragma unroll
        for (int K = 0; K < NSD; K++) {
          double v = 0.0;
          if (i < NSD && j < NSD) {
            const int ii = i < NSD ? i : 0, jj = j < NSD ? j : 0;
            const double Rij = rho * (H[ii][jj] + (i == j ? ca : 0.0));
            v = dtM[jj] * (u[K] * r[ii]) + tM * (u[K] * Rij);
            if (K == j) v += tM * r[ii];
            if (i == K) v += rho * div * dtC[jj];
          } else if (i < NSD && j == NSD) {
            v = i == K ? -1.0 : 0.0;
          } else if (i == NSD && j < NSD) {
            const int jj = j < NSD ? j : 0;
            v = (dtM[jj] * r[K] + tM * (rho * (H[K][jj] + (K == j ? ca : 0.0)))) / rho;
          }
          W.b[(int64_t)((i * NF + j) * NSD + K) * npts + q] = v;
        }
  }
  if (W.A) {           // A_iKjL = d F_iK / d (d_L U_j)
#pragma unroll
    for (int i = 0; i < NF; i++)
#pragma unroll
      for (int j = 0; j < NF; j++)
#pragma unroll
        for (int K = 0; K < NSD; K++)
#pragma unroll
          for (int L = 0; L < NSD; L++) {
            double v = 0.0;
            if (i < NSD && j < NSD) {
              if (i == j) v = rho * tM * (u[K] * u[L]) + (K == L ? mu : 0.0);
              if (i == L && j == K) v += mu;
              if (i == K && j == L) v += rho * tC;
            } else if (i < NSD && j == NSD) {
              v = i == L ? tM * u[K] : 0.0;
            } else if (i == NSD && j < NSD) {
              v = j == K ? tM * u[L] : 0.0;
            } else {
              v = K == L ? tM / rho : 0.0;
            }
            W.A[(int64_t)(((i * NF + j) * NSD + K) * NSD + L) * npts + q] = v;
          }
  }
}

// a thread per point.  (A host build -- tools/host_shim -- runs a block with ONE thread, which then takes the block's points one
// after the other; on the device that loop, even run once, costs the nsd = 2 kernel 256 registers and all but one wave)
template <int NSD>
__global__ void __launch_bounds__(TG_FLOW_BLOCK) k_flow_points(tg_flow_args W) {
#ifdef __HIP_DEVICE_COMPILE__
  const int64_t q = (int64_t)blockIdx.x * TG_FLOW_BLOCK + threadIdx.x;
  if (q < W.npts) tg_flow_point<NSD>(W, q);
#else
  for (int t = threadIdx.x; t < TG_FLOW_BLOCK; t += blockDim.x) {
    const int64_t q = (int64_t)blockIdx.x * TG_FLOW_BLOCK + t;
    if (q < W.npts) tg_flow_point<NSD>(W, q);
  }
#endif
}

static int tg_flow_array(const char *name, tg_vec_t v, int64_t each, int64_t npts, bool needed) {
  TG_REQUIRE(v || !needed, "tg_flow_points: no %s", name);
  TG_REQUIRE(!v || v->n == each * npts, "tg_flow_points: %s holds %lld values, expected %lld per point of %lld points", name,
             (long long)(v ? v->n : 0), (long long)each, (long long)npts);
  return 0;
}

extern "C" int tg_flow_points(const double *params, int nsd, int64_t npts, tg_vec_t U_q, tg_vec_t gradU_q, tg_vec_t a0_q, tg_vec_t f_q,
                              tg_vec_t G_q, tg_vec_t s_out, tg_vec_t F_out, tg_vec_t A_out, tg_vec_t b_out, tg_vec_t c_out,
                              tg_vec_t M_out, tg_vec_t tau_out) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(nsd == 2 || nsd == 3, "tg_flow_points: nsd = %d; 2 or 3", nsd);
  TG_REQUIRE(params, "tg_flow_points: params = {rho, mu, c_a, 4 / dt^2, C_I}");
  TG_REQUIRE(params[0] > 0.0 && params[1] >= 0.0 && params[3] >= 0.0 && params[4] >= 0.0,
             "tg_flow_points: rho > 0, mu >= 0, 4 / dt^2 >= 0 and C_I >= 0 (rho = %g, mu = %g, 4 / dt^2 = %g, C_I = %g)", params[0],
             params[1], params[3], params[4]);
  TG_REQUIRE(npts >= 0 && tg_cdiv(npts, TG_FLOW_BLOCK) < (1ll << 31), "tg_flow_points: too many points for one launch");
  const int64_t nF = nsd + 1, n1 = nsd, n2 = (int64_t)nsd * nsd;
  TG_TRY(tg_flow_array("U_q", U_q, nF, npts, true));
  TG_TRY(tg_flow_array("gradU_q", gradU_q, nF * n1, npts, true));
  TG_TRY(tg_flow_array("G_q", G_q, n2, npts, true));
  TG_TRY(tg_flow_array("a0_q", a0_q, n1, npts, false));
  TG_TRY(tg_flow_array("f_q", f_q, n1, npts, false));
  TG_TRY(tg_flow_array("s_out", s_out, nF, npts, false));
  TG_TRY(tg_flow_array("F_out", F_out, nF * n1, npts, false));
  TG_TRY(tg_flow_array("A_out", A_out, nF * nF * n2, npts, false));
  TG_TRY(tg_flow_array("b_out", b_out, nF * nF * n1, npts, false));
  TG_TRY(tg_flow_array("c_out", c_out, nF * nF * n1, npts, false));
  TG_TRY(tg_flow_array("M_out", M_out, nF * nF, npts, false));
  TG_TRY(tg_flow_array("tau_out", tau_out, 2, npts, false));
  if (npts == 0) return 0;
  tg_flow_args W;
  W.npts = npts;
  W.rho = params[0], W.mu = params[1], W.ca = params[2], W.dt4 = params[3], W.CI = params[4];
  W.U = U_q->d, W.gradU = gradU_q->d, W.G = G_q->d;
  W.a0 = a0_q ? a0_q->d : nullptr;
  W.f = f_q ? f_q->d : nullptr;
  W.s = s_out ? s_out->d : nullptr;
  W.F = F_out ? F_out->d : nullptr;
  W.A = A_out ? A_out->d : nullptr;
  W.b = b_out ? b_out->d : nullptr;
  W.c = c_out ? c_out->d : nullptr;
  W.M = M_out ? M_out->d : nullptr;
  W.tau = tau_out ? tau_out->d : nullptr;
  const dim3 grid((unsigned)tg_cdiv(npts, TG_FLOW_BLOCK));
  if (nsd == 2)
    hipLaunchKernelGGL((k_flow_points<2>), grid, dim3(TG_FLOW_BLOCK), 0, g_tg.stream, W);
  else
    hipLaunchKernelGGL((k_flow_points<3>), grid, dim3(TG_FLOW_BLOCK), 0, g_tg.stream, W);
  TG_LAUNCH_CHECK();
  return 0;
}
