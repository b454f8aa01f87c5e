// Inertia, mass damping and a rigid-plane penalty at the quadrature points (demos/kl-shell-svk/dynamic-tspline.py:100-293 of
// the reference: DENS*h*inner(yddot_alpha,z) and contactForce): they touch only the VALUE slots of the point data a law kernel
// has left on the device, between the law and the load / tangent assembly.  nF fields of nJ slots each, value slot first, in
// the layouts of the point forms: u and s with slot alpha of field i at (i nJ + alpha) npts + q, T with the value-value entry
// of block (i, j) at ((i nF + j) nJ^2) npts + q (nJ = 1: the reaction of tg_coef_transform_blocks), X0 and w component-major.
// With coef = {sigma, m_u, m_w, t_m, k_s, k_t, c_e} and plane = {n[0..nF), offset}:
//     g = offset - sum_c n_c (X0_c + u_c^0),   g+ = max(g, 0),   a point is active exactly when g > 0
//     s_i^alpha <- sigma s_i^alpha                                    (every slot; not touched when sigma == 1)
//     s_i^0    += m_u u_i^0 + m_w w_i - k_s g+ n_i
//     T_ij^00  += delta_ij t_m + k_t [g > 0] n_i n_j                  (no other entry of T is read or written)
//     e_q       = c_e/2 sum_i w_i^2 + k_s/2 g+^2
// A term whose coefficient is zero or whose array is absent is not added: a value it would not change keeps its bits.
//
// One thread per point; the arrays are component-major, so consecutive lanes touch consecutive addresses.  nF and nJ are
// template arguments: every index into the small arrays is a compile-time constant after unrolling.  The active points are
// counted as the inadmissible points of k_shell_points: a tree per workgroup, then one integer atomic; no floating-point
// atomics, the same inputs give the same bits.
#include "tg_common.h"
#include <cmath>

#define TG_DYN_BLOCK 256

struct tg_dyn_args {
  int64_t npts;
  double sigma, m_u, m_w, t_m, k_s, k_t, c_e;
  double n[3], offset;
  int contact;
  const double *X0, *u, *w;      // any of them may be null (X0 not with contact)
  double *s, *T, *e;             // any of them may be null
  unsigned long long *nactive;   // null: not counted
};

template <int NF, int NJ>
__global__ void __launch_bounds__(TG_DYN_BLOCK) k_point_dynamics(tg_dyn_args M) {
  __shared__ int sact[TG_DYN_BLOCK];
  const int tid = threadIdx.x;
  const int64_t npts = M.npts;
  const bool mass_u = M.u && M.m_u != 0.0, mass_w = M.w && M.m_w != 0.0, scale = M.sigma != 1.0;
  int nact = 0;
  for (int t = tid; t < TG_DYN_BLOCK; t += blockDim.x) {
    const int64_t q = (int64_t)blockIdx.x * TG_DYN_BLOCK + t;
    if (q >= npts) continue;
    double uv[NF], wv[NF];
#pragma unroll
    for (int c = 0; c < NF; c++) {
      uv[c] = M.u ? M.u[(int64_t)(c * NJ) * npts + q] : 0.0;
      wv[c] = M.w ? M.w[(int64_t)c * npts + q] : 0.0;
    }
    bool active = false;
    double gp = 0.0;
    if (M.contact) {
      double g = M.offset;
#pragma unroll
      for (int c = 0; c < NF; c++) g -= M.n[c] * (M.X0[(int64_t)c * npts + q] + uv[c]);
      active = g > 0.0;
      if (active) {
        gp = g;
        nact++;
      }
    }
    if (M.s) {
#pragma unroll
      for (int i = 0; i < NF; i++) {
        if (scale) {
#pragma unroll
          for (int al = 1; al < NJ; al++) M.s[(int64_t)(i * NJ + al) * npts + q] *= M.sigma;
        }
        if (scale || mass_u || mass_w || active) {
          double v = M.s[(int64_t)(i * NJ) * npts + q];
          if (scale) v *= M.sigma;
          if (mass_u) v += M.m_u * uv[i];
          if (mass_w) v += M.m_w * wv[i];
          if (active) v -= M.k_s * gp * M.n[i];
          M.s[(int64_t)(i * NJ) * npts + q] = v;
        }
      }
    }
    if (M.T && (M.t_m != 0.0 || active)) {
#pragma unroll
      for (int i = 0; i < NF; i++)
#pragma unroll
        for (int j = 0; j < NF; j++) {
          if (i != j && !active) continue;
          double *To = M.T + (int64_t)((i * NF + j) * NJ * NJ) * npts + q;
          double v = *To;
          if (i == j && M.t_m != 0.0) v += M.t_m;
          if (active) v += M.k_t * M.n[i] * M.n[j];
          *To = v;
        }
    }
    if (M.e) {
      double ww = 0.0;
#pragma unroll
      for (int c = 0; c < NF; c++) ww += wv[c] * wv[c];
      M.e[q] = 0.5 * M.c_e * ww + 0.5 * M.k_s * gp * gp;
    }
  }
  if (!M.nactive) return;          // (uniform over the grid)
  // the workgroup's count: a tree in LDS, then one integer atomic
  sact[tid] = nact;
  __syncthreads();
  for (int o = (int)blockDim.x >> 1; o > 0; o >>= 1) {
    if (tid < o) sact[tid] += sact[tid + o];
    __syncthreads();
  }
  if (tid == 0 && sact[0] > 0) atomicAdd(M.nactive, (unsigned long long)sact[0]);
}

template <int NF, int NJ>
static void tg_dyn_launch(const tg_dyn_args &M) {
  hipLaunchKernelGGL((k_point_dynamics<NF, NJ>), dim3((unsigned)tg_cdiv(M.npts, TG_DYN_BLOCK)), dim3(TG_DYN_BLOCK), 0, g_tg.stream, M);
}

extern "C" int tg_point_dynamics(int nF, int nJ, int64_t npts, const double *coef, const double *plane, tg_vec_t X0, tg_vec_t u,
                                 tg_vec_t w, tg_vec_t s_inout, tg_vec_t T_inout, tg_vec_t e_out, int64_t *nactive) {
  TG_REQUIRE_INIT();
  TG_REQUIRE((nF == 2 || nF == 3) && (nJ == 1 || nJ == 3 || nJ == 6),
             "tg_point_dynamics: nF = %d fields of nJ = %d slots; nF = 2, 3 and nJ = 1 (values), 3, 6 (jets of d = 1, 2) are provided", nF, nJ);
  TG_REQUIRE(coef, "tg_point_dynamics: coef = {sigma, m_u, m_w, t_m, k_s, k_t, c_e}");
  TG_REQUIRE(npts >= 0 && tg_cdiv(npts, TG_DYN_BLOCK) < (1ll << 31), "tg_point_dynamics: too many points for one launch");
  const int64_t nv = (int64_t)nF * nJ * npts;
  TG_REQUIRE(!u || u->n == nv, "tg_point_dynamics: u holds nF nJ npts = %lld values", (long long)nv);
  TG_REQUIRE(!s_inout || s_inout->n == nv, "tg_point_dynamics: s_inout holds nF nJ npts = %lld values", (long long)nv);
  TG_REQUIRE(!T_inout || T_inout->n == nv * nF * nJ, "tg_point_dynamics: T_inout holds nF^2 nJ^2 npts = %lld values", (long long)(nv * nF * nJ));
  TG_REQUIRE(!X0 || X0->n == nF * npts, "tg_point_dynamics: X0 holds nF npts = %lld values", (long long)(nF * npts));
  TG_REQUIRE(!w || w->n == nF * npts, "tg_point_dynamics: w holds nF npts = %lld values", (long long)(nF * npts));
  TG_REQUIRE(!e_out || e_out->n == npts, "tg_point_dynamics: e_out holds npts = %lld values", (long long)npts);
  TG_REQUIRE(!plane || X0, "tg_point_dynamics: a plane needs the reference positions X0 of the points");
  if (nactive) *nactive = 0;
  if (npts == 0 || (!s_inout && !T_inout && !e_out && !(nactive && plane))) return 0;
  const bool count = nactive && plane;
  tg_dbuf<unsigned long long> stat;
  if (count) {
    TG_TRY(stat.alloc(1));
    TG_CHECK_HIP(hipMemsetAsync(stat.get(), 0, sizeof(unsigned long long), g_tg.stream));
  }
  tg_dyn_args M;
  M.npts = npts;
  M.sigma = coef[0], M.m_u = coef[1], M.m_w = coef[2], M.t_m = coef[3], M.k_s = coef[4], M.k_t = coef[5], M.c_e = coef[6];
  for (int c = 0; c < 3; c++) M.n[c] = plane && c < nF ? plane[c] : 0.0;
  M.offset = plane ? plane[nF] : 0.0;
  M.contact = plane ? 1 : 0;
  M.X0 = X0 ? X0->d : nullptr;
  M.u = u ? u->d : nullptr;
  M.w = w ? w->d : nullptr;
  M.s = s_inout ? s_inout->d : nullptr;
  M.T = T_inout ? T_inout->d : nullptr;
  M.e = e_out ? e_out->d : nullptr;
  M.nactive = count ? stat.get() : nullptr;
  if (nF == 2 && nJ == 1) tg_dyn_launch<2, 1>(M);
  else if (nF == 2 && nJ == 3) tg_dyn_launch<2, 3>(M);
  else if (nF == 2 && nJ == 6) tg_dyn_launch<2, 6>(M);
  else if (nF == 3 && nJ == 1) tg_dyn_launch<3, 1>(M);
  else if (nF == 3 && nJ == 3) tg_dyn_launch<3, 3>(M);
  else tg_dyn_launch<3, 6>(M);
  TG_LAUNCH_CHECK();
  if (!count) return 0;
  TG_CHECK_HIP(hipMemcpyAsync(g_tg.host_pinned, stat.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  unsigned long long got;
  memcpy(&got, g_tg.host_pinned, sizeof(got));
  *nactive = (int64_t)got;
  return 0;
}
