// Hyperelastic material laws AT THE QUADRATURE POINTS: from the displacement gradient of a solid to the first
// Piola-Kirchhoff stress, its tangent and the energy density -- what derivative(psi*spline.dx, u) of the reference produces
// symbolically, evaluated here point by point on the device, so that a Newton step uploads nothing.
//
// nsd = 2 (plane strain) or 3; F = I + grad u, J = det F, C = F^T F.  Point arrays are component-major:
//   gradu  d u_i / d x_K            at (i nsd + K) npts + q
//   P      P_iK                     at (i nsd + K) npts + q
//   A      A_iKjL = d P_iK / d F_jL at (((i nsd + j) nsd + K) nsd + L) npts + q -- block (i, j) is a contiguous nsd x nsd tensor
//                                   A_ij[K][L], the layout tg_coef_transform(a_kind = 2) reads (tg_coef_transform_blocks)
//   psi    the energy density       at q
//
//   kind 0  linear (small strain)      psi = lambda/2 (tr eps)^2 + mu eps:eps,  eps = sym grad u
//                                      P = lambda tr eps I + 2 mu eps
//                                      A = lambda d_iK d_jL + mu (d_ij d_KL + d_iL d_jK)
//   kind 1  St. Venant-Kirchhoff       E = (C - I)/2, S = lambda tr E I + 2 mu E, psi = lambda/2 (tr E)^2 + mu E:E
//                                      P = F S
//                                      A = d_ij S_KL + lambda F_iK F_jL + mu (F_iL F_jK + d_KL (F F^T)_ij)
//   kind 2  compressible neo-Hookean   psi = mu/2 (tr C - nsd) - mu ln J + lambda/2 (ln J)^2
//                                      P = mu (F - F^-T) + lambda ln J F^-T
//                                      A = mu d_ij d_KL + (mu - lambda ln J) F^-1_Li F^-1_Kj + lambda F^-1_Ki F^-1_Lj
//
// One thread per point, the kernel templated on <KIND, NSD>: every index into F, F^-1 and S is a compile-time constant, and
// every entry of A is formed from its closed form and stored at once (no array of 81 values per thread).  The kernel
// streams: nsd^2 doubles in, nsd^2 + nsd^4 + 1 out.  Kind 2 at a point with J <= 0 writes NOTHING for that point; such points
// are counted (integer atomic, one per workgroup) and the smallest J of all points is returned (an integer-ordered minimum
// on the bits of J, one per workgroup): both are independent of the order of the atomics, the same bits in every run.
// Kinds 0 and 1 are defined for any F (they count no point; the smallest J is reported all the same).
#include "tg_common.h"
#include <cmath>

struct tg_mat_args {
  int64_t npts;
  double lambda, mu;
  const double *gradu;
  double *P, *A, *psi;         // any of them may be null
  long long *stat;             // [0] points with J <= 0 (kind 2), [1] the ordered bits of the smallest J
};

// doubles -> signed integers of the same order (and back)
__device__ __forceinline__ long long tg_mat_key(double v) {
  const long long b = __double_as_longlong(v);
  return b ^ ((b >> 63) & 0x7fffffffffffffffll);
}
static inline double tg_mat_unkey(long long k) {
  const long long b = k ^ ((k >> 63) & 0x7fffffffffffffffll);
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

#define TG_MAT_BLOCK 256

template <int KIND, int NSD>
__global__ void __launch_bounds__(TG_MAT_BLOCK) k_material_points(tg_mat_args M) {
  __shared__ long long smin[TG_MAT_BLOCK];
  __shared__ int sbad[TG_MAT_BLOCK];
  const int tid = threadIdx.x;
  const int64_t npts = M.npts;
  const double lam = M.lambda, mu = M.mu;
  long long kmin = 0x7fffffffffffffffll;
  int nbad = 0;
  for (int t = tid; t < TG_MAT_BLOCK; t += blockDim.x) {
    const int64_t q = (int64_t)blockIdx.x * TG_MAT_BLOCK + t;
    if (q >= npts) continue;
    double H[NSD][NSD], F[NSD][NSD];
#pragma unroll
    for (int i = 0; i < NSD; i++)
#pragma unroll
      for (int K = 0; K < NSD; K++) {
        H[i][K] = M.gradu[(int64_t)(i * NSD + K) * npts + q];
        F[i][K] = H[i][K] + (i == K ? 1.0 : 0.0);
      }
    // cofactors of F: Fi = cof^T / J
    double cof[NSD][NSD], J;
    if constexpr (NSD == 2) {
      cof[0][0] = F[1][1];
      cof[0][1] = -F[1][0];
      cof[1][0] = -F[0][1];
      cof[1][1] = F[0][0];
      J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int K = 0; K < 3; K++) {
          const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, K1 = (K + 1) % 3, K2 = (K + 2) % 3;
          cof[i][K] = F[i1][K1] * F[i2][K2] - F[i1][K2] * F[i2][K1];
        }
      J = F[0][0] * cof[0][0] + F[0][1] * cof[0][1] + F[0][2] * cof[0][2];
    }
    const long long kj = tg_mat_key(J);
    kmin = kj < kmin ? kj : kmin;
    if constexpr (KIND == 0) {
      double tr = 0.0;
#pragma unroll
      for (int i = 0; i < NSD; i++) tr += H[i][i];
      if (M.psi) {
        double ee = 0.0;
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int K = 0; K < NSD; K++) {
            const double e = 0.5 * (H[i][K] + H[K][i]);
            ee = fma(e, e, ee);
          }
        M.psi[q] = 0.5 * lam * tr * tr + mu * ee;
      }
      if (M.P) {
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int K = 0; K < NSD; K++)
            M.P[(int64_t)(i * NSD + K) * npts + q] = mu * (H[i][K] + H[K][i]) + (i == K ? lam * tr : 0.0);
      }
      if (M.A) {
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int j = 0; j < NSD; j++)
#pragma unroll
            for (int K = 0; K < NSD; K++)
#pragma unroll
              for (int L = 0; L < NSD; L++)
                M.A[(int64_t)(((i * NSD + j) * NSD + K) * NSD + L) * npts + q] =
                    (i == K && j == L ? lam : 0.0) + (i == j && K == L ? mu : 0.0) + (i == L && j == K ? mu : 0.0);
      }
    } else if constexpr (KIND == 1) {
      // E = (F^T F - I) / 2, S = lambda tr E I + 2 mu E (symmetric: the upper triangle is computed, the lower one copied)
      double S[NSD][NSD], trE = 0.0, EE = 0.0;
#pragma unroll
      for (int K = 0; K < NSD; K++)
#pragma unroll
        for (int L = K; L < NSD; L++) {
          double c = 0.0;
#pragma unroll
          for (int a = 0; a < NSD; a++) c = fma(F[a][K], F[a][L], c);
          const double e = 0.5 * (c - (K == L ? 1.0 : 0.0));
          S[K][L] = S[L][K] = e;
          if (K == L) trE += e;
          EE = fma(K == L ? e : 2.0 * e, e, EE);
        }
      if (M.psi) M.psi[q] = 0.5 * lam * trE * trE + mu * EE;
#pragma unroll
      for (int K = 0; K < NSD; K++)
#pragma unroll
        for (int L = 0; L < NSD; L++) S[K][L] = 2.0 * mu * S[K][L] + (K == L ? lam * trE : 0.0);
      if (M.P) {
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int K = 0; K < NSD; K++) {
            double v = 0.0;
#pragma unroll
            for (int a = 0; a < NSD; a++) v = fma(F[i][a], S[a][K], v);
            M.P[(int64_t)(i * NSD + K) * npts + q] = v;
          }
      }
      if (M.A) {
        double B[NSD][NSD];            // F F^T
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int j = i; j < NSD; j++) {
            double v = 0.0;
#pragma unroll
            for (int a = 0; a < NSD; a++) v = fma(F[i][a], F[j][a], v);
            B[i][j] = B[j][i] = v;
          }
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int j = 0; j < NSD; j++)
#pragma unroll
            for (int K = 0; K < NSD; K++)
#pragma unroll
              for (int L = 0; L < NSD; L++) {
                double v = lam * (F[i][K] * F[j][L]) + mu * (F[i][L] * F[j][K]);
                if (K == L) v += mu * B[i][j];
                if (i == j) v += S[K][L];
                M.A[(int64_t)(((i * NSD + j) * NSD + K) * NSD + L) * npts + q] = v;
              }
      }
    } else {
      if (!(J > 0.0)) {                // (a NaN counts as well)
        nbad++;
        continue;
      }
      const double rJ = 1.0 / J, lnJ = log(J);
      double Fi[NSD][NSD];             // F^-1[K][i] = cof[i][K] / J
#pragma unroll
      for (int K = 0; K < NSD; K++)
#pragma unroll
        for (int i = 0; i < NSD; i++) Fi[K][i] = cof[i][K] * rJ;
      if (M.psi) {
        double trC = 0.0;
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int K = 0; K < NSD; K++) trC = fma(F[i][K], F[i][K], trC);
        M.psi[q] = 0.5 * mu * (trC - (double)NSD) - mu * lnJ + 0.5 * lam * lnJ * lnJ;
      }
      const double c1 = mu - lam * lnJ;
      if (M.P) {
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int K = 0; K < NSD; K++) M.P[(int64_t)(i * NSD + K) * npts + q] = mu * F[i][K] - c1 * Fi[K][i];
      }
      if (M.A) {
#pragma unroll
        for (int i = 0; i < NSD; i++)
#pragma unroll
          for (int j = 0; j < NSD; j++)
#pragma unroll
            for (int K = 0; K < NSD; K++)
#pragma unroll
              for (int L = 0; L < NSD; L++) {
                double v = c1 * (Fi[L][i] * Fi[K][j]) + lam * (Fi[K][i] * Fi[L][j]);
                if (i == j && K == L) v += mu;
                M.A[(int64_t)(((i * NSD + j) * NSD + K) * NSD + L) * npts + q] = v;
              }
      }
    }
  }
  // the workgroup's minimum and count: a tree in LDS, then one integer atomic each
  smin[tid] = kmin;
  sbad[tid] = nbad;
  __syncthreads();
  for (int o = (int)blockDim.x >> 1; o > 0; o >>= 1) {
    if (tid < o) {
      smin[tid] = smin[tid + o] < smin[tid] ? smin[tid + o] : smin[tid];
      sbad[tid] += sbad[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    atomicMin(&M.stat[1], smin[0]);
    if (KIND == 2 && sbad[0] > 0) atomicAdd((unsigned long long *)&M.stat[0], (unsigned long long)sbad[0]);
  }
}

template <int KIND>
static int tg_mat_launch(int nsd, const tg_mat_args &M) {
  const dim3 grid((unsigned)tg_cdiv(M.npts, TG_MAT_BLOCK));
  if (nsd == 2)
    hipLaunchKernelGGL((k_material_points<KIND, 2>), grid, dim3(TG_MAT_BLOCK), 0, g_tg.stream, M);
  else
    hipLaunchKernelGGL((k_material_points<KIND, 3>), grid, dim3(TG_MAT_BLOCK), 0, g_tg.stream, M);
  TG_LAUNCH_CHECK();
  return 0;
}

extern "C" int tg_material_points(int kind, const double *params, int nsd, int64_t npts, tg_vec_t gradu, tg_vec_t P_out,
                                  tg_vec_t A_out, tg_vec_t psi_out, int64_t *nbad, double *Jmin) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(kind >= 0 && kind <= 2, "tg_material_points: kind %d; 0 = linear, 1 = St. Venant-Kirchhoff, 2 = neo-Hookean", kind);
  TG_REQUIRE(nsd == 2 || nsd == 3, "tg_material_points: nsd = %d; 2 (plane strain) or 3", nsd);
  TG_REQUIRE(params, "tg_material_points: params = {lambda, mu}");
  TG_REQUIRE(npts >= 0 && tg_cdiv(npts, TG_MAT_BLOCK) < (1ll << 31), "tg_material_points: too many points for one launch");
  const int64_t n2 = (int64_t)nsd * nsd;
  TG_REQUIRE(gradu && gradu->n == n2 * npts, "tg_material_points: gradu holds nsd^2 npts = %lld values", (long long)(n2 * npts));
  TG_REQUIRE(!P_out || P_out->n == n2 * npts, "tg_material_points: P_out holds nsd^2 npts = %lld values", (long long)(n2 * npts));
  TG_REQUIRE(!A_out || A_out->n == n2 * n2 * npts, "tg_material_points: A_out holds nsd^4 npts = %lld values",
             (long long)(n2 * n2 * npts));
  TG_REQUIRE(!psi_out || psi_out->n == npts, "tg_material_points: psi_out holds npts = %lld values", (long long)npts);
  if (nbad) *nbad = 0;
  if (Jmin) *Jmin = 1.0;               // (no point: the undeformed state)
  if (npts == 0) return 0;
  tg_dbuf<long long> stat;
  TG_TRY(stat.alloc(2));
  long long init[2] = {0, 0x7fffffffffffffffll};
  memcpy(g_tg.host_pinned, init, sizeof(init));
  TG_CHECK_HIP(hipMemcpyAsync(stat.get(), g_tg.host_pinned, sizeof(init), hipMemcpyHostToDevice, g_tg.stream));
  tg_mat_args M;
  M.npts = npts;
  M.lambda = params[0];
  M.mu = params[1];
  M.gradu = gradu->d;
  M.P = P_out ? P_out->d : nullptr;
  M.A = A_out ? A_out->d : nullptr;
  M.psi = psi_out ? psi_out->d : nullptr;
  M.stat = stat.get();
  if (kind == 0)
    TG_TRY(tg_mat_launch<0>(nsd, M));
  else if (kind == 1)
    TG_TRY(tg_mat_launch<1>(nsd, M));
  else
    TG_TRY(tg_mat_launch<2>(nsd, M));
  TG_CHECK_HIP(hipMemcpyAsync(g_tg.host_pinned, stat.get(), sizeof(init), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  long long got[2];
  memcpy(got, g_tg.host_pinned, sizeof(got));
  if (nbad) *nbad = (int64_t)got[0];
  if (Jmin) *Jmin = tg_mat_unkey(got[1]);
  return 0;
}
