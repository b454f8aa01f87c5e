// Kirchhoff-Love shell laws at the quadrature points (demos/kl-shell-svk/dynamic-tspline.py:135-212 of the reference): from
// the jets of the reference surface X and of the displacement u -- x = X + u, first derivatives x_,a and second derivatives
// x_,ab with respect to the patch's parametric coordinates (tg_quad_geometry_jet, tg_quad_jet) --
//     A_ab = X_,a . X_,b,  A_3 = X_,1 x X_,2 / |.|,  B_ab = X_,ab . A_3;   a_ab, a_3, b_ab likewise from x
//     eps_ab = (a_ab - A_ab) / 2,   kappa_ab = B_ab - b_ab
//     C^abcd = E / (1 - nu^2) [nu A^ab A^cd + (1 - nu)/2 (A^ac A^bd + A^ad A^bc)]
//     psi = h/2 eps:C:eps + h^3/24 kappa:C:kappa            per unit reference area
// the energy density psi, s = d psi / d jet(u) (3 fields x 6 slots, the value slot zero) and T = d^2 psi / d jet(u)^2, in
// the layouts tg_jet_load_transform and tg_jet_transform read: s_i^alpha at (i 6 + alpha) npts + q, T_ij^{alpha beta} at
// ((3 i + j) 36 + 6 alpha + beta) npts + q -- the tangent values never leave the device.
//
// Closed forms.  With n^ab = h C:eps, m^ab = h^3/12 C:kappa, the contravariant basis a^c of the current surface and
// Gamma^c_ab = x_,ab . a^c:   delta eps_ab = sym(delta x_,a . x_,b),   delta a_3 = -a^c (a_3 . delta x_,c),
//     delta kappa_ab = -(delta x_,ab - Gamma^c_ab delta x_,c) . a_3 = a_3 . (k_ab . jet(delta x))
// so that every derivative of kappa is a_3 times a scalar row k_ab over the five derivative slots, and
//     T = h De^T C De + a_3 a_3^T (x) (h^3/12 k^T C k) + n^ab I (x) e_a e_b^T
//         + m^ab [a^c a_3^T at (slot ab, slot c) and its transpose] - M . D^2 a_3,     M = m^ab x_,ab,
//     -M . D^2 a_3 [w, v] = -(M . a^d)(a_3 . w_,c)(a^c . v_,d) + a^cd (M . a_3)(a_3 . w_,c)(a_3 . v_,d) - (M . a^c)(a^d . w_,c)(a_3 . v_,d).
// Pairs (ab) are held as v = a + b in {0, 1, 2} with the multiplicities 1, 2, 1.
//
// One thread per point; every output optional -- the arithmetic of an output does not depend on which others are asked for:
// the same subsets give the same bits.  Indices into the small tensors are compile-time constants after unrolling (no
// run-time-indexed local arrays, as k_material_points).  A point whose reference or current normal is degenerate,
// |X_,1 x X_,2| or |x_,1 x x_,2| < 1e-14 |X_,1| |X_,2|, writes nothing and is counted: a tree per workgroup, then one integer
// atomic; the count does not depend on the order.
#include "tg_common.h"
#include <cmath>

#define TG_SHELL_BLOCK 256

struct tg_shell_args {
  int64_t npts;
  double E, nu, h;
  const double *X, *u;         // jets: component alpha of coordinate / field c at (6 c + alpha) npts + q
  double *s, *T, *psi;         // any of them may be null
  unsigned long long *nbad;
};

__device__ __forceinline__ void tg_shell_cross(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double tg_shell_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

template <int KIND>
__global__ void __launch_bounds__(TG_SHELL_BLOCK) k_shell_points(tg_shell_args M) {
  static_assert(KIND == 0, "kind 0: St. Venant-Kirchhoff");
  __shared__ int sbad[TG_SHELL_BLOCK];
  const int tid = threadIdx.x;
  const int64_t npts = M.npts;
  int nbad = 0;
  for (int t = tid; t < TG_SHELL_BLOCK; t += blockDim.x) {
    const int64_t q = (int64_t)blockIdx.x * TG_SHELL_BLOCK + t;
    if (q >= npts) continue;
    // derivative slots 1..5 of the reference and the current surface: G[s][c], g[s][c], s = 0, 1 first, 2, 3, 4 second (00, 01, 11)
    double G[5][3], g[5][3];
#pragma unroll
    for (int s = 0; s < 5; s++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        G[s][c] = M.X[(int64_t)(6 * c + 1 + s) * npts + q];
        g[s][c] = G[s][c] + M.u[(int64_t)(6 * c + 1 + s) * npts + q];
      }
    double N3[3], n3[3];
    tg_shell_cross(G[0], G[1], N3);
    tg_shell_cross(g[0], g[1], n3);
    const double JA = sqrt(tg_shell_dot(N3, N3)), Ja = sqrt(tg_shell_dot(n3, n3));
    const double floor_ = 1e-14 * sqrt(tg_shell_dot(G[0], G[0])) * sqrt(tg_shell_dot(G[1], G[1]));
    if (!(JA >= floor_) || !(Ja >= floor_)) {
      nbad++;
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      N3[c] /= JA;
      n3[c] /= Ja;
    }
    // metrics and curvatures by pair v = a + b
    double Am[3], am[3], eps[3], kap[3];
    Am[0] = tg_shell_dot(G[0], G[0]), Am[1] = tg_shell_dot(G[0], G[1]), Am[2] = tg_shell_dot(G[1], G[1]);
    am[0] = tg_shell_dot(g[0], g[0]), am[1] = tg_shell_dot(g[0], g[1]), am[2] = tg_shell_dot(g[1], g[1]);
#pragma unroll
    for (int v = 0; v < 3; v++) {
      eps[v] = 0.5 * (am[v] - Am[v]);
      kap[v] = tg_shell_dot(G[2 + v], N3) - tg_shell_dot(g[2 + v], n3);
    }
    // contravariant metrics: Ai[v], ai[v]
    const double detA = Am[0] * Am[2] - Am[1] * Am[1], deta = am[0] * am[2] - am[1] * am[1];
    const double Ai[3] = {Am[2] / detA, -Am[1] / detA, Am[0] / detA};
    const double ai[3] = {am[2] / deta, -am[1] / deta, am[0] / deta};
    // material tensor by pairs: C[v][w] = C^{ab cd}, (ab) = pair v, (cd) = pair w.  With Ai2[a][b] = Ai[a + b]:
    // nu A^ab A^cd + (1 - nu)/2 (A^ac A^bd + A^ad A^bc) at the representatives (00), (01), (11)
    const double cE = M.E / (1.0 - M.nu * M.nu), nu = M.nu, hn = 0.5 * (1.0 - M.nu);
    double C[3][3];
#pragma unroll
    for (int v = 0; v < 3; v++)
#pragma unroll
      for (int w = 0; w < 3; w++) {
        const int a = v == 2 ? 1 : 0, b = v == 0 ? 0 : 1, c = w == 2 ? 1 : 0, d = w == 0 ? 0 : 1;
        C[v][w] = cE * (nu * Ai[a + b] * Ai[c + d] + hn * (Ai[a + c] * Ai[b + d] + Ai[a + d] * Ai[b + c]));
      }
    const double hm = M.h, hb = M.h * M.h * M.h / 12.0;
    const double mult[3] = {1.0, 2.0, 1.0};
    double nr[3], mr[3];         // n^ab, m^ab by pair
#pragma unroll
    for (int v = 0; v < 3; v++) {
      nr[v] = hm * (C[v][0] * eps[0] + 2.0 * C[v][1] * eps[1] + C[v][2] * eps[2]);
      mr[v] = hb * (C[v][0] * kap[0] + 2.0 * C[v][1] * kap[1] + C[v][2] * kap[2]);
    }
    if (M.psi)
      M.psi[q] = 0.5 * (nr[0] * eps[0] + 2.0 * nr[1] * eps[1] + nr[2] * eps[2]) + 0.5 * (mr[0] * kap[0] + 2.0 * mr[1] * kap[1] + mr[2] * kap[2]);
    if (!M.s && !M.T) continue;
    // contravariant basis a^c and Gamma^c_v = x_,v . a^c
    double gu[2][3], Gam[2][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      gu[0][c] = ai[0] * g[0][c] + ai[1] * g[1][c];
      gu[1][c] = ai[1] * g[0][c] + ai[2] * g[1][c];
    }
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int v = 0; v < 3; v++) Gam[c][v] = tg_shell_dot(g[2 + v], gu[c]);
    // k[v][A]: d kappa_v / d jet = a_3 k[v][A] over the derivative slots A = 0..4 (jet slots 1..5)
    double k[3][5];
#pragma unroll
    for (int v = 0; v < 3; v++) {
      k[v][0] = Gam[0][v];
      k[v][1] = Gam[1][v];
#pragma unroll
      for (int w = 0; w < 3; w++) k[v][2 + w] = v == w ? -1.0 : 0.0;
    }
    // mk[A] = sum_v mult_v m_v k[v][A]: the bending part of s is a_3 mk
    double mk[5];
#pragma unroll
    for (int A = 0; A < 5; A++) mk[A] = mr[0] * k[0][A] + 2.0 * mr[1] * k[1][A] + mr[2] * k[2][A];
    if (M.s) {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        M.s[(int64_t)(6 * i) * npts + q] = 0.0;
#pragma unroll
        for (int A = 0; A < 5; A++) {
          double v = mk[A] * n3[i];
          if (A < 2) v += nr[A + 0] * g[0][i] + nr[A + 1] * g[1][i];          // n^{A b} x_,b
          M.s[(int64_t)(6 * i + 1 + A) * npts + q] = v;
        }
      }
    }
    if (!M.T) continue;
    // Kb[A][B] = h^3/12 sum_vw mult_v mult_w k[v][A] C[v][w] k[w][B]
    double Ck[3][5], Kb[5][5];
#pragma unroll
    for (int v = 0; v < 3; v++)
#pragma unroll
      for (int B = 0; B < 5; B++) Ck[v][B] = hb * (C[v][0] * k[0][B] + 2.0 * C[v][1] * k[1][B] + C[v][2] * k[2][B]);
#pragma unroll
    for (int A = 0; A < 5; A++)
#pragma unroll
      for (int B = 0; B < 5; B++) Kb[A][B] = k[0][A] * Ck[0][B] + 2.0 * k[1][A] * Ck[1][B] + k[2][A] * Ck[2][B];
    // M = m^ab x_,ab and its components on a^c, a_3
    double Mv[3];
#pragma unroll
    for (int c = 0; c < 3; c++) Mv[c] = mr[0] * g[2][c] + 2.0 * mr[1] * g[3][c] + mr[2] * g[4][c];
    const double Mu[2] = {tg_shell_dot(Mv, gu[0]), tg_shell_dot(Mv, gu[1])}, M3 = tg_shell_dot(Mv, n3);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double *To = M.T + (int64_t)((3 * i + j) * 36) * npts + q;
#pragma unroll
        for (int al = 0; al < 6; al++)
#pragma unroll
          for (int be = 0; be < 6; be++) {
            double v = 0.0;
            if (al >= 1 && be >= 1) {
              const int A = al - 1, B = be - 1;
              v = n3[i] * n3[j] * Kb[A][B];
              if (A < 2 && B < 2) {
                // membrane: h sum_bd C^{A b B d} x_,b[i] x_,d[j] + n^{AB} delta_ij
                double mem = 0.0;
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                  for (int d = 0; d < 2; d++) mem += C[A + b][B + d] * g[b][i] * g[d][j];
                v += hm * mem;
                if (i == j) v += nr[A + B];
                // -M . D^2 a_3: row slot c = A, column slot d = B
                v += -Mu[B] * n3[i] * gu[A][j] + ai[A + B] * M3 * n3[i] * n3[j] - Mu[A] * gu[B][i] * n3[j];
              }
              // m^ab (a^c a_3^T) at (second slot, first slot) and the transpose
              if (A >= 2 && B < 2) v += mult[A - 2] * mr[A - 2] * gu[B][i] * n3[j];
              if (A < 2 && B >= 2) v += mult[B - 2] * mr[B - 2] * n3[i] * gu[A][j];
            }
            To[(int64_t)(6 * al + be) * npts] = v;
          }
      }
  }
  // the workgroup's count: a tree in LDS, then one integer atomic
  sbad[tid] = nbad;
  __syncthreads();
  for (int o = (int)blockDim.x >> 1; o > 0; o >>= 1) {
    if (tid < o) sbad[tid] += sbad[tid + o];
    __syncthreads();
  }
  if (tid == 0 && sbad[0] > 0) atomicAdd(M.nbad, (unsigned long long)sbad[0]);
}

extern "C" int tg_shell_points(int kind, const double *params, int64_t npts, tg_vec_t Xjet, tg_vec_t ujet, tg_vec_t s_out, tg_vec_t T_out,
                               tg_vec_t psi_out, int64_t *nbad) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(kind == 0, "tg_shell_points: kind %d; 0 = St. Venant-Kirchhoff Kirchhoff-Love shell", kind);
  TG_REQUIRE(params, "tg_shell_points: params = {E, nu, thickness}");
  TG_REQUIRE(npts >= 0 && tg_cdiv(npts, TG_SHELL_BLOCK) < (1ll << 31), "tg_shell_points: too many points for one launch");
  TG_REQUIRE(Xjet && Xjet->n == 18 * npts && ujet && ujet->n == 18 * npts,
             "tg_shell_points: Xjet and ujet hold 3 x 6 x npts = %lld values each (nsd = nF = 3, d = 2)", (long long)(18 * npts));
  TG_REQUIRE(!s_out || s_out->n == 18 * npts, "tg_shell_points: s_out holds 18 npts = %lld values", (long long)(18 * npts));
  TG_REQUIRE(!T_out || T_out->n == 324 * npts, "tg_shell_points: T_out holds 324 npts = %lld values", (long long)(324 * npts));
  TG_REQUIRE(!psi_out || psi_out->n == npts, "tg_shell_points: psi_out holds npts = %lld values", (long long)npts);
  if (nbad) *nbad = 0;
  if (npts == 0) return 0;
  tg_dbuf<unsigned long long> stat;
  TG_TRY(stat.alloc(1));
  TG_CHECK_HIP(hipMemsetAsync(stat.get(), 0, sizeof(unsigned long long), g_tg.stream));
  tg_shell_args M;
  M.npts = npts;
  M.E = params[0], M.nu = params[1], M.h = params[2];
  M.X = Xjet->d;
  M.u = ujet->d;
  M.s = s_out ? s_out->d : nullptr;
  M.T = T_out ? T_out->d : nullptr;
  M.psi = psi_out ? psi_out->d : nullptr;
  M.nbad = stat.get();
  hipLaunchKernelGGL((k_shell_points<0>), dim3((unsigned)tg_cdiv(npts, TG_SHELL_BLOCK)), dim3(TG_SHELL_BLOCK), 0, g_tg.stream, M);
  TG_LAUNCH_CHECK();
  TG_CHECK_HIP(hipMemcpyAsync(g_tg.host_pinned, stat.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  unsigned long long got;
  memcpy(&got, g_tg.host_pinned, sizeof(got));
  if (nbad) *nbad = (int64_t)got;
  return 0;
}
