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
  static_assert(KIND == 0, "kind 0: St. Venant-Kirchhoff (kind 1 is k_shell_hyper_points)");
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

// ---- kind 1: the incompressible neo-Hookean shell integrated through the thickness (demos/kl-shell-hyper/kl-hyper.py:98-215 of
// the reference).  At the thickness coordinate xi, with the truncated metrics Gm = A - 2 xi B, gm = a - 2 xi b:
//     G_b = A_b + xi d_b A_3 = (I - xi B A^-1)_bd A_d (Weingarten),  G^a = (Gm^-1)_ab G_b,  e_0, e_1 by Gram-Schmidt on G_0, G_1,
//     R_ia = e_i . G^a = (Eg Gm^-1)_ia,  Eg_ib = e_i . G_b upper triangular from the metric G_b . G_e alone,
//     Chat = R (gm - Gm) R^T = R 2 (eps + xi kappa) R^T   (formed from the strains: small strains do not cancel),
//     psi(xi) = phi(Chat),  psi = sum_k w_k psi(xi_k).
// Chat is affine in (eps, kappa) and R depends on the reference alone, so with f = d phi / d Chat, hh = d^2 phi / d Chat^2 by pairs
// and Zm[w][v] = mult_w sym(R_ia R_jb) (w = (ij), v = (ab)):   F = Zm^T f,  H = Zm^T hh Zm,
//     n = 2 sum w F,  m = 2 sum w xi F,  D_ee = 4 sum w H,  D_ek = 4 sum w xi H,  D_kk = 4 sum w xi^2 H.
// Only these 3 + 3 + 6 + 6 + 6 values and psi outlive the thickness loop; the kinematic variations are those of kind 0 with
// h C -> D_ee, h^3/12 C -> D_kk and the cross term De^T D_ek Dk + Dk^T D_ek De.  A point is also left alone and counted when
// det Gm <= 0 or det C_2D <= 0 at a thickness point.
struct tg_shell_hyper_args {
  int64_t npts;
  double hmu;                  // mu / 2
  double xi[4], w[4];          // the thickness rule on (-h/2, h/2)
  int nth;
  const double *X, *u;
  double *s, *T, *psi;         // any of them may be null
  unsigned long long *nbad;
};

// the potential, the one place that names it: phi(Chat) = mu/2 (tr C + 1 / det C - 3), C = I + Chat, by the pairs c = (00, 01, 11);
// with t = tr Chat + det Chat = det C - 1:  phi = mu/2 (tr Chat - t / (1 + t)),  f = mu/2 (t (2 + t) I - adj Chat) / (1 + t)^2,
// hh = mu/2 (2 adj C (x) adj C / (1 + t)^3 - L / (1 + t)^2), L = d adj C / d C (adj C = tr(C) I - C); hh as the upper triangle
// (00 01 02 11 12 22) of the pairs.  Returns det C.
__device__ __forceinline__ double tg_shell_neohooke(double hmu, const double *c, double *phi, double *f, double *hh) {
  const double tr = c[0] + c[2], t = tr + (c[0] * c[2] - c[1] * c[1]), delta = 1.0 + t;
  const double i2 = 1.0 / (delta * delta), a2 = hmu * i2, a3 = 2.0 * a2 / delta;
  *phi = hmu * (tr - t / delta);
  const double tt = t * (2.0 + t);
  f[0] = a2 * (tt - c[2]), f[1] = a2 * c[1], f[2] = a2 * (tt - c[0]);
  const double A[3] = {1.0 + c[2], -c[1], 1.0 + c[0]};
  hh[0] = a3 * A[0] * A[0], hh[1] = a3 * A[0] * A[1], hh[2] = a3 * A[0] * A[2] - a2;
  hh[3] = a3 * A[1] * A[1] + 0.5 * a2, hh[4] = a3 * A[1] * A[2], hh[5] = a3 * A[2] * A[2];
  return delta;
}

// place of (v, w) in the upper triangle of a symmetric 3 x 3 matrix of pairs
__device__ __forceinline__ constexpr int tg_shell_sy(int v, int w) { return v <= w ? 3 * v - v * (v - 1) / 2 + (w - v) : 3 * w - w * (w - 1) / 2 + (v - w); }

__global__ void __launch_bounds__(TG_SHELL_BLOCK) k_shell_hyper_points(tg_shell_hyper_args M) {
  __shared__ int sbad[TG_SHELL_BLOCK];
  const int tid = threadIdx.x;
  const int64_t npts = M.npts;
  int nbad = 0;
  for (int t = tid; t < TG_SHELL_BLOCK; t += blockDim.x) {
    const int64_t q = (int64_t)blockIdx.x * TG_SHELL_BLOCK + t;
    if (q >= npts) continue;
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
    double Am[3], Bm[3], am[3], eps[3], kap[3];
    Am[0] = tg_shell_dot(G[0], G[0]), Am[1] = tg_shell_dot(G[0], G[1]), Am[2] = tg_shell_dot(G[1], G[1]);
    am[0] = tg_shell_dot(g[0], g[0]), am[1] = tg_shell_dot(g[0], g[1]), am[2] = tg_shell_dot(g[1], g[1]);
#pragma unroll
    for (int v = 0; v < 3; v++) {
      Bm[v] = tg_shell_dot(G[2 + v], N3);
      eps[v] = 0.5 * (am[v] - Am[v]);
      kap[v] = Bm[v] - tg_shell_dot(g[2 + v], n3);
    }
    const double detA = Am[0] * Am[2] - Am[1] * Am[1], deta = am[0] * am[2] - am[1] * am[1];
    const double Ai[3] = {Am[2] / detA, -Am[1] / detA, Am[0] / detA};
    const double ai[3] = {am[2] / deta, -am[1] / deta, am[0] / deta};
    // BA[b][d] = (B A^-1)_bd
    const double BA[2][2] = {{Bm[0] * Ai[0] + Bm[1] * Ai[1], Bm[0] * Ai[1] + Bm[1] * Ai[2]},
                             {Bm[1] * Ai[0] + Bm[2] * Ai[1], Bm[1] * Ai[1] + Bm[2] * Ai[2]}};
    // ---- the thickness loop: psi, the resultants and the three material matrices (upper triangles of the pairs)
    double psi = 0.0, nr[3] = {0.0, 0.0, 0.0}, mr[3] = {0.0, 0.0, 0.0};
    double Dee[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Dek[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Dkk[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    for (int kq = 0; kq < M.nth; kq++) {
      const double xi = M.xi[kq], w = M.w[kq];
      const double Q[2][2] = {{1.0 - xi * BA[0][0], -xi * BA[0][1]}, {-xi * BA[1][0], 1.0 - xi * BA[1][1]}};
      // Gg = Q A Q^T: the metric of G_0, G_1
      const double QA[2][2] = {{Q[0][0] * Am[0] + Q[0][1] * Am[1], Q[0][0] * Am[1] + Q[0][1] * Am[2]},
                               {Q[1][0] * Am[0] + Q[1][1] * Am[1], Q[1][0] * Am[1] + Q[1][1] * Am[2]}};
      const double Gg00 = QA[0][0] * Q[0][0] + QA[0][1] * Q[0][1], Gg01 = QA[0][0] * Q[1][0] + QA[0][1] * Q[1][1];
      const double Gg11 = QA[1][0] * Q[1][0] + QA[1][1] * Q[1][1];
      const double Gm[3] = {Am[0] - 2.0 * xi * Bm[0], Am[1] - 2.0 * xi * Bm[1], Am[2] - 2.0 * xi * Bm[2]};
      const double detGm = Gm[0] * Gm[2] - Gm[1] * Gm[1];
      const double Gi[3] = {Gm[2] / detGm, -Gm[1] / detGm, Gm[0] / detGm};
      const double Eg00 = sqrt(Gg00), Eg01 = Gg01 / Eg00, Eg11 = sqrt((Gg00 * Gg11 - Gg01 * Gg01) / Gg00);
      const double R[2][2] = {{Eg00 * Gi[0] + Eg01 * Gi[1], Eg00 * Gi[1] + Eg01 * Gi[2]}, {Eg11 * Gi[1], Eg11 * Gi[2]}};
      // Z[w][v] = sym(R_ia R_jb), w = (ij), v = (ab)
      double Z[3][3];
#pragma unroll
      for (int wv = 0; wv < 3; wv++)
#pragma unroll
        for (int v = 0; v < 3; v++) {
          const int i = wv == 2 ? 1 : 0, j = wv == 0 ? 0 : 1, a = v == 2 ? 1 : 0, b = v == 0 ? 0 : 1;
          Z[wv][v] = 0.5 * (R[i][a] * R[j][b] + R[i][b] * R[j][a]);
        }
      double ch[3], phi, f[3], hh[6];
#pragma unroll
      for (int wv = 0; wv < 3; wv++)
        ch[wv] = 2.0 * (Z[wv][0] * (eps[0] + xi * kap[0]) + 2.0 * Z[wv][1] * (eps[1] + xi * kap[1]) + Z[wv][2] * (eps[2] + xi * kap[2]));
      const double delta = tg_shell_neohooke(M.hmu, ch, &phi, f, hh);
      if (!(detGm > 0.0) || !(delta > 0.0)) bad = true;
      psi += w * phi;
      // F = Zm^T f, H = Zm^T hh Zm with Zm[w][v] = mult_w Z[w][v]
      double hZ[3][3];
#pragma unroll
      for (int wv = 0; wv < 3; wv++)
#pragma unroll
        for (int v = 0; v < 3; v++)
          hZ[wv][v] = hh[tg_shell_sy(wv, 0)] * Z[0][v] + 2.0 * hh[tg_shell_sy(wv, 1)] * Z[1][v] + hh[tg_shell_sy(wv, 2)] * Z[2][v];
      const double w2 = 2.0 * w, w4 = 4.0 * w;
#pragma unroll
      for (int v = 0; v < 3; v++) {
        const double F = Z[0][v] * f[0] + 2.0 * Z[1][v] * f[1] + Z[2][v] * f[2];
        nr[v] += w2 * F;
        mr[v] += w2 * xi * F;
#pragma unroll
        for (int v2 = v; v2 < 3; v2++) {
          const double H = Z[0][v] * hZ[0][v2] + 2.0 * Z[1][v] * hZ[1][v2] + Z[2][v] * hZ[2][v2];
          Dee[tg_shell_sy(v, v2)] += w4 * H;
          Dek[tg_shell_sy(v, v2)] += w4 * xi * H;
          Dkk[tg_shell_sy(v, v2)] += w4 * xi * xi * H;
        }
      }
    }
    if (bad) {
      nbad++;
      continue;
    }
    if (M.psi) M.psi[q] = psi;
    if (!M.s && !M.T) continue;
    // ---- the kinematic variations, as kind 0
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
    double k[3][5];
#pragma unroll
    for (int v = 0; v < 3; v++) {
      k[v][0] = Gam[0][v];
      k[v][1] = Gam[1][v];
#pragma unroll
      for (int w = 0; w < 3; w++) k[v][2 + w] = v == w ? -1.0 : 0.0;
    }
    const double mult[3] = {1.0, 2.0, 1.0};
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
    // Kk[v][B] = sum_w mult_w D_kk[v][w] k[w][B],  Ek likewise from D_ek;  Kb[A][B] = sum_v mult_v k[v][A] Kk[v][B]
    double Kk[3][5], Ek[3][5], Kb[5][5];
#pragma unroll
    for (int v = 0; v < 3; v++)
#pragma unroll
      for (int B = 0; B < 5; B++) {
        Kk[v][B] = Dkk[tg_shell_sy(v, 0)] * k[0][B] + 2.0 * Dkk[tg_shell_sy(v, 1)] * k[1][B] + Dkk[tg_shell_sy(v, 2)] * k[2][B];
        Ek[v][B] = Dek[tg_shell_sy(v, 0)] * k[0][B] + 2.0 * Dek[tg_shell_sy(v, 1)] * k[1][B] + Dek[tg_shell_sy(v, 2)] * k[2][B];
      }
#pragma unroll
    for (int A = 0; A < 5; A++)
#pragma unroll
      for (int B = 0; B < 5; B++) Kb[A][B] = k[0][A] * Kk[0][B] + 2.0 * k[1][A] * Kk[1][B] + k[2][A] * Kk[2][B];
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
              // the cross term: De^T D_ek Dk at the first-derivative rows, its transpose at the first-derivative columns
              if (A < 2) v += (g[0][i] * Ek[A + 0][B] + g[1][i] * Ek[A + 1][B]) * n3[j];
              if (B < 2) v += n3[i] * (g[0][j] * Ek[B + 0][A] + g[1][j] * Ek[B + 1][A]);
              if (A < 2 && B < 2) {
                double mem = 0.0;
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                  for (int d = 0; d < 2; d++) mem += Dee[tg_shell_sy(A + b, B + d)] * g[b][i] * g[d][j];
                v += mem;
                if (i == j) v += nr[A + B];
                v += -Mu[B] * n3[i] * gu[A][j] + ai[A + B] * M3 * n3[i] * n3[j] - Mu[A] * gu[B][i] * n3[j];
              }
              if (A >= 2 && B < 2) v += mult[A - 2] * mr[A - 2] * gu[B][i] * n3[j];
              if (A < 2 && B >= 2) v += mult[B - 2] * mr[B - 2] * n3[i] * gu[A][j];
            }
            To[(int64_t)(6 * al + be) * npts] = v;
          }
      }
  }
  sbad[tid] = nbad;
  __syncthreads();
  for (int o = (int)blockDim.x >> 1; o > 0; o >>= 1) {
    if (tid < o) sbad[tid] += sbad[tid + o];
    __syncthreads();
  }
  if (tid == 0 && sbad[0] > 0) atomicAdd(M.nbad, (unsigned long long)sbad[0]);
}

// ---- the follower pressure of kl-hyper.py:231, added to the law's outputs: -P (x_,1 x x_,2) / |X_,1 x X_,2| in the value slots of
// s, its derivative with respect to the first-derivative slots in T^{0,1}, T^{0,2}.  One thread per point; a point whose reference
// normal is below the law's floor is left alone.
__global__ void __launch_bounds__(TG_SHELL_BLOCK) k_shell_pressure_points(int64_t npts, double P, const double *X, const double *u,
                                                                         double *s, double *T) {
  for (int t = threadIdx.x; t < TG_SHELL_BLOCK; t += blockDim.x) {
    const int64_t q = (int64_t)blockIdx.x * TG_SHELL_BLOCK + t;
    if (q >= npts) continue;
    double G[2][3], g[2][3];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        G[a][c] = X[(int64_t)(6 * c + 1 + a) * npts + q];
        g[a][c] = G[a][c] + u[(int64_t)(6 * c + 1 + a) * npts + q];
      }
    double N3[3], n[3];
    tg_shell_cross(G[0], G[1], N3);
    tg_shell_cross(g[0], g[1], n);
    const double JA = sqrt(tg_shell_dot(N3, N3));
    if (!(JA >= 1e-14 * sqrt(tg_shell_dot(G[0], G[0])) * sqrt(tg_shell_dot(G[1], G[1]))) || !(JA > 0.0)) continue;
    const double c = -P / JA;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int j = (i + 1) % 3, k = (i + 2) % 3;            // eps_ijk = 1, eps_ikj = -1
      if (s) s[(int64_t)(6 * i) * npts + q] += c * n[i];
      if (T) {
        T[(int64_t)((3 * i + j) * 36 + 1) * npts + q] += c * g[1][k];
        T[(int64_t)((3 * i + k) * 36 + 1) * npts + q] -= c * g[1][j];
        T[(int64_t)((3 * i + k) * 36 + 2) * npts + q] += c * g[0][j];
        T[(int64_t)((3 * i + j) * 36 + 2) * npts + q] -= c * g[0][k];
      }
    }
  }
}

extern "C" int tg_shell_pressure_points(int64_t npts, double pressure, tg_vec_t Xjet, tg_vec_t ujet, tg_vec_t s_inout, tg_vec_t T_inout) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(npts >= 0 && tg_cdiv(npts, TG_SHELL_BLOCK) < (1ll << 31), "tg_shell_pressure_points: too many points for one launch");
  TG_REQUIRE(Xjet && Xjet->n == 18 * npts && ujet && ujet->n == 18 * npts,
             "tg_shell_pressure_points: Xjet and ujet hold 3 x 6 x npts = %lld values each", (long long)(18 * npts));
  TG_REQUIRE(!s_inout || s_inout->n == 18 * npts, "tg_shell_pressure_points: s_inout holds 18 npts = %lld values", (long long)(18 * npts));
  TG_REQUIRE(!T_inout || T_inout->n == 324 * npts, "tg_shell_pressure_points: T_inout holds 324 npts = %lld values", (long long)(324 * npts));
  if (npts == 0 || (!s_inout && !T_inout)) return 0;
  hipLaunchKernelGGL(k_shell_pressure_points, dim3((unsigned)tg_cdiv(npts, TG_SHELL_BLOCK)), dim3(TG_SHELL_BLOCK), 0, g_tg.stream, npts,
                     pressure, (const double *)Xjet->d, (const double *)ujet->d, s_inout ? s_inout->d : nullptr,
                     T_inout ? T_inout->d : nullptr);
  TG_LAUNCH_CHECK();
  return 0;
}

// the Gauss rules of 1 to 4 points on (-1, 1): points | weights (getQuadRule of the reference, calculusUtils.py:412-457)
static const double tg_shell_gauss[4][2][4] = {
    {{0.0}, {2.0}},
    {{-0.5773502691896257645091488, 0.5773502691896257645091488}, {1.0, 1.0}},
    {{-0.77459666924148337703585308, 0.0, 0.77459666924148337703585308},
     {0.55555555555555555555555556, 0.88888888888888888888888889, 0.55555555555555555555555556}},
    {{-0.86113631159405257524, -0.33998104358485626481, 0.33998104358485626481, 0.86113631159405257524},
     {0.34785484513745385736, 0.65214515486254614264, 0.65214515486254614264, 0.34785484513745385736}}};

extern "C" int tg_shell_points(int kind, const double *params, int64_t npts, tg_vec_t Xjet, tg_vec_t ujet, tg_vec_t s_out, tg_vec_t T_out,
                               tg_vec_t psi_out, int64_t *nbad) {
  TG_REQUIRE_INIT();
  TG_REQUIRE(kind == 0 || kind == 1, "tg_shell_points: kind %d; 0 = St. Venant-Kirchhoff, 1 = incompressible neo-Hookean through the "
             "thickness", kind);
  TG_REQUIRE(params, "tg_shell_points: params = {E, nu, thickness} (kind 0), {mu, thickness, n_thickness} (kind 1)");
  TG_REQUIRE(kind != 1 || params[2] == 1.0 || params[2] == 2.0 || params[2] == 3.0 || params[2] == 4.0,
             "tg_shell_points: kind 1 integrates with 1, 2, 3 or 4 thickness points; params[2] = %g", params[2]);
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
  const dim3 grid((unsigned)tg_cdiv(npts, TG_SHELL_BLOCK)), block(TG_SHELL_BLOCK);
  if (kind == 0) {
    tg_shell_args M;
    M.npts = npts;
    M.E = params[0], M.nu = params[1], M.h = params[2];
    M.X = Xjet->d;
    M.u = ujet->d;
    M.s = s_out ? s_out->d : nullptr;
    M.T = T_out ? T_out->d : nullptr;
    M.psi = psi_out ? psi_out->d : nullptr;
    M.nbad = stat.get();
    hipLaunchKernelGGL((k_shell_points<0>), grid, block, 0, g_tg.stream, M);
  } else {
    tg_shell_hyper_args M;
    M.npts = npts;
    M.hmu = 0.5 * params[0];
    M.nth = (int)params[2];
    for (int k = 0; k < 4; k++) {                  // the rule on (-h/2, h/2), as getQuadRuleInterval
      M.xi[k] = k < M.nth ? params[1] * tg_shell_gauss[M.nth - 1][0][k] / 2.0 : 0.0;
      M.w[k] = k < M.nth ? params[1] * tg_shell_gauss[M.nth - 1][1][k] / 2.0 : 0.0;
    }
    M.X = Xjet->d;
    M.u = ujet->d;
    M.s = s_out ? s_out->d : nullptr;
    M.T = T_out ? T_out->d : nullptr;
    M.psi = psi_out ? psi_out->d : nullptr;
    M.nbad = stat.get();
    hipLaunchKernelGGL(k_shell_hyper_points, grid, block, 0, g_tg.stream, M);
  }
  TG_LAUNCH_CHECK();
  TG_CHECK_HIP(hipMemcpyAsync(g_tg.host_pinned, stat.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, g_tg.stream));
  TG_CHECK_HIP(hipStreamSynchronize(g_tg.stream));
  unsigned long long got;
  memcpy(&got, g_tg.host_pinned, sizeof(got));
  if (nbad) *nbad = (int64_t)got;
  return 0;
}
